"""Per-kernel tests of the encoder's entrance and of the fp32 QKV scatter against the float64 references of tests/entrance_reference.py (derivation of
every bound: that module's docstring; the references themselves are tied to torch on the CPU in tests/test_entrance_reference_cpu.py).  The gate is
element-wise, |got - ref| <= bound(element); where the operation is exact (padding columns, counters, cls rows, copies, untouched memory, integer-valued
GEMMs) equality.  Every element of every returned buffer is compared.

The forms of infer() that had no kernel-level test, each reached here through its own launcher:
  preprocess_kernel as model_encoder.hip launches it (launch_preprocess: im2col scatter, K padding columns, counter zeroing, f16 output, f16 input, round16,
      the two-tap aa = 0 branch)                                               test_preprocess, test_preprocess_counters, test_preprocess_past_the_block_cap
  EPI_PATCH (launch_gemm)                                                      test_patch_epilogue
  posembed_kernel with size_mode = 1 (launch_posembed)                         test_posembed
  EPI_QKV with v_rowmajor = 0 (launch_gemm)                                    test_qkv_transposed_v
  EPI_CONVT with uv_in = 1 (launch_gemm)                                       test_convt_uv_at_the_input_pixel
  resize_bicubic_aa_kernel<f16> and its round16 form (launch_resize_bicubic_aa) test_resize_bicubic_aa_f16_and_round16

Worst observed error / bound per kernel, measured on an MI355X (61 passed, 4.3 s for the module, slowest case 0.43 s; `pytest -s` prints the table of
the run at hand):
  preprocess, fp32 store: aa = 1 0.521 (f32 image), 0.387 (f16 image / round16); aa = 0 0.423, 0.417        fp16 store: 0.987 - 0.992 (all six forms)
  posembed 0.622 (plain), 0.385 (size mode)        patch epilogue 0.057 (f32), 0.025 (f16)        convt uv_in 0.028 (f32), 0.926 (f16)
  resize_bicubic_aa 0.153 (<f32>), 0.156 (<f16>), 0.970 (round16)
The resize and position-embedding bounds have three parts - (taps_y + taps_x + 8) u sum|w v|, one ulp32 of the centre times the inverse scale times the
spread of the taps, the propagation through (r - mean) / sd - and, for the two CUBIC filters only, a fourth: the absolute error of a float32 weight under
FMA contraction (4 u inner, 12 u / 18 u outer taps).  Against the three-part form alone (ledger lines "/ three-part form", not gated) the kernels stand at
  posembed 5.57 (plain), 2.83 (size mode)        resize_bicubic_aa 0.997 (<f32>), 0.982 (<f16>)
and torch's own float32 CPU results at 3.9 (posembed 60 x 60) and 1.3 - 1.4 (antialiased bicubic, up-scaling): the three-part form has a hole for a cubic
filter - near the filter's zeros the weight error is not relative to |w v| - and the kernels are right (entrance_reference's docstring, e_w).  The
bilinear preprocess is gated on the three-part form as it is.
The 0.93 - 0.99 figures are outputs stored as fp16: the bound is the fp32 bound + HALF an fp16 ulp of the result, which a round-to-nearest store all but
reaches.  The 0.03 - 0.06 figures are bounds that admit K = 640 strictly sequential additions where the MFMA chain's errors cancel.  Exact gates: padding
columns, counters and their guard, cls rows, untouched rows, the bypass, k and v^T, the integer-valued patch matrices - all equal.  Also observed: the
identity resize is within 1 ulp32 of f32((v - mean) / sd) but in no form bit-equal to it (two roundings against one); posembed in size mode at 37 x 37 IS
bit-equal to pos.
EXPERIMENTS.md R9.1 has the table with cases and bounds, and the eight one-line kernel mutations with the cases that caught each."""
import numpy as np
import pytest
import torch

import entrance_reference as ER
import tail_reference as TR

pytestmark = pytest.mark.gpu

WORST = {}
NOTES = {}
INVALID = -1
FILL = 123.0        # exact in fp16 and fp32, far from every value a kernel here can produce


@pytest.fixture(scope="module")
def H():
    import hip_util
    yield hip_util
    print("\nworst error / bound per kernel:")
    for k in sorted(WORST):
        print(f"  {k:34s} {WORST[k][0]:8.4f}   ({WORST[k][1]} cases)")
    for k in sorted(NOTES):
        print(f"  {k}: {'mixed' if len(NOTES[k]) > 1 else 'always' if True in NOTES[k] else 'never'}")


def check(kernel, got, ref, bound, what):
    got = got.detach().cpu().double().numpy() if torch.is_tensor(got) else np.asarray(got, dtype=np.float64)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert np.isfinite(got).all(), what
    ratio = np.abs(got - ref) / bound
    worst = float(ratio.max())
    w = WORST.setdefault(kernel, [0.0, 0])
    w[0], w[1] = max(w[0], worst), w[1] + 1
    assert worst <= 1.0, f"{kernel} {what}: error / bound = {worst:.3f} at {np.unravel_index(ratio.argmax(), ratio.shape)}"


def record(kernel, got, ref, bound):
    """Ledger only, no gate: the worst error against another form of the bound."""
    got = got.detach().cpu().double().numpy() if torch.is_tensor(got) else np.asarray(got, dtype=np.float64)
    w = WORST.setdefault(kernel, [0.0, 0])
    w[0], w[1] = max(w[0], float((np.abs(got - ref) / bound).max())), w[1] + 1


def note(key, flag):
    """Record a yes / no observation (printed with the ledger): 'always', 'never' or 'mixed' over the cases seen."""
    s = NOTES.setdefault(key, set())
    s.add(bool(flag))
    NOTES[key] = s


def _np(t):
    return t.detach().cpu().numpy()


# ------------------------------------------------------------------------------------------------------------------ preprocess
# (rows, cols, H, W, B, ldk): the four grids; on 2 x 3 identity, upscale, non-integer and strong downscale, mixed (up in y, down in x); both batch sizes and
# every legal row pitch (588 = no padding, 592 = one fp16 chunk, 640 = the model's, 784 = the launcher's limit: all 196 pixels of a patch zero a column)
PRE_CASES = [(2, 3, 28, 42, 1, 640), (2, 3, 28, 42, 3, 588), (2, 3, 20, 30, 3, 592), (2, 3, 45, 61, 1, 784), (2, 3, 150, 200, 3, 640), (2, 3, 20, 61, 1, 592),
             (1, 1, 14, 14, 3, 784), (1, 1, 9, 23, 1, 588), (5, 4, 70, 56, 1, 592), (5, 4, 97, 33, 3, 640), (10, 12, 140, 168, 1, 588), (10, 12, 98, 126, 3, 784),
             (10, 12, 300, 500, 1, 640)]
_PRE_REF = {}


def _pre_image(i):
    rows, cols, Hh, Ww, B, _ = PRE_CASES[i]
    rng = np.random.default_rng(1000 + i)
    img = rng.random((B, 3, Hh, Ww)).astype(np.float32)
    img[:, :, : Hh // 2, Ww // 3:] *= 0.25                       # an edge in both directions: a shifted tap or row is not hidden by smooth content
    return img


def _pre_ref(i, rounded, aa):
    """Image and the float64 reference (NCHW, fp32 store) of one case: computed once, shared by the type combinations that read the same pixels."""
    key = (i, rounded, aa)
    if key not in _PRE_REF:
        rows, cols = PRE_CASES[i][:2]
        img = _pre_image(i)
        ref, bound = ER.preprocess(img, rows, cols, aa=bool(aa), round16=rounded)
        ref.setflags(write=False)
        bound.setflags(write=False)
        _PRE_REF[key] = (img, ref, bound)
    return _PRE_REF[key]


PRE_TYPES = [(0, 0, 0), (0, 1, 0), (1, 0, 0), (1, 1, 0), (0, 0, 1), (0, 1, 1)]          # (fp16 image, fp16 output, round16): the four instantiations + round16 on the fp32-input two


@pytest.mark.parametrize("aa", [1, 0])
@pytest.mark.parametrize("in16,out16,round16", PRE_TYPES)
def test_preprocess(H, in16, out16, round16, aa):
    """preprocess_kernel through launch_preprocess with ldk, nchw_out = 0, round16 and aa as model_encoder.hip passes them: the im2col scatter
    out[(b Np + py cols + px) ldk + c 196 + iy 14 + ix], the zeroing of the K padding columns [588, ldk), the f16 output, the f16 input, round16 and the
    two-tap aa = 0 branch.  The nchw_out = 1 form on the same inputs must agree with it bit for bit after un-patchifying."""
    kernel = f"preprocess<{'f16' if in16 else 'f32'},{'f16' if out16 else 'f32'}>{' round16' if round16 else ''} aa={aa}"
    for i, (rows, cols, Hh, Ww, B, ldk) in enumerate(PRE_CASES):
        img, ref, b32 = _pre_ref(i, bool(in16 or round16), aa)
        bound = b32 + (2.0 ** -11 * np.abs(ref) + 2.0 ** -25 if out16 else 0.0)
        what = f"B={B} ({Hh},{Ww})->{rows}x{cols} patches ldk={ldk}"
        timg = torch.from_numpy(img)
        got, _ = H.preprocess_ex(timg, rows, cols, torch.full((B * rows * cols, ldk), FILL), in16, out16, ldk, False, round16, aa)
        got = _np(got)
        assert (got[:, ER.PATCH_K:] == 0).all(), what + ": K padding columns [588, ldk) must be exactly 0"
        assert not (got == FILL).any(), what + ": an element kept the pre-fill"
        unp = ER.unpatchify(got, B, rows, cols)
        check(kernel, unp, ref, bound, what)
        nchw, _ = H.preprocess_ex(timg, rows, cols, torch.full((B, 3, 14 * rows, 14 * cols), FILL), in16, out16, ldk, True, round16, aa)
        assert np.array_equal(_np(nchw), unp), what + ": nchw_out = 1 and the un-patchified im2col form differ"
        if (Hh, Ww) == (14 * rows, 14 * cols) and not out16:
            r32 = ref.astype(np.float32)
            assert (np.abs(unp.astype(np.float64) - r32) <= TR.ulp32(r32)).all(), what + ": identity is within 1 ulp32 of f32((v - mean) / sd)"
            note(f"identity bit-equal to f32((v - mean) / sd) [{kernel}]", np.array_equal(unp, r32))


@pytest.mark.parametrize("ldk", [587, 785])
def test_preprocess_rejects_a_row_pitch_the_patch_cannot_zero(H, ldk):
    """ldk < 588 has no room for the patch; ldk - 588 > 196 has more padding columns than a patch has pixels to zero them."""
    for in16, out16 in ((0, 0), (0, 1), (1, 0), (1, 1)):
        rc = H.preprocess_ex(torch.zeros(1, 3, 28, 42), 2, 3, torch.zeros(6, ldk), in16, out16, ldk, raw=True)
        assert rc == INVALID


@pytest.mark.parametrize("out16", [0, 1])
@pytest.mark.parametrize("zero_n", [0, 1, 257, 5000])
def test_preprocess_counters(H, zero_n, out16):
    """The zeroing of the device-side counters (the fused LayerNorm finalize's row-block counters): [0, zero_n) comes back zero, the guard behind it
    untouched.  One image on the 2 x 3 grid launches 5 blocks = 1280 threads: zero_n = 5000 needs the grid stride.  The image result does not change."""
    rows, cols, Hh, Ww, _, ldk = PRE_CASES[3]
    img, ref, b32 = _pre_ref(3, False, 1)
    bound = b32 + (2.0 ** -11 * np.abs(ref) + 2.0 ** -25 if out16 else 0.0)
    guard = 64
    cnt = (torch.arange(zero_n + guard, dtype=torch.int32) * 7919 + 0x5A5A5A5).to(torch.int32)
    assert (cnt != 0).all()
    got, c = H.preprocess_ex(torch.from_numpy(img), rows, cols, torch.full((rows * cols, ldk), FILL), False, out16, ldk, counters=cnt, zero_n=zero_n)
    c = c.cpu()
    assert (c[:zero_n] == 0).all(), "counters [0, zero_n) must be zero"
    assert torch.equal(c[zero_n:], cnt[zero_n:]), "the guard past zero_n was written"
    got = _np(got)
    assert (got[:, ER.PATCH_K:] == 0).all() and not (got == FILL).any()
    check(f"preprocess<f32,{'f16' if out16 else 'f32'}> aa=1", ER.unpatchify(got, 1, rows, cols), ref, bound, f"zero_n={zero_n}")
    plain, none = H.preprocess_ex(torch.from_numpy(img), rows, cols, torch.full((rows * cols, ldk), FILL), False, out16, ldk)
    assert none is None and np.array_equal(_np(plain), got), "a null counter buffer must give the same image"


def test_preprocess_past_the_block_cap(H):
    """16 images of 64 x 64 -> 37 x 37 patches: 16 x 518 x 518 pixels = 16777 blocks of 256, over the launcher's cap of 16384: the pixel loop strides."""
    B, rows, cols, ldk = 16, 37, 37, 592
    img = np.random.default_rng(5).random((B, 3, 64, 64)).astype(np.float32)
    img[8:] *= 0.5
    ref, bound = ER.preprocess(img, rows, cols)
    assert (B * 518 * 518 + 255) // 256 > 16384
    got, _ = H.preprocess_ex(torch.from_numpy(img), rows, cols, torch.full((B * rows * cols, ldk), FILL), False, False, ldk)
    got = _np(got)
    assert (got[:, ER.PATCH_K:] == 0).all() and not (got == FILL).any()
    check("preprocess<f32,f32> aa=1", ER.unpatchify(got, B, rows, cols), ref, bound, "16 x (64,64) -> 37x37 patches")


# ------------------------------------------------------------------------------------------------------------------ position embedding
@pytest.mark.parametrize("size_mode", [0, 1])
@pytest.mark.parametrize("rows,cols", [(1, 1), (1, 37), (37, 1), (36, 38), (3, 70), (60, 60), (37, 37)])
def test_posembed(H, rows, cols, size_mode):
    """posembed_kernel through launch_posembed in both modes (size_mode = 1: onnx_compatible_mode, source scale 37 / n, never bypassed).  Row 0 is a
    copy in every case; 37 x 37 in plain mode is the bypass (bit-equal); in size mode the scale is exactly 1 and the weights 0, 1, 0, 0."""
    D = 128
    pos = (np.random.default_rng(37 * rows + cols).standard_normal((1 + 37 * 37, D)) * (0.5 + np.arange(D) / D)).astype(np.float32)
    ref, bound = ER.posembed(pos, rows, cols, bool(size_mode))
    got = _np(H.posembed_ex(torch.from_numpy(pos), rows, cols, size_mode))
    assert np.array_equal(got[0], pos[0]), "row 0 is pos[0]"
    if (rows, cols) == (37, 37) and not size_mode:
        assert np.array_equal(got, pos), "37 x 37 in plain mode is the bypass"
        return
    check(f"posembed size_mode={size_mode}", got[1:], ref[1:], bound[1:], f"{rows}x{cols}")
    record(f"posembed size_mode={size_mode} / three-part form", got[1:], ref[1:], ER.posembed(pos, rows, cols, bool(size_mode), weight_term=False)[1][1:])
    if (rows, cols) == (37, 37):
        note("posembed size mode 37 x 37 bit-equal to pos", np.array_equal(got, pos))


# ------------------------------------------------------------------------------------------------------------------ patch epilogue
PATCH_SHAPES = [(3, 1, 2), (2, 6, 8), (2, 130, 131), (1, 257, 258)]       # (B, Np, Ntok): patch 0 of image 1 at row 130, mid row tile; M = 3, 12, 260, 257; Ntok = Np + 2: a row nobody owns


def _patch_inputs(seed, M, N, K, Np, exact, prec):
    rng = np.random.default_rng(seed)
    kz = 588 if K == 640 else K                                   # K = 640: columns 588.. zero in A and in W, as the model has them
    A, W = np.zeros((M, K), dtype=np.float32), np.zeros((N, K), dtype=np.float32)
    if exact:
        lim = 2 if prec else 4                                    # partial sums below 2^24 (fp32) in any order; every input an fp16 number
        A[:, :kz] = rng.integers(-lim, lim + 1, (M, kz))
        W[:, :kz] = rng.integers(-lim, lim + 1, (N, kz))
        bias, cls = rng.integers(-64, 65, N) / 16.0, rng.integers(-64, 65, N) / 16.0
        pos = rng.integers(-64, 65, (1 + Np, N)) / 16.0
    else:
        A[:, :kz] = rng.standard_normal((M, kz)) * (0.5 + rng.random((M, 1)) * 2)
        W[:, :kz] = rng.standard_normal((N, kz)) / np.sqrt(kz)
        bias, cls, pos = rng.standard_normal(N) * 0.3, rng.standard_normal(N), rng.standard_normal((1 + Np, N))
    return A, W, bias.astype(np.float32), pos.astype(np.float32), cls.astype(np.float32)


@pytest.mark.parametrize("N", [128, 384])
@pytest.mark.parametrize("K", [640, 64])
@pytest.mark.parametrize("prec", [0, 1])
def test_patch_epilogue(H, prec, K, N):
    """EPI_PATCH through launch_gemm: row b Ntok + 1 + p of the fp32 residual stream = acc + bias + pos[1 + p]; the rows of patch 0 also write the image's
    cls row, complete across every column tile (N = 384: three), for every image, wherever patch 0 of image b falls inside a row tile; cls = null leaves
    the cls rows alone.  Exact inputs (small integers; bias, pos, cls multiples of 2^-4): the whole matrix is bit-equal to the reference."""
    for si, (B, Np, Ntok) in enumerate(PATCH_SHAPES):
        M = B * Np
        fill = np.full((B * Ntok, N), FILL)
        for exact in (False, True):
            A, W, bias, pos, cls = _patch_inputs(10 * si + K + N + exact, M, N, K, Np, exact, prec)
            for with_cls in (True, False):
                ref, e = ER.patch_embed(A, W, bias, pos, cls if with_cls else None, B, Np, Ntok, fill, prec)
                got = H.gemm_ex(H.TG_PATCH, torch.from_numpy(A), torch.from_numpy(W), torch.from_numpy(bias), prec, xres=torch.from_numpy(fill), Ntok=Ntok,
                                pos=torch.from_numpy(pos), cls=torch.from_numpy(cls) if with_cls else None, Np=Np)["xres"]
                got = _np(got).astype(np.float64)
                what = f"B={B} Np={Np} Ntok={Ntok} K={K} N={N} exact={exact} cls={with_cls}"
                own = e > 0
                assert np.array_equal(got[~own], ref[~own]), what + ": cls rows (f32(cls + pos[0]) or the pre-fill) and rows the epilogue does not own"
                if exact:
                    assert np.array_equal(got, ref), what + ": exact inputs must give a bit-equal matrix"
                else:
                    check(f"patch epilogue<{'f16' if prec else 'f32'}>", got[own], ref[own], e[own], what)


# ------------------------------------------------------------------------------------------------------------------ QKV, transposed V
def _ulp(x, prec):
    x = np.abs(x)
    return np.spacing(x.astype(np.float16)).astype(np.float64) if prec else TR.ulp32(x)


@pytest.mark.parametrize("prec,B,Ntok,nh", [(0, 1, 65, 2), (0, 2, 130, 3), (0, 1, 200, 2), (0, 1, 64, 2), (1, 2, 130, 3)])
def test_qkv_transposed_v(H, prec, B, Ntok, nh):
    """EPI_QKV with v_rowmajor = 0 through launch_gemm: V^T scatter (bh 64 + d) Npad + tok of the fp32 parity path (never the ping-pong kernel, which
    takes row-major V only: the fp16 case runs the latency kernel at any shape).  Integer inputs: k and v are bit-equal, q within 1 ulp of the storage
    type; the key padding [Ntok, Npad) keeps the pre-fill - the model zeroes it once with a memset.  Ntok = 64: no padding."""
    K, D = 128, nh * 64
    Npad = (Ntok + 63) // 64 * 64
    rng = np.random.default_rng(Ntok + nh)
    lim = 1 if prec else 3                                        # fp16: |acc + bias| <= 130 with 3 fraction bits is an fp16 number
    A = rng.integers(-lim, lim + 1, (B * Ntok, K)).astype(np.float32)
    W = rng.integers(-lim, lim + 1, (3 * D, K)).astype(np.float32)
    bias = (rng.integers(-16, 17, 3 * D) / 8.0).astype(np.float32)
    qs = 0.125 * 1.4426950408889634
    r = ER.qkv(A, W, bias, B, Ntok, nh, qs, prec)
    out = H.gemm_ex(H.TG_QKV, torch.from_numpy(A), torch.from_numpy(W), torch.from_numpy(bias), prec, nh=nh, Ntok=Ntok, qscale=qs,
                    v_prefill=torch.full((B, nh, 64, Npad), FILL))
    q, k, v = (_np(out[n]).astype(np.float64) for n in ("q", "k", "v"))
    assert v.shape == (B, nh, 64, Npad)
    assert np.array_equal(k, r["k"][0]), "k"
    assert np.array_equal(v[..., :Ntok], r["vT"][0]), "v^T"
    assert (v[..., Ntok:] == FILL).all(), "the key padding [Ntok, Npad) was written"
    assert (np.abs(q - r["q"][0]) <= _ulp(r["q"][0], prec)).all(), "q within 1 ulp of the storage type"
    # the row-major form of the same inputs is the transpose
    rm = H.gemm_ex(H.TG_QKV, torch.from_numpy(A), torch.from_numpy(W), torch.from_numpy(bias), prec, nh=nh, Ntok=Ntok, qscale=qs)
    assert np.array_equal(_np(rm["v"]).transpose(0, 1, 3, 2), v[..., :Ntok]) and np.array_equal(_np(rm["q"]), q)


# ------------------------------------------------------------------------------------------------------------------ ConvTranspose2d with uv inputs
@pytest.mark.parametrize("pixH,pixW", [(1, 1), (3, 5), (6, 9)])
@pytest.mark.parametrize("prec", [0, 1])
def test_convt_uv_at_the_input_pixel(H, prec, pixH, pixW):
    """EPI_CONVT with uv_in = 1 through launch_gemm (MoGe-1, v1.py:118-121): the uv planes are two more INPUT channels of the ConvTranspose2d, so the term
    is taken at the low-res pixel with weights per GEMM column n = (dy, dx, co).  The reference is conv_transpose2d of cat([x, uv]) with u, v from
    torch.linspace in fp32.  The opposite flag on the same inputs must give something else, or the switch is dead."""
    import torch.nn.functional as F
    B, Cin, Cout = 2, 128, 64
    g = torch.Generator().manual_seed(31 * pixH + pixW)
    x = torch.randn(B, pixH, pixW, Cin, generator=g)
    wt = torch.randn(Cin + 2, Cout, 2, 2, generator=g) / Cin ** 0.5
    wt[Cin:] *= 4                                                 # the uv channels carry weight
    bias = torch.randn(Cout, generator=g)
    rng = (-0.75, 0.81, -0.62, 0.55)
    Wg = wt.permute(2, 3, 1, 0).reshape(4 * Cout, Cin + 2).contiguous()          # row n = (dy 2 + dx) Cout + co
    A, Wk, b4, wu, wv = x.reshape(-1, Cin), Wg[:, :Cin].contiguous(), bias.repeat(4), Wg[:, Cin].contiguous(), Wg[:, Cin + 1].contiguous()
    ref, e = ER.convt_uv_in(A.numpy(), Wk.numpy(), b4.numpy(), wu.numpy(), wv.numpy(), rng, B, pixH, pixW, Cout, prec)
    if prec == 0:                                                 # the definition itself, in float64 with torch.linspace in fp32
        u32, v32 = torch.linspace(rng[0], rng[1], pixW), torch.linspace(rng[2], rng[3], pixH)
        uv = torch.stack(torch.meshgrid(u32.double(), v32.double(), indexing="xy"), 0)[None].expand(B, 2, pixH, pixW)
        want = F.conv_transpose2d(torch.cat([x.double().permute(0, 3, 1, 2), uv], 1), wt.double(), bias.double(), stride=2).permute(0, 2, 3, 1).numpy()
        np.testing.assert_allclose(ref, want, rtol=1e-12, atol=1e-12)
    got = H.gemm_ex(H.TG_CONVT, A, Wk, b4, prec, uv=(wu, wv) + rng, pix=(pixW, pixH), Cout=Cout, uv_in=True)["out"].reshape(B, 2 * pixH, 2 * pixW, Cout)
    check(f"convt uv_in<{'f16' if prec else 'f32'}>", got, ref, e, f"{pixH}x{pixW}")
    other = H.gemm_ex(H.TG_CONVT, A, Wk, b4, prec, uv=(wu, wv) + rng, pix=(pixW, pixH), Cout=Cout, uv_in=False)["out"].reshape(B, 2 * pixH, 2 * pixW, Cout)
    assert float((other - got).abs().max()) > 1e-2, "uv_in does not change the result"


# ------------------------------------------------------------------------------------------------------------------ MoGe-1 input resize
# the scale pairs of tests/test_hip_kernels.py::test_resize_bicubic_antialiased (98x126 -> 153x197, 140x150 -> 87x93, 518x518 -> 700x700, 300x500 -> 120x640),
# each cut to a 40-pixel image: the same up / down / mixed ratios on a 40 x 40 input
BICUBIC_SHAPES = [(62, 63), (25, 25), (54, 54), (16, 51)]


@pytest.mark.parametrize("OH,OW", BICUBIC_SHAPES)
def test_resize_bicubic_aa_f16_and_round16(H, OH, OW):
    """resize_bicubic_aa_kernel<f16> and the round16 form of both instantiations through launch_resize_bicubic_aa (v1.py:275 of a .half() model: the image
    is rounded to fp16 on load and the resized image on store).  round16 on an fp32 image equals the <f16> path fed the rounded image, bit for bit."""
    img = np.random.default_rng(OH).random((2, 3, 40, 40)).astype(np.float32)
    img[:, :, :17, 23:] *= 0.25
    t = torch.from_numpy(img)
    ref, e = ER.resize_bicubic_aa(img, OH, OW, in_fp16=True)
    got16 = H.resize_bicubic_aa_ex(t, OH, OW, in_fp16=True)
    check("resize_bicubic_aa<f16>", got16, ref, e, f"40x40 -> {OH}x{OW}")
    record("resize_bicubic_aa<f16> / three-part form", got16, ref, ER.resize_bicubic_aa(img, OH, OW, in_fp16=True, weight_term=False)[1])
    ref16, e16 = ER.resize_bicubic_aa(img, OH, OW, round16=True)
    a = H.resize_bicubic_aa_ex(t, OH, OW, in_fp16=False, round16=True)
    b = H.resize_bicubic_aa_ex(t.half().float(), OH, OW, in_fp16=True, round16=True)
    check("resize_bicubic_aa round16", a, ref16, e16, f"40x40 -> {OH}x{OW}")
    assert torch.equal(a, b), "round16 on the fp32 image and the <f16> kernel on the rounded image differ"
    assert torch.equal(a, a.half().float()), "round16 stores fp16 numbers"
    ref32, e32 = ER.resize_bicubic_aa(img, OH, OW)
    got32 = H.resize_bicubic_aa_ex(t, OH, OW)
    check("resize_bicubic_aa<f32>", got32, ref32, e32, f"40x40 -> {OH}x{OW}")
    record("resize_bicubic_aa<f32> / three-part form", got32, ref32, ER.resize_bicubic_aa(img, OH, OW, weight_term=False)[1])


# ------------------------------------------------------------------------------------------------------------------ rejected arguments
def test_gemm_entry_point_rejects_inconsistent_shapes(H):
    """The new kinds of moge_test_gemm_ex refuse what would index outside their buffers, before any launch."""
    t = torch.zeros
    kw = dict(xres=t(2 * 7, 128), pos=t(7, 128), raw=True)
    assert H.gemm_ex(H.TG_PATCH, t(12, 64), t(128, 64), t(128), 0, Np=6, Ntok=6, **kw) == INVALID          # Ntok < 1 + Np
    assert H.gemm_ex(H.TG_PATCH, t(13, 64), t(128, 64), t(128), 0, Np=6, Ntok=7, **kw) == INVALID          # M is no multiple of Np
    assert H.gemm_ex(H.TG_PATCH, t(12, 64), t(128, 64), t(128), 0, Np=0, Ntok=7, **kw) == INVALID
    assert H.gemm_ex(H.TG_PATCH, t(12, 64), t(128, 64), t(128), 0, Np=6, Ntok=7, xres=t(14, 128), pos=None, raw=True) == INVALID
    assert H.gemm_ex(H.TG_PATCH, t(12, 64), t(128, 64), t(128), 0, Np=6, Ntok=7, **kw) == 0
    assert H.gemm_ex(H.TG_CONVT, t(15, 64), t(256, 64), t(256), 0, pix=(5, 3), Cout=32, raw=True) == INVALID      # N != 4 Cout
    assert H.gemm_ex(H.TG_CONVT, t(14, 64), t(256, 64), t(256), 0, pix=(5, 3), Cout=64, raw=True) == INVALID      # M is no multiple of pixH pixW
    assert H.gemm_ex(H.TG_CONVT, t(15, 64), t(8, 64), t(8), 0, pix=(5, 3), Cout=2, raw=True) == INVALID           # Cout % 4
    assert H.gemm_ex(H.TG_CONVT, t(15, 64), t(256, 64), t(256), 0, pix=(5, 3), Cout=64, raw=True) == 0
    assert H.preprocess_ex(t(1, 3, 28, 42), 2, 3, t(6, 640), in_fp16=True, round16=True, raw=True) == INVALID       # round16 is for an fp32 image
