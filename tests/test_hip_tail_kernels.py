"""Per-kernel tests of the inference tail against the float64 references of tests/tail_reference.py (derivation of every bound: that module's
docstring; the references themselves are checked on the CPU in tests/test_tail_reference_cpu.py).  The gate is element-wise,
|got - ref| <= bound(element); where the operation is exact (u8 ingest, fp16 copies, padding, untouched columns, masks, INF fills) equality.

Worst observed error / bound per kernel, measured on an MI355X (271 passed, 13 s for the module; `pytest -s` prints the table of the run at hand):
  head_final<f32> 0.247   head_final<f16> 0.202   head_final32 0.078   head_final_k3<f32> 0.024   head_final_k3<f16> 0.030   head_final_dot 0.303
  mlp_layer 0.161   ln_raw 0.122   ln_finalize 0.282   fold_ln (c, bf) 0.036   resize_bilinear_uv<f32> 0.396   resize_bilinear_uv<f16> 0.990
  layernorm[f32] 0.188 (tap 0.148)   layernorm[f16] 0.9955 (tap 0.9943)   layernorm[x16] 0.9952 (tap 0.9937)   finalize 0 of 2 ulp
The 0.99 figures are the fp16 outputs: their bound is the fp32 bound + HALF an fp16 ulp of the result, which a round-to-nearest store all but reaches
somewhere in 10^7 elements; the fp32 part is used to 0.19 / 0.40.  The 0.02 - 0.08 figures are bounds that admit a long sequential sum (9 C terms of the
3x3 head, 32 of the quad kernel, depth 22 in fold_ln) where the kernel's errors cancel like sqrt(n).  EXPERIMENTS.md R7.2 has the table with cases and
bounds, and the four one-line kernel mutations (w01 / w10 swapped, quad-lane weight offset, coloff dropped, unrounded fold sum) with the cases that
caught each."""
import ctypes

import numpy as np
import pytest
import torch

import tail_fixtures as TF
import tail_reference as TR

pytestmark = pytest.mark.gpu

WORST = {}
INVALID = -1


@pytest.fixture(scope="module")
def H():
    import hip_util
    yield hip_util
    print("\nworst error / bound per kernel:")
    for k in sorted(WORST):
        print(f"  {k:28s} {WORST[k][0]:8.4f}   ({WORST[k][1]} cases)")


def check(kernel, got, ref, bound, what):
    got = got.detach().cpu().double().numpy() if torch.is_tensor(got) else np.asarray(got, dtype=np.float64)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert np.isfinite(got).all(), what
    ratio = np.abs(got - ref) / bound
    worst = float(ratio.max())
    w = WORST.setdefault(kernel, [0.0, 0])
    w[0], w[1] = max(w[0], worst), w[1] + 1
    assert worst <= 1.0, f"{kernel} {what}: error / bound = {worst:.3f} at {np.unravel_index(ratio.argmax(), ratio.shape)}"


# ------------------------------------------------------------------------------------------------------------------ head_final
LD_N4 = [(0, None), (0, "above"), (0, "below"), (1, None), (1, "above"), (1, "below")]      # (ld > C with a channel offset, n4 placement)


@pytest.mark.parametrize("kind,remap", TF.ACTS)
@pytest.mark.parametrize("prec,C", [(0, 4), (0, 32), (0, 64), (1, 8), (1, 32), (1, 64)])
def test_head_final(H, prec, C, kind, remap):
    """fp16 with C == 32 is head_final32_kernel (four lanes per pixel), the rest head_final_kernel.  Pixel counts 1 (one quad in a wave), 15 (< 16),
    45 ... 429 (no multiple of 64: partly idle waves in the quad shuffle), more than one block (3 x 13 x 11)."""
    kernel = "head_final32" if (prec, C) == (1, 32) else f"head_final<{'f16' if prec else 'f32'}>"
    for i, ((Hd, Wd), (Ho, Wo)) in enumerate(TF.HEAD_SHAPES):
        for j, (wide, n4) in enumerate(LD_N4):
            B = 1 if (i + j) % 2 == 0 else 3
            ld, choff = (C + 16, 8) if wide else (C, 0)
            d = TF.head_inputs(100 * i + j, B, Hd, Wd, C, ld, choff, kind, prec, n4 is not None, 1, Ho, Wo)
            ref, bound, pre = TR.head_final(d["xs"], d["w"], d["bias"], Ho, Wo, kind, remap, d["n4s"], d["w2"])
            assert np.abs(pre).max() < 4
            n4t = None if n4 is None else torch.from_numpy(d["n4"])
            got = H.head_final(prec, kind, torch.from_numpy(d["x"]), torch.from_numpy(d["w"]), torch.from_numpy(d["bias"]), Ho, Wo, remap, 1, C, choff,
                               n4t, None if n4 is None else torch.from_numpy(d["w2"]), n4 == "below")
            check(kernel, got, ref, bound, f"B={B} ({Hd},{Wd})->({Ho},{Wo}) C={C} ld={ld} choff={choff} n4={n4} kind={kind} remap={remap}")


K3_SHAPES = [((5, 7), (5, 7)), ((4, 4), (13, 11)), ((16, 16), (5, 9)), ((1, 6), (4, 17)), ((5, 1), (9, 4)), ((1, 1), (3, 3))]


@pytest.mark.parametrize("kind,remap", [(0, 0), (0, 2), (0, 3), (3, 0)])
@pytest.mark.parametrize("prec,C", [(0, 8), (0, 64), (1, 8), (1, 64)])
def test_head_final_k3(H, prec, C, kind, remap):
    """3x3 last conv (weights (CO,C,3,3), asymmetric in (dy,dx)); Hd or Wd == 1: every tap of that axis clamps."""
    for i, ((Hd, Wd), (Ho, Wo)) in enumerate(K3_SHAPES):
        B = 1 + 2 * (i % 2)
        d = TF.head_inputs(7 + i, B, Hd, Wd, C, C, 0, kind, prec, False, 3, Ho, Wo)
        ref, bound, pre = TR.head_final(d["xs"], d["w"], d["bias"], Ho, Wo, kind, remap)
        assert np.abs(pre).max() < 4
        got = H.head_final(prec, kind, torch.from_numpy(d["x"]), torch.from_numpy(d["w"]), torch.from_numpy(d["bias"]), Ho, Wo, remap, 3)
        check(f"head_final_k3<{'f16' if prec else 'f32'}>", got, ref, bound, f"B={B} ({Hd},{Wd})->({Ho},{Wo}) C={C} kind={kind} remap={remap}")


@pytest.mark.parametrize("kind,remap", TF.ACTS)
@pytest.mark.parametrize("zld,zoff", [(0, 0), (4, 0), (12, 0), (12, 4), (12, 8)])
def test_head_final_dot(H, kind, remap, zld, zoff):
    """Lane 3 of the 4-float tap holds a large finite value: the 3-channel kinds must ignore it; so do the other groups of z."""
    rng = np.random.default_rng(10 * zld + zoff)
    CO = 3 if kind in (0, 1) else 1
    bias = np.array([0.3, -0.2, 0.5, 77.0], dtype=np.float32)
    for i, ((Hd, Wd), (Ho, Wo)) in enumerate(TF.HEAD_SHAPES):
        B = 1 + 2 * (i % 2)
        y = (rng.standard_normal((B, Hd, Wd, 4)) * [0.4, 0.6, 0.8, 1.0]).astype(np.float32)
        y[..., CO:] = 3.0e4
        z = None
        if zld:
            z = np.full((B, Hd, Wd, zld), -2.0e4, dtype=np.float32)
            z[..., zoff:zoff + CO] = (rng.standard_normal((B, Hd, Wd, CO)) * [0.7, 0.5, 0.3][:CO]).astype(np.float32)
        ref, bound, pre = TR.head_final_dot(y, z, zoff, bias, Ho, Wo, kind, remap)
        assert np.abs(pre).max() < 4
        got = H.head_final_dot(kind, torch.from_numpy(y), torch.from_numpy(bias), Ho, Wo, remap, None if z is None else torch.from_numpy(z), zoff)
        check("head_final_dot", got, ref, bound, f"B={B} ({Hd},{Wd})->({Ho},{Wo}) kind={kind} remap={remap} zld={zld} zoff={zoff}")


@pytest.mark.parametrize("act", [0, 1, 2])
@pytest.mark.parametrize("K", [4, 252, 256, 260, 384, 1024])
def test_mlp_layer(H, K, act):
    rng = np.random.default_rng(K)
    for B in (1, 3):
        for N in (1, 3, 5):                         # B N = 1, 3, 5, 9, 15: no multiple of the 4 waves of a block
            x = (rng.standard_normal((B, K)) * (0.5 + np.arange(K) / K)).astype(np.float32)
            W = (rng.standard_normal((N, K)) * 0.5 * (1 + np.arange(N))[:, None] / np.sqrt(K)).astype(np.float32)
            b = rng.standard_normal(N).astype(np.float32) * 0.3
            ref, bound = TR.mlp_layer(x, W, b, act)
            got = H.mlp_layer(torch.from_numpy(x), torch.from_numpy(W), torch.from_numpy(b), act)
            check("mlp_layer", got, ref, bound, f"B={B} K={K} N={N} act={act}")


# ------------------------------------------------------------------------------------------------------------------ LayerNorm
def _ln_rows(rng, rows, D):
    x = (rng.standard_normal((rows, D)) * (0.5 + rng.random((rows, 1)) * 2) + rng.standard_normal((rows, 1))).astype(np.float32)
    x[rows // 2] = (50 + 0.1 * rng.standard_normal(D)).astype(np.float32)          # mean >> spread: a one-pass variance fails here
    w = (1 + 0.3 * rng.standard_normal(D)).astype(np.float32)
    b = (0.2 * rng.standard_normal(D)).astype(np.float32)
    return x, w, b


FILL = 123.0        # exact in fp16 and fp32
_LN_REF = {}


def _ln_plain_ref(rows, D, s16):
    """Inputs and the float64 reference of one (rows, D): computed once, shared by the storage modes that read the same stream, left unchanged."""
    key = (rows, D, s16)
    if key not in _LN_REF:
        x, w, b = _ln_rows(np.random.default_rng(rows + D), rows, D)
        r = TR.layernorm(TR.to_storage(x, 1) if s16 else x, w, b)
        for v in (r["y"], r["e_y"]):
            v.setflags(write=False)
        if rows > 16384:
            _LN_REF.clear()                          # one big reference at a time
        _LN_REF[key] = (x, w, b, r["y"], r["e_y"])
    return _LN_REF[key]


# one list, (rows, D) outermost: the two modes that read the fp32 stream run back to back on one reference, whatever order stacked marks would give
@pytest.mark.parametrize("rows,D,mode", [(r, d, m) for r in (1, 5, 777, 16385, 16389) for d in (128, 384, 640, 1024)
                                         for m in ("f32", "f16", "x16")])          # fp32 stream -> fp32 / fp16 output; fp16 stream -> fp16 output
def test_layernorm_plain(H, rows, D, mode):
    """rows > 16384: four rows per wave with a ragged last wave.  ldo > D and coloff > 0: the columns outside [coloff, coloff + D) keep their fill."""
    prec, s16 = (0, False) if mode == "f32" else (1, mode == "x16")
    x, w, b, y_ref, e32 = _ln_plain_ref(rows, D, s16)
    r = dict(y=y_ref, e_y=e32 + (2.0 ** -11 * np.abs(y_ref) + 2.0 ** -25 if prec else 0.0))          # fp16 storage: + half an ulp
    for ldo, coloff in ((D, 0), (D + 24, 8)):
        y, _ = H.layernorm_ex(prec, torch.from_numpy(x), torch.from_numpy(w), torch.from_numpy(b), torch.full((rows, ldo), FILL), s16, coloff)
        y = y.cpu().numpy()
        check(f"layernorm[{mode}]", y[:, coloff:coloff + D], r["y"], r["e_y"], f"rows={rows} D={D} ldo={ldo} coloff={coloff}")
        assert (y[:, :coloff] == FILL).all() and (y[:, coloff + D:] == FILL).all(), "columns outside [coloff, coloff + D) were written"


@pytest.mark.parametrize("mode", ["f32", "f16", "x16"])
@pytest.mark.parametrize("B,Ntok", [(3, 2), (5, 17), (1000, 17)])
def test_layernorm_tap(H, B, Ntok, mode):
    """Tap mode: token 0 -> cls_out (fp32) or nowhere, token t > 0 -> row b (Ntok - 1) + t - 1 at coloff.  17000 rows: the four-rows-per-wave form,
    where a null cls_out skips a row in the MIDDLE of a wave's four."""
    D, ldo, coloff = 384, 2 * 384 + 8, 384
    rows = B * Ntok
    rng = np.random.default_rng(rows)
    x, w, b = _ln_rows(rng, rows, D)
    prec, s16 = (0, False) if mode == "f32" else (1, mode == "x16")
    r = TR.layernorm(TR.to_storage(x, 1) if s16 else x, w, b, out_fp16=bool(prec))
    r32 = TR.layernorm(TR.to_storage(x, 1) if s16 else x, w, b)                    # cls_out is fp32 in every mode
    tok = np.arange(rows) % Ntok
    for with_cls in (True, False):
        y, cls = H.layernorm_ex(prec, torch.from_numpy(x), torch.from_numpy(w), torch.from_numpy(b), torch.full((B * (Ntok - 1), ldo), FILL), s16, coloff, True, Ntok,
                                torch.full((B, D), FILL) if with_cls else None)
        y = y.cpu().numpy()
        check(f"layernorm[{mode}] tap", y[:, coloff:coloff + D], r["y"][tok > 0], r["e_y"][tok > 0], f"B={B} Ntok={Ntok} cls={with_cls}")
        assert (y[:, :coloff] == FILL).all() and (y[:, coloff + D:] == FILL).all()
        if with_cls:
            check(f"layernorm[{mode}] tap", cls, r32["y"][tok == 0], r32["e_y"][tok == 0], f"B={B} Ntok={Ntok} cls_out")


@pytest.mark.parametrize("D", [128, 384, 640, 1024])
@pytest.mark.parametrize("rows", [1, 6, 4099])
def test_ln_raw(H, rows, D):
    rng = np.random.default_rng(rows * D)
    x, w, b = _ln_rows(rng, rows, D)
    x16, mr = H.ln_raw(torch.from_numpy(x))
    assert torch.equal(x16.cpu(), torch.from_numpy(x).half().float()), "fp16 copy"
    r = TR.layernorm(x, w, b)
    check("ln_raw", mr[:, 0], r["mean"], r["e_mean"], f"rows={rows} D={D} mean")
    check("ln_raw", mr[:, 1], r["rstd"], r["e_rstd"], f"rows={rows} D={D} rstd")


@pytest.mark.parametrize("NP", [4, 12, 24, 32])
@pytest.mark.parametrize("rows", [1, 7, 33, 4099])
def test_ln_finalize(H, rows, NP):
    """Partials as the RESID epilogue leaves them: fp32 (sum, sum of squares) of every 32-column group of real rows; row 0 constant (the variance
    clamps at 0, rstd = 1 / sqrt(1e-6) - 0.5 keeps every partial exact), the middle row with a large mean."""
    D = 32 * NP
    rng = np.random.default_rng(rows + NP)
    x, _, _ = _ln_rows(rng, rows, D)
    x[0] = 0.5
    g = x.reshape(rows, NP, 32)
    part = np.stack([g.sum(-1, dtype=np.float32), (g * g).sum(-1, dtype=np.float32)], -1).astype(np.float32)
    mean, e_mean, rstd, e_rstd = TR.ln_finalize(part, D)
    assert rstd[0] == 1.0 / np.sqrt(1e-6)
    mr = H.ln_finalize(torch.from_numpy(part), D)
    check("ln_finalize", mr[:, 0], mean, e_mean, f"rows={rows} NP={NP} mean")
    check("ln_finalize", mr[:, 1], rstd, e_rstd, f"rows={rows} NP={NP} rstd")


@pytest.mark.parametrize("N,K", [(1, 4), (5, 72), (3, 256), (7, 384), (2, 1024)])
def test_fold_ln(H, N, K):
    rng = np.random.default_rng(K)
    W = (rng.standard_normal((N, K)) * (1 + np.arange(N))[:, None]).astype(np.float32)
    g, beta, b = (1 + 0.3 * rng.standard_normal(K)).astype(np.float32), (0.3 * rng.standard_normal(K)).astype(np.float32), rng.standard_normal(N).astype(np.float32)
    Wf, c, bf = H.fold_ln(*(torch.from_numpy(v) for v in (W, g, beta, b)))
    rWf, rc, e_c, rbf, e_bf = TR.fold_ln(W, g, beta, b)
    Wf = Wf.cpu().double().numpy()
    assert np.array_equal(Wf, rWf), "Wf = fp16(fp32(g w))"
    check("fold_ln", c, Wf.sum(-1), e_c, f"N={N} K={K} c = sum of the RETURNED (rounded) Wf")
    check("fold_ln", bf, rbf, e_bf, f"N={N} K={K} bf")


# ------------------------------------------------------------------------------------------------------------------ MoGe-1 resize, ingest
@pytest.mark.parametrize("prec,C", [(0, 4), (0, 12), (1, 8), (1, 16)])
@pytest.mark.parametrize("pad_chunks", [1, 2])
def test_resize_bilinear_uv(H, prec, C, pad_chunks):
    from oracle import moge_oracle as O
    CH = 8 if prec else 4
    Cp = C + pad_chunks * CH                                  # two chunks: the second one is all zero
    rng = np.random.default_rng(C + pad_chunks)
    for i, ((hs, ws), (OH, OW)) in enumerate([((4, 4), (13, 11)), ((16, 16), (5, 9)), ((5, 7), (5, 7)), ((1, 6), (4, 17)), ((3, 1), (2, 7)), ((1, 1), (1, 1))]):
        B = 1 + (i % 2)
        x = (rng.standard_normal((B, hs, ws, C)) * (0.5 + np.arange(C) / C)).astype(np.float32)
        uv = O.view_plane_uv(OW, OH).numpy().astype(np.float64)
        rng_uv = (float(uv[0, 0, 0]), float(uv[0, -1, 0]), float(uv[0, 0, 1]), float(uv[-1, 0, 1]))
        got = H.resize_bilinear_uv(prec, torch.from_numpy(x), OH, OW, Cp, rng_uv).cpu().double().numpy()
        ref, bound = TR.resize_bilinear_uv(TR.to_storage(x, prec), OH, OW, out_fp16=bool(prec))
        what = f"B={B} ({hs},{ws})->({OH},{OW}) C={C} Cp={Cp}"
        check(f"resize_bilinear_uv<{'f16' if prec else 'f32'}>", got[..., :C], ref, bound, what)
        e_uv = 3 * TR.ulp32(max(abs(v) for v in rng_uv)) + ((2.0 ** -11) * np.abs(uv) + 2.0 ** -25 if prec else 0.0)
        check(f"resize_bilinear_uv<{'f16' if prec else 'f32'}>", got[..., C:C + 2], np.broadcast_to(uv, (B, OH, OW, 2)), np.broadcast_to(e_uv + np.zeros_like(uv), (B, OH, OW, 2)), what + " uv")
        assert (got[..., C + 2:] == 0).all(), what + " padding"


def test_u8_ingest_is_bit_exact(H):
    img = np.random.default_rng(0).integers(0, 256, (2, 7, 37, 3), dtype=np.uint8)
    for c in range(3):
        img.reshape(-1, 3)[:256, c] = np.roll(np.arange(256, dtype=np.uint8), 85 * c)          # every byte value in every channel
    assert all(len(np.unique(img[..., c])) == 256 for c in range(3))
    ref = torch.from_numpy(TR.u8_ingest(img))
    assert torch.equal(H.u8_ingest(0, torch.from_numpy(img)).cpu(), ref)
    assert torch.equal(H.u8_ingest(1, torch.from_numpy(img)).cpu(), ref.half().float())


# ------------------------------------------------------------------------------------------------------------------ moge_postprocess
@pytest.fixture(scope="module")
def handles():
    """A MoGe-2 and a MoGe-1 handle (no weights: moge_postprocess reads none) - both values of the v1 flag and of the mask threshold."""
    from moge_amd.model import import_model_class_by_version
    from oracle import moge_oracle as O
    from oracle import moge_oracle_v1 as O1
    m2 = import_model_class_by_version("v2")(**O.named_configs()["tiny-vits-normal"]).to("cuda")
    m1 = import_model_class_by_version("v1")(**{**O1.named_configs()["tiny-v1-vits"], "mask_threshold": 0.3}).to("cuda")
    yield {False: (m2, 0.5), True: (m1, 0.3)}
    m2._release(); m1._release()


def _postprocess(model, s, fov, flags, normal, metric, alias=False):
    from moge_amd import _lib as L
    B, Hh, Ww, _ = s["points"].shape
    dev = lambda t: None if t is None else t.to("cuda", torch.float32).contiguous()        # noqa: E731
    pin, nin, mp, met, fv = dev(s["points"]), dev(normal), dev(s["mask_prob"]), dev(metric), dev(fov)
    o = dict(points=pin if alias else torch.empty_like(pin), depth=torch.empty(B, Hh, Ww, device="cuda"), normal=None if nin is None else torch.empty_like(nin),
             mask=torch.zeros(B, Hh, Ww, device="cuda", dtype=torch.uint8), intrinsics=torch.empty(B, 3, 3, device="cuda"), focal=torch.empty(B, device="cuda"),
             shift=torch.empty(B, device="cuda"))
    out = L.Outputs()
    for k, v in o.items():
        setattr(out, k, None if v is None else v.data_ptr())
    p = lambda t: None if t is None else t.data_ptr()                                      # noqa: E731
    L.check(L.lib.moge_postprocess(model._handle, p(pin), p(nin), p(mp), p(met), B, Hh, Ww, p(fv), flags, ctypes.byref(out), L.stream_ptr()))
    L.check(L.lib.moge_sync(model._handle, L.stream_ptr()))
    return {k: (None if v is None else v.cpu()) for k, v in o.items()}


def _ulps(a, b):
    return np.abs(a.astype(np.float64) - b.astype(np.float64)) / np.spacing(np.abs(b)).astype(np.float64)


@pytest.mark.parametrize("flags", [0, 1, 2, 3])
@pytest.mark.parametrize("use_fov", [False, True])
@pytest.mark.parametrize("size", [(70, 90), (64, 64), (33, 129)])
@pytest.mark.parametrize("v1", [False, True])
def test_postprocess(handles, v1, size, use_fov, flags):
    from oracle import moge_oracle as O
    model, thr = handles[v1]
    B, (Hh, Ww) = 2, size
    s = TF.pinhole_scene(B, Hh, Ww, thr=thr)
    fov = s["fov"] if use_fov else None
    # normal and metric given / null, independently of each other (MoGe-1 has neither): every pairing occurs over the (flags, fov, size) grid
    pick = flags + 2 * use_fov + size[0] % 3
    normal = s["normal"] if not v1 and pick % 2 == 0 else None
    metric = s["metric"] if not v1 and (pick // 2) % 2 == 0 else None
    ref = TR.postprocess(s["points"], normal, s["mask_prob"], metric, fov, flags, v1, thr)
    # conditions on the INPUTS, checked on the reference before the GPU is touched: no pixel is excluded below
    assert (torch.abs(s["mask_prob"] - thr) >= 0.05).all()
    assert (torch.abs(s["points"][..., 2] + ref["shift"][:, None, None]) >= 1e-3).all()
    got = _postprocess(model, s, fov, flags, normal, metric)
    np.testing.assert_allclose(got["shift"].numpy(), ref["shift"].numpy(), rtol=1e-4, atol=1e-6)
    np.testing.assert_allclose(got["focal"].numpy(), ref["focal"].numpy(), rtol=1e-4)
    np.testing.assert_allclose(got["intrinsics"].numpy(), ref["intrinsics"].numpy(), rtol=1e-4)
    a = Ww / Hh
    K = O._intrinsics(got["focal"] / 2 * (1 + a ** 2) ** 0.5 / a, got["focal"] / 2 * (1 + a ** 2) ** 0.5).numpy()
    gi = got["intrinsics"].numpy()
    assert ((K == 0) == (gi == 0)).all() and _ulps(gi[K != 0], K[K != 0]).max() <= 2, "intrinsics of the returned focal"
    f = TR.finalize_f32(s["points"].numpy(), None if normal is None else normal.numpy(), s["mask_prob"].numpy(), None if metric is None else metric.numpy(),
                        got["shift"].numpy(), gi, flags, v1, thr)
    assert np.array_equal(got["mask"].numpy().astype(bool), f["mask"]) and set(np.unique(got["mask"].numpy())) <= {0, 1}, "mask byte"
    assert np.array_equal(f["mask"], ref["mask"].numpy())
    for k in ("points", "depth") + (("normal",) if normal is not None else ()):
        g, r = got[k].numpy(), f[k]
        assert np.array_equal(np.isinf(g), np.isinf(r)) and (g[np.isinf(r)] == np.inf).all(), k + " INF fill"
        fin = np.isfinite(r)
        if k == "normal":
            assert np.array_equal(g, r), "normal: a copy with exact zeros outside the mask"
        else:
            worst = float(_ulps(g[fin], r[fin]).max())
            WORST.setdefault("finalize (ulp / 2)", [0.0, 0])
            WORST["finalize (ulp / 2)"] = [max(WORST["finalize (ulp / 2)"][0], worst / 2), WORST["finalize (ulp / 2)"][1] + 1]
            assert worst <= 2, f"{k}: {worst} ulp"
    if flags & 1:
        alias = _postprocess(model, s, fov, flags, normal, metric, alias=True)          # points_out aliasing points_in
        assert torch.equal(alias["points"], got["points"]) and torch.equal(alias["depth"], got["depth"])


# ------------------------------------------------------------------------------------------------------------------ rejected arguments
def test_entry_points_reject_what_their_launchers_reject(H, handles):
    from moge_amd import _lib as L
    t = torch.zeros
    x8 = t(1, 2, 2, 8)
    assert H.head_final(1, 0, t(1, 2, 2, 12), t(3, 12), t(3), 4, 4, raw=True) == INVALID                   # fp16: C % 8
    assert H.head_final(0, 0, t(1, 2, 2, 72), t(3, 72), t(3), 4, 4, raw=True) == INVALID                   # C > 64
    assert H.head_final(1, 0, t(1, 2, 2, 16), t(3, 8), t(3), 4, 4, C=8, choff=4, raw=True) == INVALID      # slice not on a 16-byte chunk
    assert H.head_final(0, 1, x8, t(3, 8, 3, 3), t(3), 4, 4, ksize=3, raw=True) == INVALID                 # the 3x3 form has no normal / sigmoid kind
    assert H.head_final(0, 4, x8, t(3, 8), t(3), 4, 4, raw=True) == INVALID
    assert L.lib.moge_test_head_final(None, H.st()) == INVALID
    assert H.head_final_dot(0, t(1, 2, 2, 4), t(4), 4, 4, z=t(1, 2, 2, 6), raw=True) == INVALID            # zld % 4
    assert H.head_final_dot(0, t(1, 2, 2, 4), t(4), 4, 4, z=t(1, 2, 2, 8), zoff=8, raw=True) == INVALID
    assert H.mlp_layer(t(1, 6), t(2, 6), t(2), 0, raw=True) == INVALID                                     # K % 4
    assert H.layernorm_ex(0, t(2, 1028), t(1028), t(1028), t(2, 1028), raw=True) == INVALID                # D > 1024
    assert H.layernorm_ex(0, t(2, 128), t(128), t(128), t(2, 136), coloff=6, raw=True) == INVALID          # coloff % 4 (ldo is aligned)
    assert H.layernorm_ex(0, t(2, 128), t(128), t(128), t(2, 134), coloff=4, raw=True) == INVALID          # ldo % 4
    assert H.layernorm_ex(0, t(2, 128), t(128), t(128), t(2, 128), stream16=True, raw=True) == INVALID     # the fp16 stream writes fp16
    assert H.layernorm_ex(0, t(5, 128), t(128), t(128), t(4, 128), tap_mode=True, Ntok=2, raw=True) == INVALID
    assert H.ln_raw(t(2, 1028), raw=True) == INVALID
    assert H.ln_finalize(t(2, 3, 2), 96, raw=True) == INVALID                                              # odd NP
    assert H.resize_bilinear_uv(1, t(1, 2, 2, 4), 4, 4, 16, (0, 1, 0, 1), raw=True) == INVALID             # fp16: C % 8
    assert H.resize_bilinear_uv(0, t(1, 2, 2, 4), 4, 4, 4, (0, 1, 0, 1), raw=True) == INVALID              # no room for uv
    assert L.lib.moge_test_fold_ln(None, None, None, None, None, None, None, 1, 4, H.st()) == INVALID
    assert L.lib.moge_test_u8_ingest(0, None, None, 1, 2, 2, H.st()) == INVALID
    model, _ = handles[False]
    out = L.Outputs()
    p = torch.zeros(1, 4, 4, 3, device="cuda")
    assert L.lib.moge_postprocess(None, p.data_ptr(), None, None, None, 1, 4, 4, None, 0, ctypes.byref(out), H.st()) == INVALID
    assert L.lib.moge_postprocess(model._handle, None, None, None, None, 1, 4, 4, None, 0, ctypes.byref(out), H.st()) == INVALID
    assert L.lib.moge_postprocess(model._handle, p.data_ptr(), None, None, None, 1, 4, 4, None, 0, None, H.st()) == INVALID
    assert L.lib.moge_postprocess(model._handle, p.data_ptr(), None, None, None, 1, 4, 4, None, 0, ctypes.byref(out), H.st()) == INVALID      # points / depth out
