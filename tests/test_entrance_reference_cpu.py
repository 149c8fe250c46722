"""CPU: every float64 numpy reference of tests/entrance_reference.py against an independent torch formulation of the same operation, so that a wrong
reference cannot pass a wrong kernel in tests/test_hip_entrance_kernels.py.  Where torch can run the operation in float32 too, that result must sit
inside the derived bound: a bound a correct fp32 implementation misses would be useless.

What agreement the resize references can reach.  They form range, centre and unnormalised weights in float32 (what ATen does for a float32 image, and
what the kernels do); torch on DOUBLES forms them in float64.  The two differ by (a) the rounding of scale and of scale * (o + 0.5): up to two ulp32 of the
centre, i.e. twice the coordinate term of the bound, and (b) the rounding of each filter value, which the bound's e_sum (and, for the cubic, e_w) grants any
fp32 implementation.  So the float32-formed reference is held to e_sum + e_w + 2 e_coord of torch float64, and the same code with the weights formed in float64
(aa_axis(..., form_dtype=np.float64)) to 1e-13: that pins the structure (ranges, filter, normalisation, pass order) to the last bits, and leaves to the
float32 forms only what float32 rounding explains."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import entrance_reference as ER

AA_SHAPES = [((28, 42), (28, 42)), ((20, 30), (28, 42)), ((45, 61), (28, 42)), ((150, 200), (28, 42)), ((20, 61), (28, 42)), ((7, 5), (14, 14)), ((64, 64), (37, 41))]


@pytest.mark.parametrize("kind", ["bilinear", "bicubic"])
@pytest.mark.parametrize("src,dst", AA_SHAPES)
def test_aa_resize_reference_matches_torch(kind, src, dst):
    (H, W), (OH, OW) = src, dst
    x = np.random.default_rng(H + W).random((2, 3, H, W)).astype(np.float32)
    x[0, 0, : H // 2] += 3.0                                          # an edge: the coordinate term is about slopes
    x64 = x.astype(np.float64)
    want = F.interpolate(torch.from_numpy(x64), size=(OH, OW), mode=kind, align_corners=False, antialias=True).numpy()
    exact = ER.aa_resize(x64, OH, OW, kind, form_dtype=np.float64)[0]
    assert np.abs(exact - want).max() <= 1e-13, float(np.abs(exact - want).max())
    ref, bound, e_sum, e_coord, e_w = ER.aa_resize(x64, OH, OW, kind, parts=True)
    assert (bound > 0).all() and np.isfinite(bound).all()
    d = np.abs(ref - want)
    assert (d <= e_sum + e_w + 2 * e_coord).all(), float((d / (e_sum + e_w + 2 * e_coord)).max())
    assert (e_w > 0).all() == (kind == "bicubic")
    if (H, W) == (OH, OW):
        assert np.array_equal(ref, x64), "scale 1: the weights are exactly 1 and 0"
    got32 = F.interpolate(torch.from_numpy(x), size=(OH, OW), mode=kind, align_corners=False, antialias=True).double().numpy()
    assert (np.abs(got32 - ref) <= bound).all(), float((np.abs(got32 - ref) / bound).max())
    if kind == "bicubic" and (H, W) == (7, 5):
        # the cubic's weight term is needed: torch's own float32 result is outside the three-part form e_sum + e_coord when up-scaling
        assert (np.abs(got32 - ref) > e_sum + e_coord).any()


@pytest.mark.parametrize("aa", [True, False])
@pytest.mark.parametrize("src,rows,cols", [((28, 42), 2, 3), ((20, 30), 2, 3), ((45, 61), 2, 3), ((150, 200), 2, 3), ((20, 61), 2, 3), ((9, 11), 1, 1)])
def test_preprocess_reference_matches_torch(aa, src, rows, cols):
    H, W = src
    x = np.random.default_rng(H).random((2, 3, H, W)).astype(np.float32)
    ref, bound = ER.preprocess(x, rows, cols, aa=aa)
    mean, sd = torch.from_numpy(ER.MEAN).view(1, 3, 1, 1), torch.from_numpy(ER.SD).view(1, 3, 1, 1)
    want = (F.interpolate(torch.from_numpy(x).double(), size=(14 * rows, 14 * cols), mode="bilinear", align_corners=False, antialias=aa) - mean) / sd
    assert (np.abs(ref - want.numpy()) <= 2 * bound).all()           # float64 weights against float32-formed ones: twice the coordinate term at most
    got32 = (F.interpolate(torch.from_numpy(x), size=(14 * rows, 14 * cols), mode="bilinear", align_corners=False, antialias=aa) - mean.float()) / sd.float()
    assert (np.abs(got32.double().numpy() - ref) <= bound).all(), float((np.abs(got32.double().numpy() - ref) / bound).max())
    # rounding the image first is all that round16 / an fp16 input change; an fp16 store widens the bound by half an fp16 ulp
    r16, b16 = ER.preprocess(x, rows, cols, aa=aa, round16=True, out_fp16=True)
    rr, bb = ER.preprocess(x.astype(np.float16).astype(np.float32), rows, cols, aa=aa)
    assert np.array_equal(r16, rr) and np.array_equal(r16, ER.preprocess(x, rows, cols, aa=aa, in_fp16=True)[0])
    assert np.allclose(b16 - bb, 2.0 ** -11 * np.abs(rr) + 2.0 ** -25, rtol=1e-9, atol=0)


def test_patchify_and_patch_epilogue_match_conv2d():
    """patch_embed.py:75 + vision_transformer.py:228-231: Conv2d(3, N, 14, stride 14), flatten, + pos; cls row = cls + pos[0]."""
    g = torch.Generator().manual_seed(0)
    B, rows, cols, N = 2, 2, 3, 8
    Np, Ntok = rows * cols, rows * cols + 1
    img = torch.randn(B, 3, 14 * rows, 14 * cols, generator=g)
    w, bias = torch.randn(N, 3, 14, 14, generator=g) / 24, torch.randn(N, generator=g)
    pos, cls = torch.randn(1 + Np, N, generator=g), torch.randn(N, generator=g)
    A = ER.patchify(img.numpy().astype(np.float64), 640)
    assert A.shape == (B * Np, 640) and (A[:, 588:] == 0).all()
    assert np.array_equal(ER.unpatchify(A, B, rows, cols), img.numpy().astype(np.float64))
    Wm = np.zeros((N, 640), dtype=np.float32)
    Wm[:, :588] = w.reshape(N, 588).numpy()
    fill = np.full((B * Ntok, N), 123.0)
    ref, e = ER.patch_embed(A.astype(np.float32), Wm, bias.numpy(), pos.numpy(), cls.numpy(), B, Np, Ntok, fill, 0)
    tok = F.conv2d(img.double(), w.double(), bias.double(), stride=14).flatten(2).transpose(1, 2) + pos.double()[None, 1:]
    want = torch.cat([(cls + pos[0]).double().expand(B, 1, N), tok], 1).reshape(B * Ntok, N).numpy()
    np.testing.assert_allclose(ref, want, rtol=1e-12, atol=1e-12)
    assert (e.reshape(B, Ntok, N)[:, 0] == 0).all() and (e.reshape(B, Ntok, N)[:, 1:] > 0).all()
    got32 = torch.cat([(cls + pos[0]).expand(B, 1, N), F.conv2d(img, w, bias, stride=14).flatten(2).transpose(1, 2) + pos[None, 1:]], 1).reshape(B * Ntok, N)
    assert (np.abs(got32.double().numpy() - ref) <= e).all()
    ref2, e2 = ER.patch_embed(A.astype(np.float32), Wm, bias.numpy(), pos.numpy(), None, B, Np, Ntok, fill, 0)
    assert (ref2.reshape(B, Ntok, N)[:, 0] == 123.0).all() and np.array_equal(ref2.reshape(B, Ntok, N)[:, 1:], ref.reshape(B, Ntok, N)[:, 1:])


@pytest.mark.parametrize("size_mode", [False, True])
@pytest.mark.parametrize("rows,cols", [(1, 1), (1, 37), (37, 1), (36, 38), (3, 70), (60, 60), (37, 37), (10, 12)])
def test_posembed_reference_matches_the_oracle(rows, cols, size_mode):
    from oracle import moge_oracle as O
    D = 8
    pos = torch.randn(1, 1 + 37 * 37, D, generator=torch.Generator().manual_seed(rows * cols))
    ref, bound = ER.posembed(pos[0].numpy(), rows, cols, size_mode)
    want32 = O.pos_embed_for_grid(pos, rows, cols, onnx_compatible_mode=size_mode)[0].double().numpy()          # ATen in float32
    assert ref.shape == want32.shape
    assert np.array_equal(ref[0], want32[0]) and (bound[0] == 0).all()
    assert (np.abs(ref - want32) <= bound).all(), float((np.abs(ref - want32)[1:] / bound[1:]).max())
    if (rows, cols, size_mode) == (60, 60, False):
        # the weight term is needed: without it torch's own float32 result is outside (small src: no coordinate term, the cubic's absolute error shows)
        assert (np.abs(ref - want32)[1:] > ER.posembed(pos[0].numpy(), rows, cols, size_mode, weight_term=False)[1][1:]).any()
    if (rows, cols) == (37, 37):
        assert np.array_equal(ref, pos[0].double().numpy()), "plain mode: the bypass; size mode: scale exactly 1, weights 0 1 0 0"
        assert ((bound[1:] == 0).all()) == (not size_mode)
        return
    # ... and the float64 interpolate of the same grid, which differs by the float32 source coordinate and weights only (twice the bound's share)
    grid = pos[0, 1:].double().reshape(1, 37, 37, D).permute(0, 3, 1, 2)
    if size_mode:
        up = F.interpolate(grid, size=(rows, cols), mode="bicubic", antialias=False)
    else:
        up = F.interpolate(grid, scale_factor=((rows + 0.1) / 37, (cols + 0.1) / 37), mode="bicubic", antialias=False)
    want64 = up.permute(0, 2, 3, 1).reshape(rows * cols, D).numpy()
    assert (np.abs(ref[1:] - want64) <= 2 * bound[1:]).all(), float((np.abs(ref[1:] - want64) / bound[1:]).max())
    # a neighbouring-tap mistake is far outside: shifting the grid by one cell moves the result by many bounds
    if rows * cols > 1:
        assert np.median(np.abs(np.roll(want64, 1, 0) - ref[1:]) / bound[1:]) > 100


def test_pos_rscale_is_what_the_two_modes_define():
    assert ER.pos_rscale(37, True) == np.float32(1.0) and ER.pos_rscale(37, False) != np.float32(1.0)
    assert ER.pos_rscale(60, False) == np.float32(1.0 / (60.1 / 37)) and ER.pos_rscale(60, True) == np.float32(37) / np.float32(60)


@pytest.mark.parametrize("prec", [0, 1])
def test_qkv_reference_matches_the_attention_split(prec):
    g = torch.Generator().manual_seed(1)
    B, Ntok, nh, K = 2, 5, 2, 16
    D = nh * 64
    x, W, b = torch.randn(B * Ntok, K, generator=g), torch.randn(3 * D, K, generator=g) / 4, torch.randn(3 * D, generator=g)
    r = ER.qkv(x.numpy(), W.numpy(), b.numpy(), B, Ntok, nh, 0.25, prec)
    xs, Ws = (x.half().double(), W.half().double()) if prec else (x.double(), W.double())
    q, k, v = F.linear(xs, Ws, b.double()).reshape(B, Ntok, 3, nh, 64).permute(2, 0, 3, 1, 4).unbind(0)          # attention.py:72-74
    np.testing.assert_allclose(r["q"][0], (q * 0.25).numpy(), rtol=1e-13, atol=1e-13)
    np.testing.assert_allclose(r["k"][0], k.numpy(), rtol=1e-13, atol=1e-13)
    np.testing.assert_allclose(r["vT"][0], v.transpose(-1, -2).numpy(), rtol=1e-13, atol=1e-13)
    assert all((e > 0).all() for _, e in r.values())


@pytest.mark.parametrize("pixH,pixW", [(1, 1), (3, 5), (6, 9)])
def test_convt_uv_in_reference_matches_conv_transpose2d(pixH, pixW):
    """v1.py:118-121: x = cat([x, uv]); ConvTranspose2d(Cin + 2, Cout, 2, 2) - the GEMM carries the Cin channels, the epilogue the two uv channels."""
    g = torch.Generator().manual_seed(pixW)
    B, Cin, Cout = 2, 8, 4
    x = torch.randn(B, pixH, pixW, Cin, generator=g)
    wt = torch.randn(Cin + 2, Cout, 2, 2, generator=g) / 3
    bias = torch.randn(Cout, generator=g)
    rng = (-0.8, 0.8, -0.6, 0.6)
    u32, v32 = torch.linspace(rng[0], rng[1], pixW), torch.linspace(rng[2], rng[3], pixH)
    assert np.array_equal(ER.linspace32(rng[0], rng[1], pixW), u32.double().numpy()) and np.array_equal(ER.linspace32(rng[2], rng[3], pixH), v32.double().numpy())
    for n in (2, 7, 8, 41):
        assert np.array_equal(ER.linspace32(-0.3, 0.7, n), torch.linspace(-0.3, 0.7, n).double().numpy())
    uv = torch.stack(torch.meshgrid(u32.double(), v32.double(), indexing="xy"), 0)[None].expand(B, 2, pixH, pixW)
    want = F.conv_transpose2d(torch.cat([x.double().permute(0, 3, 1, 2), uv], 1), wt.double(), bias.double(), stride=2).permute(0, 2, 3, 1).numpy()
    Wg = wt.permute(2, 3, 1, 0).reshape(4 * Cout, Cin + 2)                   # row n = (dy 2 + dx) Cout + co
    ref, e = ER.convt_uv_in(x.reshape(-1, Cin).numpy(), Wg[:, :Cin].numpy(), bias.repeat(4).numpy(), Wg[:, Cin].numpy(), Wg[:, Cin + 1].numpy(), rng, B, pixH, pixW, Cout, 0)
    np.testing.assert_allclose(ref, want, rtol=1e-12, atol=1e-12)
    assert (e > 0).all()


def test_bicubic_reference_round16_is_the_rounded_image():
    x = np.random.default_rng(3).random((1, 3, 20, 17)).astype(np.float32)
    a, ea = ER.resize_bicubic_aa(x, 31, 9, round16=True)
    b, eb = ER.resize_bicubic_aa(x.astype(np.float16).astype(np.float32), 31, 9)
    c, ec = ER.resize_bicubic_aa(x, 31, 9, in_fp16=True)
    assert np.array_equal(a, b) and np.array_equal(a, c) and np.array_equal(eb, ec)
    assert np.allclose(ea - eb, 2.0 ** -11 * np.abs(a) + 2.0 ** -25, rtol=1e-9, atol=0)
