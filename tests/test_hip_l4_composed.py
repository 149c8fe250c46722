"""GPU: level 4 of the fp16 decoder with the 1x1 output conv folded into the resampler's weights (csrc/l4c.hip).

Kernel level (moge_test_conv_ex, up2 = 2), every output pixel, against torch on the CPU in float64:
  A  the kernel is exact for its operands: the same fp16-rounded composed weights and fp16 inputs; per output |d| <= K 2^-24 sum|w x| with K the number of
     accumulated terms (9 x 64 products + bias + the two uv terms) - fp32 accumulation of exact fp16 x fp16 products, any order;
  B  the composition is right: the un-composed chain F.interpolate(x2, bilinear) -> F.conv2d on a replicate pad (+ bias + uv) -> the 1x1 rows with UNROUNDED
     weights; per output |d| <= 2^-11 sum|Wc| |x| + A's bound - one fp16 rounding per composed weight.
Neither bound is measured.  Shapes: one pixel, sizes below one tile, exactly one tile, tiles that overhang in both directions, several tiles; the head forms
(one group, 3 and 1 real rows) and the neck forms (2 and 3 groups with the uv term, zero padding rows inside and at the end).
Model level: a tiny model with the released decoders' 64 -> 32 level-4 widths (the named tiny configs are 32 -> 32 and never take this path) against the real
reference's fp32 output inside the reference's own fp16 band, both fp16 forms (fixtures: tools/make_l4_composed_golden.py)."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1, 1), (2, 5, 7), (1, 16, 16), (2, 17, 33), (1, 40, 24)]
# (nd, rows handed to the entry, real rows, uv): a head with 3 outputs, a head with 1, the neck under (3, 1) and under (3, 3, 1) outputs
FORMS = {"head3": (1, 3, [0, 1, 2], False), "head1": (1, 1, [0], False), "neck2": (2, 8, [0, 1, 2, 4], True), "neck3": (3, 9, [0, 1, 2, 4, 5, 6, 8], True)}
UV = (-0.8, 0.8, -0.6, 0.6)
RB = torch.tensor([[[.75, .25, 0.], [.25, .75, 0.], [0., .75, .25]], [[.25, .75, 0.], [0., .75, .25], [0., .25, .75]]], dtype=torch.float64)     # R[p][dy][a]


@pytest.fixture(scope="module")
def H():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from tests import hip_util
    return hip_util


def run_l4c(H, x, w, b, d, uvw=None):
    """x (B,H,W,64), w (32,64,3,3), b (32), d (rows,32), uvw = (wu, wv) of 32 -> (B,2H,2W,4 nd) fp32 on the CPU"""
    L = H.L
    keep = [H._f(t) for t in (x, w, b, d)] + ([H._f(t) for t in uvw] if uvw else [])
    B, Hh, Ww, _ = x.shape
    nd = (d.shape[0] + 3) // 4
    y = torch.full((nd, B, 2 * Hh, 2 * Ww, 4), float("nan"), device="cuda", dtype=torch.float32)          # the kernel's layout: one map per group of four rows
    a = L.TestConvArgs()
    a.precision, a.B, a.H, a.W, a.Cin, a.Cout = 1, B, Hh, Ww, 64, 32
    a.relu_in, a.act, a.up2 = 0, 0, 2
    a.x, a.w, a.bias, a.dot_w, a.dot_rows = keep[0].data_ptr(), keep[1].data_ptr(), keep[2].data_ptr(), keep[3].data_ptr(), int(d.shape[0])
    if uvw:
        a.wu, a.wv = keep[4].data_ptr(), keep[5].data_ptr()
        a.u0, a.u1, a.v0, a.v1 = UV
    a.y = y.data_ptr()
    L.check(L.lib.moge_test_conv_ex(C.byref(a), H.st()))
    torch.cuda.synchronize()
    return y.cpu().permute(1, 2, 3, 0, 4).reshape(B, 2 * Hh, 2 * Ww, 4 * nd)


def operands(B, Hh, Ww, form, seed):
    nd, rows, real, uv = FORMS[form]
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, Hh, Ww, 64, generator=g).half().float()
    w = torch.randn(32, 64, 3, 3, generator=g) / 24.0
    b = torch.randn(32, generator=g)
    d = torch.zeros(rows, 32)
    d[real] = torch.randn(len(real), 32, generator=g) / 32 ** 0.5
    uvw = (torch.randn(32, generator=g), torch.randn(32, generator=g)) if uv else None
    return x, w, b, d, uvw


def uv_grids(Ho, Wo):
    u0, u1, v0, v1 = UV
    return torch.linspace(u0, u1, Wo, dtype=torch.float32).double(), torch.linspace(v0, v1, Ho, dtype=torch.float32).double()


_refs = {}


def references(B, Hh, Ww, form, seed):
    """-> operands, A (same rounded operands), A's bound, B (un-composed chain), B's bound; (B,2H,2W,4 nd) float64, computed once per case"""
    key = (B, Hh, Ww, form, seed)
    if key in _refs:
        return _refs[key]
    x, w, b, d, uvw = operands(B, Hh, Ww, form, seed)
    nd = FORMS[form][0]
    dp = torch.zeros(4 * nd, 32, dtype=torch.float64)
    dp[:d.shape[0]] = d.double()
    xd = x.double().permute(0, 3, 1, 2)
    Ho, Wo = 2 * Hh, 2 * Ww
    # composed weights: Wc[q][r][ci][a][b] = sum_m d[r][m] sum_{dy,dx} w[m][ci][dy][dx] R[py][dy][a] R[px][dx][b]
    w4 = torch.einsum("mcyx,pya,qxb->pqmcab", w.double(), RB, RB)
    wc = torch.einsum("rm,pqmcab->pqrcab", dp, w4)
    wc16 = wc.to(torch.float16).double()
    xp = F.pad(xd, (1, 1, 1, 1), mode="replicate")
    A = torch.zeros(B, 4 * nd, Ho, Wo, dtype=torch.float64)
    S = torch.zeros_like(A)            # sum |w x| over every accumulated term
    SB = torch.zeros_like(A)           # sum |Wc| |x|
    for py in range(2):
        for px in range(2):
            A[:, :, py::2, px::2] = F.conv2d(xp, wc16[py, px])
            S[:, :, py::2, px::2] = F.conv2d(xp.abs(), wc16[py, px].abs())
            SB[:, :, py::2, px::2] = F.conv2d(xp.abs(), wc[py, px].abs())
    bc = dp @ b.double()
    A += bc[None, :, None, None]
    S += bc.abs()[None, :, None, None]
    # the chain: bilinear x2 -> 3x3 on a replicate pad -> + bias (+ uv) -> the rows
    up = F.interpolate(xd, scale_factor=2, mode="bilinear", align_corners=False)
    x4 = F.conv2d(F.pad(up, (1, 1, 1, 1), mode="replicate"), w.double(), b.double())
    if uvw:
        u, v = uv_grids(Ho, Wo)
        wu, wv = uvw[0].double(), uvw[1].double()
        x4 = x4 + wu[None, :, None, None] * u[None, None, None, :] + wv[None, :, None, None] * v[None, None, :, None]
        tu, tv = (dp @ wu)[None, :, None, None] * u[None, None, None, :], (dp @ wv)[None, :, None, None] * v[None, None, :, None]
        A = A + tu + tv
        S = S + tu.abs() + tv.abs()
    Bref = torch.einsum("rm,bmyx->bryx", dp, x4)
    K = 9 * 64 + 3
    boundA = K * 2.0 ** -24 * S
    boundB = 2.0 ** -11 * SB + boundA
    out = (x, w, b, d, uvw), A.permute(0, 2, 3, 1), boundA.permute(0, 2, 3, 1), Bref.permute(0, 2, 3, 1), boundB.permute(0, 2, 3, 1)
    _refs[key] = out
    return out


@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("B,Hh,Ww", SHAPES)
def test_composed_resampler_against_float64(H, B, Hh, Ww, form):
    (x, w, b, d, uvw), A, boundA, Bref, boundB = references(B, Hh, Ww, form, 100 + Hh)
    got = run_l4c(H, x, w, b, d, uvw).double()
    assert got.shape == A.shape and bool(torch.isfinite(got).all()), "every output pixel is written"
    nd, rows, real, _ = FORMS[form]
    pad = [r for r in range(4 * nd) if r not in real]
    if pad:
        assert float(got[..., pad].abs().max()) == 0.0, "padding rows are exactly zero"
    eA, eB = (got - A).abs(), (got - Bref).abs()
    worstA, worstB = float((eA / boundA.clamp_min(1e-300))[..., real].max()), float((eB / boundB.clamp_min(1e-300))[..., real].max())
    print(f"[l4c] {B}x{Hh}x{Ww} {form}: max err / bound  A {worstA:.3f}  B {worstB:.3f}")
    assert bool((eA <= boundA).all()), ("A: same operands", worstA)
    assert bool((eB <= boundB).all()), ("B: un-composed chain", worstB)
    # the production grid is the chip's residency and a workgroup walks tiles t, t + grid, ...: these sizes fit in one round, so the walk is forced with
    # a grid of 1 (every tile behind another in the same LDS image) and of 3 (a stride that divides neither tile count per row nor per image)
    for grid in (1, 3):
        with H.L.tuned(CONV_GRID=grid):
            again = run_l4c(H, x, w, b, d, uvw).double()
        assert torch.equal(again, got), f"grid {grid}: a tile walked by a workgroup differs from the same tile alone"


@pytest.mark.parametrize("form", ["head3", "neck2"])
def test_batch_item_equals_single_image(H, form):
    x, w, b, d, uvw = operands(3, 17, 33, form, 7)
    batch = run_l4c(H, x, w, b, d, uvw)
    for i in range(3):
        single = run_l4c(H, x[i:i + 1], w, b, d, uvw)
        assert torch.equal(batch[i:i + 1], single), f"image {i} of the batch differs from the same image alone"


# ---- model level ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def MoGeModel():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from moge_amd.model import import_model_class_by_version
    return import_model_class_by_version("v2")


_model = {}


def l4c_model(MoGeModel, case, meta, tmp_path_factory):
    from oracle import moge_oracle as O
    from oracle.make_golden import weights_digest
    if "m" not in _model:
        cfg = O.make_config("dinov2_vits14", (2, 5, 8, 11), tuple(case["dims"]), True, scale_hidden=128)
        assert cfg["neck"]["dim_res_blocks"][3:] == [64, 32]
        sd = O.synth_state_dict(cfg, case["seed"], case["sane"])
        assert weights_digest(sd) == meta["weights_sha256"], "the fixture was made with other weights"
        path = os.path.join(str(tmp_path_factory.mktemp("ckpt")), "model.pt")
        O.save_checkpoint(path, cfg, sd)
        _model["m"] = MoGeModel.from_pretrained(path).to("cuda").eval()
    return _model["m"]


@pytest.mark.parametrize("name", ["l4c_tiny_b2_up", "l4c_tiny_wide"])
def test_model_with_64_to_32_level4_within_reference_fp16_band(MoGeModel, name, tmp_path_factory):
    from oracle.make_golden import make_input
    from tests.golden_util import GOLDEN_DIR, check_fp16, check_fp32, fp16_band, gate_line, subsample
    z = np.load(os.path.join(GOLDEN_DIR, name + ".npz"))
    meta = json.loads(bytes(z["meta"]).decode())
    gold = {k: z[k] for k in z.files if k != "meta"}
    case = meta["case"]
    model = l4c_model(MoGeModel, case, meta, tmp_path_factory)
    x = make_input(case)
    st = case["stride"]
    g = {k[6:]: v for k, v in gold.items() if k.startswith("infer.")}

    def sub(out):
        return {k: subsample(k, v.cpu().numpy(), st) for k, v in out.items()}

    kw = dict(case["kwargs"])
    try:
        check_fp32(sub(model.float().infer(x, **kw)), g)              # the layer-by-layer fp32 path of the same layout
        kw["use_fp16"] = True
        out = model.float().infer(x, **kw)
        out_h = model.half().infer(x, **kw)
    finally:
        model.float()
    for form, o in (("autocast", out), ("half", out_h)):
        band = fp16_band(meta, gold, form)
        seen = check_fp16(sub(o), g, band)
        print(f"[l4c gate] {name} {form}: " + gate_line(seen, band))
