"""GPU: moge_amd.losses (csrc/losses.hip) against the unmodified reference - values AND gradients, from the float32 and float64 runs stored in
tests/golden/losses_*.npz - and, for the shapes the goldens do not cover, against the restatement tests/losses_reference.py.

The gates, eps32 = 2^-23, with the reference's own float32 rounding as the yardstick:
    |got - ref64| <= max(4 |ref32 - ref64|, 8 eps32 |ref64|)                         losses
    max |g - g64| <= max(4 max |g32 - g64|, 8 eps32 max |g64|)   per instance        gradients, over all pixels
The factor 4 allows for another summation order of the same fp32 terms; the floor covers a float32 run that happens to land on the float64
value.  Then: a batch equals the stack of its instances bit for bit, two calls give the same bits, and the sampler's statistics."""
import os

import numpy as np
import pytest
import torch

import losses_reference as R

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
EPS32 = 2.0 ** -23
DEV = "cuda:0"


def M():
    import moge_amd.losses as m
    return m


def gate(name, got, g, v32, v64, g32, g64):
    """got / g: (B, ...) float64 arrays of the kernels; v*/g*: the yardstick's float32 and float64 runs"""
    got, v32, v64 = (np.asarray(a, np.float64).reshape(-1) for a in (got, v32, v64))
    nan = np.isnan(v64)
    assert (np.isnan(got) == nan).all(), f"{name}: NaN where the reference has none, or the other way round"
    err, bound = np.abs(got - v64)[~nan], np.maximum(4 * np.abs(v32 - v64), 8 * EPS32 * np.abs(v64))[~nan]
    print(f"{name}: loss err {err.max() if err.size else 0:.3e} bound {bound.min() if bound.size else 0:.3e}", end="; ")
    assert (err <= bound).all(), f"{name}: loss {got} vs {v64}: err {err} > {bound}"
    g, g32, g64 = (np.asarray(a, np.float64).reshape(a.shape[0], -1) for a in (g, g32, g64))
    assert g.shape == g64.shape and np.isfinite(g).all()
    for i in range(g.shape[0]):
        e, b = np.abs(g[i] - g64[i]).max(), max(4 * np.abs(g32[i] - g64[i]).max(), 8 * EPS32 * np.abs(g64[i]).max())
        print(f"grad[{i}] err {e:.3e} bound {b:.3e}", end="; ")
        assert e <= b, f"{name}: gradient of instance {i}: {e} > {b}"
    print()


def to_dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def run_gpu(fn, arrays):
    """-> (loss, gradient of loss.sum() for the first argument) as float64 numpy"""
    args = [to_dev(a) for a in arrays]
    args[0].requires_grad_()
    loss, misc = fn(*args)
    assert misc == {} and loss.dtype == torch.float32
    grad, = torch.autograd.grad(loss.sum(), args[0])
    return loss.detach().cpu().double().numpy(), grad.cpu().double().numpy()


def run_restated(fn, dtype, arrays):
    args = [torch.from_numpy(a).to(dtype) if a.dtype.kind == "f" else torch.from_numpy(a) for a in arrays]
    args[0].requires_grad_()
    loss = fn(*args)
    grad, = torch.autograd.grad(loss.sum(), args[0])
    return loss.detach().double().numpy(), grad.double().numpy()


def functions():
    m = M()
    return {"normal": (m.normal_loss, R.normal_loss), "edge": (m.edge_loss, R.edge_loss), "mask_l2": (m.mask_l2_loss, R.mask_l2_loss),
            "mask_bce": (m.mask_bce_loss, R.mask_bce_loss), "normal_map": (m.normal_map_loss, R.normal_map_loss),
            "metric_scale": (m.metric_scale_loss, R.metric_scale_loss)}


STENCIL = ["losses_stencil_b2_24x40", "losses_stencil_33x65"]
GOLDEN_CASES = [(f, k, ("points", "gt_points")) for f in STENCIL for k in ("normal", "edge")] + [
    ("losses_pixel_b2_24x40", "mask_l2", ("pred_mask", "gt_mask_pos", "gt_mask_neg")),
    ("losses_pixel_b2_24x40", "mask_bce", ("pred_mask_prob", "gt_mask_pos", "gt_mask_neg")),
    ("losses_pixel_b2_24x40", "normal_map", ("pred_normal", "gt_normal")),
    ("losses_pixel_b2_24x40", "metric_scale", ("scale_pred", "scale_gt")),
]


@pytest.mark.parametrize("fixture,key,inputs", GOLDEN_CASES, ids=[f"{c[0]}-{c[1]}" for c in GOLDEN_CASES])
def test_parity_with_the_reference_values_and_gradients(fixture, key, inputs):
    z = np.load(os.path.join(GOLDEN, fixture + ".npz"))
    got, g = run_gpu(functions()[key][0], [z[k] for k in inputs])
    assert got.shape == z[key + "_f64"].shape
    gate(f"{fixture} {key}", got, g, z[key + "_f32"], z[key + "_f64"], z[key + "_grad_f32"], z[key + "_grad_f64"])


# ---- edge shapes against the restatement ------------------------------------------------------------------------------------------------------
def inputs_for(key, rng, B, H, W, invalid="some"):
    """float32 inputs of one function on a (B, H, W) map.  invalid: "some" (a few non-finite gt pixels), "all", "one" (a single valid pixel), "none" """
    if key in ("normal", "edge", "normal_map"):
        pred, gt = R.scene(rng, B, H, W)
        if key == "normal_map":
            pred = rng.normal(0, 1, pred.shape).astype(np.float32)
            gt = rng.normal(0, 1, gt.shape).astype(np.float32)
        if invalid == "some" and H * W >= 6:
            gt.reshape(B, -1, 3)[:, rng.integers(0, H * W), 0] = np.nan
            gt[0, H // 2, W // 2] = np.inf
        elif invalid in ("all", "one"):
            keep = gt[:, H // 2, W // 2].copy()
            gt[:] = np.nan
            if invalid == "one":
                gt[:, H // 2, W // 2] = keep
        return [pred, gt]
    if key in ("mask_l2", "mask_bce"):
        pos = rng.random((B, H, W)) < 0.4
        neg = ~pos & (rng.random((B, H, W)) < 0.7)
        if invalid == "all":
            pos[:], neg[:] = False, False
        pred = rng.normal(0.5, 0.6, (B, H, W)) if key == "mask_l2" else rng.uniform(1e-3, 1 - 1e-3, (B, H, W))
        return [pred.astype(np.float32), pos, neg]
    s_gt = rng.uniform(0.2, 5, (B, H, W)).astype(np.float32)
    if invalid != "none":
        s_gt[rng.random(s_gt.shape) < (1.0 if invalid == "all" else 0.2)] = -1
    return [rng.uniform(0.2, 5, (B, H, W)).astype(np.float32), s_gt]


def check_against_restatement(key, arrays, name):
    fn, ref = functions()[key]
    got, g = run_gpu(fn, arrays)
    v64, g64 = run_restated(ref, torch.float64, arrays)
    v32, g32 = run_restated(ref, torch.float32, arrays)
    gate(name, got, g, v32, v64, g32, g64)


def tile_shapes():
    m = M()
    around = lambda t: (t - 1, t, t + 1)
    return [(h, w) for h in around(m.TILE_H) for w in around(m.TILE_W)] + [(2 * m.TILE_H + 1, 2 * m.TILE_W + 1)]


@pytest.mark.parametrize("key", ["normal", "edge"])
def test_stencil_losses_at_small_and_tile_edge_shapes(key):
    rng = np.random.default_rng(7)
    for H, W in [(2, 2), (2, 3), (3, 5), (5, 7)] + tile_shapes():
        check_against_restatement(key, inputs_for(key, rng, 2, H, W), f"{key} {H}x{W}")


@pytest.mark.parametrize("key", ["edge", "mask_l2", "mask_bce", "normal_map", "normal"])
def test_single_row_and_single_column(key):
    """1 x W and H x 1: edge_loss (and normal_loss) take a mean over nothing there - NaN, as torch - with a finite gradient from the other mean"""
    rng = np.random.default_rng(8)
    for H, W in ((1, 37), (41, 1), (1, 1)):
        check_against_restatement(key, inputs_for(key, rng, 2, H, W, invalid="none"), f"{key} {H}x{W}")


@pytest.mark.parametrize("key", ["mask_l2", "mask_bce", "normal_map", "metric_scale"])
def test_elementwise_losses_around_the_span_of_a_workgroup(key):
    rng = np.random.default_rng(9)
    span = M().SPAN
    for H, W in ((3, 5), (1, span - 1), (1, span), (1, span + 1), (33, 65)):          # 33 x 65 = 2145: three workgroups per image
        check_against_restatement(key, inputs_for(key, rng, 2, H, W), f"{key} {H}x{W}")


@pytest.mark.parametrize("key", ["normal", "edge", "mask_l2", "mask_bce", "normal_map", "metric_scale"])
def test_all_invalid_a_single_valid_pixel_and_one_empty_instance(key):
    rng = np.random.default_rng(10)
    for invalid in ("all", "one"):
        check_against_restatement(key, inputs_for(key, rng, 1, 9, 11, invalid), f"{key} {invalid}")
    arrays = inputs_for(key, rng, 3, 9, 35)
    empty = inputs_for(key, rng, 1, 9, 35, "all")
    for a, e in zip(arrays, empty):
        a[1] = e[0]                                                 # B = 3 with instance 1 empty
    check_against_restatement(key, arrays, f"{key} B=3, one empty")


# ---- bit-level properties --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", ["normal", "edge", "mask_l2", "mask_bce", "normal_map", "metric_scale"])
def test_batch_equals_the_stack_of_instances_and_calls_repeat_bit_for_bit(key):
    rng = np.random.default_rng(11)
    fn = functions()[key][0]
    arrays = inputs_for(key, rng, 3, 19, 70)
    loss, grad = run_gpu(fn, arrays)
    again = run_gpu(fn, arrays)
    assert np.array_equal(loss, again[0], equal_nan=True) and np.array_equal(grad, again[1])
    for i in range(3):
        li, gi = run_gpu(fn, [a[i:i + 1] for a in arrays])
        assert np.array_equal(li[0], loss[i], equal_nan=True) and np.array_equal(gi[0], grad[i]), (key, i)
    # leading batch dims: (3, 1, ...) is the same numbers
    l2, g2 = run_gpu(fn, [a[:, None] for a in arrays])
    assert l2.shape == (3, 1) + loss.shape[1:] and np.array_equal(l2[:, 0], loss) and np.array_equal(g2[:, 0], grad)


def test_gradients_scale_with_the_incoming_gradient_and_gt_gets_none():
    m = M()
    rng = np.random.default_rng(12)
    pred, gt = (to_dev(a) for a in R.scene(rng, 2, 9, 33))
    pred.requires_grad_()
    gt.requires_grad_()
    w = torch.tensor([2.0, -0.5], device=DEV)
    for fn in (m.normal_loss, m.edge_loss, m.normal_map_loss):
        loss, _ = fn(pred, gt)
        g, ggt = torch.autograd.grad((loss * w).sum(), (pred, gt), allow_unused=True)
        assert ggt is None
        g1, = torch.autograd.grad(fn(pred, gt)[0].sum(), pred)
        assert torch.equal(g, g1 * w[:, None, None, None])          # scaling by a power of two is exact
    half = pred.detach().half().requires_grad_()                     # other dtypes are upcast, and the results come back in them
    loss, _ = m.edge_loss(half, gt.detach().half())
    g, = torch.autograd.grad(loss.sum(), half)
    assert loss.dtype == torch.float16 and g.dtype == torch.float16 and torch.isfinite(g).all()


# ---- the sampler ---------------------------------------------------------------------------------------------------------------------------
def test_anchor_sampling_weight():
    m = M()
    rng = np.random.default_rng(13)
    B, H, W, r2 = 2, 24, 40, 6
    _, gt = R.scene(rng, B, H, W)
    mask = rng.random((B, H, W)) < 0.85
    mask[1, :5] = False
    r3 = (0.5 / 4 / 0.9 * gt[..., 2]).astype(np.float32)
    pts, msk, rad = to_dev(gt), to_dev(mask), to_dev(r3)

    def draw(seed):
        gen = torch.Generator(device=DEV)
        gen.manual_seed(seed)
        return m.anchor_sampling_counts(pts, msk, r2, rad, 64, gen)

    w, c = draw(1)
    assert w.dtype == torch.float32 and w.shape == (B, H, W) and c.dtype == torch.int32
    assert (w >= 0).all() and (w[~msk] == 0).all() and (c[~msk] == 0).all() and (w[msk] > 0).all()
    assert (w.double().sum(dim=(-2, -1)) - 1).abs().max() <= 1e-6
    cc = c.cpu().numpy()
    expect = 1 / np.maximum(cc, 1) * mask
    assert np.allclose(w.cpu().numpy(), expect / expect.sum(axis=(1, 2), keepdims=True), rtol=1e-5, atol=0)
    w1, c1 = draw(1)
    w2, c2 = draw(2)
    assert torch.equal(w, w1) and torch.equal(c, c1) and not torch.equal(c, c2)
    gen = torch.Generator(device=DEV)
    gen.manual_seed(1)
    m.compute_anchor_sampling_weight(pts, msk, r2, rad, generator=gen)
    assert not torch.equal(m.anchor_sampling_counts(pts, msk, r2, rad, 64, gen)[1], c)       # the call advanced the generator
    assert torch.equal(m.anchor_sampling_counts(pts[1], msk[1], r2, rad[1], 64, torch.Generator(device=DEV).manual_seed(1))[1], c[1])     # alone = in the batch
    # counts against the binomial: sum(count) within 5 sigma of 64 sum(p), p the exact in-window fraction
    for b in range(B):
        p = R.in_window_fraction(torch.from_numpy(gt[b]), torch.from_numpy(mask[b]), r2, torch.from_numpy(r3[b])).numpy()
        mean, sigma = 64 * p.sum(), np.sqrt(64 * (p * (1 - p)).sum())
        print(f"sampler image {b}: sum(count) {cc[b].sum()} expected {mean:.1f} sigma {sigma:.1f}")
        assert abs(cc[b].sum() - mean) <= 5 * sigma
        assert (cc[b][p == 0] == 0).all() and (cc[b] <= 64).all()
    # the default generator is taken, and advanced, when none is given
    torch.cuda.manual_seed(5)
    a = m.compute_anchor_sampling_weight(pts, msk, r2, rad)
    b_ = m.compute_anchor_sampling_weight(pts, msk, r2, rad)
    torch.cuda.manual_seed(5)
    assert torch.equal(m.compute_anchor_sampling_weight(pts, msk, r2, rad), a) and not torch.equal(a, b_)


# ---- affine_invariant_global_loss ---------------------------------------------------------------------------------------------------------
GLOBAL = ["losses_global_b2_24x40", "losses_global_33x65"]


def global_config(z, case):
    return dict(align_resolution=int(z[case + "_align_resolution"]), beta=float(z[case + "_beta"]), trunc=float(z[case + "_trunc"]),
                sparsity_aware=bool(z[case + "_sparsity_aware"]))


def lr_inputs(m, pred, gt, res):
    """what moge_amd.losses hands its solve: (pred_lr, gt_lr, weight, lr_mask) of a (B, H, W, 3) batch on the GPU"""
    lr_mask, rows, cols = m.lr_samples(gt, (res, res))
    image = torch.arange(pred.shape[0], device=DEV)[:, None]
    gt_lr = gt[image, rows, cols]
    gt_lr = torch.where(torch.isfinite(gt_lr).all(-1, keepdim=True), gt_lr, torch.ones_like(gt_lr))
    return pred[image, rows, cols], gt_lr, lr_mask.float() / gt_lr[..., 2].clamp_min(1e-2), lr_mask


def hip_selection(m, pred, gt, res, trunc):
    """the (anchor sample, solution element) pairs the HIP solve selects, (B, 2) on the host"""
    from moge_amd import alignment as A
    src, tgt, w, _ = lr_inputs(m, pred, gt, res)
    k, i2 = A._anchor_search(src.detach().contiguous(), tgt.contiguous(), w.contiguous(), 0b100, trunc)
    return torch.stack([k, i2], -1).cpu().numpy()


def same_line(sel, want):
    """the same two samples: as selected, or anchor and solution sample swapped (the same line through both)"""
    (k, i2), (wk, wi2) = (int(v) for v in sel), (int(v) for v in want)
    return (k, i2) == (wk, wi2) or (wi2 % 3 == 2 and (k, i2) == (wi2 // 3, 3 * wk + 2))


def global_gate(name, z, case, loss, misc, scale, grad):
    gate(name + " loss", loss, grad, z[case + "_loss_f32"], z[case + "_loss_f64"], z[case + "_grad_f32"], z[case + "_grad_f64"])
    none = np.zeros((loss.shape[0], 1))
    gate(name + " truncated_error", misc["truncated_error"].cpu().double().numpy(), none, z[case + "_te_f32"], z[case + "_te_f64"], none, none)
    gate(name + " delta", misc["delta"].cpu().double().numpy(), none, z[case + "_delta_f32"], z[case + "_delta_f64"], none, none)
    if scale is not None:
        gate(name + " scale", scale.cpu().double().numpy(), none, z[case + "_scale_f32"], z[case + "_scale_f64"], none, none)


@pytest.mark.parametrize("fixture", GLOBAL)
@pytest.mark.parametrize("case", ["c0", "c1"])
def test_global_loss_parity_with_the_reference(fixture, case):
    m = M()
    z = np.load(os.path.join(GOLDEN, fixture + ".npz"))
    cfg = global_config(z, case)
    pred, gt = to_dev(z["points"]).requires_grad_(), to_dev(z["gt_points"])
    # 1. the fused op apart from the solve: scale and shift are the line through the fixture's selected samples (differentiable, so the full
    #    gradient - direct term plus the path through scale / shift - is comparable with the reference's)
    src, tgt, _, lr_mask = lr_inputs(m, pred, gt, cfg["align_resolution"])
    lines = [R.scale_z_shift(src[b], tgt[b], *(int(v) for v in z[case + "_selection"][b])) for b in range(pred.shape[0])]
    scale, shift = torch.stack([l[0] for l in lines]), torch.stack([l[1] for l in lines])
    lr_frac = lr_mask.float().mean(-1) if cfg["sparsity_aware"] else None
    loss, misc = m.affine_dense_loss(pred, gt, scale, shift, lr_frac, cfg["beta"])
    grad, = torch.autograd.grad(loss.sum(), pred)
    global_gate(f"{fixture} {case} dense", z, case, loss.detach().cpu().double().numpy(), misc, scale.detach(), grad.cpu().double().numpy())
    # 2. end to end through the HIP solve: it selects the fixture's samples (a hard assert), then the same gates
    sel = hip_selection(m, pred.detach(), gt, cfg["align_resolution"], cfg["trunc"])
    for b in range(pred.shape[0]):
        assert same_line(sel[b], z[case + "_selection"][b]), (b, sel[b], z[case + "_selection"][b])
    loss, misc, scale = m.affine_invariant_global_loss(pred, gt, **cfg)
    assert not scale.requires_grad and misc["delta"].shape == loss.shape == scale.shape
    grad, = torch.autograd.grad(loss.sum(), pred)
    global_gate(f"{fixture} {case} end to end", z, case, loss.detach().cpu().double().numpy(), misc, scale, grad.cpu().double().numpy())


def global_against_restatement(m, pred_np, gt_np, name, **cfg):
    """the restatement is handed the samples the HIP solve selected (the solvers have their own tests): what is compared is everything else"""
    pred, gt = to_dev(pred_np).requires_grad_(), to_dev(gt_np)
    loss, misc, scale = m.affine_invariant_global_loss(pred, gt, **cfg)
    grad, = torch.autograd.grad(loss.sum(), pred)
    sel = hip_selection(m, pred.detach(), gt, cfg["align_resolution"], cfg["trunc"])
    ref = {}
    for tag, dtype in (("f32", torch.float32), ("f64", torch.float64)):
        rows = []
        for b in range(pred_np.shape[0]):
            p = torch.from_numpy(pred_np[b]).to(dtype).requires_grad_()
            l, te, dl, sc = R.affine_invariant_global_loss(p, torch.from_numpy(gt_np[b]).to(dtype), selection=tuple(int(v) for v in sel[b]), **cfg)
            g, = torch.autograd.grad(l, p)
            rows.append([v.detach().double().numpy() for v in (l, te, dl, sc, g)])
        for i, key in enumerate(("loss", "te", "delta", "scale", "grad")):
            ref[f"c_{key}_{tag}"] = np.stack([r[i] for r in rows])
    global_gate(name, ref, "c", loss.detach().cpu().double().numpy(), misc, scale, grad.cpu().double().numpy())


def test_global_loss_at_edge_shapes():
    m = M()
    rng = np.random.default_rng(21)
    for (H, W), res in (((3, 5), 2), ((5, 7), 3), ((1, m.SPAN - 1), 3), ((1, m.SPAN + 1), 3), ((32, 32), 4), ((33, 65), 4)):
        pred, gt = R.scene(rng, 2, H, W, noise=0.1)
        if H * W > 20:
            gt[0, H // 2, W // 3:W // 3 + 3] = np.nan
            gt[1, 0, 0, 2] = 0.003                                  # the weight clamp
        global_against_restatement(m, pred, gt, f"global {H}x{W}", align_resolution=res, beta=0.01 * (H % 2), trunc=0.05, sparsity_aware=bool(W % 2))
    # a single valid pixel: one sample, whose x or y element fixes the scale
    pred, gt = R.scene(rng, 1, 6, 9)
    keep = gt[0, 2, 3].copy()
    gt[:] = np.inf
    gt[0, 2, 3] = keep
    global_against_restatement(m, pred, gt, "global, a single valid pixel", align_resolution=3, beta=0.0, trunc=1.0, sparsity_aware=True)
    p = to_dev(pred)
    with pytest.raises(ValueError):                                 # no finite gt pixel at all: the solve has no anchor
        m.affine_invariant_global_loss(p, torch.full_like(p, float("nan")), align_resolution=3)


def test_global_loss_batch_equals_stack_and_repeats_bit_for_bit():
    m = M()
    rng = np.random.default_rng(22)
    pred_np, gt_np = R.scene(rng, 3, 19, 70, noise=0.1)
    gt_np[1, 3:6, 10:30] = np.nan

    def run(p_np, g_np):
        p = to_dev(p_np).requires_grad_()
        loss, misc, scale = m.affine_invariant_global_loss(p, to_dev(g_np), align_resolution=6, beta=0.01, trunc=0.05, sparsity_aware=True)
        g, = torch.autograd.grad(loss.sum(), p)
        return [t.detach().cpu().numpy() for t in (loss, misc["truncated_error"], misc["delta"], scale, g)]

    full, again = run(pred_np, gt_np), run(pred_np, gt_np)
    assert all(np.array_equal(a, b) for a, b in zip(full, again))
    for i in range(3):
        one = run(pred_np[i:i + 1], gt_np[i:i + 1])
        assert all(np.array_equal(a[0], b[i]) for a, b in zip(one, full)), i
    single = run(pred_np[0], gt_np[0])                               # no batch dims: 0-d results
    assert single[0].shape == () and all(np.array_equal(a, b[0]) for a, b in zip(single, full))


# ---- affine_invariant_local_loss ----------------------------------------------------------------------------------------------------------
def local_config(z, case):
    return dict(level=int(z[case + "_level"]), align_resolution=int(z[case + "_align_resolution"]), num_patches=int(z[case + "_num_patches"]),
                beta=float(z[case + "_beta"]), trunc=float(z[case + "_trunc"]), sparsity_aware=bool(z[case + "_sparsity_aware"]))


def local_anchors(ai, aj):
    """(B, n) anchor arrays -> the (patch_image, patch_i, patch_j) the mirror takes"""
    B, n = ai.shape
    return to_dev(np.repeat(np.arange(B), n).astype(np.int64)), to_dev(ai.reshape(-1).astype(np.int64)), to_dev(aj.reshape(-1).astype(np.int64))


def local_gate(name, loss, misc, grad, v, has_patch):
    none = np.zeros((loss.shape[0], 1))
    gate(name + " loss", loss, grad, v["loss_f32"], v["loss_f64"], v["grad_f32"], v["grad_f64"])
    for key, mk in (("te", "truncated_error"), ("delta", "delta")):
        got = misc[mk].cpu().double().numpy()
        gate(f"{name} {key}", got[has_patch], none[has_patch], v[key + "_f32"][has_patch], v[key + "_f64"][has_patch], none[has_patch], none[has_patch])
        assert (got[~has_patch] == 0).all()


@pytest.mark.parametrize("case", ["c0", "c1", "c2"])
def test_local_loss_parity_with_the_reference(case):
    m = M()
    from moge_amd import alignment as A
    z = np.load(os.path.join(GOLDEN, "losses_local_b2_24x40.npz"))
    cfg = local_config(z, case)
    v = {k[len(case) + 1:]: z[k] for k in z.files if k.startswith(case + "_")}
    pred, gt, focal = to_dev(z["points"]).requires_grad_(), to_dev(z["gt_points"]), to_dev(v["focal"])
    gs = None if np.isnan(v["global_scale"]).all() else to_dev(v["global_scale"])
    anchors = local_anchors(v["anchor_i"], v["anchor_j"])
    has_patch = np.array([(v["patch_image"] == b).any() for b in range(2)])
    # the patches: the fixture's non-empty ones, in (image, anchor row) order; `order` maps them back to the fixture's
    patches = m.local_patches(gt, focal, anchors, cfg["level"], cfg["align_resolution"])
    order = patches["order"].cpu().numpy()
    assert len(order) == len(v["patch_image"]) and patches["mask"].shape[1:] == (13, 13)
    kept_sorted = np.sort(order)
    fixture_of = {int(o): k for k, o in enumerate(kept_sorted)}
    idx = np.array([fixture_of[int(o)] for o in order])
    assert (v["patch_image"][idx] == patches["image"].cpu().numpy()).all()
    # 1. the fused patch L1 apart from the solve: the line through the fixture's selected samples of every patch (differentiable)
    image = patches["image"].long()[:, None]
    src, tgt = pred[image, patches["rows"], patches["cols"]], gt[image, patches["rows"], patches["cols"]]
    tgt = torch.where(torch.isfinite(tgt).all(-1, keepdim=True), tgt, torch.ones_like(tgt))
    lines = [R.scale_xyz_shift(src[k], tgt[k], *(int(x) for x in v["selection"][idx[k]])) for k in range(len(idx))]
    scale, shift = torch.stack([l[0] for l in lines]), torch.stack([l[1] for l in lines])
    gate(f"local {case} patch scales", scale.detach().cpu().double().numpy(), np.zeros((len(idx), 1)), v["patch_scale_f32"][idx], v["patch_scale_f64"][idx],
         np.zeros((len(idx), 1)), np.zeros((len(idx), 1)))
    if gs is not None:
        ratio = scale.detach() / gs[image[:, 0]]
        ok = (ratio > 0.1) & (ratio < 10) & (gs[image[:, 0]] > 0)
    else:
        ok = scale > 0
    scale, shift = torch.where(ok, scale, torch.zeros_like(scale)), torch.where(ok[:, None], shift, torch.zeros_like(shift))
    loss, misc = m.local_patch_loss(pred, gt, patches, scale, shift, cfg["num_patches"], cfg["beta"], cfg["sparsity_aware"])
    grad, = torch.autograd.grad(loss.sum(), pred)
    local_gate(f"local {case} fused", loss.detach().cpu().double().numpy(), {"truncated_error": misc[:, 0], "delta": misc[:, 1]}, grad.cpu().double().numpy(), v, has_patch)
    # 2. end to end through the HIP solve: it selects the fixture's samples (hard assert), then the same gates
    w = patches["lr_mask"].float() / (patches["radius"][:, None] + 1e-7)
    k, i2 = A._anchor_search(src.detach().contiguous(), tgt.contiguous(), w.contiguous(), 0b111, cfg["trunc"])
    for q in range(len(idx)):
        want = tuple(int(x) for x in v["selection"][idx[q]])
        mirror = (want[1] // 3, 3 * want[0] + want[1] % 3)                     # anchor and solution sample swapped: the same line
        assert (int(k[q]), int(i2[q])) in (want, mirror), (q, int(k[q]), int(i2[q]), want)
    cfg2 = dict(cfg)
    level = cfg2.pop("level")
    loss, misc = m.affine_invariant_local_loss(pred, gt, focal, gs, level, anchors=anchors, **cfg2)
    grad, = torch.autograd.grad(loss.sum(), pred)
    local_gate(f"local {case} end to end", loss.detach().cpu().double().numpy(), misc, grad.cpu().double().numpy(), v, has_patch)


def local_against_restatement(m, pred_np, gt_np, focal, gscale, ai, aj, name, **cfg):
    """the restatement is handed the samples the HIP solve selected (the solvers have their own tests)"""
    from moge_amd import alignment as A
    B = pred_np.shape[0]
    pred, gt, fo = to_dev(pred_np).requires_grad_(), to_dev(gt_np), to_dev(np.array(focal, np.float32))
    gs = None if gscale is None else to_dev(np.array(gscale, np.float32))
    anchors = local_anchors(ai, aj)
    level = cfg.pop("level")
    out = m.affine_invariant_local_loss(pred, gt, fo, gs, level, anchors=anchors, **cfg)
    patches = m.local_patches(gt, fo, anchors, level, cfg["align_resolution"])
    sel = {}
    if patches["image"].numel():
        image = patches["image"].long()[:, None]
        src, tgt = pred.detach()[image, patches["rows"], patches["cols"]], gt[image, patches["rows"], patches["cols"]]
        tgt = torch.where(torch.isfinite(tgt).all(-1, keepdim=True), tgt, torch.ones_like(tgt))
        k, i2 = A._anchor_search(src.contiguous(), tgt.contiguous(), (patches["lr_mask"].float() / (patches["radius"][:, None] + 1e-7)).contiguous(), 0b111, cfg["trunc"])
        sel = {int(o): (int(a), int(b_)) for o, a, b_ in zip(patches["order"], k, i2)}
    else:
        assert out[1] == {} and not out[0].any()
        return
    loss, misc = out
    grad, = torch.autograd.grad(loss.sum(), pred)
    n = ai.shape[1]
    ref = {}
    has_patch = np.array([any(b * n + a in sel for a in range(n)) for b in range(B)])
    for tag, dtype in (("f32", torch.float32), ("f64", torch.float64)):
        rows = []
        for b in range(B):
            p = torch.from_numpy(pred_np[b]).to(dtype).requires_grad_()
            selections = [sel[b * n + a] for a in range(n) if b * n + a in sel]
            l, te, dl = R.affine_invariant_local_loss(p, torch.from_numpy(gt_np[b]).to(dtype), float(focal[b]), None if gscale is None else float(gscale[b]), level,
                                                      (ai[b], aj[b]), selections=selections, **cfg)
            g = torch.autograd.grad(l, p)[0] if l.requires_grad else torch.zeros_like(p)
            rows.append([np.asarray(0.0 if x is None else x.detach().double().numpy()) for x in (l, te, dl)] + [g.double().numpy()])
        for i, key in enumerate(("loss", "te", "delta", "grad")):
            ref[f"{key}_{tag}"] = np.stack([r[i] for r in rows])
    local_gate(name, loss.detach().cpu().double().numpy(), misc, grad.cpu().double().numpy(), ref, has_patch)


def test_local_loss_at_edge_shapes():
    m = M()
    rng = np.random.default_rng(31)
    # level 4 at 5 x 7: radius 2, 5 x 5 windows of at most 25 points, so EVERY patch is empty and what is checked is the (0, {}) return and that the clamped
    # window reads stay in bounds - no arithmetic is compared here; the parity case for windows that span the whole image is 9 x 11 below
    pred, gt = R.scene(rng, 1, 5, 7, noise=0.05)
    local_against_restatement(m, pred, gt, [0.3], None, np.array([[0, 2, 4, 2]]), np.array([[0, 3, 6, 0]]), "local 5x7", level=4, align_resolution=3, num_patches=4,
                              beta=0.0, trunc=1.0, sparsity_aware=False)
    # level 2 at 9 x 11: radius 4, 9 x 9 windows covering the whole height, anchors on corners and edges
    pred, gt = R.scene(rng, 1, 9, 11, noise=0.05)
    gt[0, 4, 5] = np.nan
    local_against_restatement(m, pred, gt, [0.2], None, np.array([[0, 8, 4, 0]]), np.array([[0, 10, 5, 10]]), "local 9x11", level=2, align_resolution=4, num_patches=4,
                              beta=0.01, trunc=0.1, sparsity_aware=True)
    # B = 3 with one instance without a non-empty patch (its focal makes every radius tiny), global_scale given
    pred, gt = R.scene(rng, 3, 19, 33, noise=0.05)
    gt[2, :3, :9] = np.inf
    ai, aj = rng.integers(0, 19, (3, 5)), rng.integers(0, 33, (3, 5))
    local_against_restatement(m, pred, gt, [0.4, 1e4, 0.5], [1.0, 1.0, 2.0], ai, aj, "local B=3, one empty", level=4, align_resolution=5, num_patches=5, beta=0.0,
                              trunc=0.2, sparsity_aware=True)


def test_local_loss_overlapping_anchors_repeat_and_batch_equals_stack():
    """the same anchor four times and neighbours one pixel apart: the per-pixel sums of the backward meet many patches"""
    m = M()
    rng = np.random.default_rng(32)
    pred_np, gt_np = R.scene(rng, 2, 24, 40, noise=0.05)
    ai = np.array([[12, 12, 12, 12, 12, 13, 11, 12], [5, 5, 6, 20, 20, 20, 21, 23]])
    aj = np.array([[20, 20, 20, 20, 21, 20, 20, 19], [7, 8, 7, 30, 30, 31, 30, 39]])
    focal = np.array([0.45, 0.5], np.float32)

    def run(sl):
        p = to_dev(pred_np[sl]).requires_grad_()
        loss, misc = m.affine_invariant_local_loss(p, to_dev(gt_np[sl]), to_dev(focal[sl]), None, 4, align_resolution=6, num_patches=8, beta=0.01, trunc=0.2,
                                                   sparsity_aware=True, anchors=local_anchors(ai[sl], aj[sl]))
        g, = torch.autograd.grad(loss.sum(), p)
        return [t.detach().cpu().numpy() for t in (loss, misc["truncated_error"], misc["delta"], g)]

    full, again = run(slice(0, 2)), run(slice(0, 2))
    assert full[0].all() and all(np.array_equal(a, b) for a, b in zip(full, again))
    for i in range(2):
        one = run(slice(i, i + 1))
        assert all(np.array_equal(a[0], b[i]) for a, b in zip(one, full)), i


def test_local_loss_samples_its_own_anchors_on_valid_pixels():
    m = M()
    rng = np.random.default_rng(33)
    pred_np, gt_np = R.scene(rng, 2, 24, 40, noise=0.05)
    gt_np[0, :, :15] = np.nan
    pred, gt, focal = to_dev(pred_np).requires_grad_(), to_dev(gt_np), to_dev(np.array([0.45, 0.5], np.float32))
    drawn = []
    real = m.local_patches
    m.local_patches = lambda g, f, anchors, *a: drawn.append(anchors) or real(g, f, anchors, *a)
    try:
        gen = torch.Generator(device=DEV).manual_seed(3)
        loss, misc = m.affine_invariant_local_loss(pred, gt, focal, None, 4, align_resolution=6, num_patches=16, generator=gen)
        loss2, _ = m.affine_invariant_local_loss(pred, gt, focal, None, 4, align_resolution=6, num_patches=16, generator=torch.Generator(device=DEV).manual_seed(3))
    finally:
        m.local_patches = real
    g, = torch.autograd.grad(loss.sum(), pred)
    assert torch.isfinite(loss).all() and torch.isfinite(g).all() and torch.isfinite(misc["delta"]).all() and torch.equal(loss, loss2)
    pb, pi, pj = drawn[0]
    assert pb.shape == (2, 16) and torch.isfinite(gt[pb, pi, pj]).all() and (pj[0] >= 15).all()


def test_local_loss_clamps_out_of_range_anchors_in_forward_and_backward_alike():
    m = M()
    rng = np.random.default_rng(34)
    pred_np, gt_np = R.scene(rng, 2, 24, 40, noise=0.05)
    focal = to_dev(np.array([0.45, 0.5], np.float32))

    def run(pb, pi, pj):
        p = to_dev(pred_np).requires_grad_()
        loss, _ = m.affine_invariant_local_loss(p, to_dev(gt_np), focal, None, 4, align_resolution=6, num_patches=3,
                                                anchors=tuple(to_dev(np.array(a, np.int64)) for a in (pb, pi, pj)))
        g, = torch.autograd.grad(loss.sum(), p)
        return loss.detach().cpu().numpy(), g.cpu().numpy()

    wild = run([0, 0, 5, 1, -2, 1], [-7, 12, 12, 100, 3, 10], [20, 90, -1, 20, 8, 45])
    tame = run([0, 0, 1, 1, 0, 1], [0, 12, 12, 23, 3, 10], [20, 39, 0, 20, 8, 39])
    assert wild[0].all() and np.array_equal(wild[0], tame[0]) and np.array_equal(wild[1], tame[1])
