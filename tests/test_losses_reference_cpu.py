"""CPU: tests/losses_reference.py, the project's own restatement of the training losses, against the goldens of the unmodified reference
(tests/golden/losses_*.npz, tools/make_losses_golden.py): values and autograd gradients, per instance and batched.  In float64 the two agree to
rounding (different expression order); in float32 the restatement sits inside the gate the GPU tests apply to the kernels."""
import os

import numpy as np
import pytest
import torch

import losses_reference as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
EPS32 = 2.0 ** -23
STENCIL = ["losses_stencil_b2_24x40", "losses_stencil_33x65"]
CASES = [(f, k, fn, ("points", "gt_points")) for f in STENCIL for k, fn in (("normal", R.normal_loss), ("edge", R.edge_loss))] + [
    ("losses_pixel_b2_24x40", "mask_l2", R.mask_l2_loss, ("pred_mask", "gt_mask_pos", "gt_mask_neg")),
    ("losses_pixel_b2_24x40", "mask_bce", R.mask_bce_loss, ("pred_mask_prob", "gt_mask_pos", "gt_mask_neg")),
    ("losses_pixel_b2_24x40", "normal_map", R.normal_map_loss, ("pred_normal", "gt_normal")),
    ("losses_pixel_b2_24x40", "metric_scale", R.metric_scale_loss, ("scale_pred", "scale_gt")),
]


def restated(fn, dtype, arrays):
    args = [torch.from_numpy(a).to(dtype) if a.dtype.kind == "f" else torch.from_numpy(a) for a in arrays]
    args[0].requires_grad_()
    loss = fn(*args)
    g, = torch.autograd.grad(loss.sum(), args[0])
    return loss.detach().double().numpy(), g.double().numpy()


@pytest.mark.parametrize("fixture,key,fn,inputs", CASES, ids=[f"{c[0]}-{c[1]}" for c in CASES])
def test_restatement_matches_the_reference(fixture, key, fn, inputs):
    z = np.load(os.path.join(GOLDEN, fixture + ".npz"))
    arrays = [z[k] for k in inputs]
    v64, g64 = z[key + "_f64"], z[key + "_grad_f64"]
    v, g = restated(fn, torch.float64, arrays)                     # a batch at once: result[i] = the reference called on instance i
    assert v.shape == v64.shape and np.abs(v - v64).max() <= 1e-13 * np.abs(v64).max()
    assert g.shape == g64.shape and np.abs(g - g64).max() <= 1e-12 * np.abs(g64).max()
    v32, g32 = restated(fn, torch.float32, arrays)
    rv, rg = z[key + "_f32"].astype(np.float64), z[key + "_grad_f32"].astype(np.float64)
    assert (np.abs(v32 - v64) <= np.maximum(4 * np.abs(rv - v64), 8 * EPS32 * np.abs(v64))).all()
    for i in range(g64.shape[0]):
        assert np.abs(g32[i] - g64[i]).max() <= max(4 * np.abs(rg[i] - g64[i]).max(), 8 * EPS32 * np.abs(g64[i]).max())


@pytest.mark.parametrize("fixture", STENCIL)
def test_stencil_fixtures_take_every_branch(fixture):
    """what makes the fixtures worth comparing against: non-finite gt, and terms below the clamp, on the quadratic and on the linear piece"""
    z = np.load(os.path.join(GOLDEN, fixture + ".npz"))
    p, g = torch.from_numpy(z["points"]).double(), torch.from_numpy(z["gt_points"]).double()
    assert np.isinf(z["gt_points"]).any() and np.isnan(z["gt_points"]).any()
    for fn, lo in ((R.normal_angles, R.NORMAL_MIN), (R.edge_angles, R.EDGE_MIN)):
        a = torch.cat([x[m] for x, m in fn(p, g)])
        assert ((a - lo).abs() > 1e-4).all() and ((a - R.BETA).abs() > 1e-4).all() and ((a - R.ANGLE_MAX).abs() > 1e-4).all()
        assert (a < R.BETA).any() and ((a > R.BETA) & (a < R.ANGLE_MAX)).any()
        assert not all(m.all() for _, m in fn(p, g))


def test_in_window_fraction_counts_the_window():
    pts = torch.zeros(3, 4, 3)
    mask = torch.ones(3, 4, dtype=torch.bool)
    mask[0, 0] = False
    p = R.in_window_fraction(pts, mask, 1, torch.ones(3, 4))
    assert p[0, 0] == 0 and p[1, 1] == 8 / 9 and p[2, 3] == 4 / 9 and p[1, 2] == 1
    assert R.in_window_fraction(pts, mask, 1, -torch.ones(3, 4)).sum() == 0


GLOBAL = ["losses_global_b2_24x40", "losses_global_33x65"]


@pytest.mark.parametrize("fixture", GLOBAL)
@pytest.mark.parametrize("case", ["c0", "c1"])
def test_global_loss_restatement_matches_the_reference(fixture, case):
    """the restated solve selects the fixture's samples, and the loss, misc values, scale and full gradient (direct term + the path through scale
    and shift) are the reference's"""
    z = np.load(os.path.join(GOLDEN, fixture + ".npz"))
    cfg = dict(align_resolution=int(z[case + "_align_resolution"]), beta=float(z[case + "_beta"]), trunc=float(z[case + "_trunc"]),
               sparsity_aware=bool(z[case + "_sparsity_aware"]))
    for b in range(z["points"].shape[0]):
        sel = R.global_selection(z["points"][b], z["gt_points"][b], (cfg["align_resolution"],) * 2, cfg["trunc"])
        assert sel == tuple(z[case + "_selection"][b])
        for tag, dtype, tol in (("f64", torch.float64, 1e-12), ("f32", torch.float32, 2e-5)):
            p = torch.from_numpy(z["points"][b]).to(dtype).requires_grad_()
            loss, te, delta, scale = R.affine_invariant_global_loss(p, torch.from_numpy(z["gt_points"][b]).to(dtype), **cfg)
            g, = torch.autograd.grad(loss, p)
            for got, key in ((loss, "loss"), (te, "te"), (delta, "delta"), (scale, "scale")):
                want = float(z[f"{case}_{key}_{tag}"][b])
                # float32 also in the reference's float64 run: `(err < 1).float()` (losses.py:66) and the sparsity ratio of `.float()` means (:58)
                lim = max(tol, 2e-7) if key == "delta" or (key == "loss" and cfg["sparsity_aware"]) else tol
                assert abs(float(got.detach()) - want) <= lim * abs(want), (key, tag, float(got.detach()), want)
            want = z[f"{case}_grad_{tag}"][b].astype(np.float64)
            assert np.abs(g.double().numpy() - want).max() <= (max(tol, 2e-7) if cfg["sparsity_aware"] else 10 * tol) * np.abs(want).max(), tag


def test_global_fixtures_take_every_branch():
    z = np.load(os.path.join(GOLDEN, GLOBAL[0] + ".npz"))
    gt, mask = R.clean(torch.from_numpy(z["gt_points"]).double())
    assert not mask.all()
    w0 = mask / gt[..., 2].clamp_min(1e-5)
    cap = 10 * (w0 * mask).mean(dim=(-2, -1)) / (mask.double().mean(dim=(-2, -1)) + 1e-7)
    assert (w0 > cap[:, None, None]).any()                               # the weight clamp bites somewhere
    assert 0 < z["c1_delta_f64"].min() and z["c1_delta_f64"].max() < 1          # err < 1 on both sides
    assert float(z["c1_beta"]) > 0 and float(z["c0_beta"]) == 0 and bool(z["c1_sparsity_aware"]) and not bool(z["c0_sparsity_aware"])
    assert (z["c1_shift_f64"][:, :2] == 0).all() and (z["c1_scale_f64"] > 0).all()


@pytest.mark.parametrize("case", ["c0", "c1", "c2"])
def test_local_loss_restatement_matches_the_reference(case):
    """level 4 at 24 x 40: 13 x 13 windows with anchors on a corner and on an edge, global_scale None (c0, c2) and given (c1), an image whose every
    patch is below 32 points (c2, image 1); the restated solve selects the fixture's samples"""
    z = np.load(os.path.join(GOLDEN, "losses_local_b2_24x40.npz"))
    cfg = dict(align_resolution=int(z[case + "_align_resolution"]), num_patches=int(z[case + "_num_patches"]), beta=float(z[case + "_beta"]),
               trunc=float(z[case + "_trunc"]), sparsity_aware=bool(z[case + "_sparsity_aware"]))
    H, W = z["points"].shape[1:3]
    assert (H - 1, W - 1) in zip(z[case + "_anchor_i"][0], z[case + "_anchor_j"][0]) and 0 in z[case + "_anchor_i"][0]
    for b in range(2):
        gs = None if np.isnan(z[case + "_global_scale"][b]) else float(z[case + "_global_scale"][b])
        want_sel = [tuple(s) for s, o in zip(z[case + "_selection"], z[case + "_patch_image"]) if o == b]
        for tag, dtype, tol in (("f64", torch.float64, 1e-11), ("f32", torch.float32, 3e-5)):
            p = torch.from_numpy(z["points"][b]).to(dtype).requires_grad_()
            d = {}
            loss, te, delta = R.affine_invariant_local_loss(p, torch.from_numpy(z["gt_points"][b]).to(dtype), float(z[case + "_focal"][b]), gs, int(z[case + "_level"]),
                                                            (z[case + "_anchor_i"][b], z[case + "_anchor_j"][b]), diag=d, **cfg)
            assert [tuple(s) for s in d.get("selection", [])] == want_sel
            want = float(z[f"{case}_loss_{tag}"][b])
            lim = max(tol, 2e-7) if cfg["sparsity_aware"] else tol       # the reference's sparsity ratio is float32 in its float64 run too
            assert abs(float(loss.detach()) - want) <= lim * abs(want)
            if not want_sel:
                assert te is None and want == 0
                continue
            assert abs(float(te) - float(z[f"{case}_te_{tag}"][b])) <= max(tol, 2e-7) and abs(float(delta) - float(z[f"{case}_delta_{tag}"][b])) <= max(tol, 2e-7)
            g, = torch.autograd.grad(loss, p)
            wg = z[f"{case}_grad_{tag}"][b].astype(np.float64)
            assert np.abs(g.double().numpy() - wg).max() <= 10 * lim * np.abs(wg).max()
