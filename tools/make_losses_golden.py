"""Golden fixtures of the training losses (tests/golden/losses_*.npz) from the reference's unmodified `moge/train/losses.py`, run on the CPU.

    python tools/make_losses_golden.py          (build machine: needs the reference checkout of oracle/make_golden.py)

Each fixture holds float32 inputs and, for every loss, the reference's value and its autograd gradient for the prediction, computed twice on
those same inputs: in float32 (`*_f32`) and in float64 (`*_f64`).  The reference is called per instance, as its train.py does, and the
results are stacked.  `utils3d.pt.angle_between`, which is not vendored, is handed to the reference as the stub atan2(|a x b|, a . b)
(UNPINNED).

The maker ASSERTS the fixture conditions and re-seeds a scene until they hold, so that no element has to be left out of any comparison: the
float32 and the float64 run take the same branch at every angle clamp (MIN_ANGLE, MAX_ANGLE) and at the BETA_RAD switch of `_smooth`, and no
angle lies within 1e-4 rad of such a boundary."""
from __future__ import annotations

import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

from oracle.make_golden import GOLDEN_DIR, install_stubs                 # noqa: E402
import losses_reference as R                                             # noqa: E402  (the scene and the angle helpers of the condition check)

MARGIN = 1e-4
MAX_TRIES = 2000
LOCAL_TRIES = 400
MIN_LOCAL_MARGIN = 1e-3      # every patch solve's best candidate leads its runner-up by this much, relative (recorded as c*_margin)


def save(name, **arrays):
    path = os.path.join(GOLDEN_DIR, name + ".npz")
    np.savez_compressed(path, **arrays)
    print(name, os.path.getsize(path), "bytes", {k: v.shape for k, v in arrays.items()})


def branches_hold(pred, gt):
    """the fixture conditions of normal_loss and edge_loss on one scene"""
    for fn, lo in ((R.normal_angles, R.NORMAL_MIN), (R.edge_angles, R.EDGE_MIN)):
        a32, a64 = fn(torch.from_numpy(pred), torch.from_numpy(gt)), fn(torch.from_numpy(pred).double(), torch.from_numpy(gt).double())
        for (x32, m), (x64, _) in zip(a32, a64):
            for bound in (lo, R.BETA, R.ANGLE_MAX):
                d32, d64 = x32[m].double() - bound, x64[m] - bound
                if (d64.abs() <= MARGIN).any() or (d32.abs() <= MARGIN).any() or ((d32 > 0) != (d64 > 0)).any():
                    return False
    return True


def stencil_scene(seed, B, H, W):
    for k in range(MAX_TRIES):
        rng = np.random.default_rng(seed + k)
        pred, gt = R.scene(rng, B, H, W)
        gt[0, :4, :5] = np.inf                                    # an inf corner block
        gt[B - 1, H // 2, W // 3, 1] = np.nan                      # a lone NaN
        if branches_hold(pred, gt):
            print(f"  {B} x {H} x {W}: seed {seed + k} after {k} re-seeds")
            return pred, gt, seed + k
    raise AssertionError("no scene met the fixture conditions")


def run(fn, dtype, pred, *rest):
    """the reference's fn per instance -> (values (B, ...), gradient of their sum for pred)"""
    vals, grads = [], []
    for i in range(pred.shape[0]):
        p = torch.from_numpy(pred[i]).to(dtype).requires_grad_()
        args = [torch.from_numpy(r[i]).to(dtype) if r.dtype.kind == "f" else torch.from_numpy(r[i]) for r in rest]
        loss, misc = fn(p, *args)
        assert misc == {}
        g, = torch.autograd.grad(loss.sum(), p)
        vals.append(loss.detach().numpy())
        grads.append(g.numpy())
    return np.stack(vals), np.stack(grads)


def both(out, key, fn, pred, *rest):
    for tag, dtype in (("f32", torch.float32), ("f64", torch.float64)):
        out[f"{key}_{tag}"], out[f"{key}_grad_{tag}"] = run(fn, dtype, pred, *rest)
    assert np.isfinite(out[f"{key}_f64"]).all() and np.isfinite(out[f"{key}_grad_f64"]).all(), key


def runner_up_gap(pred, gt, size, trunc):
    """the truncated objective's best candidate against the runner-up, relative, over every (anchor, extremum) pair of the scale / z-shift solve of
    ONE image; the pair that is the best line's own mirror image (anchor and solution sample swapped: the same line) is not a rival"""
    import alignment_trunc_reference as AT
    lm, rows, cols = R.global_samples(gt, size)
    src, tgt = pred[rows, cols], np.where(np.isfinite(gt).all(-1, keepdims=True), gt, 1)[rows, cols].astype(np.float32)
    w = (lm / np.maximum(tgt[:, 2], 1e-2)).astype(np.float32)
    k, i2 = R.global_selection(pred, gt, size, trunc)
    m = np.array([0, 0, 1], np.float32)
    cands = []
    for a in np.nonzero(w > 0)[0]:
        x, y, ww = (src - src[a] * m).reshape(1, -1), (tgt - tgt[a] * m).reshape(1, -1), np.repeat(w, 3)[None]
        xs, ys, ws, wx, wy, A, B, C = AT.keys(x, y, ww, trunc)
        for e in np.nonzero(AT.extrema(A[0], B[0], C[0], wx[0]))[0]:
            cands.append((float(AT.objective(A[0][e], xs[0], ys[0], ws[0], trunc)), int(a), int(e)))
    best = min(c[0] for c in cands if (c[1], c[2]) == (k, i2))
    mirror = (i2 // 3, 3 * k + 2) if i2 % 3 == 2 else None
    rival = min(c[0] for c in cands if (c[1], c[2]) != (k, i2) and (c[1], c[2]) != mirror)
    return (rival - best) / best, (k, i2)


def global_case(REF, captured, pred, gt, res, beta, trunc, sparse):
    """the reference's global loss per instance in float32 and float64 (+ the fixture conditions) -> dict of arrays"""
    out, B = {}, pred.shape[0]
    sel = []
    for b in range(B):
        gap, ki = runner_up_gap(pred[b], gt[b], (res, res), trunc)
        assert gap > 1e-3, f"the solve's best candidate leads by {gap:.2e} only"
        sel.append(ki)
    out["selection"] = np.array(sel, np.int64)
    for tag, dtype in (("f32", torch.float32), ("f64", torch.float64)):
        rows = {k: [] for k in ("loss", "te", "delta", "scale", "shift", "grad")}
        for b in range(B):
            p = torch.from_numpy(pred[b]).to(dtype).requires_grad_()
            captured.clear()
            loss, misc, scale = REF.affine_invariant_global_loss(p, torch.from_numpy(gt[b]).to(dtype), align_resolution=res, beta=beta, trunc=trunc, sparsity_aware=sparse)
            g, = torch.autograd.grad(loss, p)
            assert scale > 0 and len(captured) == 1
            for k, v in zip(rows, (loss.detach().numpy(), misc["truncated_error"], misc["delta"], scale.numpy(), captured[0][1].detach().numpy(), g.numpy())):
                rows[k].append(np.asarray(v))
            # the restated line through the selected samples is the reference's
            gtc = R.clean(torch.from_numpy(gt[b]).to(dtype))[0]
            lm, rr, cc = R.global_samples(gt[b], (res, res))
            s, t = R.scale_z_shift(p.detach()[rr, cc], gtc[rr, cc], *sel[b])
            tol = 1e-12 if dtype == torch.float64 else 1e-5
            assert abs(float(s) - float(scale)) <= tol * abs(float(scale)), (float(s), float(scale), tag)
            # no element on a branch boundary: the weight clamp, the beta switch, err < 1
            mask = torch.from_numpy(np.isfinite(gt[b]).all(-1))
            w0 = mask.to(dtype) / gtc[..., 2].clamp_min(1e-5)
            cap = 10 * (w0 * mask).mean() / (mask.to(dtype).mean() + 1e-7)
            diff = scale * p.detach() + captured[0][1].detach() - gtc
            e = (diff.abs() * torch.minimum(w0, cap)[..., None])[mask]
            err = (diff.norm(dim=-1) / gtc[..., 2])[mask]
            assert ((w0[mask] / cap - 1).abs() > MARGIN).all() and ((err - 1).abs() > MARGIN).all() and (beta == 0 or ((e / beta - 1).abs() > MARGIN).all())
            rows.setdefault("branch", []).append(np.concatenate([(w0[mask] > cap).numpy().ravel(), (err < 1).numpy().ravel(), (e < beta).numpy().ravel()]))
        for k, v in rows.items():
            out[f"{k}_{tag}"] = np.concatenate(v) if k == "branch" else np.stack(v)
    assert np.array_equal(out.pop("branch_f32"), out.pop("branch_f64")), "the float32 and the float64 run take different branches"
    out.update(align_resolution=np.int64(res), beta=np.float64(beta), trunc=np.float64(trunc), sparsity_aware=np.bool_(sparse))
    return out


def _batched_nearest_resize(*image, mask, size, return_index=False):
    """utils3d.pt.masked_nearest_resize for a batch of (P, S, S) masks: the project's convention per patch"""
    from tools.make_metrics_golden import masked_nearest_resize_np
    if mask.dim() == 2:
        from tools.make_metrics_golden import _stub_masked_nearest_resize
        return _stub_masked_nearest_resize(*image, mask=mask, size=size, return_index=return_index)
    outs = [[] for _ in image] + [[]]
    for p in range(mask.shape[0]):
        lm, r, c = masked_nearest_resize_np(mask[p].numpy().astype(bool), size)
        rows, cols = torch.from_numpy(r), torch.from_numpy(c)
        for o, im in zip(outs, image):
            o.append(im[p][rows, cols])
        outs[-1].append(torch.from_numpy(lm))
    return tuple(torch.stack(o) for o in outs)


def patch_margin(src, tgt, w, trunc, sel):
    """one patch's scale / xyz-shift solve: how far, relative, the best candidate leads the runner-up over every (anchor, extremum) pair; the best line's
    mirror image (anchor and solution sample swapped) is the same line and no rival"""
    import alignment_trunc_reference as AT
    k, i2 = sel
    cands = []
    for a in np.nonzero(w > 0)[0]:
        x, y, ww = (src - src[a]).reshape(1, -1), (tgt - tgt[a]).reshape(1, -1), np.repeat(w, 3)[None]
        xs, ys, ws, wx, wy, A, B, C = AT.keys(x, y, ww, trunc)
        for e in np.nonzero(AT.extrema(A[0], B[0], C[0], wx[0]))[0]:
            cands.append((float(AT.objective(A[0][e], xs[0], ys[0], ws[0], trunc)), int(a), int(e)))
    best = min(c[0] for c in cands if (c[1], c[2]) == (k, i2))
    rivals = [c[0] for c in cands if (c[1], c[2]) not in ((k, i2), (i2 // 3, 3 * k + i2 % 3))]
    return (min(rivals) - best) / best if rivals else np.inf


def local_case(REF, captured, forced, pred, gt, focal, gscale, level, res, npatch, beta, trunc, sparse):
    """the reference's local loss per instance in float32 and float64 with the same anchors (+ the fixture conditions) -> dict of arrays"""
    import alignment_trunc_reference as AT
    out, B = {}, pred.shape[0]
    anchors, per_patch = [], {"f32": [], "f64": []}
    diags = {}
    for tag, dtype in (("f32", torch.float32), ("f64", torch.float64)):
        rows = {k: [] for k in ("loss", "te", "delta", "grad")}
        for b in range(B):
            p = torch.from_numpy(pred[b]).to(dtype).requires_grad_()
            captured.clear()
            forced["anchors"] = anchors[b] if tag == "f64" else None
            forced["corner"] = [(pred.shape[1] - 1, pred.shape[2] - 1), (0, pred.shape[2] // 2)]
            gs = None if gscale is None else torch.tensor([gscale[b]], dtype=dtype)
            loss, misc = REF.affine_invariant_local_loss(p, torch.from_numpy(gt[b]).to(dtype), torch.tensor([focal[b]], dtype=dtype), gs, level, align_resolution=res,
                                                         num_patches=npatch, beta=beta, trunc=trunc, sparsity_aware=sparse)
            if tag == "f32":
                anchors.append(forced["used"])
            g = torch.autograd.grad(loss, p)[0].numpy() if loss.requires_grad else np.zeros(pred[b].shape)
            for k, v in zip(rows, (loss.detach().numpy(), misc.get("truncated_error", np.nan), misc.get("delta", np.nan), g)):
                rows[k].append(np.asarray(v, np.float64 if k != "grad" else g.dtype))
            per_patch[tag].append([(s.detach().numpy(), t.detach().numpy()) for s, t in captured])
            # the restatement on the same anchors: conditions, and the selection it makes
            d = {}
            ai, aj = anchors[b]
            R.affine_invariant_local_loss(p.detach(), torch.from_numpy(gt[b]).to(dtype), focal[b], None if gscale is None else gscale[b], level, (ai, aj), res, npatch, beta,
                                          trunc, sparse, diag=d, selections=diags[("f32", b)].get("selection") if tag == "f64" else None)
            diags[(tag, b)] = d
        for k, v in rows.items():
            out[f"{k}_{tag}"] = np.stack(v)
    sel, sc32, sc64, sh32, sh64, owner, margins = [], [], [], [], [], [], []
    for b in range(B):
        d32, d64 = diags[("f32", b)], diags[("f64", b)]
        assert d32.get("count") == d64.get("count") and d32.get("valid") == d64.get("valid"), "patch counts or patch_valid differ between float32 and float64"
        n = len(d32.get("count", []))
        assert len(per_patch["f32"][b]) == len(per_patch["f64"][b]) == (1 if n else 0)
        for r32, r64 in zip(d32.get("ratios", []), d64.get("ratios", [])):
            assert ((r64 - 1).abs() > MARGIN).all() and ((r32 - 1).abs() > MARGIN).all() and ((r32 > 1) == (r64 > 1)).all(), "an element sits on a branch boundary"
        if n:
            (s32, t32), (s64, t64) = per_patch["f32"][b][0], per_patch["f64"][b][0]
            assert np.allclose(d64["scale"], s64, rtol=1e-10, atol=0) and np.allclose(d32["scale"], s32, rtol=1e-4, atol=0), "the restated solve is not the reference's"
            margins += [patch_margin(*smp, trunc, ki) for smp, ki in zip(d32["samples"], d32["selection"])]
            sel += d32["selection"]; sc32 += list(s32); sc64 += list(s64); sh32 += list(t32); sh64 += list(t64); owner += [b] * n
    assert min(margins, default=1.0) > MIN_LOCAL_MARGIN, f"a patch's best candidate leads by {min(margins):.2e} only"
    out["margin"] = np.array(margins)                              # recorded: a later flip of a patch's selection can be read against it
    out.update(anchor_i=np.array([a[0] for a in anchors], np.int64), anchor_j=np.array([a[1] for a in anchors], np.int64), patch_image=np.array(owner, np.int64),
               selection=np.array(sel, np.int64).reshape(-1, 2), patch_scale_f32=np.array(sc32, np.float32), patch_scale_f64=np.array(sc64), patch_shift_f32=np.array(sh32, np.float32).reshape(-1, 3),
               patch_shift_f64=np.array(sh64).reshape(-1, 3), focal=np.array(focal, np.float32), level=np.int64(level), align_resolution=np.int64(res),
               num_patches=np.int64(npatch), beta=np.float64(beta), trunc=np.float64(trunc), sparsity_aware=np.bool_(sparse),
               global_scale=np.array(gscale if gscale is not None else [np.nan] * B, np.float32))
    return out


def main():
    install_stubs()
    import utils3d
    utils3d.pt.angle_between = R.angle_between                   # the stub the reference's normal_map_loss calls
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    from moge.train import losses as REF                           # the reference, unmodified
    import torch.nn.functional as F
    bce = F.binary_cross_entropy                                   # losses.py:278 hands it a `.float()` target, a dtype error in the float64 run:
    F.binary_cross_entropy = lambda input, target, **kw: bce(input, target.to(input.dtype), **kw)      # wrapped (not replaced) to cast the target
    os.makedirs(GOLDEN_DIR, exist_ok=True)

    # ---- affine_invariant_global_loss: the reference with the project's nearest-resize convention for utils3d's, and its solve's shift recorded ----
    from tools.make_metrics_golden import _stub_masked_nearest_resize
    utils3d.pt.masked_nearest_resize = _stub_masked_nearest_resize
    captured, solve = [], REF.align_points_scale_z_shift

    def recording_solve(*a, **kw):                                  # wrapped, not replaced: the solve's (scale, shift) as the loss saw them
        captured.append(solve(*a, **kw))
        return captured[-1]
    REF.align_points_scale_z_shift = recording_solve
    for name, seed, (B, H, W), res in (("losses_global_b2_24x40", 20261021, (2, 24, 40), 4), ("losses_global_33x65", 20261121, (1, 33, 65), 5)):
        for k in range(MAX_TRIES):
            try:
                rng = np.random.default_rng(seed + k)
                pred, gt = R.scene(rng, B, H, W, noise=0.1)
                gt[0, :4, :5] = np.inf
                gt[B - 1, H // 2, W // 3, 1] = np.nan
                gt[0, 10:14, 20:24, 2] = 0.004                      # extremely small depths: the weight clamp at 10 x the weighted mean
                out = dict(points=pred, gt_points=gt, seed=np.int64(seed + k))
                for c, (beta, trunc, sparse) in enumerate(((0.0, 1.0, False), (0.02, 0.03, True))):
                    out.update({f"c{c}_{key}": v for key, v in global_case(REF, captured, pred, gt, res, beta, trunc, sparse).items()})
                break
            except AssertionError as e:
                if k % 50 == 0:
                    print("  re-seeding:", str(e)[:100])
        else:
            raise AssertionError("no scene met the fixture conditions")
        save(name, **out)
    REF.align_points_scale_z_shift = solve

    # ---- affine_invariant_local_loss: level 4 (radius 6, 13 x 13 windows), align_resolution 6, 4 patches per image, B = 2 at 24 x 40 -------------
    utils3d.pt.masked_nearest_resize = _batched_nearest_resize
    solve3 = REF.align_points_scale_xyz_shift

    def recording_solve3(*a, **kw):
        captured.append(solve3(*a, **kw))
        return captured[-1]
    REF.align_points_scale_xyz_shift = recording_solve3
    forced, multinomial = {}, torch.multinomial

    def wrapped_multinomial(weights, n, **kw):
        """wrapped, not replaced: torch's draw, except that the float64 run repeats the float32 run's anchors and that the first two anchors are put on a
        corner and on an edge pixel; the anchors used are recorded, mapped through torch.where(gt_mask) as the reference maps them"""
        pick = multinomial(weights, n, **kw)
        valid = forced["where"]
        flat = {(int(i), int(j)): k for k, (i, j) in enumerate(zip(valid[1], valid[2]))}
        if forced.get("anchors") is not None:
            pick = torch.tensor([flat[(i, j)] for i, j in zip(*forced["anchors"])])
        else:
            for k, ij in enumerate(forced["corner"]):
                pick[k] = flat[ij]
        forced["used"] = ([int(valid[1][k]) for k in pick], [int(valid[2][k]) for k in pick])
        return pick
    where = torch.where

    def recording_where(*a, **kw):
        res = where(*a, **kw)
        if len(a) == 1 and a[0].dim() == 3:
            forced["where"] = res
        return res
    for name, seed in (("losses_local_b2_24x40", 20261022),):
        B, H, W = 2, 24, 40
        for k in range(LOCAL_TRIES):
            try:
                torch.multinomial, torch.where = wrapped_multinomial, recording_where
                torch.manual_seed(seed + k)
                rng = np.random.default_rng(seed + k)
                pred, gt = R.scene(rng, B, H, W, noise=0.05)
                gt[0, :4, :5] = np.inf
                gt[1, H // 2, W // 3, 1] = np.nan
                out = dict(points=pred, gt_points=gt, seed=np.int64(seed + k))
                cases = ((0.0, 1.0, False, None, [0.45, 0.55]), (0.02, 0.05, True, [1.3, 0.9], [0.45, 0.55]), (0.0, 1.0, False, None, [0.45, 1e4]))
                for c, (beta, trunc, sparse, gscale, focal) in enumerate(cases):
                    out.update({f"c{c}_{key}": v for key, v in local_case(REF, captured, forced, pred, gt, focal, gscale, 4, 6, 4, beta, trunc, sparse).items()})
                assert out["c2_loss_f64"][1] == 0 and len(out["c2_patch_image"]) > 0 and (out["c2_patch_image"] == 0).all(), (      # an image whose every patch is below 32 points
                    out["c2_loss_f64"], out["c2_patch_image"])
                assert len(out["c0_patch_image"]) >= 6
                break
            except (AssertionError, KeyError) as e:
                if k % 20 == 0:
                    import traceback
                    print("  re-seeding:", repr(e)[:120], traceback.format_exc().splitlines()[-3:-1])
            finally:
                torch.multinomial, torch.where = multinomial, where
        else:
            raise AssertionError("no scene met the fixture conditions")
        save(name, **out)
    REF.align_points_scale_xyz_shift = solve3

    # ---- normal_loss, edge_loss: B = 2 at 24 x 40 and one 33 x 65 image ---------------------------------------------------------------
    for name, seed, (B, H, W) in (("losses_stencil_b2_24x40", 20261019, (2, 24, 40)), ("losses_stencil_33x65", 20261119, (1, 33, 65))):
        pred, gt, used = stencil_scene(seed, B, H, W)
        out = dict(points=pred, gt_points=gt, seed=np.int64(used))
        both(out, "normal", REF.normal_loss, pred, gt)
        both(out, "edge", REF.edge_loss, pred, gt)
        save(name, **out)

    # ---- the elementwise losses: B = 2 at 24 x 40 ------------------------------------------------------------------------------------------
    rng = np.random.default_rng(20261020)
    B, H, W = 2, 24, 40
    out = {}
    pos = rng.random((B, H, W)) < 0.45
    neg = ~pos & (rng.random((B, H, W)) < 0.7)                     # pos | neg does not cover the map
    assert (~(pos | neg)).sum() > 50 and not (pos & neg).any()
    out["pred_mask"] = rng.normal(0.5, 0.6, (B, H, W)).astype(np.float32)          # mask_l2_loss takes any real value
    prob = rng.uniform(1e-4, 1 - 1e-4, (B, H, W)).astype(np.float32)
    prob[0, 3, 4], pos[0, 3, 4], neg[0, 3, 4] = 0.0, True, False    # log(0): the -100 clamp, and the 1e-12 clamp of the backward
    prob[1, 5, 6], pos[1, 5, 6], neg[1, 5, 6] = 1.0, False, True
    prob[1, 7, 8], pos[1, 7, 8], neg[1, 7, 8] = 0.0, False, False   # ... and one outside pos | neg: no value, no gradient
    out["pred_mask_prob"], out["gt_mask_pos"], out["gt_mask_neg"] = prob, pos, neg
    both(out, "mask_l2", REF.mask_l2_loss, out["pred_mask"], pos, neg)
    both(out, "mask_bce", REF.mask_bce_loss, prob, pos, neg)

    n_pred = rng.normal(0, 1, (B, H, W, 3)).astype(np.float32)
    n_gt = rng.normal(0, 1, (B, H, W, 3))
    n_gt = (n_gt / np.linalg.norm(n_gt, axis=-1, keepdims=True)).astype(np.float32)
    n_gt[0, 20:, 30:] = np.inf
    n_gt[1, 2, 3, 0] = np.nan
    n_pred[1, 4, 5] = 2.5 * n_gt[1, 4, 5]                            # parallel: |a x b| = 0, torch.norm's zero subgradient
    out["pred_normal"], out["gt_normal"] = n_pred, n_gt
    both(out, "normal_map", REF.normal_map_loss, n_pred, n_gt)

    s_pred = rng.uniform(0.2, 5.0, (2, 7)).astype(np.float32)
    s_gt = rng.uniform(0.2, 5.0, (2, 7)).astype(np.float32)
    s_gt[0, 2], s_gt[1, 5], s_gt[1, 6] = 0.0, -1.5, np.float32(1e-30)      # non-positive gt: no value, no gradient
    out["scale_pred"], out["scale_gt"] = s_pred, s_gt
    both(out, "metric_scale", REF.metric_scale_loss, s_pred, s_gt)
    save("losses_pixel_b2_24x40", **out)


if __name__ == "__main__":
    sys.exit(main())
