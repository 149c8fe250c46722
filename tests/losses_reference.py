"""The project's own restatement of the training losses that moge_amd.losses covers, written from the formulas of DESIGN.md section 15 (not from
the reference's code): plain torch, any dtype and device, differentiable through autograd.  tests/test_losses_reference_cpu.py pins it to the
goldens of the unmodified reference (tests/golden/losses_*.npz); the GPU tests use it, in float64 and in float32, for the shapes the goldens do
not cover.  Every function takes ONE instance or a batch and returns one value per instance."""
import math

import torch

DEG = math.pi / 180.0
NORMAL_MIN, EDGE_MIN, ANGLE_MAX, BETA = 1.0 * DEG, 0.1 * DEG, 90.0 * DEG, 3.0 * DEG
# the four corner normals of a quad; corners 0 left-up, 1 right-up, 2 left-down, 3 right-down: normal = (P[A] - P[O]) x (P[B] - P[O])
QUAD_TERMS = ((1, 2, 3), (0, 3, 1), (2, 1, 0), (3, 0, 2))


def clean(gt):
    """-> (gt with every non-finite pixel replaced by ones, the mask of finite pixels)"""
    mask = torch.isfinite(gt).all(dim=-1)
    return torch.where(mask[..., None], gt, torch.ones_like(gt)), mask


def angle(u, v, eps):
    return torch.atan2(torch.linalg.cross(u, v, dim=-1).norm(dim=-1) + eps, (u * v).sum(dim=-1))


def huber(a, beta):
    return torch.where(a < beta, a * a / (2 * beta), a - beta / 2)


def corners(x):
    """the four (H-1, W-1) corner views of a (..., H, W[, 3]) map, the pixel axes at dims `-3, -2` (3 channels) or `-2, -1`"""
    if x.dim() >= 3 and x.shape[-1] == 3 and x.dtype != torch.bool:
        return x[..., :-1, :-1, :], x[..., :-1, 1:, :], x[..., 1:, :-1, :], x[..., 1:, 1:, :]
    return x[..., :-1, :-1], x[..., :-1, 1:], x[..., 1:, :-1], x[..., 1:, 1:]


def normal_angles(points, gt_points):
    """-> [(angle (..., H-1, W-1), mask)] for the four corner terms, before the clamp"""
    gt, mask = clean(gt_points)
    P, G, M = corners(points), corners(gt), corners(mask)
    out = []
    for a, b, o in QUAD_TERMS:
        n = torch.linalg.cross(P[a] - P[o], P[b] - P[o], dim=-1)
        g = torch.linalg.cross(G[a] - G[o], G[b] - G[o], dim=-1)
        out.append((angle(n, g, 1e-12), M[a] & M[b] & M[o]))
    return out


def normal_loss(points, gt_points):
    H, W = points.shape[-3:-1]
    total = 0
    for ang, m in normal_angles(points, gt_points):
        total = total + m * huber(ang.clamp(NORMAL_MIN, ANGLE_MAX), BETA)
    return total.mean(dim=(-2, -1)) / (4 * max(H, W))


def edge_angles(points, gt_points):
    """-> [(angle, mask)] for the row differences (H-1, W) and the column differences (H, W-1)"""
    gt, mask = clean(gt_points)
    rows = (angle(points[..., :-1, :, :] - points[..., 1:, :, :], gt[..., :-1, :, :] - gt[..., 1:, :, :], 1e-12), mask[..., :-1, :] & mask[..., 1:, :])
    cols = (angle(points[..., :, :-1, :] - points[..., :, 1:, :], gt[..., :, :-1, :] - gt[..., :, 1:, :], 1e-12), mask[..., :, :-1] & mask[..., :, 1:])
    return [rows, cols]


def edge_loss(points, gt_points):
    H, W = points.shape[-3:-1]
    means = [(m * huber(ang.clamp(EDGE_MIN, ANGLE_MAX), BETA)).mean(dim=(-2, -1)) for ang, m in edge_angles(points, gt_points)]
    return (means[0] + means[1]) / (2 * max(H, W))


def mask_l2_loss(pred_mask, pos, neg):
    return (neg.to(pred_mask.dtype) * pred_mask ** 2 + pos.to(pred_mask.dtype) * (1 - pred_mask) ** 2).mean(dim=(-2, -1))


def mask_bce_loss(prob, pos, neg):
    """binary cross entropy with the logs clamped at -100; where p (1 - p) < 1e-12 the gradient is (p - t) / 1e-12, torch's backward"""
    t = pos.to(prob.dtype)
    return ((pos | neg) * torch.nn.functional.binary_cross_entropy(prob, t, reduction="none")).mean(dim=(-2, -1))


def metric_scale_loss(scale_pred, scale_gt):
    valid = scale_gt > 0
    d = scale_pred.log() - torch.where(valid, scale_gt, torch.ones_like(scale_gt)).log()
    return torch.where(valid, d * d, torch.zeros_like(d))


def angle_between(a, b):
    """the stand-in for utils3d.pt.angle_between (UNPINNED): atan2(|a x b|, a . b)"""
    return torch.atan2(torch.linalg.cross(a, b, dim=-1).norm(dim=-1), (a * b).sum(dim=-1))


def normal_map_loss(pred_normal, gt_normal):
    gt, mask = clean(gt_normal)
    return (mask * angle_between(pred_normal, gt) ** 2).mean(dim=(-2, -1))


def in_window_fraction(points, mask, radius_2d, radius_3d):
    """compute_anchor_sampling_weight's expectation, brute force for ONE image: p[i, j] = the fraction of the (2 r + 1)^2 offsets around a valid
    pixel that land in the image, on a valid pixel and within radius_3d[i, j] of its point (0 off the mask)"""
    H, W = mask.shape
    p = torch.zeros(H, W, dtype=torch.float64)
    for i in range(H):
        for j in range(W):
            if not mask[i, j]:
                continue
            i0, i1, j0, j1 = max(i - radius_2d, 0), min(i + radius_2d, H - 1), max(j - radius_2d, 0), min(j + radius_2d, W - 1)
            d = (points[i0:i1 + 1, j0:j1 + 1] - points[i, j]).norm(dim=-1)          # in the dtype the kernel compares in
            hit = mask[i0:i1 + 1, j0:j1 + 1] & (d <= radius_3d[i, j])
            p[i, j] = float(hit.sum()) / (2 * radius_2d + 1) ** 2
    return p


# ---- affine_invariant_global_loss ----------------------------------------------------------------------------------------------------------
def smooth_l1(e, beta):
    return e if beta == 0 else huber(e, beta)


def affine_dense_loss(pred, gt_points, scale, shift, lr_frac=None, beta=0.0):
    """the global loss behind its solve: pred / gt (..., H, W, 3), scale (...), shift (..., 3) -> loss, truncated_error, delta, each (...).
    lr_frac (...): the valid fraction of the low-resolution samples, which turns the sparsity term on."""
    gt, mask = clean(gt_points)
    area = (-2, -1)
    valid = scale > 0
    s = torch.where(valid, scale, torch.zeros_like(scale))[..., None, None, None]
    t = torch.where(valid[..., None], shift, torch.zeros_like(shift))[..., None, None, :]
    fill = mask.to(pred.dtype).mean(dim=area)
    w0 = (valid[..., None, None] & mask).to(pred.dtype) / gt[..., 2].clamp_min(1e-5)
    cap = 10 * (w0 * mask).mean(dim=area) / (fill + 1e-7)
    w = torch.minimum(w0, cap[..., None, None])
    diff = s * pred + t - gt
    loss = smooth_l1(diff.abs() * w[..., None], beta).mean(dim=(-3, -2, -1))
    if lr_frac is not None:
        loss = loss / (fill / lr_frac + 1e-7)
    err = diff.detach().norm(dim=-1) / gt[..., 2]
    return loss, (err.clamp_max(1) * mask).mean(dim=area) / (fill + 1e-7), ((err < 1) * mask).to(pred.dtype).mean(dim=area) / (fill + 1e-7)


def global_samples(gt_np, size):
    """ONE image: the low-resolution samples of the solve by the project's nearest-resize convention -> lr_mask (n,) bool, rows, cols (n,) int64"""
    import numpy as np
    from tools.make_metrics_golden import masked_nearest_resize_np
    lm, rows, cols = masked_nearest_resize_np(np.isfinite(gt_np).all(-1), size)
    return lm.reshape(-1), rows.reshape(-1), cols.reshape(-1)


def global_selection(pred_np, gt_np, size, trunc):
    """ONE image (numpy float32): the two samples the truncated scale / z-shift solve selects -> (k, i2): anchor sample, solution element in [0, 3 n)"""
    import numpy as np
    import alignment_trunc_reference as AT
    lm, rows, cols = global_samples(gt_np, size)
    src, tgt = pred_np[rows, cols], np.where(np.isfinite(gt_np).all(-1, keepdims=True), gt_np, 1)[rows, cols]
    w = (lm / np.maximum(tgt[:, 2], 1e-2)).astype(np.float32)
    k, i2 = AT._anchor(src[None].astype(np.float32), tgt[None].astype(np.float32), w[None], [0, 0, 1], trunc)
    return int(k[0]), int(i2[0])


def scale_z_shift(pred_lr, gt_lr, k, i2):
    """the line through the two selected samples, differentiable: pred_lr / gt_lr (n, 3) -> scale (), shift (3,) = (0, 0, z)"""
    s2, t2 = pred_lr.reshape(-1)[i2], gt_lr.reshape(-1)[i2]
    on_z = i2 % 3 == 2                                             # the anchor's z is subtracted from z elements only
    s1, t1 = (pred_lr[k, 2], gt_lr[k, 2]) if on_z else (pred_lr.new_zeros(()), gt_lr.new_zeros(()))
    d = s2 - s1
    scale = (t2 - t1) / torch.where(d != 0, d, torch.ones_like(d))
    z = gt_lr[k, 2] - scale * pred_lr[k, 2]
    return scale, torch.stack([torch.zeros_like(z), torch.zeros_like(z), z])


def affine_invariant_global_loss(pred, gt_points, align_resolution=64, beta=0.0, trunc=1.0, sparsity_aware=False, selection=None):
    """ONE image, any dtype.  selection: the (k, i2) of the solve if already known, else restated (float32 keys, float64 sums).
    -> loss, truncated_error, delta, scale (detached), all 0-d"""
    import numpy as np
    size = (align_resolution, align_resolution)
    gt_np = gt_points.detach().cpu().numpy().astype(np.float32)
    k, i2 = selection if selection is not None else global_selection(pred.detach().cpu().numpy().astype(np.float32), gt_np, size, trunc)
    lm, rows, cols = global_samples(gt_np, size)
    gt, _ = clean(gt_points)
    scale, shift = scale_z_shift(pred[rows, cols], gt[rows, cols], k, i2)
    lr_frac = torch.tensor(float(lm.mean()), dtype=pred.dtype) if sparsity_aware else None
    return affine_dense_loss(pred, gt_points, scale, shift, lr_frac, beta) + (scale.detach(),)


# ---- affine_invariant_local_loss -----------------------------------------------------------------------------------------------------------
def scale_xyz_shift(pred_lr, gt_lr, k, i2):
    """the line through the two selected samples with the anchor subtracted from every component: -> scale (), shift (3,)"""
    c = i2 % 3
    d = pred_lr.reshape(-1)[i2] - pred_lr[k, c]
    scale = (gt_lr.reshape(-1)[i2] - gt_lr[k, c]) / torch.where(d != 0, d, torch.ones_like(d))
    return scale, gt_lr[k] - scale * pred_lr[k]


def local_selection(src, tgt, w, trunc):
    """numpy float32 samples of ONE patch -> (k, i2) of the truncated scale / xyz-shift solve"""
    import numpy as np
    import alignment_trunc_reference as AT
    k, i2 = AT._anchor(src[None].astype(np.float32), tgt[None].astype(np.float32), w[None].astype(np.float32), [1, 1, 1], trunc)
    return int(k[0]), int(i2[0])


def affine_invariant_local_loss(pred, gt_points, focal, global_scale, level, anchors, align_resolution=32, num_patches=16, beta=0.0, trunc=1.0,
                                sparsity_aware=False, selections=None, diag=None):
    """ONE image (H, W, 3), any dtype; focal / global_scale python floats (global_scale may be None); anchors = (rows, cols) integer lists, in the
    order the patches are to be taken.  selections: per NON-EMPTY patch the (k, i2) of its solve if known, else restated.  diag: a dict that
    receives, per non-empty patch, what the fixture conditions look at.  -> (loss, truncated_error, delta) 0-d, or (0, None, None) without a patch"""
    import numpy as np
    from tools.make_metrics_golden import masked_nearest_resize_np
    H, W = pred.shape[:2]
    dt = pred.dtype
    gt, mask = clean(gt_points)
    r = math.ceil(0.5 / level * (H ** 2 + W ** 2) ** 0.5)
    S, area = 2 * r + 1, (2 * r + 1) ** 2
    fill = mask.to(dt).mean()
    gt_mean = 1 / ((mask / (gt[..., 2] + 1e-7)).mean() / (fill + 1e-7) + 1e-7)
    off = torch.arange(-r, r + 1)
    total, te_sum, dl_sum, m_sum, kept = 0, 0, 0, 0, 0
    for ai, aj in zip(*anchors):
        ii, jj = torch.meshgrid(off + int(ai), off + int(aj), indexing="ij")
        inside = (ii >= 0) & (ii < H) & (jj >= 0) & (jj < W)
        ii, jj = ii.clamp(0, H - 1), jj.clamp(0, W - 1)
        anchor = gt[int(ai), int(aj)]
        radius = 0.5 / level / focal * anchor[2]
        gp, pp = gt[ii, jj], pred[ii, jj]
        dist = (gp - anchor).norm(dim=-1)
        pmask = inside & mask[ii, jj] & (dist <= radius)
        if int(pmask.sum()) < 32:
            continue
        lm, lr, lc = masked_nearest_resize_np(pmask.numpy(), (align_resolution, align_resolution))
        lm, lr, lc = lm.reshape(-1), lr.reshape(-1), lc.reshape(-1)
        src, tgt = pp[lr, lc], gp[lr, lc]
        w = lm / (float(radius) + 1e-7)
        sel = selections[kept] if selections is not None else local_selection(src.detach().numpy().astype(np.float32), tgt.numpy().astype(np.float32), w, trunc)
        scale, shift = scale_xyz_shift(src, tgt, *sel)
        ok = bool(scale > 0) if global_scale is None else bool(0.1 < scale / global_scale < 10.0 and global_scale > 0)
        if diag is not None:
            diag.setdefault("selection", []).append(sel)
            diag.setdefault("samples", []).append((src.detach().numpy().astype(np.float32), tgt.numpy().astype(np.float32), np.asarray(w, np.float32)))
            diag.setdefault("scale", []).append(float(scale))
            diag.setdefault("valid", []).append(ok)
            diag.setdefault("count", []).append(int(pmask.sum()))
            cand = inside & mask[ii, jj]
            diag.setdefault("ratios", []).append(torch.cat([(dist / radius)[cand], (scale.detach() / (global_scale or 1.0)).reshape(1) / 0.1, (scale.detach() / (global_scale or 1.0)).reshape(1) / 10.0]))
        kept += 1
        if not ok:
            scale, shift, pmask = scale * 0, shift * 0, pmask & False
        wt = pmask.to(dt) / gp[..., 2].clamp_min(0.1 * gt_mean)
        diff = scale * pp + shift - gp
        e = diff.abs() * wt[..., None]
        l = smooth_l1(e, beta).mean()
        if sparsity_aware:
            l = l / (pmask.to(dt).mean() / float(lm.mean()) + 1e-7)
        total = total + l
        err = diff.detach().norm(dim=-1) / radius
        te_sum, dl_sum, m_sum = te_sum + (err.clamp_max(1) * pmask).sum(), dl_sum + ((err < 1) & pmask).sum(), m_sum + pmask.sum()
        if diag is not None and ok:
            diag["ratios"].append(torch.cat([(gp[..., 2] / (0.1 * gt_mean))[pmask], err[pmask]] + ([(e / beta)[pmask].reshape(-1)] if beta else [])))
    if kept == 0:
        return torch.zeros((), dtype=dt), None, None
    n = kept * area
    return total / num_patches, (te_sum / n) / (m_sum / n + 1e-7), (dl_sum.to(dt) / n) / (m_sum / n + 1e-7)


# ---- scenes shared by the golden maker and the GPU tests ---------------------------------------------------------------------------------
def scene(rng, B, H, W, noise=0.35):
    """numpy float32 (pred, gt) point maps (B, H, W, 3): gt a bumpy surface seen through a pinhole, pred a scaled, shifted and noisy copy"""
    import numpy as np
    v, u = np.meshgrid(np.linspace(-0.6, 0.6, H), np.linspace(-0.8, 0.8, W), indexing="ij")
    gt = np.empty((B, H, W, 3), np.float32)
    for b in range(B):
        f = rng.uniform(1.5, 4.0, 4)
        z = 2.5 + 0.5 * np.sin(f[0] * u + f[1]) * np.cos(f[2] * v + f[3]) + 0.3 * (u > 0.1 * b) + rng.normal(0, 0.02, (H, W))
        gt[b] = np.stack([u * z, v * z, z], -1)
    pred = (gt * rng.uniform(0.5, 2.0, (B, 1, 1, 1)) + rng.normal(0, noise, gt.shape) * np.array([0.05, 0.05, 0.25])).astype(np.float32)
    return pred, gt
