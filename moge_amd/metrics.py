"""Evaluation metrics on the MI355X: the host-side mirror of the reference's `moge/test/metrics.py` (same function names, arguments, return
values), with the per-pixel scoring in the HIP kernels of `csrc/metrics.hip` (C ABI `moge_metrics_*`) and the alignment solves in
`moge_amd.alignment`.

    from moge_amd.metrics import compute_metrics          # instead of moge.test.metrics (eval_baseline.py)
    metrics, misc = compute_metrics(pred, gt, vis=False)

One image per call; every tensor lives on the GPU (`cuda`) - there is no CPU path.  What differs from the reference, by design:
  * all variants of one prediction are scored in ONE read of pred / gt / mask (moge_metrics_error), sums in float64 (the reference takes fp32
    means); delta1 / boundary counts are exact integers, computed with the reference's fp32 operation order;
  * the local-points metric (metrics.py:283-311) packs every segment into one padded problem and solves it in ONE batched anchored solve; the
    host synchronises a fixed number of times whatever the segment count;
  * `masked_nearest_resize` and `depth_map_to_point_map` stand in for the un-vendored utils3d functions (conventions in csrc/metrics.hip and
    DESIGN.md section 10: unpinned, like the other utils3d stand-ins)."""
from __future__ import annotations

import math
from typing import Dict, Optional, Tuple

import numpy as np
import torch

from . import _lib as L
from . import alignment as A
from ._lib import ptr

PARTIALS = 256                      # MOGE_METRICS_PARTIALS (include/moge_hip.h)
MAX_SEGMENTS = 512                  # MOGE_METRICS_MAX_SEGMENTS
LR_SIZE = (64, 64)                  # metrics.py:128
BOUNDARY_T = torch.linspace(0.05, 0.25, 10).tolist()      # metrics.py:80 (weights = thresholds)

# error-pass transform modes (moge_metrics_error)
_SCALE, _AFFINE, _SHIFT, _DISP = 0, 1, 2, 3


def _h2d(values, dtype, device) -> torch.Tensor:
    """a small host list -> device tensor through pinned memory, asynchronously (no host synchronisation)"""
    return torch.tensor(values, dtype=dtype).pin_memory().to(device, non_blocking=True)


def _u8(mask: torch.Tensor) -> torch.Tensor:
    return mask.to(torch.bool).contiguous().view(torch.uint8)


def _f32(t: torch.Tensor) -> torch.Tensor:
    return t.float().contiguous()


# ------------------------------------------------------------------------------------------------------------------------------------------
# utils3d stand-ins
# ------------------------------------------------------------------------------------------------------------------------------------------
def masked_nearest_resize(*image: torch.Tensor, mask: torch.Tensor, size: Tuple[int, int], return_index: bool = False):
    """utils3d.pt.masked_nearest_resize for one (H, W) mask: -> (*resized images, lr_mask (h, w) bool[, (rows, cols) int64 (h, w)]) with
    `image[rows, cols]` the nearest valid pixel of each low-resolution cell (convention: csrc/metrics.hip, lr_sample_kernel)."""
    dev = L.device_of("metrics", mask, *image)
    H, W = mask.shape[-2:]
    h, w = size
    lr_mask = torch.empty((h, w), device=dev, dtype=torch.uint8)
    index = torch.empty((2, h, w), device=dev, dtype=torch.int32)
    with L.on(dev) as st:
        L.check(L.lib.moge_metrics_lr_sample(ptr(_u8(mask)), H, W, h, w, ptr(lr_mask), ptr(index), st))
    rows, cols = index[0].long(), index[1].long()
    out = tuple(im[..., rows, cols, :] if im.dim() == 3 else im[..., rows, cols] for im in image) + (lr_mask.bool(),)
    if return_index:
        out = out + ((rows, cols),)
    return out


def depth_map_to_point_map(depth: torch.Tensor, intrinsics: torch.Tensor) -> torch.Tensor:
    """utils3d.pt.depth_map_to_point_map with normalised intrinsics: pixel centres ((x + 0.5) / W, (y + 0.5) / H) unprojected at `depth`."""
    H, W = depth.shape[-2:]
    u = (torch.arange(W, dtype=depth.dtype, device=depth.device) + 0.5) / W
    v = (torch.arange(H, dtype=depth.dtype, device=depth.device) + 0.5) / H
    fx, fy, cx, cy = intrinsics[..., 0, 0], intrinsics[..., 1, 1], intrinsics[..., 0, 2], intrinsics[..., 1, 2]
    x = (u[None, :] - cx[..., None, None]) / fx[..., None, None] * depth
    y = (v[:, None] - cy[..., None, None]) / fy[..., None, None] * depth
    return torch.stack([x, y, depth], dim=-1)


def intrinsics_to_fov(intrinsics: torch.Tensor):
    """geometry_torch.py:75-87"""
    return 2 * torch.atan(0.5 / intrinsics[..., 0, 0]), 2 * torch.atan(0.5 / intrinsics[..., 1, 1])


def key_average(list_of_dicts: list) -> Dict[str, float]:
    """tools.py:65-82 for flat dicts: keys sorted, NaN values skipped."""
    keys = sorted({k for d in list_of_dicts for k in d})
    out = {}
    for k in keys:
        vals = [d[k] for d in list_of_dicts if d.get(k) is not None and not math.isnan(d[k])]
        out[k] = sum(vals) / len(vals) if vals else float('nan')
    return out


# ------------------------------------------------------------------------------------------------------------------------------------------
# kernels
# ------------------------------------------------------------------------------------------------------------------------------------------
def _params(mode: int, scale=None, shift=None, clamp: float = 0.0, device=None) -> torch.Tensor:
    """one (6,) row of moge_metrics_error: (mode, s, t0, t1, t2, c), built on the device (scale / shift stay tensors: no host sync)."""
    one = torch.ones((), device=device)
    s = scale.reshape(()).float() if scale is not None else one
    t = shift.reshape(-1).float() if shift is not None else torch.zeros(1, device=device)
    t = torch.cat([t, torch.zeros(3 - t.numel(), device=device)])
    return torch.cat([_h2d([float(mode)], torch.float32, device), s[None], t, _h2d([clamp], torch.float32, device)])


def error_pass(pred: torch.Tensor, gt: torch.Tensor, mask: torch.Tensor, params: torch.Tensor) -> torch.Tensor:
    """pred / gt (..., d) or (...) with mask (...); params (K, 6) -> (K, 3) float64 on the device: (sum rel, delta1 count, mask count)."""
    dev = L.device_of("metrics", pred, gt, mask, params)
    dim = 3 if pred.dim() == mask.dim() + 1 else 1
    pred, gt, params = _f32(pred), _f32(gt), _f32(params)
    K = params.shape[0]
    part = torch.empty(PARTIALS * K * 3, device=dev, dtype=torch.float64)
    out = torch.empty((K, 3), device=dev, dtype=torch.float64)
    with L.on(dev) as st:
        L.check(L.lib.moge_metrics_error(ptr(pred), ptr(gt), ptr(_u8(mask)), mask.numel(), dim, ptr(params), K, ptr(part), ptr(out), st))
    return out


def masked_max(x: torch.Tensor, mask: torch.Tensor) -> torch.Tensor:
    dev = L.device_of("metrics", x, mask)
    x = _f32(x)
    part = torch.empty(PARTIALS, device=dev, dtype=torch.float32)
    out = torch.empty(1, device=dev, dtype=torch.float32)
    with L.on(dev) as st:
        L.check(L.lib.moge_metrics_masked_max(ptr(x), ptr(_u8(mask)), mask.numel(), ptr(part), ptr(out), st))
    return out[0]


def boundary_counts(pred: torch.Tensor, gt: torch.Tensor, mask: torch.Tensor) -> torch.Tensor:
    """(H, W) maps -> (3, 10, 3) int64 on the device: per radius 1..3 and threshold, (TP, gt-label, pred-label) over the valid pairs."""
    dev = L.device_of("metrics", pred, gt, mask)
    H, W = mask.shape[-2:]
    pred, gt = _f32(pred), _f32(gt)
    counts = torch.empty((3, 10, 3), device=dev, dtype=torch.int64)
    with L.on(dev) as st:
        L.check(L.lib.moge_metrics_boundary(ptr(pred), ptr(gt), ptr(_u8(mask)), H, W, ptr(counts), st))
    return counts


def boundary_f1_from_counts(counts) -> list:
    """metrics.py:79-92 on the counts of one radius (10, 3): fp32 arithmetic in the reference's order, weighted average in Python floats."""
    f32 = np.float32
    f1s = []
    for t in range(len(BOUNDARY_T)):
        tp, gl, pl = (f32(v) for v in counts[t])
        precision = f32(tp / max(gl, f32(1e-12)))
        recall = f32(tp / max(pl, f32(1e-12)))
        f1s.append(float(f32(f32(f32(2) * precision) * recall) / max(f32(precision + recall), f32(1e-12))))
    return f1s


def _weighted(f1s):
    return sum(w * f for w, f in zip(BOUNDARY_T, f1s)) / sum(BOUNDARY_T)


# ------------------------------------------------------------------------------------------------------------------------------------------
# the reference's metric functions (metrics.py:25-92), on CUDA tensors
# ------------------------------------------------------------------------------------------------------------------------------------------
def _single(pred, gt, eps):
    L.device_of("metrics", pred, gt)
    if eps != 1e-6:
        raise NotImplementedError("the kernels use the reference's eps = 1e-6")
    mask = torch.ones(gt.shape[:-1] if pred.dim() > 1 and pred.shape[-1] == 3 and pred.dim() == gt.dim() and gt.dim() >= 2 else gt.shape,
                      device=gt.device, dtype=torch.bool)
    r = error_pass(pred, gt, mask, _params(_SCALE, device=pred.device)[None]).cpu()
    return float(r[0, 0] / r[0, 2]), float(r[0, 1] / r[0, 2])


def rel_depth(pred: torch.Tensor, gt: torch.Tensor, eps: float = 1e-6):
    return _single(pred, gt, eps)[0]


def delta1_depth(pred: torch.Tensor, gt: torch.Tensor, eps: float = 1e-6):
    return _single(pred, gt, eps)[1]


def rel_point(pred: torch.Tensor, gt: torch.Tensor, eps: float = 1e-6):
    return _single(pred, gt, eps)[0]


def delta1_point(pred: torch.Tensor, gt: torch.Tensor, eps: float = 1e-6):
    return _single(pred, gt, eps)[1]


def _local(pred, gt, diameter):
    L.device_of("metrics", pred, gt, diameter)
    n = pred.shape[0]
    seg = torch.zeros(n, device=pred.device, dtype=torch.int32)
    labels = torch.zeros(1, device=pred.device, dtype=torch.int32)
    r = _segment_error(seg, torch.ones(n, device=pred.device, dtype=torch.bool), _f32(pred), _f32(gt), labels, 1,
                       torch.zeros(1, device=pred.device, dtype=torch.int32), torch.zeros(1, device=pred.device, dtype=torch.int32),
                       torch.ones(1, device=pred.device), torch.zeros(1, 3, device=pred.device),
                       _f32(diameter.reshape(1))).cpu()
    return float(r[0, 0] / r[0, 2]), float(r[0, 1] / r[0, 2])


def rel_point_local(pred: torch.Tensor, gt: torch.Tensor, diameter: torch.Tensor):
    return _local(pred, gt, diameter)[0]


def delta1_point_local(pred: torch.Tensor, gt: torch.Tensor, diameter: torch.Tensor):
    return _local(pred, gt, diameter)[1]


def boundary_f1(pred: torch.Tensor, gt: torch.Tensor, mask: torch.Tensor, radius: int = 1):
    if radius not in (1, 2, 3):
        raise NotImplementedError("the boundary kernel covers radii 1, 2 and 3 (the ones compute_metrics uses)")
    counts = boundary_counts(pred, gt, mask).cpu().numpy()
    return _weighted(boundary_f1_from_counts(counts[radius - 1]))


# ------------------------------------------------------------------------------------------------------------------------------------------
# local points (metrics.py:283-311)
# ------------------------------------------------------------------------------------------------------------------------------------------
def _segment_error(seg, mask, pred, gt, labels, U, row, kept, scale, shift, diameter):
    E = kept.numel()
    dev = pred.device
    part = torch.empty(PARTIALS * E * 3, device=dev, dtype=torch.float64)
    out = torch.empty((E, 3), device=dev, dtype=torch.float64)
    with L.on(dev) as st:
        L.check(L.lib.moge_metrics_segment_error(ptr(seg), ptr(_u8(mask)), ptr(pred), ptr(gt), mask.numel(), ptr(labels), U, ptr(row), ptr(kept), E,
                                                 ptr(_f32(scale)), ptr(_f32(shift)), ptr(diameter), ptr(part), ptr(out), st))
    return out


def local_points(pred_points, gt_points, mask, segmentation_mask, segmentation_labels, lr_mask, lr_index, details: Optional[dict] = None):
    """metrics.py:283-311 -> key_average of the kept segments' {'rel', 'delta1'}.  Two host synchronisations (the low-resolution counts, the
    results) plus those of the one batched solve, whatever the number of segments.  `details` (optional dict) receives per-entry diameter /
    scale / shift / rel / delta1 of the kept segments, in segmentation_labels order."""
    dev = L.device_of("metrics", pred_points, gt_points, mask, segmentation_mask, lr_mask, *lr_index)
    H, W = mask.shape[-2:]
    h, w = lr_mask.shape
    entries = list(segmentation_labels.values())
    uniq = sorted(set(int(v) for v in entries))
    U = len(uniq)
    if U == 0:
        return key_average([])
    if U > MAX_SEGMENTS:
        raise ValueError(f"at most {MAX_SEGMENTS} distinct segment labels per call")
    seg = segmentation_mask.to(torch.int32).contiguous()
    labels = _h2d(uniq, torch.int32, dev)
    lr_u8 = _u8(lr_mask)
    index = torch.stack([lr_index[0], lr_index[1]]).to(torch.int32).contiguous()
    pred_points, gt_points = _f32(pred_points), _f32(gt_points)
    bbox = torch.empty(U * 6, device=dev, dtype=torch.int32)
    lr_count = torch.empty(U, device=dev, dtype=torch.int32)
    diameter = torch.empty(U, device=dev, dtype=torch.float32)
    m8 = _u8(mask)
    with L.on(dev) as st:
        L.check(L.lib.moge_metrics_segment_stats(ptr(seg), ptr(m8), ptr(gt_points), H, W, ptr(lr_u8), ptr(index), h, w, ptr(labels), U, ptr(bbox),
                                                 ptr(lr_count), ptr(diameter), st))
    counts = lr_count.cpu().tolist()                                                            # host sync 1
    kept_u = [u for u in range(U) if counts[u] >= 10]                                           # :299-300
    if not kept_u:
        return key_average([])
    E, n_max = len(kept_u), max(counts[u] for u in kept_u)
    kept = _h2d(kept_u, torch.int32, dev)
    row_h = [-1] * U
    for e, u in enumerate(kept_u):
        row_h[u] = e
    row = _h2d(row_h, torch.int32, dev)
    src = torch.empty((E, n_max, 3), device=dev)
    tgt = torch.empty_like(src)
    wt = torch.empty((E, n_max), device=dev)
    with L.on(dev) as st:
        L.check(L.lib.moge_metrics_segment_pack(ptr(seg), W, ptr(lr_u8), ptr(index), h, w, ptr(labels), U, ptr(kept), E, n_max, ptr(pred_points), ptr(gt_points),
                                                ptr(diameter), ptr(src), ptr(tgt), ptr(wt), st))
    scale, shift = A.align_points_scale_xyz_shift(src, tgt, wt)                                  # all segments, one batched solve
    res = _segment_error(seg, mask, pred_points, gt_points, labels, U, row, kept, scale, shift, diameter)
    res = res.cpu().numpy()                                                                     # host sync 2
    per = []
    for v in entries:                                                                           # the reference's order (dict order)
        e = row_h[uniq.index(int(v))]
        if e < 0:
            continue
        per.append({'rel': float(res[e, 0] / res[e, 2]), 'delta1': float(res[e, 1] / res[e, 2])})
    if details is not None:
        ent_rows = [row_h[uniq.index(int(v))] for v in entries]
        details.update(rows=ent_rows, diameter=diameter[kept.long()], scale=scale, shift=shift, per_entry=per, src=src, tgt=tgt, weight=wt)
    return key_average(per)


# ------------------------------------------------------------------------------------------------------------------------------------------
# compute_metrics (metrics.py:95-341)
# ------------------------------------------------------------------------------------------------------------------------------------------
def compute_metrics(pred: Dict[str, torch.Tensor], gt: Dict[str, torch.Tensor], vis: bool = False, stages: Optional[dict] = None):
    """metrics.py:95-341: same keys, fall-backs, gates, nested output keys in the same order (Python floats) and the same `misc` with vis=True.
    `stages` (optional dict) receives CUDA events around the stages for tools/bench_metrics.py."""
    dev = L.device_of("metrics", *(v for v in pred.values() if isinstance(v, torch.Tensor)), gt['depth_mask'], gt['depth'], gt.get('points'))
    ev = _Stages(stages)
    metrics, misc = {}, {}
    mask = gt['depth_mask'].bool()
    gt_depth = _f32(gt['depth'])
    gt_points = gt.get('points')
    H, W = mask.shape[-2:]

    ev.mark('lr_sample')
    lr_mask, lr_index = masked_nearest_resize(mask=mask, size=LR_SIZE, return_index=True)       # :128
    lr_flat = (lr_index[0] * W + lr_index[1]).reshape(-1)
    lr_sel = lr_flat[lr_mask.reshape(-1)]                                                       # host sync: the lr sample count

    def lr(x):                                                                                  # x[lr_index][lr_mask]
        return x.reshape(H * W, *x.shape[2:])[lr_sel]

    only_depth = not any('point' in k for k in pred)                                            # :130
    pred_depth_aligned, pred_points_aligned = None, None
    jobs = []                  # (metric name, source tensor, params row): scored together per source tensor after the solves

    ev.mark('align')
    if 'depth_metric' in pred and gt['is_metric']:                                              # :134-143
        jobs.append(('depth_metric', pred['depth_metric'], _params(_SCALE, device=dev)))
        metrics['depth_metric'] = None
        if pred_depth_aligned is None:
            pred_depth_aligned = pred['depth_metric']

    pdsi = pred.get('depth_scale_invariant', pred.get('depth_metric'))                         # :146-151
    if pdsi is not None:
        g = lr(gt_depth)
        scale = A.align_depth_scale(lr(pdsi), g, 1 / g)                                         # :157-158
        jobs.append(('depth_scale_invariant', pdsi, _params(_SCALE, scale, device=dev)))
        metrics['depth_scale_invariant'] = None
        if pred_depth_aligned is None:
            pred_depth_aligned = pdsi * scale

    pdai = next((pred[k] for k in ('depth_affine_invariant', 'depth_scale_invariant', 'depth_metric') if k in pred), None)    # :170-177
    if pdai is not None:
        g = lr(gt_depth)
        scale, shift = A.align_depth_affine(lr(pdai), g, 1 / g)                                 # :183-184
        jobs.append(('depth_affine_invariant', pdai, _params(_AFFINE, scale, shift, device=dev)))
        metrics['depth_affine_invariant'] = None
        if pred_depth_aligned is None:
            pred_depth_aligned = pdai * scale + shift

    if 'disparity_affine_invariant' in pred:                                                    # :195-202
        pdisp = pred['disparity_affine_invariant']
    elif 'depth_scale_invariant' in pred:
        pdisp = 1 / pred['depth_scale_invariant']
    elif 'depth_metric' in pred:
        pdisp = 1 / pred['depth_metric']
    else:
        pdisp = None
    if pdisp is not None:
        pdisp = _f32(pdisp)
        midx = mask.reshape(-1).nonzero().squeeze(1)                                            # order-preserving compaction (host sync)
        scale, shift = A.align_affine_lstsq(pdisp.reshape(-1)[midx], 1 / gt_depth.reshape(-1)[midx])     # :207
        gmax = float(masked_max(gt_depth, mask).item())                                         # :212 .item() (host sync)
        clamp = float(np.float32(1 / gmax))
        jobs.append(('disparity_affine_invariant', pdisp, _params(_DISP, scale, shift, clamp, device=dev)))
        metrics['disparity_affine_invariant'] = None
        if pred_depth_aligned is None:
            pred_depth_aligned = 1 / (pdisp * scale + shift).clamp_min(1e-6)                    # :220

    if 'points_metric' in pred and gt['is_metric']:                                             # :223-235
        p = pred['points_metric']
        g = lr(gt_points)
        shift = A.align_points_xyz_shift(lr(p), g, 1 / g.norm(dim=-1))
        jobs.append(('points_metric', p, _params(_SHIFT, None, shift, device=dev)))
        metrics['points_metric'] = None
        if pred_points_aligned is None:
            pred_points_aligned = p

    ppsi = pred.get('points_scale_invariant', pred.get('points_metric'))                       # :238-255
    if ppsi is not None:
        g = lr(gt_points)
        scale = A.align_points_scale(lr(ppsi), g, 1 / g.norm(dim=-1))
        jobs.append(('points_scale_invariant', ppsi, _params(_SCALE, scale, device=dev)))
        metrics['points_scale_invariant'] = None
        if vis and pred_points_aligned is None:
            pred_points_aligned = pred['points_scale_invariant'] * scale

    ppai = next((pred[k] for k in ('points_affine_invariant', 'points_scale_invariant', 'points_metric') if k in pred), None)    # :258-280
    if ppai is not None:
        g = lr(gt_points)
        scale, shift = A.align_points_scale_xyz_shift(lr(ppai), g, 1 / g.norm(dim=-1))
        jobs.append(('points_affine_invariant', ppai, _params(_AFFINE, scale, shift, device=dev)))
        metrics['points_affine_invariant'] = None
        if vis and pred_points_aligned is None:
            pred_points_aligned = pred['points_affine_invariant'] * scale + shift

    ev.mark('error')
    groups = {}                                                                                 # one error pass per source tensor
    for name, src, prm in jobs:
        groups.setdefault((src.data_ptr(), src.dim()), (src, []))[1].append((name, prm))
    results = {}
    for (_, dim), (src, items) in groups.items():
        gtt = gt_points if src.dim() == mask.dim() + 1 else gt_depth
        out = error_pass(src, gtt, mask, torch.stack([p for _, p in items]))
        for (name, _), r in zip(items, out):
            results[name] = r
    if results:
        names = list(results)
        host = torch.stack([results[k] for k in names]).cpu().numpy()                           # host sync
        for k, r in zip(names, host):
            metrics[k] = {'rel': float(r[0] / r[2]), 'delta1': float(r[1] / r[2])}

    ev.mark('local_points')
    if 'segmentation_mask' in gt and 'points' in gt and any('points' in k for k in pred.keys()):      # :283-311
        p = next(pred[k] for k in pred.keys() if 'points' in k)
        metrics['local_points'] = local_points(p, gt['points'], mask, gt['segmentation_mask'], gt['segmentation_labels'], lr_mask, lr_index)

    if 'intrinsics' in pred and 'intrinsics' in gt:                                             # :315-323
        pfx, _ = intrinsics_to_fov(pred['intrinsics'])
        gfx, _ = intrinsics_to_fov(gt['intrinsics'])
        d = torch.rad2deg(pfx - gfx)
        metrics['fov_x'] = {'mae': d.abs().mean().item(), 'deviation': d.item()}

    ev.mark('boundary')
    if pred_depth_aligned is not None and gt['has_sharp_boundary']:                             # :326-331
        counts = boundary_counts(pred_depth_aligned, gt_depth, mask).cpu().numpy()
        metrics['boundary'] = {f'radius{r}_f1': _weighted(boundary_f1_from_counts(counts[r - 1])) for r in (1, 2, 3)}
    ev.mark('end')

    if vis:                                                                                     # :333-339
        if pred_points_aligned is not None:
            misc['pred_points'] = pred_points_aligned
        if only_depth:
            misc['pred_points'] = depth_map_to_point_map(pred_depth_aligned, intrinsics=gt['intrinsics'])
        if pred_depth_aligned is not None:
            misc['pred_depth'] = pred_depth_aligned
    return metrics, misc


class _Stages:
    def __init__(self, out):
        self.out = out

    def mark(self, name):
        if self.out is not None:
            e = torch.cuda.Event(enable_timing=True)
            e.record()
            self.out.setdefault('_events', []).append((name, e))
