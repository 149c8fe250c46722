"""Optimal-alignment solvers of the evaluation path on the MI355X: the host-side mirror of the reference's `moge/utils/alignment.py`
(same function names, arguments, return values), calling the HIP kernels of `csrc/alignment.hip` through the C ABI (`moge_align_*`).

    from moge_amd.alignment import align_points_scale_xyz_shift      # instead of moge.utils.alignment
    scale, shift = align_points_scale_xyz_shift(pred_points_lr, gt_points_lr, 1 / gt_points_lr.norm(dim=-1))     # test/metrics.py:264

Every tensor must live on the GPU (`cuda`); there is no CPU path here (the library raises without a device).  The reference builds an
(anchors, n, 3) tensor per call for the affine solvers; the kernels subtract the anchor while loading, so the only temporaries are the
per-anchor results.

The truncated objective (alignment.py:91-144: min sum_i min(trunc, w_i |a x_i - y_i|), what the affine-invariant training losses call,
train/losses.py:45 / :175) runs in its own kernels (`moge_align_trunc*`).  Every solver that takes `trunc` accepts it, except the 1-D `align`
itself: `align(..., trunc=...)` keeps raising NotImplementedError as it always has (nothing in the reference calls it with trunc; the losses go
through the affine solvers), and the truncated 1-D solve is `align_trunc(x, y, w, trunc)`, which returns what the reference's
`align(x, y, w, trunc)` returns.  `trunc` must be one scalar (a number or a one-element tensor): the reference cannot use a per-element or
per-row one, and here that raises ValueError.  The truncated solutions are differentiable as in the reference: the kernels return indices, and
`a` (alignment.py:139) or scale / shift (:199-209, :286-297, :341-351) are recomputed in torch from the selected samples, so
`torch.autograd.grad` reaches the same two samples.

Not mirrored: `align_depth_affine_irls` (alignment.py:214-226), which nothing in the reference calls."""
from __future__ import annotations

import ctypes as C
from typing import Optional, Tuple

import torch

from . import _lib as L
from ._lib import ptr

MAX_ROW = 15360          # residuals per row (csrc/alignment.hip: a row is sorted inside one CU's LDS)


def _trunc_value(trunc) -> float:
    """trunc as the reference can use it: a number or a tensor of one element (it is broadcast against the (extrema, n) block, :47)."""
    if torch.is_tensor(trunc):
        if trunc.numel() != 1:
            raise ValueError(f"trunc must be a scalar, got a tensor of shape {tuple(trunc.shape)}: the reference broadcasts trunc against the "
                             "(extrema, n) block of its objective (alignment.py:47) and fails on a per-element or per-row trunc")
        return float(trunc.item())
    return float(trunc)


def _trunc_workspace(n: int, rows: int, device):
    b = C.c_int64(0)
    L.check(L.lib.moge_align_trunc_workspace(n, rows, C.byref(b)))          # also rejects rows over MAX_ROW
    return torch.empty(b.value, device=device, dtype=torch.uint8) if b.value else None


def _no_trunc(trunc):
    if trunc is not None:
        raise NotImplementedError("align() solves the untruncated objective only (trunc=None); the truncated 1-D solve of alignment.py:91-144 is "
                                  "align_trunc(x, y, w, trunc), and every other solver of this module accepts trunc")


def align(x: torch.Tensor, y: torch.Tensor, w: torch.Tensor, trunc=None, eps: float = 1e-7) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """alignment.py:52-89: min_a sum_i w_i |a x_i - y_i| per row of the broadcast (..., n) inputs -> a (...), loss (...), index (...) (int64).
    With trunc: NotImplementedError, use align_trunc."""
    _no_trunc(trunc)
    dev = L.device_of("alignment", x, y, w)
    x, y, w = torch.broadcast_tensors(x, y, w)
    bshape, n = x.shape[:-1], x.shape[-1]
    x, y, w = (t.reshape(-1, n).float().contiguous() for t in (x, y, w))
    rows = x.shape[0]
    a = torch.empty(rows, device=dev, dtype=torch.float32)
    loss = torch.empty_like(a)
    index = torch.empty(rows, device=dev, dtype=torch.int32)
    with L.on(dev) as st:
        L.check(L.lib.moge_align_l1(ptr(x), ptr(y), ptr(w), rows, n, eps, ptr(a), ptr(loss), ptr(index), st))
    return a.reshape(bshape), loss.reshape(bshape), index.long().reshape(bshape)


def align_trunc(x: torch.Tensor, y: torch.Tensor, w: torch.Tensor, trunc, eps: float = 1e-7) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """alignment.py:91-144, the reference's align(x, y, w, trunc): min_a sum_i min(trunc, w_i |a x_i - y_i|) per row of the broadcast (..., n)
    inputs -> a (...), loss (...), index (...) (int64).  The kernel picks the element; `a` is gathered outside no_grad as in the reference (:139),
    so it is differentiable."""
    trunc = _trunc_value(trunc)
    dev = L.device_of("alignment", x, y, w)
    x, y, w = torch.broadcast_tensors(x, y, w)
    bshape, n = x.shape[:-1], x.shape[-1]
    x, y, w = x.reshape(-1, n), y.reshape(-1, n), w.reshape(-1, n)
    xk, yk, wk = (t.detach().float().contiguous() for t in (x, y, w))
    rows = xk.shape[0]
    ws = _trunc_workspace(n, rows, dev)
    a = torch.empty(rows, device=dev, dtype=torch.float32)
    loss = torch.empty_like(a)
    index = torch.empty(rows, device=dev, dtype=torch.int32)
    with L.on(dev) as st:
        L.check(L.lib.moge_align_trunc(ptr(xk), ptr(yk), ptr(wk), rows, n, trunc, eps, ptr(ws), ptr(a), ptr(loss), ptr(index), st))
    index = index.long()
    sign = torch.sign(x)
    xs, ys = x * sign, y * sign                                                             # :94-95
    a = ys.gather(-1, index[:, None]) / xs.gather(-1, index[:, None]).clamp_min(eps)        # :139
    return a.reshape(bshape), loss.reshape(bshape), index.reshape(bshape)


def _anchor_search(src: torch.Tensor, tgt: torch.Tensor, weight: torch.Tensor, comp_mask: int, trunc: Optional[float] = None):
    """src / tgt (B, n, d), weight (B, n): one solve per sample with weight > 0 (alignment.py:184 / :269 / :324), then the best anchor per batch
    element (alignment.py:197 / :284 / :339).  -> anchor sample (B,), solution element (B,) in [0, n*d)"""
    B, n, d = src.shape
    dev = src.device
    ab, an = torch.where(weight > 0)
    rows = ab.numel()
    if rows == 0:
        raise ValueError("no sample with weight > 0")
    rb, rk = ab.int().contiguous(), an.int().contiguous()
    scale = torch.empty(rows, device=dev, dtype=torch.float32)
    loss = torch.empty_like(scale)
    index = torch.empty(rows, device=dev, dtype=torch.int32)
    min_loss = torch.empty(B, device=dev, dtype=torch.float32)
    min_row = torch.empty(B, device=dev, dtype=torch.int32)
    ws = _trunc_workspace(n * d, rows, dev) if trunc is not None else None
    with L.on(dev) as st:
        if trunc is None:
            L.check(L.lib.moge_align_l1_anchored(ptr(src), ptr(tgt), ptr(weight), n, d, comp_mask, ptr(rb), ptr(rk), rows, 1e-7, ptr(scale), ptr(loss), ptr(index), st))
        else:
            L.check(L.lib.moge_align_trunc_anchored(ptr(src), ptr(tgt), ptr(weight), n, d, comp_mask, ptr(rb), ptr(rk), rows, trunc, 1e-7, ptr(ws), ptr(scale), ptr(loss),
                                                    ptr(index), st))
        L.check(L.lib.moge_align_select(ptr(loss), ptr(rb), rows, B, ptr(min_loss), ptr(min_row), st))
    sel = min_row.long()
    if bool((sel < 0).any()):
        raise ValueError("a batch element has no sample with weight > 0")       # the reference indexes with -1 here (last anchor of the batch)
    return an[sel], index.long()[sel]


def _align_any(x, y, w, trunc):
    """the solution `a` of the 1-D problem the solvers below reduce to (alignment.py:52-144), with or without trunc"""
    return (align(x, y, w) if trunc is None else align_trunc(x, y, w, trunc))[0]


def align_depth_scale(depth_src: torch.Tensor, depth_tgt: torch.Tensor, weight: Optional[torch.Tensor], trunc=None):
    """alignment.py:149-160"""
    return _align_any(depth_src, depth_tgt, weight, trunc)


def align_depth_affine(depth_src: torch.Tensor, depth_tgt: torch.Tensor, weight: Optional[torch.Tensor], trunc=None):
    """alignment.py:163-212: (..., n) -> scale (...), shift (...)"""
    trunc = None if trunc is None else _trunc_value(trunc)
    L.device_of("alignment", depth_src, depth_tgt, weight)
    bshape, n = depth_src.shape[:-1], depth_src.shape[-1]
    src, tgt, w = (t.reshape(-1, n).float().contiguous() for t in (depth_src, depth_tgt, weight))
    i1, i2 = _anchor_search(src[..., None].detach(), tgt[..., None].detach(), w, 0b1, trunc)
    t1, s1 = tgt.gather(1, i1[:, None])[:, 0], src.gather(1, i1[:, None])[:, 0]
    t2, s2 = tgt.gather(1, i2[:, None])[:, 0], src.gather(1, i2[:, None])[:, 0]
    scale = (t2 - t1) / torch.where(s2 != s1, s2 - s1, torch.full_like(s1, 1e-7))          # :206
    shift = t1 - scale * s1                                                                 # :207
    return scale.reshape(bshape), shift.reshape(bshape)


def align_points_scale(points_src: torch.Tensor, points_tgt: torch.Tensor, weight: Optional[torch.Tensor], trunc=None):
    """alignment.py:228-243: (..., n, 3) -> scale (...)"""
    return _align_any(points_src.flatten(-2), points_tgt.flatten(-2), weight[..., None].expand_as(points_src).flatten(-2), trunc)


def _points_anchor_solve(points_src, points_tgt, weight, comp_mask: int, trunc=None):
    L.device_of("alignment", points_src, points_tgt, weight)
    bshape, n = points_src.shape[:-2], points_src.shape[-2]
    src, tgt, w = points_src.reshape(-1, n, 3).float().contiguous(), points_tgt.reshape(-1, n, 3).float().contiguous(), weight.reshape(-1, n).float().contiguous()
    B = src.shape[0]
    k, i2 = _anchor_search(src.detach(), tgt.detach(), w, comp_mask, trunc)
    i1 = k * 3 + i2 % 3                                                                     # :288 / :342
    m = torch.tensor([(comp_mask >> c) & 1 for c in range(3)], device=src.device, dtype=src.dtype)
    src_a, tgt_a = src * m, tgt * m                                                         # :290-291 (zeros where the anchor is not subtracted)
    t1, s1 = tgt_a.reshape(B, -1).gather(1, i1[:, None])[:, 0], src_a.reshape(B, -1).gather(1, i1[:, None])[:, 0]
    t2, s2 = tgt.reshape(B, -1).gather(1, i2[:, None])[:, 0], src.reshape(B, -1).gather(1, i2[:, None])[:, 0]
    scale = (t2 - t1) / torch.where(s2 != s1, s2 - s1, torch.ones_like(s1))                 # :295 / :348
    rows = torch.arange(B, device=src.device)
    shift = tgt_a[rows, k] - scale[:, None] * src_a[rows, k]                                # :296 / :349
    return scale.reshape(bshape), shift.reshape(*bshape, 3)


def align_points_scale_z_shift(points_src: torch.Tensor, points_tgt: torch.Tensor, weight: Optional[torch.Tensor], trunc=None):
    """alignment.py:246-299: shared xyz scale + shift along z."""
    return _points_anchor_solve(points_src, points_tgt, weight, 0b100, None if trunc is None else _trunc_value(trunc))


def align_points_scale_xyz_shift(points_src: torch.Tensor, points_tgt: torch.Tensor, weight: Optional[torch.Tensor], trunc=None, max_iters: int = 30, eps: float = 1e-6):
    """alignment.py:302-354: shared xyz scale + xyz shift (max_iters / eps are unused in the reference as well)."""
    return _points_anchor_solve(points_src, points_tgt, weight, 0b111, None if trunc is None else _trunc_value(trunc))


def align_points_z_shift(points_src: torch.Tensor, points_tgt: torch.Tensor, weight: Optional[torch.Tensor], trunc=None, max_iters: int = 30, eps: float = 1e-6):
    """alignment.py:357-376"""
    shift = _align_any(torch.ones_like(points_src[..., 2]), points_tgt[..., 2] - points_src[..., 2], weight, trunc)
    return torch.stack([torch.zeros_like(shift), torch.zeros_like(shift), shift], dim=-1)


def align_points_xyz_shift(points_src: torch.Tensor, points_tgt: torch.Tensor, weight: Optional[torch.Tensor], trunc=None, max_iters: int = 30, eps: float = 1e-6):
    """alignment.py:379-396"""
    return _align_any(torch.ones_like(points_src).swapaxes(-2, -1), (points_tgt - points_src).swapaxes(-2, -1), weight[..., None, :], trunc)


def align_affine_lstsq(x: torch.Tensor, y: torch.Tensor, w: torch.Tensor = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """alignment.py:399-415: least-squares (a, b) of sqrt(w) x a + b ~ sqrt(w) y per row of (..., N)."""
    dev = L.device_of("alignment", x, y, w)
    bshape, n = x.shape[:-1], x.shape[-1]
    xs, ys = x.reshape(-1, n).float().contiguous(), y.reshape(-1, n).float().contiguous()
    ws = w.reshape(-1, n).float().contiguous() if w is not None else None
    rows = xs.shape[0]
    a = torch.empty(rows, device=dev, dtype=torch.float32)
    b = torch.empty_like(a)
    with L.on(dev) as st:
        L.check(L.lib.moge_align_lstsq(ptr(xs), ptr(ys), ptr(ws), rows, n, ptr(a), ptr(b), st))
    return a.reshape(bshape), b.reshape(bshape)
