"""Training losses on the MI355X: the mirror of the reference's `moge/train/losses.py` (same names, argument order and defaults), calling the HIP
kernels of `csrc/losses.hip` through the C ABI (`moge_loss_*`), forward and backward through `torch.autograd.Function`.
DESIGN.md section 15 has the formulas, the launch structure and the reproducibility scheme.

    from moge_amd.losses import normal_loss, edge_loss, mask_bce_loss
    loss, misc = edge_loss(pred_points, gt_points)         # (B,) for (B, H, W, 3) inputs: one value per image
    loss.sum().backward()

Covered: `affine_invariant_global_loss`, `normal_loss`, `edge_loss`, `mask_l2_loss`, `mask_bce_loss`, `metric_scale_loss`, `normal_map_loss`,
`affine_invariant_local_loss`, `compute_anchor_sampling_weight`: every loss of the reference.

Every tensor must live on the GPU (`cuda`); there is no CPU path here.  Computed in fp32 (other dtypes are upcast and the results cast back),
per-image sums carried in fp64.  Differences from the reference, all on purpose:
  * leading batch dims are accepted everywhere and `result[i]` equals the reference called on instance `i`, which is how its train.py calls it.
    `normal_loss`, whose reference takes `.mean()` over everything it is given, therefore returns one value per instance;
  * the `misc` values are 0-d / (B,) device tensors, not Python floats: nothing calls `.item()`;
  * no call synchronises with the host - except `affine_invariant_global_loss` and `affine_invariant_local_loss`: their alignment solve is
    `moge_amd.alignment`'s as it stands (it sizes its anchor search on the host, and raises ValueError from there), and the local loss reads the
    number of non-empty patches - and nothing is validated on the host that would need the data (`mask_bce_loss` does not check that the
    probabilities lie in [0, 1] as `F.binary_cross_entropy` does);
  * gradients flow to the prediction only (`points`, `pred_mask`, `pred_mask_prob`, `scale_pred`, `pred_normal`), never to a `gt_*` argument;
  * the same inputs give the same loss and gradient bits on every call, and an instance gives the same bits alone as inside a batch: sums run
    in a fixed order and gradients are gathered per pixel, without float atomics;
  * `normal_map_loss` needs `utils3d.pt.angle_between`, which is not vendored: it is restated as atan2(|a x b|, a . b), an UNPINNED convention
    like the other utils3d stand-ins;
  * `compute_anchor_sampling_weight` draws its test offsets from a counter-based hash inside the kernel (seed and offset from `generator`, or
    from torch's default CUDA generator).  It does not reproduce torch's `randint` stream and does not claim to; a pixel's draws do not
    depend on the image it is in: the images of one call test the same offsets at the same pixel, where the reference's draws are independent.
    Each image's weights are the same unbiased estimate either way, and the anchors are then drawn per image by `torch.multinomial`, so anchors
    of different images are correlated only through that shared noise of the weights;
  * `affine_invariant_local_loss` takes the randomness as an input: `anchors=(patch_image, patch_i, patch_j)` (int64) is fully deterministic;
    `anchors=None` samples `num_patches` anchors per image (the reference draws `num_patches * batch` over the whole batch, which it can only be
    given one image of: its line 134 is a shape error for a batch).  `global_scale` and `focal` are indexed by the patch's image."""
from __future__ import annotations

import ctypes as C
import math
from typing import Optional, Tuple

import torch

from . import _lib as L
from . import alignment as A
from ._lib import ptr

TILE_W, TILE_H, SPAN = L.LOSS_TILE_W, L.LOSS_TILE_H, L.LOSS_SPAN      # csrc/losses.hip: the tests place shapes around them


def _workspace(dev, B: int, H: int, W: int) -> torch.Tensor:
    nbytes = C.c_int64(0)
    L.check(L.lib.moge_loss_workspace(B, H, W, C.byref(nbytes)))
    return torch.empty(nbytes.value, device=dev, dtype=torch.uint8)


def _maps(name: str, pred: torch.Tensor, channels: int, **others: torch.Tensor) -> Tuple[int, int, int]:
    """Shape check of a (..., H, W[, channels]) prediction and the maps that go with it -> (B, H, W)."""
    tail = (channels,) if channels else ()
    if pred.dim() < 2 + len(tail) or (channels and pred.shape[-1] != channels):
        raise ValueError(f"{name}: expected (..., H, W{', %d' % channels if channels else ''}), got {tuple(pred.shape)}")
    for key, t in others.items():
        want = pred.shape if t.dim() == pred.dim() else pred.shape[:pred.dim() - len(tail)]
        if t.shape != want:
            raise ValueError(f"{name}: {key} {tuple(t.shape)} does not match {tuple(pred.shape)}")
    H, W = pred.shape[-2 - len(tail):pred.dim() - len(tail)]
    if H < 1 or W < 1:
        raise ValueError(f"{name}: an empty {H} x {W} map")
    B = 1
    for s in pred.shape[:-2 - len(tail)]:
        B *= s
    return B, H, W


class _Stencil(torch.autograd.Function):
    """normal_loss / edge_loss on flat fp32 (B, H, W, 3) tensors -> (B,)"""

    @staticmethod
    def forward(ctx, points, gt, edge: bool):
        B, H, W, _ = points.shape
        dev = points.device
        loss = torch.empty(B, device=dev, dtype=torch.float32)
        if B:
            ws = _workspace(dev, B, H, W)
            with L.on(dev) as st:
                L.check((L.lib.moge_loss_edge if edge else L.lib.moge_loss_normal)(ptr(points), ptr(gt), B, H, W, ptr(ws), ptr(loss), st))
        ctx.save_for_backward(points, gt)
        ctx.edge = edge
        return loss

    @staticmethod
    def backward(ctx, grad_loss):
        points, gt = ctx.saved_tensors
        B, H, W, _ = points.shape
        grad = torch.empty_like(points)
        if B:
            go = grad_loss.float().contiguous()
            with L.on(points.device) as st:
                L.check((L.lib.moge_loss_edge_backward if ctx.edge else L.lib.moge_loss_normal_backward)(ptr(points), ptr(gt), ptr(go), B, H, W, ptr(grad), st))
        return grad, None, None


class _Pixel(torch.autograd.Function):
    """the per-image mean of an elementwise term (moge_loss_pixel) on flat fp32 tensors -> (B,)"""

    @staticmethod
    def forward(ctx, pred, gt, pos, neg, kind: int):
        B, H, W = pred.shape[:3]
        dev = pred.device
        loss = torch.empty(B, device=dev, dtype=torch.float32)
        if B:
            ws = _workspace(dev, B, H, W)
            with L.on(dev) as st:
                L.check(L.lib.moge_loss_pixel(kind, ptr(pred), ptr(gt), ptr(pos), ptr(neg), B, H, W, ptr(ws), ptr(loss), st))
        ctx.save_for_backward(pred, gt, pos, neg)
        ctx.kind = kind
        return loss

    @staticmethod
    def backward(ctx, grad_loss):
        pred, gt, pos, neg = ctx.saved_tensors
        B, H, W = pred.shape[:3]
        grad = torch.empty_like(pred)
        if B:
            go = grad_loss.float().contiguous()
            with L.on(pred.device) as st:
                L.check(L.lib.moge_loss_pixel_backward(ctx.kind, ptr(pred), ptr(gt), ptr(pos), ptr(neg), ptr(go), B, H, W, ptr(grad), st))
        return grad, None, None, None, None


class _MetricScale(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pred, gt):
        out = torch.empty_like(pred)
        if pred.numel():
            with L.on(pred.device) as st:
                L.check(L.lib.moge_loss_metric_scale(ptr(pred), ptr(gt), None, pred.numel(), ptr(out), st))
        ctx.save_for_backward(pred, gt)
        return out

    @staticmethod
    def backward(ctx, grad_out):
        pred, gt = ctx.saved_tensors
        grad = torch.empty_like(pred)
        if pred.numel():
            go = grad_out.float().contiguous()
            with L.on(pred.device) as st:
                L.check(L.lib.moge_loss_metric_scale(ptr(pred), ptr(gt), ptr(go), pred.numel(), ptr(grad), st))
        return grad, None


class _AffineDense(torch.autograd.Function):
    """moge_loss_affine_dense on flat fp32 tensors: pred / gt (B, H, W, 3), scale (B), shift (B, 3), lr_frac (B) or None -> loss (B), misc (B, 2)"""

    @staticmethod
    def forward(ctx, pred, gt, scale, shift, lr_frac, beta: float):
        B, H, W, _ = pred.shape
        dev = pred.device
        loss = torch.empty(B, device=dev, dtype=torch.float32)
        misc = torch.empty(B, 2, device=dev, dtype=torch.float32)
        cap = torch.empty(B, device=dev, dtype=torch.float32)
        norm = torch.empty(B, device=dev, dtype=torch.float64)
        scale, shift = scale.contiguous(), shift.contiguous()
        if B:
            ws = _workspace(dev, B, H, W)
            with L.on(dev) as st:
                L.check(L.lib.moge_loss_affine_dense(ptr(pred), ptr(gt), ptr(scale), ptr(shift), ptr(lr_frac), B, H, W, beta, ptr(ws), ptr(cap), ptr(norm), ptr(loss),
                                                     ptr(misc), st))
        ctx.save_for_backward(pred, gt, scale, shift, cap, norm)
        ctx.beta = beta
        ctx.mark_non_differentiable(misc)
        return loss, misc

    @staticmethod
    def backward(ctx, grad_loss, _grad_misc):
        pred, gt, scale, shift, cap, norm = ctx.saved_tensors
        B, H, W, _ = pred.shape
        grad_pred, grad_scale, grad_shift = torch.empty_like(pred), torch.empty_like(scale), torch.empty_like(shift)
        if B:
            go = grad_loss.float().contiguous()
            ws = _workspace(pred.device, B, H, W)
            with L.on(pred.device) as st:
                L.check(L.lib.moge_loss_affine_dense_backward(ptr(pred), ptr(gt), ptr(scale), ptr(shift), ptr(cap), ptr(norm), ptr(go), B, H, W, ctx.beta, ptr(ws),
                                                              ptr(grad_pred), ptr(grad_scale), ptr(grad_shift), st))
        return grad_pred, None, grad_scale, grad_shift, None, None


def affine_dense_loss(pred_points: torch.Tensor, gt_points: torch.Tensor, scale: torch.Tensor, shift: torch.Tensor, lr_frac: Optional[torch.Tensor] = None,
                      beta: float = 0.0):
    """The part of `affine_invariant_global_loss` behind its alignment solve (losses.py:49-67), for a scale (...) and shift (..., 3) that are
    given: -> (loss (...), misc).  lr_frac (...), the valid fraction of the solve's low-resolution samples, turns the sparsity term on.
    Differentiable for pred_points, scale and shift."""
    L.device_of("losses", pred_points, gt_points, scale, shift, lr_frac)
    B, H, W = _maps("affine_dense_loss", pred_points, 3, gt_points=gt_points)
    batch = pred_points.shape[:-3]
    if scale.shape != batch or shift.shape != batch + (3,) or (lr_frac is not None and lr_frac.shape != batch):
        raise ValueError(f"affine_dense_loss: expected scale {tuple(batch)}, shift {tuple(batch) + (3,)}, got {tuple(scale.shape)}, {tuple(shift.shape)}")
    if not beta >= 0:
        raise ValueError(f"affine_dense_loss: beta must be >= 0, got {beta}")
    valid = scale > 0                                          # losses.py:46-47: a non-positive scale reads as scale 0, shift 0
    scale, shift = torch.where(valid, scale, torch.zeros_like(scale)), torch.where(valid[..., None], shift, torch.zeros_like(shift))
    loss, misc = _AffineDense.apply(pred_points.reshape(B, H, W, 3).float().contiguous(), gt_points.detach().reshape(B, H, W, 3).float().contiguous(),
                                    scale.reshape(B).float(), shift.reshape(B, 3).float(), None if lr_frac is None else lr_frac.detach().reshape(B).float().contiguous(),
                                    float(beta))
    return loss.reshape(batch).to(pred_points.dtype), {"truncated_error": misc[:, 0].reshape(batch), "delta": misc[:, 1].reshape(batch)}


def lr_samples(gt_points: torch.Tensor, size: Tuple[int, int]):
    """The low-resolution sampling of an alignment solve for a batch: gt_points (B, H, W, 3) fp32 contiguous -> lr_mask (B, h * w) bool, rows, cols
    (B, h * w) int64: per cell the nearest finite gt pixel, by the convention of `moge_amd.metrics.masked_nearest_resize` (UNPINNED)."""
    B, H, W, _ = gt_points.shape
    h, w = size
    lr_mask = torch.empty(B, h * w, device=gt_points.device, dtype=torch.uint8)
    index = torch.empty(B, 2, h * w, device=gt_points.device, dtype=torch.int32)
    if B:
        with L.on(gt_points.device) as st:
            L.check(L.lib.moge_loss_lr_sample(ptr(gt_points), B, H, W, h, w, ptr(lr_mask), ptr(index), st))
    return lr_mask.bool(), index[:, 0].long(), index[:, 1].long()


def affine_invariant_global_loss(pred_points: torch.Tensor, gt_points: torch.Tensor, align_resolution: int = 64, beta: float = 0.0, trunc: float = 1.0,
                                 sparsity_aware: bool = False):
    """losses.py:30-69.  pred_points, gt_points (..., H, W, 3) -> (loss (...), misc, scale (...) detached): the truncated-L1 scale / z-shift
    alignment of the align_resolution^2 nearest valid samples (`moge_amd.alignment.align_points_scale_z_shift`, trunc=), then the weighted
    smooth-L1 of the aligned prediction.  The gradient for pred_points is the direct term plus the path through scale and shift, which the
    solver recomputes in torch from the samples it selected.  misc = {'truncated_error', 'delta'} as (...) device tensors.  An instance without
    a finite gt pixel raises ValueError in the solve (the reference indexes its anchors with -1 there)."""
    L.device_of("losses", pred_points, gt_points)
    B, H, W = _maps("affine_invariant_global_loss", pred_points, 3, gt_points=gt_points)
    align_resolution = int(align_resolution)
    if align_resolution < 1:
        raise ValueError(f"affine_invariant_global_loss: align_resolution must be >= 1, got {align_resolution}")
    if not beta >= 0:
        raise ValueError(f"affine_invariant_global_loss: beta must be >= 0, got {beta}")
    batch = pred_points.shape[:-3]
    pred = pred_points.reshape(B, H, W, 3).float().contiguous()
    gt = gt_points.detach().reshape(B, H, W, 3).float().contiguous()
    lr_mask, rows, cols = lr_samples(gt, (align_resolution, align_resolution))
    image = torch.arange(B, device=pred.device)[:, None]
    pred_lr, gt_lr = pred[image, rows, cols], gt[image, rows, cols]                                  # (B, n, 3); cells without a valid pixel carry weight 0
    gt_lr = torch.where(torch.isfinite(gt_lr).all(dim=-1, keepdim=True), gt_lr, torch.ones_like(gt_lr))
    weight = lr_mask.float() / gt_lr[..., 2].clamp_min(1e-2)                                           # :45
    scale, shift = A.align_points_scale_z_shift(pred_lr, gt_lr, weight, trunc=trunc)
    valid = scale > 0                                                                                   # :46-47
    scale, shift = torch.where(valid, scale, torch.zeros_like(scale)), torch.where(valid[:, None], shift, torch.zeros_like(shift))
    lr_frac = lr_mask.float().mean(dim=-1) if sparsity_aware else None
    loss, misc = _AffineDense.apply(pred, gt, scale, shift, lr_frac, float(beta))
    return (loss.reshape(batch).to(pred_points.dtype), {"truncated_error": misc[:, 0].reshape(batch), "delta": misc[:, 1].reshape(batch)},
            scale.detach().reshape(batch))


class _PatchLoss(torch.autograd.Function):
    """moge_loss_patch on flat fp32 tensors and sorted patches -> loss (B), misc (B, 2); differentiable for pred, scale (P) and shift (P, 3)"""

    @staticmethod
    def forward(ctx, pred, gt, scale, shift, patches, radius, mask, gt_mean, lr_frac, row_start, r: int, num_patches: int, beta: float):
        B, H, W, _ = pred.shape
        pb, pi, pj = patches
        P, dev = pb.numel(), pred.device
        loss = torch.empty(B, device=dev, dtype=torch.float32)
        misc = torch.empty(B, 2, device=dev, dtype=torch.float32)
        out = torch.empty(max(P, 1), 4, device=dev, dtype=torch.float64)
        norm = torch.empty(max(P, 1), device=dev, dtype=torch.float64)
        scale, shift = scale.contiguous(), shift.contiguous()
        with L.on(dev) as st:
            L.check(L.lib.moge_loss_patch(ptr(pred), ptr(gt), ptr(pb), ptr(pi), ptr(pj), ptr(radius), ptr(mask), ptr(scale), ptr(shift), ptr(gt_mean), ptr(lr_frac), P, B,
                                          H, W, r, num_patches, beta, ptr(out), ptr(norm), ptr(loss), ptr(misc), st))
        ctx.save_for_backward(pred, gt, scale, shift, pb, pi, pj, mask, gt_mean, norm, row_start)
        ctx.r, ctx.beta = r, beta
        ctx.mark_non_differentiable(misc)
        return loss, misc

    @staticmethod
    def backward(ctx, grad_loss, _grad_misc):
        pred, gt, scale, shift, pb, pi, pj, mask, gt_mean, norm, row_start = ctx.saved_tensors
        B, H, W, _ = pred.shape
        grad_pred, grad_scale, grad_shift = torch.empty_like(pred), torch.empty_like(scale), torch.empty_like(shift)
        go = grad_loss.float().contiguous()
        with L.on(pred.device) as st:
            L.check(L.lib.moge_loss_patch_backward(ptr(pred), ptr(gt), ptr(pb), ptr(pi), ptr(pj), ptr(mask), ptr(scale), ptr(shift), ptr(gt_mean), ptr(norm), ptr(go),
                                                   ptr(row_start), pb.numel(), B, H, W, ctx.r, ctx.beta, ptr(grad_pred), ptr(grad_scale), ptr(grad_shift), st))
        return (grad_pred, None, grad_scale, grad_shift) + (None,) * 9


def local_patches(gt: torch.Tensor, focal: torch.Tensor, anchors, level: float, align_resolution: int):
    """The patches of `affine_invariant_local_loss` for gt (B, H, W, 3) fp32 contiguous and focal (B) fp32: anchors = (patch_image, patch_i, patch_j) ->
    dict of the NON-EMPTY patches (>= 32 points) sorted by (image, anchor row): image / i / j (P) int32, order (P) = their places in `anchors`,
    radius (P), mask (P, S, S) u8, lr_mask (P, n) bool and rows / cols (P, n) int64 = the full-map pixels of the n = align_resolution^2 samples."""
    B, H, W, _ = gt.shape
    dev = gt.device
    r = math.ceil(0.5 / level * (H ** 2 + W ** 2) ** 0.5)
    S = 2 * r + 1
    pb, pi, pj = (a.reshape(-1).to(dev).long().clamp(0, hi - 1) for a, hi in zip(anchors, (B, H, W)))      # out-of-range anchors: clamped before the sort
    order = torch.argsort(pb * H + pi, stable=True)
    pb, pi, pj = (a[order].int().contiguous() for a in (pb, pi, pj))
    P = pb.numel()
    mask = torch.empty(P, S, S, device=dev, dtype=torch.uint8)
    count = torch.empty(P, device=dev, dtype=torch.int32)
    radius = torch.empty(P, device=dev, dtype=torch.float32)
    with L.on(dev) as st:
        L.check(L.lib.moge_loss_patch_mask(ptr(gt), ptr(focal), ptr(pb), ptr(pi), ptr(pj), P, B, H, W, r, 0.5 / level, ptr(mask), ptr(count), ptr(radius), st))
    keep = torch.where(count >= 32)[0]                                                       # losses.py:159-160 (reads the count on the host)
    pb, pi, pj, mask, radius, order = pb[keep].contiguous(), pi[keep].contiguous(), pj[keep].contiguous(), mask[keep].contiguous(), radius[keep].contiguous(), order[keep]
    P, n = pb.numel(), align_resolution * align_resolution
    lr_mask = torch.empty(P, n, device=dev, dtype=torch.uint8)
    index = torch.empty(P, 2, n, device=dev, dtype=torch.int32)
    if P:
        with L.on(dev) as st:
            L.check(L.lib.moge_loss_patch_lr_sample(ptr(mask), P, S, align_resolution, align_resolution, ptr(lr_mask), ptr(index), st))
    rows = (pi[:, None].long() - r + index[:, 0].long()).clamp(0, H - 1)
    cols = (pj[:, None].long() - r + index[:, 1].long()).clamp(0, W - 1)
    return dict(image=pb, i=pi, j=pj, order=order, radius=radius, mask=mask, lr_mask=lr_mask.bool(), rows=rows, cols=cols, radius_2d=r)


def local_patch_loss(pred: torch.Tensor, gt: torch.Tensor, patches: dict, scale: torch.Tensor, shift: torch.Tensor, num_patches: int, beta: float = 0.0,
                     sparsity_aware: bool = False):
    """The part of `affine_invariant_local_loss` behind the per-patch solve, for patch scales (P) and shifts (P, 3) that are given (0 scale: the patch
    takes no part): pred / gt (B, H, W, 3) fp32 contiguous, patches from `local_patches` -> loss (B), misc (B, 2)."""
    B, H, W, _ = pred.shape
    dev = pred.device
    gt_mean = torch.empty(B, device=dev, dtype=torch.float32)
    ws = _workspace(dev, B, H, W)
    with L.on(dev) as st:
        L.check(L.lib.moge_loss_harmonic_mean(ptr(gt), B, H, W, ptr(ws), ptr(gt_mean), st))
    key = patches["image"].long() * H + patches["i"].long()
    row_start = torch.searchsorted(key, torch.arange(B * H + 1, device=dev)).int().contiguous()
    lr_frac = patches["lr_mask"].float().mean(dim=-1).contiguous() if sparsity_aware else None
    return _PatchLoss.apply(pred, gt, scale.float(), shift.float(), (patches["image"], patches["i"], patches["j"]), patches["radius"], patches["mask"], gt_mean, lr_frac,
                            row_start, patches["radius_2d"], int(num_patches), float(beta))


def affine_invariant_local_loss(pred_points: torch.Tensor, gt_points: torch.Tensor, focal: torch.Tensor, global_scale: Optional[torch.Tensor], level: int,
                                align_resolution: int = 32, num_patches: int = 16, beta: float = 0.0, trunc: float = 1.0, sparsity_aware: bool = False,
                                anchors=None, generator: Optional[torch.Generator] = None):
    """losses.py:112-206.  pred_points, gt_points (..., H, W, 3), focal (...), global_scale (...) or None -> (loss (...), misc): per image, `num_patches`
    windows of radius ceil(0.5 / level * diagonal) around anchor pixels, each cut to the gt points within radius_3d of its anchor, aligned on its own
    (truncated-L1 scale / xyz-shift of align_resolution^2 samples) and scored; loss[i] = the sum over image i's patches / num_patches, which is the
    reference called on instance i with those anchors.  anchors = (patch_image, patch_i, patch_j) int64 tensors, or None: then they are drawn as
    the reference draws them (`compute_anchor_sampling_weight`, then `torch.multinomial` per image, both from `generator`).  With no non-empty
    patch in the whole call the result is (0, {}) as in the reference; an image without one contributes 0.  misc = {'truncated_error', 'delta'}
    as (...) device tensors."""
    dev = L.device_of("losses", pred_points, gt_points, focal, global_scale)
    B, H, W = _maps("affine_invariant_local_loss", pred_points, 3, gt_points=gt_points)
    batch = pred_points.shape[:-3]
    if focal.numel() != B or (global_scale is not None and global_scale.numel() != B):
        raise ValueError(f"affine_invariant_local_loss: focal and global_scale must have one value per image ({B}), got {tuple(focal.shape)}")
    if not level > 0 or int(align_resolution) < 1 or int(num_patches) < 1 or not beta >= 0:
        raise ValueError("affine_invariant_local_loss: need level > 0, align_resolution >= 1, num_patches >= 1 and beta >= 0")
    align_resolution, num_patches = int(align_resolution), int(num_patches)
    pred = pred_points.reshape(B, H, W, 3).float().contiguous()
    gt = gt_points.detach().reshape(B, H, W, 3).float().contiguous()
    focal = focal.detach().reshape(B).float().contiguous()
    gscale = None if global_scale is None else global_scale.detach().reshape(B).float()
    if anchors is None:
        gt_mask = torch.isfinite(gt).all(dim=-1)
        gt_clean = torch.where(gt_mask[..., None], gt, torch.ones_like(gt))
        radius_2d = math.ceil(0.5 / level * (H ** 2 + W ** 2) ** 0.5)
        weight = compute_anchor_sampling_weight(gt_clean, gt_mask, radius_2d, 0.5 / level / focal[:, None, None] * gt_clean[..., 2], 64, generator).reshape(B, -1)
        weight = torch.where(weight.sum(dim=-1, keepdim=True) > 0, weight, torch.ones_like(weight))      # no valid pixel: any anchors, every patch is empty
        pick = torch.multinomial(weight, num_patches, replacement=True, generator=generator)
        anchors = (torch.arange(B, device=dev)[:, None].expand_as(pick), pick // W, pick % W)
    elif len(anchors) != 3 or not (anchors[0].numel() == anchors[1].numel() == anchors[2].numel()):
        raise ValueError("affine_invariant_local_loss: anchors must be (patch_image, patch_i, patch_j) of one length")
    patches = local_patches(gt, focal, anchors, level, align_resolution)
    if patches["image"].numel() == 0:
        return torch.zeros(batch, dtype=pred_points.dtype, device=dev), {}
    image = patches["image"].long()[:, None]
    pred_lr, gt_lr = pred[image, patches["rows"], patches["cols"]], gt[image, patches["rows"], patches["cols"]]
    gt_lr = torch.where(torch.isfinite(gt_lr).all(dim=-1, keepdim=True), gt_lr, torch.ones_like(gt_lr))
    weight = patches["lr_mask"].float() / (patches["radius"][:, None] + 1e-7)                           # :175
    scale, shift = A.align_points_scale_xyz_shift(pred_lr, gt_lr, weight, trunc=trunc)
    if gscale is not None:                                                                             # :176-181
        ratio = scale.detach() / gscale[image[:, 0]]
        valid = (ratio > 0.1) & (ratio < 10.0) & (gscale[image[:, 0]] > 0)
    else:
        valid = scale > 0
    scale, shift = torch.where(valid, scale, torch.zeros_like(scale)), torch.where(valid[:, None], shift, torch.zeros_like(shift))
    loss, misc = local_patch_loss(pred, gt, patches, scale, shift, num_patches, beta, sparsity_aware)
    return loss.reshape(batch).to(pred_points.dtype), {"truncated_error": misc[:, 0].reshape(batch), "delta": misc[:, 1].reshape(batch)}


def _stencil(name: str, points: torch.Tensor, gt_points: torch.Tensor, edge: bool):
    L.device_of("losses", points, gt_points)
    B, H, W = _maps(name, points, 3, gt_points=gt_points)
    loss = _Stencil.apply(points.reshape(B, H, W, 3).float().contiguous(), gt_points.detach().reshape(B, H, W, 3).float().contiguous(), edge)
    return loss.reshape(points.shape[:-3]).to(points.dtype), {}


def normal_loss(points: torch.Tensor, gt_points: torch.Tensor):
    """losses.py:209-243.  points, gt_points (..., H, W, 3) -> (loss (...), {}): per instance, the mean over the (H-1)(W-1) quads of the four
    corner-normal angle terms (clamp [1, 90] degrees, smooth-L1 at 3 degrees), divided by 4 max(H, W).  The reference's `.mean()` runs over the
    batch too; here every instance has its own value (the reference called on that instance).  H = 1 or W = 1: NaN, torch's mean of nothing."""
    return _stencil("normal_loss", points, gt_points, False)


def edge_loss(points: torch.Tensor, gt_points: torch.Tensor):
    """losses.py:246-268.  points, gt_points (..., H, W, 3) -> (loss (...), {}): the angle terms of the row and column neighbour differences (clamp
    [0.1, 90] degrees, smooth-L1 at 3 degrees), (mean + mean) / (2 max(H, W)).  H = 1 or W = 1: NaN, as the reference (one mean is over nothing)."""
    return _stencil("edge_loss", points, gt_points, True)


def _mask_loss(name: str, kind: int, pred: torch.Tensor, gt_mask_pos: torch.Tensor, gt_mask_neg: torch.Tensor):
    L.device_of("losses", pred, gt_mask_pos, gt_mask_neg)
    B, H, W = _maps(name, pred, 0, gt_mask_pos=gt_mask_pos, gt_mask_neg=gt_mask_neg)
    pos, neg = (m.reshape(B, H, W).to(torch.bool).to(torch.uint8).contiguous() for m in (gt_mask_pos, gt_mask_neg))
    loss = _Pixel.apply(pred.reshape(B, H, W).float().contiguous(), None, pos, neg, kind)
    return loss.reshape(pred.shape[:-2]).to(pred.dtype), {}


def mask_l2_loss(pred_mask: torch.Tensor, gt_mask_pos: torch.Tensor, gt_mask_neg: torch.Tensor):
    """losses.py:271-274.  pred_mask (..., H, W), gt_mask_pos / gt_mask_neg (..., H, W) bool -> (mean of neg p^2 + pos (1 - p)^2 over H, W, {})."""
    return _mask_loss("mask_l2_loss", L.LOSS_MASK_L2, pred_mask, gt_mask_pos, gt_mask_neg)


def mask_bce_loss(pred_mask_prob: torch.Tensor, gt_mask_pos: torch.Tensor, gt_mask_neg: torch.Tensor):
    """losses.py:277-280.  (pos | neg) * F.binary_cross_entropy(prob, pos), mean over H, W, with its log clamp at -100 and its backward's 1e-12.
    The probabilities must lie in [0, 1]; unlike F.binary_cross_entropy this is not checked (it would synchronise)."""
    return _mask_loss("mask_bce_loss", L.LOSS_MASK_BCE, pred_mask_prob, gt_mask_pos, gt_mask_neg)


def metric_scale_loss(scale_pred: torch.Tensor, scale_gt: torch.Tensor):
    """losses.py:283-285.  Elementwise (log scale_pred - log scale_gt)^2 where scale_gt > 0, else 0 (value and gradient); any common shape."""
    L.device_of("losses", scale_pred, scale_gt)
    if not isinstance(scale_pred, torch.Tensor) or not isinstance(scale_gt, torch.Tensor) or scale_pred.shape != scale_gt.shape:
        raise ValueError(f"metric_scale_loss: scale_gt {tuple(scale_gt.shape)} does not match scale_pred {tuple(scale_pred.shape)}")
    out = _MetricScale.apply(scale_pred.reshape(-1).float().contiguous(), scale_gt.detach().reshape(-1).float().contiguous())
    return out.reshape(scale_pred.shape).to(scale_pred.dtype), {}


def normal_map_loss(pred_normal: torch.Tensor, gt_normal: torch.Tensor):
    """losses.py:288-293.  pred_normal, gt_normal (..., H, W, 3) -> (mean over H, W of mask * angle_between(pred, gt)^2, {}) with mask = gt finite.
    `utils3d.pt.angle_between` is not vendored: restated as atan2(|a x b|, a . b), UNPINNED (see the module docstring)."""
    L.device_of("losses", pred_normal, gt_normal)
    B, H, W = _maps("normal_map_loss", pred_normal, 3, gt_normal=gt_normal)
    loss = _Pixel.apply(pred_normal.reshape(B, H, W, 3).float().contiguous(), gt_normal.detach().reshape(B, H, W, 3).float().contiguous(), None, None,
                        L.LOSS_NORMAL_MAP)
    return loss.reshape(pred_normal.shape[:-3]).to(pred_normal.dtype), {}


def _philox(generator: Optional[torch.Generator], dev) -> Tuple[int, int]:
    """(seed, offset) for one kernel call, advancing the generator (None: the device's default CUDA generator) by one step.  The offset is read
    from and written back to the generator's state on the host; no device synchronisation."""
    gen = generator if generator is not None else torch.cuda.default_generators[dev.index if dev.index is not None else torch.cuda.current_device()]
    seed, offset = gen.initial_seed(), gen.get_offset()
    gen.set_offset(offset + 4)            # torch keeps the offset a multiple of 4
    return seed & (2 ** 64 - 1), offset & (2 ** 64 - 1)


def anchor_sampling_counts(points: torch.Tensor, mask: torch.Tensor, radius_2d: int, radius_3d: torch.Tensor, num_test: int = 64,
                           generator: Optional[torch.Generator] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """`compute_anchor_sampling_weight` together with what it normalises: -> (weight (..., H, W) fp32, count (..., H, W) int32), count = how many
    of a valid pixel's num_test draws fell inside the image, on a valid pixel and within radius_3d of its point (0 off the mask)."""
    dev = L.device_of("losses", points, mask, radius_3d)
    B, H, W = _maps("compute_anchor_sampling_weight", points, 3, mask=mask)
    radius_2d, num_test = int(radius_2d), int(num_test)
    if radius_2d < 0 or num_test < 1:
        raise ValueError(f"compute_anchor_sampling_weight: need radius_2d >= 0 and num_test >= 1, got {radius_2d} and {num_test}")
    try:
        r3 = radius_3d.expand(mask.shape)
    except RuntimeError:
        raise ValueError(f"compute_anchor_sampling_weight: radius_3d {tuple(radius_3d.shape)} does not broadcast to {tuple(mask.shape)}") from None
    p = points.detach().reshape(B, H, W, 3).float().contiguous()
    m = mask.reshape(B, H, W).to(torch.bool).to(torch.uint8).contiguous()
    r3 = r3.detach().reshape(B, H, W).float().contiguous()
    weight = torch.empty(B, H, W, device=dev, dtype=torch.float32)
    count = torch.empty(B, H, W, device=dev, dtype=torch.int32)
    if B:
        seed, offset = _philox(generator, dev)
        ws = _workspace(dev, B, H, W)
        with L.on(dev) as st:
            L.check(L.lib.moge_loss_anchor_weight(ptr(p), ptr(m), ptr(r3), B, H, W, radius_2d, num_test, seed, offset, ptr(ws), ptr(count), ptr(weight), st))
    return weight.reshape(mask.shape), count.reshape(mask.shape)


def compute_anchor_sampling_weight(points: torch.Tensor, mask: torch.Tensor, radius_2d: int, radius_3d: torch.Tensor, num_test: int = 64,
                                   generator: Optional[torch.Generator] = None) -> torch.Tensor:
    """losses.py:78-109.  points (..., H, W, 3), mask (..., H, W) bool, radius_2d an int, radius_3d broadcastable to (..., H, W) -> the sampling
    weight (..., H, W) fp32: 1 / max(count, 1) on the mask, 0 off it, each image normalised to sum 1 (all zero where an image's mask is empty).
    `generator` (an extension; None: the default CUDA generator) seeds the kernel's hash RNG, and is advanced by the call."""
    return anchor_sampling_counts(points, mask, radius_2d, radius_3d, num_test, generator)[0]
