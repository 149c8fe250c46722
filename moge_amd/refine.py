"""Normal-guided depth refinement on the MI355X: the mirror of the reference's `moge.utils.geometry_torch.refine_depth_with_normal`
(geometry_torch.py:206-233; same name, argument order and defaults), calling the HIP kernels of `csrc/refine.hip` through the C ABI
(`moge_refine_depth`).  DESIGN.md section 12 has the formula and the launch structure.

    from moge_amd.refine import refine_depth_with_normal
    out = model.infer(image)
    depth = refine_depth_with_normal(out["depth"], out["normal"], out["intrinsics"], mask=out["mask"])      # or model.refine_depth(out)

Every tensor must live on the GPU (`cuda`); there is no CPU path here.  The reference materialises two (H-4)(W-4) x 25 tensors per iteration; the
kernels recompute the bilateral weights from an LDS tile, and the only device memory besides the result is four fp32 planes per image."""
from __future__ import annotations

import ctypes as C
from typing import Optional

import torch

from . import _lib as L
from ._lib import ptr

TILE = 32                   # csrc/refine.hip REFINE_TILE: the square output tile of one workgroup (the tests place shapes around it)
KERNEL_SIZES = (3, 5, 7)


def refine_depth_with_normal(depth: torch.Tensor, normal: torch.Tensor, intrinsics: torch.Tensor, iterations: int = 10, damp: float = 1e-3,
                             eps: float = 1e-12, kernel_size: int = 5, mask: Optional[torch.Tensor] = None) -> torch.Tensor:
    """geometry_torch.py:206-233.  depth (..., H, W), normal (..., H, W, 3) in the camera frame, intrinsics (..., 3, 3) normalised (uv at pixel
    centres in [0, 1], as `moge_amd.io.uv_map`), any leading batch dims -> refined depth, shape and dtype of `depth`.  Computed in fp32.

    Differences from the reference, both on purpose:
      * `depth` is NOT clamped in place (the reference's `depth.clamp_min_(eps)` changes the caller's tensor; here it is left untouched);
      * `mask` (..., H, W) bool, an extension: masked-out pixels take no part, neither as a window tap nor as a centre, whatever they hold
        (inf, NaN), and come back as the bits of their input depth.  mask=None is the reference's formula.

    Outside the contract without a mask, as in the reference, which turns both into NaN regions that grow by the window radius per iteration:
    non-finite depth, and rays perpendicular to the normal (n_z + n_xy . (Kinv[:2,:2] uv + Kinv[:2,2]) = 0, a zero denominator of the
    gradient).  With a mask the same holds for the masked-in pixels.  kernel_size is 3, 5 or 7 and H, W >= kernel_size (ValueError otherwise).
    The call does not synchronise with the host."""
    dev = L.device_of("refine", depth, normal, intrinsics, mask)
    if kernel_size not in KERNEL_SIZES:
        raise ValueError(f"kernel_size must be one of {KERNEL_SIZES}, got {kernel_size}")
    if depth.dim() < 2 or normal.shape[-1] != 3 or normal.shape[:-1] != depth.shape or intrinsics.shape[-2:] != (3, 3):
        raise ValueError(f"expected depth (..., H, W), normal (..., H, W, 3), intrinsics (..., 3, 3); got {tuple(depth.shape)}, "
                         f"{tuple(normal.shape)}, {tuple(intrinsics.shape)}")
    H, W = depth.shape[-2:]
    if H < kernel_size or W < kernel_size:
        raise ValueError(f"a {H} x {W} map is smaller than the {kernel_size} x {kernel_size} window")
    if iterations < 0:
        raise ValueError("iterations must be >= 0")
    if mask is not None and mask.shape != depth.shape:
        raise ValueError(f"mask {tuple(mask.shape)} does not match depth {tuple(depth.shape)}")
    batch = depth.shape[:-2]
    d = depth.reshape(-1, H, W).float().contiguous()
    n = normal.reshape(-1, H, W, 3).float().contiguous()
    k = intrinsics.expand(batch + (3, 3)).reshape(-1, 3, 3).float().contiguous()
    m = mask.reshape(-1, H, W).to(torch.uint8).contiguous() if mask is not None else None
    B = d.shape[0]
    out = torch.empty_like(d)
    if B:
        nbytes = C.c_int64(0)
        L.check(L.lib.moge_refine_depth_workspace(B, H, W, C.byref(nbytes)))
        ws = torch.empty(nbytes.value, device=dev, dtype=torch.uint8)
        with L.on(dev) as st:
            L.check(L.lib.moge_refine_depth(ptr(d), ptr(n), ptr(k), ptr(m), B, H, W, int(kernel_size), int(iterations), float(damp), float(eps), ptr(ws),
                                            ptr(out), st))
    return out.reshape(depth.shape).to(depth.dtype)
