"""Panorama split and merge on the MI355X: the device twins of `moge_amd.panorama.split_panorama_image`, `merge_panorama_depth` and
`infer_panorama` (the host module is the specification, pinned to the reference by tests/test_panorama_reference.py), calling the kernels of
`csrc/panorama.hip` through the C ABI (`moge_pano_*`).  DESIGN.md section 14 has the algorithm, the launches and the determinism rule.

    from moge_amd.panorama_gpu import infer_panorama
    out = infer_panorama(model, torch.from_numpy(panorama_rgb_uint8).cuda())      # {"distance", "mask", "points", ...} CUDA tensors

Same function names and argument order as the host module.  Every tensor must live on the GPU (`cuda`); there is no CPU path here
(`moge_amd.panorama` is the host form).  The cameras (extrinsics, intrinsics) are a few small matrices and stay on the host, as numpy arrays or
tensors.  The merge is a matrix-free LSMR in fp64: the least-squares system is never stored, `merge_system` returns its right-hand side and row
mask and `lsmr` solves it with scipy's recurrences and stopping rule evaluated on the device; the host reads the solver's state once per `poll`
iterations and nothing else synchronises.  The utils3d / cv2 caveat of the host module applies unchanged: the same conventions are restated in
the kernels and pinned through the same golden files."""
from __future__ import annotations

import ctypes as C
from typing import Dict, NamedTuple, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib as L
from ._lib import ptr
from .panorama import get_panorama_cameras, intrinsics_to_fov_x_deg

MAX_VIEWS = L.PANO_MAX_VIEWS        # include/moge_hip.h MOGE_PANO_MAX_VIEWS
SPAN = L.PANO_SPAN                  # MOGE_PANO_SPAN: elements one workgroup sums in the solver's norms
MAX_PIXELS = L.PANO_MAX_PIXELS
POLL = 32                           # iterations enqueued between two reads of the solver's state
LAUNCHES_PER_ITERATION = 6          # av, beta, atu, givens, update, test (csrc/panorama.hip)


class PanoSystem(NamedTuple):
    """One level's least-squares system in the kernels' row layout (include/moge_hip.h): b (M,) float64 and rows (M,) uint8 over the x rows, the
    y rows, the column-0 y rows once more and the Laplacian rows; seen (height, width) bool.  bx / by / bl and rx / ry / rl are views of them in
    the shapes of the host's `merge_system`."""
    width: int
    height: int
    b: torch.Tensor
    rows: torch.Tensor
    seen: torch.Tensor

    def _cut(self, t):
        W, H = self.width, self.height
        N, ny = W * H, (H - 1) * W
        return t[:N], t[N:N + ny], t[N + ny + (H - 1):]

    @property
    def bx(self): return self._cut(self.b)[0].view(self.height, self.width)
    @property
    def by(self): return self._cut(self.b)[1].view(self.height - 1, self.width)
    @property
    def bl(self): return self._cut(self.b)[2].view(self.height, self.width)
    @property
    def rx(self): return self._cut(self.rows)[0].bool()
    @property
    def ry(self): return self._cut(self.rows)[1].bool()
    @property
    def rl(self): return self._cut(self.rows)[2].bool()


def system_rows(width: int, height: int) -> int:
    """M: rows of the system in the kernels' layout."""
    return 2 * width * height + (height - 1) * width + (height - 1)


def workspace_bytes(width: int, height: int, n: int) -> int:
    """moge_pano_merge_workspace: pure arithmetic, no GPU call."""
    nb = C.c_int64(0)
    L.check(L.lib.moge_pano_merge_workspace(int(width), int(height), int(n), C.byref(nb)))
    return nb.value


def _device(*tensors) -> torch.device:
    return L.device_of("panorama_gpu", *tensors, host="moge_amd.panorama", tensors_only=True)


def _cameras(extrinsics, intrinsics, n: Optional[int] = None):
    """-> host float32 arrays (n, 4, 4) and (n, 3, 3), contiguous"""
    def host(a):
        if isinstance(a, torch.Tensor):
            return a.detach().cpu().numpy()
        return np.stack([np.asarray(x.detach().cpu() if isinstance(x, torch.Tensor) else x) for x in a]) if len(a) else np.zeros((0,))
    E, K = np.ascontiguousarray(host(extrinsics), dtype=np.float32), np.ascontiguousarray(host(intrinsics), dtype=np.float32)
    if len(E) == 0 or len(K) == 0:
        raise ValueError("need at least one view (n == 0)")
    if E.ndim != 3 or E.shape[1:] != (4, 4) or K.shape != (len(E), 3, 3):
        raise ValueError(f"expected extrinsics (n, 4, 4) and intrinsics (n, 3, 3), got {E.shape} and {K.shape}")
    if n is not None and len(E) != n:
        raise ValueError(f"{n} views but {len(E)} cameras")
    if len(E) > MAX_VIEWS:
        raise ValueError(f"at most {MAX_VIEWS} views, got {len(E)}")
    return E, K


def _hp(a: np.ndarray):
    return a.ctypes.data_as(C.c_void_p)


def _check_map(width: int, height: int):
    if width < 2 or height < 2 or width * height > MAX_PIXELS:
        raise ValueError(f"need width >= 2, height >= 2 and width * height <= 2^29, got width = {width}, height = {height}")


# ---------------------------------------------------------------------------------------------------------------------------------------
# split
# ---------------------------------------------------------------------------------------------------------------------------------------
def split_panorama_image(image: torch.Tensor, extrinsics, intrinsics, resolution: int) -> torch.Tensor:
    """`moge_amd.panorama.split_panorama_image` on the device: image (H, W, 3) uint8 or float32 -> views (n, resolution, resolution, 3) of the
    image's dtype (uint8 views are ready for `model.infer_uint8`)."""
    dev = _device(image)
    if image.dim() != 3 or image.shape[-1] != 3 or image.dtype not in (torch.uint8, torch.float32):
        raise ValueError(f"expected an (H, W, 3) uint8 or float32 image, got {tuple(image.shape)} {image.dtype}")
    H, W = image.shape[:2]
    resolution = int(resolution)
    if H < 1 or W < 1 or H * W > MAX_PIXELS or not 1 <= resolution <= 16384:
        raise ValueError(f"need a non-empty image of at most 2^29 pixels and 1 <= resolution <= 16384, got {H} x {W}, resolution {resolution}")
    E, K = _cameras(extrinsics, intrinsics)
    img = image.contiguous()
    out = torch.empty((len(E), resolution, resolution, 3), device=dev, dtype=img.dtype)
    with L.on(dev) as st:
        L.check(L.lib.moge_pano_split(ptr(img), int(img.dtype == torch.uint8), H, W, _hp(E), _hp(K), len(E), resolution, ptr(out), st))
    return out


# ---------------------------------------------------------------------------------------------------------------------------------------
# merge
# ---------------------------------------------------------------------------------------------------------------------------------------
def _views(distance_maps, pred_masks):
    if not isinstance(distance_maps, torch.Tensor):
        distance_maps = list(distance_maps)
        if len(distance_maps) == 0:
            raise ValueError("need at least one view (n == 0)")
        _device(*distance_maps)
        distance_maps = torch.stack(distance_maps)
    if not isinstance(pred_masks, torch.Tensor):
        pred_masks = list(pred_masks)
        if len(pred_masks) == 0:
            raise ValueError("need at least one view (n == 0)")
        _device(*pred_masks)
        pred_masks = torch.stack(pred_masks)
    _device(distance_maps, pred_masks)
    if distance_maps.dim() != 3 or distance_maps.dtype != torch.float32:
        raise ValueError(f"distance_maps must be (n, h, w) float32, got {tuple(distance_maps.shape)} {distance_maps.dtype}")
    if pred_masks.shape != distance_maps.shape or pred_masks.dtype not in (torch.bool, torch.uint8):
        raise ValueError(f"pred_masks must be (n, h, w) bool like distance_maps, got {tuple(pred_masks.shape)} {pred_masks.dtype}")
    n, vh, vw = distance_maps.shape
    if n == 0:
        raise ValueError("need at least one view (n == 0)")
    if vh < 1 or vw < 1 or vh * vw > MAX_PIXELS:
        raise ValueError(f"views must be non-empty and at most 2^29 pixels, got {vh} x {vw}")
    return distance_maps.contiguous(), pred_masks.contiguous().view(torch.uint8)


def merge_system(width: int, height: int, distance_maps, pred_masks, extrinsics, intrinsics) -> PanoSystem:
    """The least-squares system of ONE level of the merge, as `moge_amd.panorama.merge_system` builds it on the host: the per-view warps and the
    masked means over the views (two launches) -> PanoSystem.  The matrix itself is never formed."""
    width, height = int(width), int(height)
    dist, masks = _views(distance_maps, pred_masks)
    _check_map(width, height)
    E, K = _cameras(extrinsics, intrinsics, dist.shape[0])
    return _system(width, height, dist, masks, E, K)


def _system(width, height, dist, masks, E, K, _ws=None) -> PanoSystem:
    n, vh, vw = dist.shape
    dev = dist.device
    M = system_rows(width, height)
    ws = _ws if _ws is not None else torch.empty(workspace_bytes(width, height, n), device=dev, dtype=torch.uint8)
    b = torch.empty(M, device=dev, dtype=torch.float64)
    rows = torch.empty(M, device=dev, dtype=torch.uint8)
    seen = torch.empty((height, width), device=dev, dtype=torch.uint8)
    with L.on(dev) as st:
        L.check(L.lib.moge_pano_system(width, height, ptr(dist), ptr(masks), n, vh, vw, _hp(E), _hp(K), ptr(ws), ptr(b), ptr(rows), ptr(seen), st))
    return PanoSystem(width, height, b, rows, seen.view(torch.bool))


def lsmr(system: PanoSystem, x0: Optional[torch.Tensor] = None, atol: float = 1e-5, btol: float = 1e-5, conlim: float = 1e8, maxiter: Optional[int] = None,
         poll: int = POLL, _ws: Optional[torch.Tensor] = None):
    """`scipy.sparse.linalg.lsmr(A, b, atol=, btol=, conlim=, maxiter=, x0=)` for the system of `merge_system`, in fp64 on the device, with scipy's
    recurrences, stopping rule and return values: -> x (width * height,) float64 CUDA, istop, itn, normr, normar, normA, condA, normx.
    maxiter None: min(selected rows, pixels).  The host reads the solver's state once per `poll` iterations; the result does not depend on
    `poll`, and two calls give the same bits."""
    dev = _device(system.b, system.rows)
    W, H = system.width, system.height
    N, M = W * H, system_rows(W, H)
    if system.b.shape != (M,) or system.b.dtype != torch.float64 or system.rows.shape != (M,) or system.rows.dtype != torch.uint8:
        raise ValueError(f"a {W} x {H} system has b float64 and rows uint8 of {M} entries")
    if x0 is not None:
        _device(system.b, x0)
        if x0.numel() != N or x0.dtype != torch.float64:
            raise ValueError(f"x0 must hold {N} float64 values")
        x0 = x0.reshape(-1).contiguous()
    if maxiter is not None and maxiter < 1:
        raise ValueError("maxiter must be >= 1 (or None)")
    if not 1 <= int(poll) <= 65536:
        raise ValueError("poll must be 1 ... 65536")
    info = (C.c_double * 8)()
    ws = _ws if _ws is not None else torch.empty(workspace_bytes(W, H, 0), device=dev, dtype=torch.uint8)
    x = torch.empty(N, device=dev, dtype=torch.float64)
    with L.on(dev) as st:
        L.check(L.lib.moge_pano_lsmr(W, H, ptr(system.b.contiguous()), ptr(system.rows.contiguous()), ptr(x0), float(atol), float(btol), float(conlim),
                                     int(maxiter or 0), int(poll), ptr(ws), ptr(x), info, st))
    return x, int(info[0]), int(info[1]), info[2], info[3], info[4], info[5], info[6]


def _resize_bilinear(src: torch.Tensor, height: int, width: int) -> torch.Tensor:
    H, W = src.shape
    out = torch.empty((height, width), device=src.device, dtype=torch.float32)
    with L.on(src.device) as st:
        L.check(L.lib.moge_pano_resize_bilinear(ptr(src.contiguous()), H, W, height, width, ptr(out), st))
    return out


def _resize_nearest(src: torch.Tensor, height: int, width: int) -> torch.Tensor:
    H, W = src.shape
    out = torch.empty((height, width), device=src.device, dtype=torch.uint8)
    with L.on(src.device) as st:
        L.check(L.lib.moge_pano_resize_nearest(ptr(src.contiguous().view(torch.uint8)), H, W, height, width, ptr(out), st))
    return out.view(torch.bool)


def _merge(width, height, dist, masks, E, K, poll, itns):
    init = None
    if max(width, height) > 256:
        if width // 2 < 1 or height // 2 < 1:          # (the host's recursion fails there too)
            raise ValueError(f"the coarse level of a {width} x {height} map is empty")
        coarse, _ = _merge(width // 2, height // 2, dist, masks, E, K, poll, itns)
        init = _resize_bilinear(coarse, height, width)
    dev = dist.device
    ws = torch.empty(workspace_bytes(width, height, dist.shape[0]), device=dev, dtype=torch.uint8)
    system = _system(width, height, dist, masks, E, K, _ws=ws)
    x0 = None
    if init is not None:
        x0 = torch.empty(width * height, device=dev, dtype=torch.float64)
        with L.on(dev) as st:
            L.check(L.lib.moge_pano_log(ptr(init), width * height, ptr(x0), st))
    x, _, itn, *_ = lsmr(system, x0=x0, atol=1e-5, btol=1e-5, poll=poll, _ws=ws)
    itns.append(itn)
    distance = torch.empty((height, width), device=dev, dtype=torch.float32)
    with L.on(dev) as st:
        L.check(L.lib.moge_pano_finish(ptr(x), ptr(distance), height, width, None, st))
    return distance, system.seen


def merge_panorama_depth(width: int, height: int, distance_maps, pred_masks, extrinsics, intrinsics, poll: int = POLL,
                         iterations: Optional[list] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """`moge_amd.panorama.merge_panorama_depth` on the device: distance_maps (n, h, w) float32 and pred_masks (n, h, w) bool, CUDA (or sequences
    of such maps) -> (panorama distance (height, width) float32, panorama mask bool).  Coarse to fine as on the host: above 256 pixels the
    half-size solution, resized, is the solver's starting point.  `iterations`, if a list, receives the solver's iteration count per level,
    coarsest first."""
    width, height = int(width), int(height)
    dist, masks = _views(distance_maps, pred_masks)
    _check_map(width, height)
    E, K = _cameras(extrinsics, intrinsics, dist.shape[0])
    return _merge(width, height, dist, masks, E, K, int(poll), iterations if iterations is not None else [])


# ---------------------------------------------------------------------------------------------------------------------------------------
# the whole pipeline
# ---------------------------------------------------------------------------------------------------------------------------------------
@torch.inference_mode()
def infer_panorama(model, image_u8: torch.Tensor, resolution: int = 512, batch_size: int = 4, merge_size: Tuple[int, int] = (1920, 960),
                   **infer_kwargs) -> Dict[str, torch.Tensor]:
    """`moge_amd.panorama.infer_panorama` with every step on the device: split -> batched `model.infer(views / 255, fov_x=..., apply_mask=False)` ->
    merge at most at `merge_size` (width, height) -> resize to the image -> points = distance x direction.  The uint8 views become the host
    caller's float32 `view / 255` on the device (a 256-entry table of the host's values) and go through `infer`, not
    `infer_uint8`: with float32 weights and `use_fp16=True` (the autocast form, the panorama command's default) `infer_uint8` stages the bytes
    in fp16 and its distances differ from `infer(view / 255)` by up to 3.8e-4 relative, and the view outputs here are the
    host pipeline's bit for bit.  image_u8 (H, W, 3) uint8 CUDA.  Returns CUDA tensors: distance (H, W) float32, mask (H, W) bool, points
    (H, W, 3) float32, and the per-view intermediates "views" (n, res, res, 3) uint8, "view_distance" (n, res, res) float32, "view_mask"
    (n, res, res) bool."""
    dev = _device(image_u8)
    if image_u8.dim() != 3 or image_u8.shape[-1] != 3 or image_u8.dtype != torch.uint8:
        raise ValueError(f"expected an (H, W, 3) uint8 image, got {tuple(image_u8.shape)} {image_u8.dtype}")
    H, W = image_u8.shape[:2]
    E, Ks = get_panorama_cameras()
    views = split_panorama_image(image_u8, E, Ks, resolution)
    fov = intrinsics_to_fov_x_deg(np.array(Ks))
    # float32(i / 255.0) per byte value, the host caller's numbers, as a table: torch's division by a host scalar multiplies by the rounded
    # reciprocal instead, which is a last bit off for some bytes and moves the model's output
    unit = torch.tensor(np.arange(256) / 255, dtype=torch.float32, device=dev)
    dist, masks = [], []
    for i in range(0, len(views), batch_size):
        fov_x = torch.tensor(fov[i:i + batch_size], dtype=torch.float32, device=dev)
        image_tensor = unit[views[i:i + batch_size].long()].permute(0, 3, 1, 2)          # infer_panorama.py:99, on the device
        out = model.infer(image_tensor, fov_x=fov_x, apply_mask=False, **infer_kwargs)
        dist.append(out["points"].norm(dim=-1))
        masks.append(out["mask"])
    view_dist, view_mask = torch.cat(dist).float(), torch.cat(masks)
    mw, mh = min(merge_size[0], W), min(merge_size[1], H)
    distance, mask = merge_panorama_depth(mw, mh, view_dist, view_mask, E, Ks)
    distance = _resize_bilinear(distance, H, W)
    mask = _resize_nearest(mask, H, W)
    points = torch.empty((H, W, 3), device=dev, dtype=torch.float32)
    with L.on(dev) as st:
        L.check(L.lib.moge_pano_finish(None, ptr(distance), H, W, ptr(points), st))
    return {"distance": distance, "mask": mask, "points": points, "views": views, "view_distance": view_dist, "view_mask": view_mask}
