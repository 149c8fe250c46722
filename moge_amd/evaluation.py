"""Evaluation data on the MI355X: the host-side mirror of the reference's `moge/test/dataloader.py` (`EvalDataLoaderPipeline`) with the
per-sample view warp of `_process_instance` in the HIP kernels of `csrc/evaldata.hip` (C ABI `moge_eval_*`).

    from moge_amd.evaluation import EvalDataLoader        # instead of moge.test.dataloader.EvalDataLoaderPipeline
    with EvalDataLoader(**benchmark_config) as loader:
        for _ in range(len(loader)):
            sample = loader.get()                          # the reference's keys; the warped maps are CUDA tensors

What stays on the host: PNG / JPEG decoding and meta.json (a few prefetching threads, no process pool), the 3 x 3 geometry of
`_process_instance` (:108-152, numpy, with the reference's float32 / float64 promotions: `int(raw_width * raw_pixel_w / tgt_pixel_w)`
decides a shape) and the segment-label sort (:183-189).  Everything per pixel is on the GPU: Lanczos resize, masked nearest resize and
distance, nearest resize of the segmentation, the homography remap, the exact 1 % quantile cut, the points and the label histogram.  The host
reads back one flag and the label counts per sample.

utils3d and cv2 are not vendored; their functions are restated below and in csrc/evaldata.hip from their call sites."""
from __future__ import annotations

import concurrent.futures as cf
import ctypes as C
import io
import json
import math
import os
from pathlib import Path
from typing import Any, Dict, List, Optional, Tuple, Union

import numpy as np
import torch
from PIL import Image, PngImagePlugin

from . import _lib as L
from ._lib import ptr
from .io import uv_map

QUANTILE = 0.01                       # dataloader.py:167
SEG_BINS = 65536                      # MOGE_EVAL_SEG_BINS (include/moge_hip.h)
QUANTILE_WORKSPACE = 520              # MOGE_EVAL_QUANTILE_WORKSPACE
DROPPED_LABELS = ("undefined", "unannotated", "background", "sky")      # dataloader.py:184


# ------------------------------------------------------------------------------------------------------------------------------------------
# file formats of the benchmark directories (written independently from the format: 16-bit PNGs with text chunks)
# ------------------------------------------------------------------------------------------------------------------------------------------
def _read_bytes(path) -> bytes:
    return Path(path).read_bytes() if isinstance(path, (str, os.PathLike)) else path.read()


def read_image(path) -> np.ndarray:
    """image.jpg -> (H, W, 3) uint8 RGB (PIL's decoder)."""
    with Image.open(io.BytesIO(_read_bytes(path))) as im:
        return np.array(im.convert("RGB"))


def read_depth(path) -> np.ndarray:
    """depth.png -> (H, W) float32.  uint16 code c: 0 -> NaN, 65535 -> inf, else near^(1 - t) far^t with t = (c - 1) / 65533 (log encoding
    between the `near` / `far` text chunks), times the legacy `unit` chunk when present."""
    with Image.open(io.BytesIO(_read_bytes(path))) as im:
        near, far = float(im.info["near"]), float(im.info["far"])
        unit = float(im.info["unit"]) if "unit" in im.info else None
        code = np.array(im).astype(np.uint16)
    t = (code.astype(np.float32) - 1) / 65533
    depth = near ** (1 - t) * far ** t
    if unit is not None:
        depth = depth * unit
    depth[code == 0] = np.nan
    depth[code == 65535] = np.inf
    return depth


def write_depth(path, depth: np.ndarray, max_range: float = 1e5, compression_level: int = 7) -> None:
    """The inverse of read_depth: near / far are the smallest / largest finite depth (far at most near * max_range)."""
    depth = np.asarray(depth, dtype=np.float32)
    finite = np.isfinite(depth) & (depth > 0)
    near = float(depth[finite].min()) if finite.any() else 1.0
    far = min(float(depth[finite].max()) if finite.any() else 1.0, near * max_range)
    span = math.log(far / near)
    with np.errstate(divide="ignore", invalid="ignore"):
        t = np.log(np.clip(depth, near, far) / near) / span if span > 0 else np.zeros_like(depth)
    code = np.where(finite, np.clip(np.rint(1 + t * 65533), 1, 65534), 0).astype(np.uint16)
    code[np.isinf(depth) & (depth > 0)] = 65535
    info = PngImagePlugin.PngInfo()
    info.add_text("near", repr(near))
    info.add_text("far", repr(far))
    Image.fromarray(code).save(path, pnginfo=info, compress_level=compression_level)


def read_segmentation(path) -> Tuple[np.ndarray, Optional[Dict[str, int]]]:
    """segmentation.png -> (uint8 / uint16 label map (H, W), {name: id} from the JSON `labels` text chunk or None)."""
    with Image.open(io.BytesIO(_read_bytes(path))) as im:
        labels = json.loads(im.info["labels"]) if "labels" in im.info else None
        mask = np.array(im)
    if mask.dtype not in (np.uint8, np.uint16):
        mask = mask.astype(np.uint16)
    return mask, labels


def write_segmentation(path, mask: np.ndarray, labels: Optional[Dict[str, int]] = None, compression_level: int = 7) -> None:
    assert mask.dtype in (np.uint8, np.uint16)
    info = PngImagePlugin.PngInfo()
    if labels is not None:
        info.add_text("labels", json.dumps(labels))
    Image.fromarray(mask).save(path, pnginfo=info, compress_level=compression_level)


def read_meta(path) -> Dict[str, Any]:
    return json.loads(_read_bytes(path))


# ------------------------------------------------------------------------------------------------------------------------------------------
# utils3d.np stand-ins (un-vendored dependency): restated from the call sites in dataloader.py, normalised intrinsics, OpenCV camera axes
# ------------------------------------------------------------------------------------------------------------------------------------------
def uv_to_pixel(uv: np.ndarray, size: Tuple[int, int]) -> np.ndarray:
    """uv in [0, 1] -> pixel coordinates of an (h, w) image: uv * (w, h) - 0.5 (pixel centres at integers), in uv's dtype."""
    h, w = size
    return uv * np.array([w, h], dtype=uv.dtype) - np.asarray(0.5, dtype=uv.dtype)


def unproject_cv(uv: np.ndarray, depth: np.ndarray, intrinsics: np.ndarray) -> np.ndarray:
    """([u, v, 1] @ inv(K)^T) * depth."""
    homo = np.concatenate([uv, np.ones_like(uv[..., :1])], axis=-1)
    return (homo @ np.linalg.inv(intrinsics).T) * depth[..., None]


def rotation_matrix_from_vectors(v1: np.ndarray, v2: np.ndarray) -> np.ndarray:
    """The rotation taking direction v1 to direction v2 about their common normal (Rodrigues), in their dtype; identity when parallel."""
    a, b = v1 / np.linalg.norm(v1), v2 / np.linalg.norm(v2)
    axis = np.cross(a, b)
    s, c = np.linalg.norm(axis), np.dot(a, b)
    eye = np.eye(3, dtype=a.dtype)
    if s == 0:
        return eye
    k = axis / s
    kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]], dtype=a.dtype)
    return eye + s * kx + (1 - c) * (kx @ kx)


def ray_intersection(p1: np.ndarray, d1: np.ndarray, p2: np.ndarray, d2: np.ndarray):
    """2-D lines p1 + t1 d1 and p2 + t2 d2 (broadcast) -> (intersection points, (t1, t2)); parallel lines give inf / nan."""
    def cross(a, b):
        return a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]
    with np.errstate(divide="ignore", invalid="ignore"):
        den = cross(d1, d2)
        t1 = cross(p2 - p1, d2) / den
        t2 = cross(p2 - p1, d1) / den
    return p1 + t1[..., None] * d1, (t1, t2)


def intrinsics_from_focal_center(fx, fy, cx, cy) -> np.ndarray:
    return np.array([[fx, 0, cx], [0, fy, cy], [0, 0, 1]])


def depth_map_to_point_map(depth: np.ndarray, intrinsics: np.ndarray) -> np.ndarray:
    """(x, y, depth) at pixel centres: x = (u - cx) / fx * depth, u = (j + 0.5) / W (float32 like the GPU kernel)."""
    H, W = depth.shape[-2:]
    uv = uv_map(H, W)
    x = (uv[..., 0] - intrinsics[0, 2]) / intrinsics[0, 0] * depth
    y = (uv[..., 1] - intrinsics[1, 2]) / intrinsics[1, 1] * depth
    return np.stack([x, y, depth], axis=-1)


def masked_nearest_resize(image: np.ndarray, mask: np.ndarray, size: Tuple[int, int]) -> Tuple[np.ndarray, np.ndarray]:
    """(H, W) image and mask -> resized (h, w) image and mask (convention of csrc/evaldata.hip masked_nearest_kernel: windows of
    ceil(max(1, H / h)) x ceil(max(1, W / w)) pixels starting at rint(centre - f / 2); the valid pixel nearest the cell centre, first in
    row-major order on a tie; no valid pixel -> invalid cell with the nearest in-image pixel)."""
    H, W = mask.shape
    h, w = size
    fh, fw = max(1.0, H / h), max(1.0, W / w)
    cy = (np.arange(h) + 0.5) * H / h
    cx = (np.arange(w) + 0.5) * W / w
    y0, x0 = np.rint(cy - fh / 2).astype(np.int64), np.rint(cx - fw / 2).astype(np.int64)
    best_v = np.full((h, w), np.inf)
    best_a = np.full((h, w), np.inf)
    by = np.full((h, w), -1, np.int64)
    bx = np.full((h, w), -1, np.int64)
    ay = np.broadcast_to(np.clip(y0, 0, H - 1)[:, None], (h, w)).copy()
    ax = np.broadcast_to(np.clip(x0, 0, W - 1)[None, :], (h, w)).copy()
    for dy in range(math.ceil(fh)):
        y = y0 + dy
        ey = (y + 0.5 - cy)[:, None]
        for dx in range(math.ceil(fw)):
            x = x0 + dx
            ex = (x + 0.5 - cx)[None, :]
            inside = ((y >= 0) & (y < H))[:, None] & ((x >= 0) & (x < W))[None, :]
            d = ey * ey + ex * ex
            yy, xx = np.broadcast_to(np.clip(y, 0, H - 1)[:, None], (h, w)), np.broadcast_to(np.clip(x, 0, W - 1)[None, :], (h, w))
            take_a = inside & (d < best_a)
            best_a, ay, ax = np.where(take_a, d, best_a), np.where(take_a, yy, ay), np.where(take_a, xx, ax)
            take_v = inside & mask[yy, xx] & (d < best_v)
            best_v, by, bx = np.where(take_v, d, best_v), np.where(take_v, yy, by), np.where(take_v, xx, bx)
    valid = by >= 0
    return image[np.where(valid, by, ay), np.where(valid, bx, ax)], valid


# ------------------------------------------------------------------------------------------------------------------------------------------
# host geometry (dataloader.py:108-152)
# ------------------------------------------------------------------------------------------------------------------------------------------
def warp_geometry(raw_height: int, raw_width: int, intrinsics: np.ndarray, width: int, height: int) -> Dict[str, Any]:
    """The target view of one sample: its intrinsics, the size of the antialiased resize, the homography (target uv -> source uv) and
    inv(target intrinsics).  numpy's promotions are kept on purpose (float32 intrinsics, float64 ray intersections)."""
    K = intrinsics
    fov_x, fov_y = abs(1.0 / K[0, 0]), abs(1.0 / K[1, 1])                       # view extent on the z = 1 plane, float32
    src_px_w, src_px_h = fov_x / raw_width, fov_y / raw_height
    aspect = width / height
    view_x = min(fov_x, fov_y * aspect)
    view_y = view_x / aspect

    # rotate the view to look through the principal point of the image centre
    look = unproject_cv(np.array([[0.5, 0.5]], dtype=np.float32), np.array([1.0], dtype=np.float32), intrinsics=K)[0]
    R = rotation_matrix_from_vectors(look, np.array([0, 0, 1], dtype=np.float32))

    # keep the target frustum inside the source image: its corners on the rotated camera plane, against the two diagonals of the target
    quad = np.concatenate([np.array([[0, 0], [0, 1], [1, 1], [1, 0]], dtype=np.float32), np.ones((4, 1), dtype=np.float32)], axis=1)
    quad = quad @ (np.linalg.inv(K).T @ R.T)
    quad = quad[:, :2] / quad[:, 2:3]
    lim_x, lim_y = abs(1.0 / K[0, 0]), abs(1.0 / K[1, 1])
    diagonals = np.array([[aspect, 1.0], [aspect, -1.0]])
    for i in range(4):
        hit, _ = ray_intersection(np.array([0., 0.]), diagonals, quad[i - 1], quad[i] - quad[i - 1])
        lim_x = min(lim_x, 2 * np.abs(hit[:, 0]).min())
        lim_y = min(lim_y, 2 * np.abs(hit[:, 1]).min())
    view_x, view_y = min(view_x, lim_x), min(view_y, lim_y)

    tgt_K = intrinsics_from_focal_center(1.0 / view_x, 1.0 / view_y, 0.5, 0.5).astype(np.float32)
    tgt_px_w, tgt_px_h = view_x / width, view_y / height
    rescaled_w, rescaled_h = int(raw_width * src_px_w / tgt_px_w), int(raw_height * src_px_h / tgt_px_h)
    transform = K @ np.linalg.inv(R) @ np.linalg.inv(tgt_K)
    return {"tgt_intrinsics": tgt_K, "rescaled_size": (rescaled_h, rescaled_w), "transform": transform, "tgt_intrinsics_inv": np.linalg.inv(tgt_K),
            "R": R}


# ------------------------------------------------------------------------------------------------------------------------------------------
# GPU warp
# ------------------------------------------------------------------------------------------------------------------------------------------
def _host_f32(a: np.ndarray):
    buf = np.ascontiguousarray(a, dtype=np.float32).ravel()
    return buf, C.c_void_p(buf.ctypes.data)


def lanczos_resize(image: torch.Tensor, height: int, width: int) -> torch.Tensor:
    """PIL Image.resize((width, height), LANCZOS) of an (H, W, 3) uint8 CUDA tensor, bit-exact to Pillow."""
    dev = L.device_of("evaluation", image)
    image = image.contiguous()
    H, W = image.shape[:2]
    tmp_bytes, n_coeff = C.c_int64(), C.c_int64()
    L.check(L.lib.moge_eval_lanczos_workspace(H, W, height, width, C.byref(tmp_bytes), C.byref(n_coeff)))
    tmp = torch.empty(tmp_bytes.value, dtype=torch.uint8, device=dev)
    coeffs = torch.empty(n_coeff.value, dtype=torch.int32, device=dev)
    out = torch.empty((height, width, 3), dtype=torch.uint8, device=dev)
    with L.on(dev) as st:
        L.check(L.lib.moge_eval_lanczos(ptr(image), H, W, height, width, ptr(tmp), ptr(coeffs), ptr(out), st))
    return out


def masked_nearest_resize_distance(depth: torch.Tensor, mask: torch.Tensor, size: Tuple[int, int], intrinsics: np.ndarray):
    """dataloader.py:147-148 -> (depth, mask (uint8), distance) of size (h, w)."""
    dev = L.device_of("evaluation", depth, mask)
    H, W = depth.shape
    h, w = size
    out_depth = torch.empty((h, w), dtype=torch.float32, device=dev)
    out_mask = torch.empty((h, w), dtype=torch.uint8, device=dev)
    distance = torch.empty((h, w), dtype=torch.float32, device=dev)
    K = intrinsics
    with L.on(dev) as st:
        L.check(L.lib.moge_eval_masked_nearest(ptr(depth.float().contiguous()), ptr(mask.to(torch.uint8).contiguous()), H, W, h, w, float(K[0, 0]), float(K[1, 1]),
                                               float(K[0, 2]), float(K[1, 2]), ptr(out_depth), ptr(out_mask), ptr(distance), st))
    return out_depth, out_mask, distance


def resize_nearest(seg: torch.Tensor, size: Tuple[int, int]) -> torch.Tensor:
    """cv2.resize(seg, (w, h), INTER_NEAREST) of a uint8 / uint16 (H, W) CUDA label map."""
    dev = L.device_of("evaluation", seg)
    H, W = seg.shape
    h, w = size
    out = torch.empty((h, w), dtype=seg.dtype, device=dev)
    with L.on(dev) as st:
        L.check(L.lib.moge_eval_resize_nearest(ptr(seg.contiguous()), seg.element_size(), H, W, h, w, ptr(out), st))
    return out


def warp_sample(image: torch.Tensor, depth: torch.Tensor, depth_mask: torch.Tensor, intrinsics: np.ndarray, width: int, height: int,
                segmentation: Optional[torch.Tensor] = None, drop_max_depth: float = 1000.0, depth_unit: Optional[float] = None,
                geometry: Optional[dict] = None) -> Dict[str, Any]:
    """dataloader.py:108-180 on the GPU for one sample whose raw maps are already CUDA tensors (image (H, W, 3) uint8, depth (H, W) float32
    with invalid pixels already replaced, depth_mask (H, W) bool, segmentation (H, W) uint8 / uint16 or None).  Returns the target maps
    (CUDA), the host geometry and the device-side `count` of the final mask (0 means the empty-mask fallback ran).  No host synchronisation."""
    dev = L.device_of("evaluation", image, depth, depth_mask, segmentation)
    geo = geometry or warp_geometry(image.shape[0], image.shape[1], intrinsics, width, height)
    h, w = geo["rescaled_size"]
    rescaled = lanczos_resize(image, h, w)
    _, r_mask, distance = masked_nearest_resize_distance(depth, depth_mask, (h, w), intrinsics)
    r_seg = resize_nearest(segmentation, (h, w)) if segmentation is not None else None

    n = height * width
    image_u8 = torch.empty((height, width, 3), dtype=torch.uint8, device=dev)
    image_f = torch.empty((3, height, width), dtype=torch.float32, device=dev)
    tgt_depth = torch.empty((height, width), dtype=torch.float32, device=dev)
    tgt_mask = torch.empty((height, width), dtype=torch.uint8, device=dev)
    tgt_seg = torch.empty((height, width), dtype=torch.int32, device=dev) if r_seg is not None else None
    hist = torch.empty(SEG_BINS, dtype=torch.int32, device=dev) if r_seg is not None else None
    mats, mats_p = _host_f32(np.concatenate([np.asarray(geo["transform"], np.float32).ravel(), np.asarray(geo["tgt_intrinsics_inv"], np.float32).ravel()]))
    workspace = torch.empty(QUANTILE_WORKSPACE, dtype=torch.int32, device=dev)
    count = torch.empty(1, dtype=torch.int32, device=dev)
    points = torch.empty((height, width, 3), dtype=torch.float32, device=dev)
    kinv, kinv_p = _host_f32(geo["tgt_intrinsics_inv"])
    with L.on(dev) as st:
        L.check(L.lib.moge_eval_remap(ptr(rescaled), ptr(distance), ptr(r_mask), ptr(r_seg), 0 if r_seg is None else r_seg.element_size(), h, w, height, width,
                                      mats_p, ptr(image_u8), ptr(image_f), ptr(tgt_depth), ptr(tgt_mask), ptr(tgt_seg), ptr(hist), st))
        L.check(L.lib.moge_eval_quantile_cut(ptr(tgt_depth), ptr(tgt_mask), n, QUANTILE, float(drop_max_depth), float(depth_unit or 0.0),
                                             int(depth_unit is not None), ptr(workspace), ptr(count), st))
        L.check(L.lib.moge_eval_unproject(ptr(tgt_depth), ptr(tgt_mask), height, width, kinv_p, ptr(count), ptr(points), st))
    del mats, kinv          # read during the calls (host pointers)
    return {"geometry": geo, "rescaled_image": rescaled, "image_u8": image_u8, "image": image_f, "depth": tgt_depth, "depth_mask": tgt_mask.bool(),
            "points": points, "segmentation_mask": tgt_seg, "segmentation_hist": hist, "count": count,
            "max_depth": workspace[5:6].view(torch.float32)}


def select_segments(labels: Dict[str, int], counts: Dict[int, int], max_segments: int, min_seg_area: int) -> Dict[str, int]:
    """dataloader.py:183-189: drop the background-like labels, order by pixel count (descending, stable on ties), keep the first
    `max_segments` that cover at least `min_seg_area` pixels."""
    labels = {k: v for k, v in labels.items() if k not in DROPPED_LABELS}
    order = sorted(labels.keys(), key=lambda k: counts.get(labels[k], 0), reverse=True)
    return {k: labels[k] for k in order[:max_segments] if counts.get(labels[k], 0) >= min_seg_area}


def finish_sample(instance: Dict[str, Any], warped: Dict[str, Any], include_segmentation: bool, max_segments: int, min_seg_area: int,
                  depth_unit: Optional[float], has_sharp_boundary: bool) -> Dict[str, Any]:
    """The one host read of a sample (the fallback flag and the counts of the named labels) and the output dict of dataloader.py:191-203."""
    labels = instance.get("segmentation_labels")
    seg_ids = [] if labels is None or warped["segmentation_hist"] is None else \
        [v for k, v in labels.items() if k not in DROPPED_LABELS and 0 <= v < SEG_BINS]
    read = warped["count"]
    if seg_ids:
        read = torch.cat([read, warped["segmentation_hist"][torch.tensor(seg_ids, dtype=torch.long).to(read.device, non_blocking=True)]])
    read = read.cpu().tolist()
    out = {k: v for k, v in instance.items() if k not in ("image", "depth", "depth_mask", "intrinsics", "segmentation_mask", "segmentation_labels")}
    if read[0] == 0:
        out["label_type"] = "invalid"
    seg_labels = None
    if include_segmentation and warped["segmentation_mask"] is not None and labels is not None:
        seg_labels = select_segments(labels, dict(zip(seg_ids, read[1:])), max_segments, min_seg_area)
    dev = warped["image"].device
    out.update({
        "image": warped["image"],
        "depth": warped["depth"],
        "depth_mask": warped["depth_mask"],
        "intrinsics": torch.from_numpy(warped["geometry"]["tgt_intrinsics"]).float().to(dev),
        "points": warped["points"],
        "segmentation_mask": warped["segmentation_mask"].long() if warped["segmentation_mask"] is not None else None,
        "segmentation_labels": seg_labels,
        "is_metric": depth_unit is not None,
        "has_sharp_boundary": has_sharp_boundary,
    })
    return {k: v for k, v in out.items() if v is not None}


# ------------------------------------------------------------------------------------------------------------------------------------------
# the loader
# ------------------------------------------------------------------------------------------------------------------------------------------
def load_instance(path: Path, filename: str, width: int, height: int, include_segmentation: bool) -> Dict[str, Any]:
    """dataloader.py:73-104 on the host: decode one sample directory; the raw maps are pinned for the upload."""
    d = path.joinpath(filename)
    depth = read_depth(d / "depth.png")
    inst = {"filename": filename, "width": width, "height": height, "image": torch.from_numpy(read_image(d / "image.jpg")).pin_memory(),
            "depth": torch.from_numpy(np.nan_to_num(depth, nan=1, posinf=1, neginf=1)).pin_memory(),
            "depth_mask": torch.from_numpy(np.isfinite(depth)).pin_memory(), "depth_mask_inf": np.isinf(depth)}
    if include_segmentation:
        seg, labels = read_segmentation(d / "segmentation.png")
        inst["segmentation_mask"] = torch.from_numpy(seg.view(np.int16) if seg.dtype == np.uint16 else seg).pin_memory()    # uint16 bits as int16
        inst["segmentation_labels"] = labels
    inst["intrinsics"] = np.array(read_meta(d / "meta.json")["intrinsics"], dtype=np.float32)
    return inst


class EvalDataLoader:
    """EvalDataLoaderPipeline (dataloader.py:18-218) with the warp on the GPU.  Same constructor, `len`, `get()` order (file order),
    context-manager use and output keys.  `num_load_workers` host threads decode ahead of the GPU; `num_process_workers` is accepted and
    unused (the warp is a few kernel launches on the caller's stream).  `include_normal` / `depth_to_normal` are accepted like the
    reference, which does not use them either."""

    def __init__(self, path: str, width: int, height: int, split: str = ".index.txt", drop_max_depth: float = 1000., num_load_workers: int = 4,
                 num_process_workers: int = 8, include_segmentation: bool = False, include_normal: bool = False, depth_to_normal: bool = False,
                 max_segments: int = 100, min_seg_area: int = 1000, depth_unit: Optional[float] = None, has_sharp_boundary: bool = False,
                 subset: Optional[int] = None, device: Union[str, torch.device] = "cuda"):
        self.path = Path(path)
        self.filenames = self.path.joinpath(split).read_text(encoding="utf-8").splitlines()[::subset]
        self.width, self.height = width, height
        self.drop_max_depth = drop_max_depth
        self.include_segmentation = include_segmentation
        self.max_segments, self.min_seg_area = max_segments, min_seg_area
        self.depth_unit = depth_unit
        self.has_sharp_boundary = has_sharp_boundary
        self.num_load_workers = max(1, num_load_workers)
        self.device = torch.device(device)
        self.stages = None              # set to a dict to collect per-stage seconds (tools/bench_eval.py)
        self._pool = None
        self._futures = {}
        self._next = 0

    def __len__(self):
        return len(self.filenames)

    def _load(self, idx):
        import time
        t0 = time.perf_counter()
        inst = load_instance(self.path, self.filenames[idx], self.width, self.height, self.include_segmentation)
        inst["_decode_s"] = time.perf_counter() - t0
        return inst

    def _prefetch(self):
        ahead = self.num_load_workers + 4
        for idx in range(self._next, min(self._next + ahead, len(self))):
            if idx not in self._futures:
                self._futures[idx] = self._pool.submit(self._load, idx)

    def start(self):
        if self._pool is None:
            self._pool = cf.ThreadPoolExecutor(max_workers=self.num_load_workers, thread_name_prefix="moge-eval-load")
            self._next = 0
            self._prefetch()

    def stop(self):
        if self._pool is not None:
            self._pool.shutdown(wait=True, cancel_futures=True)
            self._pool, self._futures = None, {}

    def __enter__(self):
        self.start()
        return self

    def __exit__(self, exc_type, exc_value, traceback):
        self.stop()

    def process(self, inst: Dict[str, Any]) -> Dict[str, Any]:
        """Upload one decoded sample and warp it (the GPU half of dataloader.py:106-205)."""
        dev = self.device
        stages = self.stages
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)] if stages is not None else None
        if ev:
            ev[0].record()
        image = inst["image"].to(dev, non_blocking=True)
        depth = inst["depth"].to(dev, non_blocking=True)
        mask = inst["depth_mask"].to(dev, non_blocking=True)
        seg = inst.get("segmentation_mask")
        if seg is not None:
            seg = seg.to(dev, non_blocking=True)          # uint8, or uint16 bits held as int16: the kernels read 2-byte labels as uint16
        if ev:
            ev[1].record()
        warped = warp_sample(image, depth, mask, inst["intrinsics"], self.width, self.height, segmentation=seg, drop_max_depth=self.drop_max_depth,
                             depth_unit=self.depth_unit)
        if ev:
            ev[2].record()
        meta = {k: v for k, v in inst.items() if k != "_decode_s"}
        out = finish_sample(meta, warped, self.include_segmentation, self.max_segments, self.min_seg_area, self.depth_unit, self.has_sharp_boundary)
        if ev:
            stages.setdefault("decode", []).append(inst["_decode_s"])
            stages.setdefault("upload", []).append(ev[0].elapsed_time(ev[1]) / 1e3)
            stages.setdefault("warp", []).append(ev[1].elapsed_time(ev[2]) / 1e3)
        return out

    def get(self) -> Optional[Dict[str, Any]]:
        """The next sample in file order (None after the last one)."""
        if self._pool is None:
            raise RuntimeError("EvalDataLoader.get() outside `with` / start()")
        if self._next >= len(self):
            return None
        idx = self._next
        inst = self._futures.pop(idx).result()
        self._next += 1
        self._prefetch()
        return self.process(inst)


# ------------------------------------------------------------------------------------------------------------------------------------------
# results
# ------------------------------------------------------------------------------------------------------------------------------------------
def _nested_keys(d: dict, prefix: tuple = ()) -> List[tuple]:
    keys = []
    for k, v in d.items():
        keys.extend(_nested_keys(v, prefix + (k,)) if isinstance(v, dict) else [prefix + (k,)])
    return keys


def _get_nested(d: dict, keys: tuple):
    for k in keys:
        if not isinstance(d, dict) or k not in d:
            return None
        d = d[k]
    return d


def key_average(list_of_dicts: List[dict]) -> Dict[str, Any]:
    """moge.utils.tools.key_average: every nested key path of any dict, in sorted order; the mean of the values that are present and not NaN,
    NaN when none is."""
    paths = sorted({p for d in list_of_dicts for p in _nested_keys(d)})
    out: Dict[str, Any] = {}
    for path in paths:
        vals = [v for v in (_get_nested(d, path) for d in list_of_dicts) if v is not None and not math.isnan(v)]
        node = out
        for k in path[:-1]:
            node = node.setdefault(k, {})
        node[path[-1]] = sum(vals) / len(vals) if vals else float("nan")
    return out
