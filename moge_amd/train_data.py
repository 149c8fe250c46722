"""Training data on the MI355X: the host-side mirror of the reference's `moge/train/dataloader.py` (`TrainDataLoaderPipeline`) with the
geometric half of `_process_instance` (:143-229) in the HIP kernels of `csrc/traindata.hip` (C ABI `moge_train_*`).

    from moge_amd.train_data import TrainDataLoader          # instead of moge.train.dataloader.TrainDataLoaderPipeline
    with TrainDataLoader(config["data"], batch_size=8, color_augmentation="skip") as loader:
        batch = loader.get()                                   # the reference's keys; the maps are CUDA tensors, ready for moge_amd.losses

What stays on the host: decoding (the readers of moge_amd.evaluation, in prefetching threads), the dataset / size / seed sampling of
`_sample_batch`, and the 3 x 3 geometry: `sample_perspective` with the reference's dtype promotions, the flip draw, and the scales that
decide the sizes of the two pre-resizes.  Everything per pixel is on the GPU: the normal map, the 5 x 5 depth edge, both pre-resizes, the
fused projective warp, the fallback, the unit, the 1 % quantile clamp and the masks, written straight into slot b of the batch tensors.  Per
batch the host reads back the invalid flags, in one copy.

The colour augmentations of `image_color_augmentation` are NOT built: `color_augmentation="refuse"` (the default)
raises when a config asks for one, `"skip"` drops them with one warning.  They draw last from the per-instance generator, so the geometry of
a seed is the reference's either way.

utils3d and cv2 are not vendored; their functions are restated below and in csrc/traindata.hip from their call sites."""
from __future__ import annotations

import concurrent.futures as cf
import ctypes as C
import random
import warnings
from collections import deque
from pathlib import Path
from typing import Any, Dict, List, Optional, Tuple, Union

import numpy as np
import torch

from . import _lib as L
from ._lib import ptr
from . import evaluation as E
from .evaluation import intrinsics_from_focal_center, ray_intersection, read_depth, read_image, read_meta, rotation_matrix_from_vectors, unproject_cv

QUANTILE = 0.01                       # dataloader.py:212
EDGE_THRESHOLD = 88.0                 # dataloader.py:145, degrees
EDGE_KERNEL, EDGE_LTOL = 5, 0.01      # dataloader.py:171


# ------------------------------------------------------------------------------------------------------------------------------------------
# utils3d stand-ins (un-vendored dependency): normalised intrinsics, so a focal length is in units of the image side
# ------------------------------------------------------------------------------------------------------------------------------------------
def focal_to_fov(focal):
    return 2 * np.arctan(0.5 / focal)


def fov_to_focal(fov):
    return 0.5 / np.tan(fov / 2)


def intrinsics_to_fov(intrinsics: np.ndarray):
    """(fov_x, fov_y) in radians of normalised intrinsics, in their dtype"""
    return focal_to_fov(intrinsics[..., 0, 0]), focal_to_fov(intrinsics[..., 1, 1])


# ------------------------------------------------------------------------------------------------------------------------------------------
# host geometry (data_augmentation.py:21-68, :86-105; dataloader.py:154-167, :189)
# ------------------------------------------------------------------------------------------------------------------------------------------
def sample_perspective(src_intrinsics: np.ndarray, tgt_aspect: float, center_augmentation: float, fov_range_absolute: Tuple[float, float],
                       fov_range_relative: Tuple[float, float], rng: np.random.Generator) -> Tuple[np.ndarray, np.ndarray]:
    """The random target view: (target intrinsics float32, rotation R).  Three `rng.uniform` draws, in the reference's order.  The reference's
    quirk is kept: the absolute maximum lands in a name nobody reads (`:37`), so only the absolute minimum is applied."""
    K = src_intrinsics
    raw_fov_x, raw_fov_y = intrinsics_to_fov(K)
    abs_min, abs_max = fov_range_absolute
    rel_min, rel_max = fov_range_relative
    fov_x_min = min(rel_min * raw_fov_x, focal_to_fov(fov_to_focal(rel_min * raw_fov_y) / tgt_aspect))
    fov_x_max = min(rel_max * raw_fov_x, focal_to_fov(fov_to_focal(rel_max * raw_fov_y) / tgt_aspect))
    fov_x_min = max(np.deg2rad(abs_min), fov_x_min)
    _unapplied = min(np.deg2rad(abs_max), fov_x_max)            # noqa: F841  (the reference's `tgt_fov_max`)
    tgt_fov_x = rng.uniform(min(fov_x_min, fov_x_max), fov_x_max)
    tgt_fov_y = focal_to_fov(fov_to_focal(tgt_fov_x) * tgt_aspect)

    # the principal point of the target, as a direction of the raw camera
    dtheta = center_augmentation * rng.uniform(-0.5, 0.5) * (raw_fov_x - tgt_fov_x)
    dphi = center_augmentation * rng.uniform(-0.5, 0.5) * (raw_fov_y - tgt_fov_y)
    cu = 0.5 + 0.5 * np.tan(dtheta) / np.tan(raw_fov_x / 2)
    cv = 0.5 + 0.5 * np.tan(dphi) / np.tan(raw_fov_y / 2)
    direction = unproject_cv(np.array([[cu, cv]], dtype=np.float32), np.array([1.0], dtype=np.float32), intrinsics=K)[0]
    R = rotation_matrix_from_vectors(direction, np.array([0, 0, 1], dtype=np.float32))

    # keep the target frustum inside the warped source image: its corners on the rotated camera plane, against the two target diagonals
    quad = np.concatenate([np.array([[0, 0], [0, 1], [1, 1], [1, 0]], dtype=np.float32), np.ones((4, 1), dtype=np.float32)], axis=1)
    quad = quad @ (np.linalg.inv(K).T @ R.T)
    quad = quad[:, :2] / quad[:, 2:3]
    view_x, view_y = np.tan(tgt_fov_x / 2) * 2, np.tan(tgt_fov_y / 2) * 2
    lim_x, lim_y = float("inf"), float("inf")
    diagonals = np.array([[tgt_aspect, 1.0], [tgt_aspect, -1.0]])
    for i in range(4):
        hit, _ = ray_intersection(np.array([0., 0.]), diagonals, quad[i - 1], quad[i] - quad[i - 1])
        lim_x, lim_y = min(lim_x, 2 * np.abs(hit[:, 0]).min()), min(lim_y, 2 * np.abs(hit[:, 1]).min())
    view_x, view_y = min(view_x, lim_x), min(view_y, lim_y)
    return intrinsics_from_focal_center(1 / view_x, 1 / view_y, 0.5, 0.5).astype(np.float32), R


def pixel_transform(transform: np.ndarray, src_size: Tuple[int, int], tgt_size: Tuple[int, int]) -> np.ndarray:
    """uv-space `transform` (source -> target) as a source pixel -> target pixel matrix (data_augmentation.py:90), float32"""
    (sh, sw), (th, tw) = src_size, tgt_size
    to_pixel = np.array([[tw, 0, -0.5], [0, th, -0.5], [0, 0, 1]], dtype=np.float32)
    to_uv = np.array([[1 / sw, 0, 0.5 / sw], [0, 1 / sh, 0.5 / sh], [0, 0, 1]], dtype=np.float32)
    return to_pixel @ transform @ to_uv


def resize_scales(transform: np.ndarray, src_size: Tuple[int, int], tgt_size: Tuple[int, int]):
    """(scale_x, scale_y): target pixels per source pixel at the target centre (data_augmentation.py:90-93), in the reference's dtypes"""
    th, tw = tgt_size
    M = pixel_transform(transform, src_size, tgt_size)
    w = np.dot(np.linalg.inv(M)[2, :], np.array([tw / 2, th / 2, 1], dtype=np.float32))
    scale_x, scale_y = w * np.linalg.norm(M[:2, :2], axis=0)
    return scale_x, scale_y


def pre_resize_sizes(transform: np.ndarray, src_size: Tuple[int, int], tgt_size: Tuple[int, int]) -> Tuple[Tuple[int, int], Tuple[int, int]]:
    """((h, w) the image is Lanczos-resized to, (h, w) the depth is sparse-nearest-resized to); the source size where no resize runs
    (data_augmentation.py:95-102)"""
    sh, sw = src_size
    sx, sy = resize_scales(transform, src_size, tgt_size)
    image = (max(round(sh * sy * 1.25), 16), max(round(sw * sx * 1.25), 16)) if (sx < 0.8 or sy < 0.8) else (sh, sw)
    nearest = (max(round(sh * sy), 16), max(round(sw * sx), 16)) if (sx < 1 or sy < 1) else (sh, sw)
    return image, nearest


def inverse_pixel_matrix(transform: np.ndarray, src_size: Tuple[int, int], tgt_size: Tuple[int, int]) -> np.ndarray:
    """target pixel -> source pixel: the float64 inverse of the float32 pixel matrix, rounded to float32 (the cv2.warpPerspective stand-in)"""
    return np.linalg.inv(pixel_transform(transform, src_size, tgt_size).astype(np.float64)).astype(np.float32)


def warp_geometry(raw_height: int, raw_width: int, intrinsics: np.ndarray, width: int, height: int, seed: int, *, center_augmentation: float,
                  fov_range_absolute: Tuple[float, float], fov_range_relative: Tuple[float, float]) -> Dict[str, Any]:
    """Everything 3 x 3 of one instance: the sampled view, the flip, the pre-resize sizes and the `mats` of moge_train_warp."""
    rng = np.random.default_rng(seed)
    tgt_K, R = sample_perspective(intrinsics, width / height, center_augmentation, fov_range_absolute, fov_range_relative, rng)
    flip = bool(rng.choice([True, False]))
    transform = tgt_K @ R @ np.linalg.inv(intrinsics)
    raw, tgt = (raw_height, raw_width), (height, width)
    image_size, nearest_size = pre_resize_sizes(transform, raw, tgt)
    mats = np.concatenate([inverse_pixel_matrix(transform, s, tgt).ravel() for s in (image_size, nearest_size, raw)] +
                          [np.asarray(R, np.float32).ravel(), np.asarray(np.linalg.inv(transform)[2, :], np.float32)]).astype(np.float32)
    return {"tgt_intrinsics": tgt_K, "R": R, "transform": transform, "flip": flip, "image_size": image_size, "nearest_size": nearest_size, "mats": mats}


# ------------------------------------------------------------------------------------------------------------------------------------------
# GPU warp
# ------------------------------------------------------------------------------------------------------------------------------------------
def normal_map(depth: torch.Tensor, intrinsics: np.ndarray, edge_threshold: float = EDGE_THRESHOLD) -> torch.Tensor:
    """depth_map_to_normal_map(depth, intrinsics, mask=isfinite, edge_threshold) with NaN where the mask is off: (H, W) -> (H, W, 3)"""
    dev = L.device_of("train_data", depth)
    H, W = depth.shape
    out = torch.empty((H, W, 3), dtype=torch.float32, device=dev)
    K = intrinsics
    with L.on(dev) as st:
        L.check(L.lib.moge_train_normal_map(ptr(depth), H, W, float(K[0, 0]), float(K[1, 1]), float(K[0, 2]), float(K[1, 2]), float(edge_threshold), ptr(out), st))
    return out


def depth_edge(depth: torch.Tensor, kernel_size: int = EDGE_KERNEL, ltol: float = EDGE_LTOL) -> Tuple[torch.Tensor, torch.Tensor]:
    """-> (isfinite & ~depth_map_edge(depth, mask=isfinite, kernel_size, ltol) as float32 0 / 1, ~isnan as uint8)"""
    dev = L.device_of("train_data", depth)
    H, W = depth.shape
    eligible = torch.empty((H, W), dtype=torch.float32, device=dev)
    known = torch.empty((H, W), dtype=torch.uint8, device=dev)
    with L.on(dev) as st:
        L.check(L.lib.moge_train_depth_edge(ptr(depth), H, W, int(kernel_size), float(ltol), ptr(eligible), ptr(known), st))
    return eligible, known


def allocate_batch(batch_size: int, height: int, width: int, device) -> Dict[str, torch.Tensor]:
    """The tensors `warp_train_sample(..., out=, slot=)` fills: the reference's batch keys and dtypes, plus `image_u8`, `bilinear` (the depth took the bilinear branch), and per slot the finite
    `count`, the `invalid` flag and the quantile `workspace` (max_depth's bits at [:, 5])."""
    B, H, W = batch_size, height, width
    return {"image": torch.empty((B, 3, H, W), dtype=torch.float32, device=device), "image_u8": torch.empty((B, H, W, 3), dtype=torch.uint8, device=device),
            "depth": torch.empty((B, H, W), dtype=torch.float32, device=device), "depth_mask_fin": torch.empty((B, H, W), dtype=torch.bool, device=device),
            "depth_mask_inf": torch.empty((B, H, W), dtype=torch.bool, device=device), "normal": torch.empty((B, H, W, 3), dtype=torch.float32, device=device),
            "bilinear": torch.empty((B, H, W), dtype=torch.bool, device=device), "count": torch.empty(B, dtype=torch.int32, device=device), "invalid": torch.empty(B, dtype=torch.int32, device=device),
            "workspace": torch.empty((B, E.QUANTILE_WORKSPACE), dtype=torch.int32, device=device)}


def warp_train_sample(image: torch.Tensor, depth: torch.Tensor, intrinsics: np.ndarray, width: int, height: int, seed: int, *, center_augmentation: float,
                      fov_range_absolute: Tuple[float, float], fov_range_relative: Tuple[float, float], clamp_max_depth: float,
                      depth_unit: Optional[float] = None, finite_depth_mask: Optional[str] = None, geometry: Optional[dict] = None,
                      out: Optional[Dict[str, torch.Tensor]] = None, slot: int = 0) -> Dict[str, Any]:
    """dataloader.py:143-219 without the colour augmentation, on the GPU, for one instance whose raw maps are already CUDA tensors: image
    (H, W, 3) uint8, depth (H, W) float32 with NaN = unknown and +inf = sky; intrinsics (3, 3) float32 on the host.  Writes slot `slot` of
    `out` (allocate_batch; a batch of one is allocated when None) and returns views of that slot, the host geometry, and the device-side
    `count` of finite target depths, `invalid` flag and `max_depth`.  No host synchronisation."""
    dev = L.device_of("train_data", image, depth)
    if image.dtype != torch.uint8 or image.dim() != 3 or image.shape[2] != 3 or depth.dtype != torch.float32 or depth.shape != image.shape[:2]:
        raise ValueError(f"expected image (H, W, 3) uint8 and depth (H, W) float32, got {tuple(image.shape)} {image.dtype} and {tuple(depth.shape)} {depth.dtype}")
    image, depth = image.contiguous(), depth.contiguous()
    H, W = depth.shape
    intrinsics = np.asarray(intrinsics, dtype=np.float32)
    geo = geometry or warp_geometry(H, W, intrinsics, width, height, seed, center_augmentation=center_augmentation,
                                    fov_range_absolute=fov_range_absolute, fov_range_relative=fov_range_relative)
    if out is None:
        out, slot = allocate_batch(1, height, width, dev), 0
    if out["depth"].shape[1:] != (height, width) or not 0 <= slot < out["depth"].shape[0]:
        raise ValueError(f"`out` holds {tuple(out['depth'].shape)} maps; slot {slot} of size {(height, width)} does not fit")

    normal = normal_map(depth, intrinsics)
    eligible, known = depth_edge(depth)
    (ih, iw), (nh, nw) = geo["image_size"], geo["nearest_size"]
    src_image = E.lanczos_resize(image, ih, iw) if (ih, iw) != (H, W) else image
    nearest = E.masked_nearest_resize_distance(depth, known, (nh, nw), intrinsics)[0] if (nh, nw) != (H, W) else depth

    mats = np.ascontiguousarray(geo["mats"], dtype=np.float32)
    assert mats.size == L.TRAIN_WARP_MATS
    o = {k: out[k][slot] for k in ("image", "image_u8", "depth", "depth_mask_fin", "depth_mask_inf", "normal", "bilinear", "workspace")}
    count, invalid = out["count"][slot:slot + 1], out["invalid"][slot:slot + 1]
    with L.on(dev) as st:
        L.check(L.lib.moge_train_warp(ptr(src_image), ih, iw, ptr(nearest), nh, nw, ptr(depth), ptr(eligible), ptr(normal), H, W, height, width,
                                      C.c_void_p(mats.ctypes.data), int(geo["flip"]), ptr(o["image_u8"]), ptr(o["image"]), ptr(o["depth"]), ptr(o["normal"]),
                                      ptr(o["bilinear"]), ptr(count), st))
        L.check(L.lib.moge_train_finish(ptr(o["depth"]), height * width, ptr(count), float(depth_unit or 0.0), int(depth_unit is not None), QUANTILE,
                                        float(clamp_max_depth), int(finite_depth_mask == "only_known"), ptr(o["workspace"]), ptr(o["depth_mask_fin"]),
                                        ptr(o["depth_mask_inf"]), ptr(invalid), st))
    o.pop("workspace")
    o.update(geometry=geo, count=count, invalid=invalid, max_depth=out["workspace"][slot, 5:6].view(torch.float32), raw_normal=normal, eligible=eligible,
             nearest_depth=nearest, resized_image=src_image)
    return o


# ------------------------------------------------------------------------------------------------------------------------------------------
# the loader
# ------------------------------------------------------------------------------------------------------------------------------------------
class TrainDataLoader:
    """TrainDataLoaderPipeline (dataloader.py:26-256) with the warp on the GPU.  Same config keys and per-dataset overrides, the same sampling
    calls on the `random` module in the same order (dataset, filename, seed per instance, then the batch's size), `get()` / `start()` /
    `stop()` / context-manager use and batch keys.  `num_load_workers` host threads decode up to `buffer_size` batches ahead;
    `num_process_workers` is accepted and unused (the warp is a few kernel launches on the caller's stream)."""

    def __init__(self, config: dict, batch_size: int, num_load_workers: int = 4, num_process_workers: int = 8, buffer_size: int = 8, *,
                 color_augmentation: str = "refuse", device: Union[str, torch.device] = "cuda"):
        self.config = config
        self.batch_size = batch_size
        self.clamp_max_depth = config["clamp_max_depth"]
        self.fov_range_absolute = config.get("fov_range_absolute", 0.0)
        self.fov_range_relative = config.get("fov_range_relative", 0.0)
        self.center_augmentation = config.get("center_augmentation", 0.0)
        self.image_augmentation = config.get("image_augmentation", [])
        if "image_sizes" in config:
            self.image_size_strategy = "fixed"
            self.image_sizes = config["image_sizes"]
        elif "aspect_ratio_range" in config and "area_range" in config:
            self.image_size_strategy = "aspect_area"
            self.aspect_ratio_range = config["aspect_ratio_range"]
            self.area_range = config["area_range"]
        else:
            raise ValueError("Invalid image size configuration")

        self.datasets = {}
        for dataset in config["datasets"]:
            filenames = Path(dataset["path"], dataset.get("index", ".index.txt")).read_text().splitlines()
            self.datasets[dataset["name"]] = {**dataset, "filenames": filenames}
        self.dataset_names = [d["name"] for d in config["datasets"]]
        self.dataset_weights = [d["weight"] for d in config["datasets"]]

        if color_augmentation not in ("refuse", "skip"):
            raise ValueError(f"color_augmentation must be 'refuse' or 'skip', got {color_augmentation!r}")
        asked = sorted({a for d in [config] + list(config["datasets"]) for a in d.get("image_augmentation", [])})
        if asked and color_augmentation == "refuse":
            raise NotImplementedError(f"moge_amd.train_data does not build the colour augmentations {asked} (image_augmentation of the config); "
                                      "pass color_augmentation='skip' to run the geometric warp without them")
        if asked:
            warnings.warn(f"moge_amd.train_data: the colour augmentations {asked} are skipped", stacklevel=2)

        self.invalid_instance = {"intrinsics": np.array([[1.0, 0.0, 0.5], [0.0, 1.0, 0.5], [0.0, 0.0, 1.0]], dtype=np.float32),
                                 "image": np.zeros((256, 256, 3), dtype=np.uint8), "depth": np.ones((256, 256), dtype=np.float32), "label_type": "invalid"}
        self.num_load_workers = max(1, num_load_workers)
        self.buffer_size = max(1, buffer_size)
        self.device = torch.device(device)
        self._batch_id = 0
        self._pool = None
        self._queue: deque = deque()

    # ---- host: sampling (dataloader.py:82-122) and decoding (:124-141) ----
    def sample_batch(self) -> List[Dict[str, Any]]:
        self._batch_id += 1
        batch = []
        for _ in range(self.batch_size):
            name = random.choices(self.dataset_names, weights=self.dataset_weights)[0]
            filename = random.choice(self.datasets[name]["filenames"])
            batch.append({"batch_id": self._batch_id, "seed": random.randint(0, 2 ** 32 - 1), "dataset": name, "filename": filename,
                          "path": Path(self.datasets[name]["path"], filename), "label_type": self.datasets[name]["label_type"]})
        if self.image_size_strategy == "fixed":
            width, height = random.choice(self.config["image_sizes"])
        else:
            area = random.uniform(*self.area_range)
            ranges = [self.datasets[inst["dataset"]].get("aspect_ratio_range", self.aspect_ratio_range) for inst in batch]
            aspect = random.uniform(min(r[0] for r in ranges), max(r[1] for r in ranges))
            width, height = int((area * aspect) ** 0.5), int((area / aspect) ** 0.5)
        for inst in batch:
            inst["width"], inst["height"] = width, height
        return batch

    def load_instance(self, instance: Dict[str, Any]) -> Dict[str, Any]:
        try:
            image = read_image(Path(instance["path"], "image.jpg"))
            depth = read_depth(Path(instance["path"], self.datasets[instance["dataset"]].get("depth", "depth.png")))
            intrinsics = np.array(read_meta(Path(instance["path"], "meta.json"))["intrinsics"], dtype=np.float32)
            instance.update(image=image, depth=depth, intrinsics=intrinsics)
        except Exception as e:
            print(f"Failed to load instance {instance['dataset']}/{instance['filename']} because of exception:", e)
            instance.update(self.invalid_instance)
        if self.device.type == "cuda" and torch.cuda.is_available():          # pinned in the loader thread, for the asynchronous upload
            instance["image"] = torch.from_numpy(instance["image"]).pin_memory()
            instance["depth"] = torch.from_numpy(instance["depth"]).pin_memory()
        return instance

    def _setting(self, instance, key, default=None):
        return self.datasets[instance["dataset"]].get(key, default)

    def _prefetch(self):
        while len(self._queue) < self.buffer_size:
            self._queue.append([self._pool.submit(self.load_instance, inst) for inst in self.sample_batch()])

    def start(self):
        if self._pool is None:
            self._pool = cf.ThreadPoolExecutor(max_workers=self.num_load_workers, thread_name_prefix="moge-train-load")
            self._prefetch()

    def stop(self):
        if self._pool is not None:
            self._pool.shutdown(wait=True, cancel_futures=True)
            self._pool = None
            self._queue.clear()

    def __enter__(self):
        self.start()
        return self

    def __exit__(self, exc_type, exc_value, traceback):
        self.stop()
        return False

    # ---- GPU: upload, warp into the batch tensors, collate (dataloader.py:143-239) ----
    def process(self, instances: List[Dict[str, Any]]) -> Dict[str, Any]:
        dev = self.device
        width, height = instances[0]["width"], instances[0]["height"]
        out = allocate_batch(len(instances), height, width, dev)
        intrinsics = []
        for b, inst in enumerate(instances):
            image = torch.as_tensor(inst["image"]).to(dev, non_blocking=True)
            depth = torch.as_tensor(inst["depth"]).to(dev, non_blocking=True)
            unit = self._setting(inst, "depth_unit")
            res = warp_train_sample(image, depth, inst["intrinsics"], width, height, inst["seed"],
                                    center_augmentation=self._setting(inst, "center_augmentation", self.center_augmentation),
                                    fov_range_absolute=self._setting(inst, "fov_range_absolute", self.fov_range_absolute),
                                    fov_range_relative=self._setting(inst, "fov_range_relative", self.fov_range_relative),
                                    clamp_max_depth=self.clamp_max_depth, depth_unit=unit, finite_depth_mask=self._setting(inst, "finite_depth_mask"),
                                    out=out, slot=b)
            intrinsics.append(res["geometry"]["tgt_intrinsics"])
            inst["is_metric"] = unit is not None
        invalid = out["invalid"].cpu().tolist()              # the one host read of the batch
        return {"label_type": ["invalid" if flag else inst["label_type"] for flag, inst in zip(invalid, instances)],
                "is_metric": [inst["is_metric"] for inst in instances],
                "info": [{"dataset": inst["dataset"], "filename": inst["filename"]} for inst in instances],
                "image": out["image"], "depth": out["depth"], "depth_mask_fin": out["depth_mask_fin"], "depth_mask_inf": out["depth_mask_inf"],
                "normal": out["normal"], "intrinsics": torch.from_numpy(np.stack(intrinsics)).float().to(dev)}

    def get(self) -> Dict[str, Any]:
        """The next batch (the stream never ends)."""
        if self._pool is None:
            raise RuntimeError("TrainDataLoader.get() outside `with` / start()")
        instances = [f.result() for f in self._queue.popleft()]
        self._prefetch()
        return self.process(instances)
