"""Inputs of the training-data fixtures (tests/golden/train_*.npz, written by tools/make_train_data_golden.py from the reference's
`TrainDataLoaderPipeline._process_instance`).  A fixture stores a compact recipe; `build_instance` turns it into the raw maps with integer and
float32 elementwise arithmetic, and the stored sha256 checks that the rebuilt maps are the ones the reference warped."""
from __future__ import annotations

import hashlib
import json
import os

import numpy as np

GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
# (a) up-scale; (b) both pre-resizes; (c) nearest pre-resize only; (d) holes, sky and a step; (e) off-centre with centre augmentation;
# (f) flip_yes / flip_no; (g) all-NaN fallback; (h) depth_unit with finite_depth_mask = "only_known"
CASES = ["upscale", "downscale", "mild", "holes", "offcentre", "flip_yes", "flip_no", "allnan", "metric"]
RECIPE_KEYS = ("name", "H", "W", "tgt_H", "tgt_W", "K", "image_coef", "plane", "curve", "step_col", "step_factor", "nan_mod", "nan_box", "inf_rows", "all_nan", "seed",
               "config_json")


def load(name):
    return np.load(os.path.join(GOLDEN_DIR, f"train_{name}.npz"))


def build_instance(r: dict) -> dict:
    """recipe -> (image (H, W, 3) uint8, depth (H, W) float32 with NaN = unknown and inf = sky, intrinsics).  Recipe keys: H, W, K (3, 3) float32,
    image_coef (3, 3) int (third column: checker shift), plane (3,) float32 = depth a + b x / W + c y / H, curve (float32, times the squared
    offset from the centre column), step_col / step_factor (columns from step_col on are scaled), nan_mod (0 = none), nan_box (y0, y1, x0, x1: a block of NaN), inf_rows (top rows of
    sky), all_nan."""
    H, W = int(r["H"]), int(r["W"])
    y, x = np.mgrid[0:H, 0:W].astype(np.int64)
    c = np.asarray(r["image_coef"], np.int64)
    image = np.stack([(c[k, 0] * x + c[k, 1] * y + 96 * (((x >> c[k, 2]) + (y >> 3)) & 1)) & 255 for k in range(3)], axis=-1).astype(np.uint8)
    f = np.float32
    a, b, cc = [f(v) for v in np.asarray(r["plane"], f)]
    xf, yf = x.astype(f) / f(W), y.astype(f) / f(H)
    depth = (a + b * xf) + cc * yf
    off = xf - f(0.5)
    depth = depth + f(r["curve"]) * (off * off)
    if int(r["step_col"]):
        depth[:, int(r["step_col"]):] = depth[:, int(r["step_col"]):] * f(r["step_factor"])
    if int(r["nan_mod"]):
        depth[(x * 7 + y * 13) % int(r["nan_mod"]) == 0] = np.nan
    y0, y1, x0, x1 = [int(v) for v in r["nan_box"]]
    depth[y0:y1, x0:x1] = np.nan
    if int(r["inf_rows"]):
        depth[:int(r["inf_rows"])] = np.inf
    if int(r["all_nan"]):
        depth[:] = np.nan
    return {"image": image, "depth": depth.astype(f), "intrinsics": np.asarray(r["K"], f), "width": int(r["tgt_W"]), "height": int(r["tgt_H"]),
            "seed": int(r["seed"])}


def instance_digest(inst: dict) -> str:
    h = hashlib.sha256()
    for k in ("image", "depth", "intrinsics"):
        h.update(k.encode())
        h.update(np.ascontiguousarray(inst[k]).tobytes())
    return h.hexdigest()


def recipe(z) -> dict:
    return {k: z[f"recipe_{k}"] for k in RECIPE_KEYS if f"recipe_{k}" in z.files}


def config(z) -> dict:
    """center_augmentation, fov_range_absolute, fov_range_relative, clamp_max_depth, depth_unit, finite_depth_mask of the case"""
    return json.loads(str(z["recipe_config_json"]))


def warp_kwargs(cfg: dict) -> dict:
    return dict(center_augmentation=cfg["center_augmentation"], fov_range_absolute=cfg["fov_range_absolute"], fov_range_relative=cfg["fov_range_relative"],
                clamp_max_depth=cfg["clamp_max_depth"], depth_unit=cfg["depth_unit"], finite_depth_mask=cfg["finite_depth_mask"])


def knife_map(inst: dict, geo: dict) -> np.ndarray:
    """Target pixels where the reference itself sits on a decision boundary: a nearest coordinate within 1e-4 px of a
    half, a bilinear coordinate within 1e-4 px of an integer, or one of the four bilinear taps on a raw pixel whose 5 x 5 log spread is within
    1e-5 of ltol or which has a face angle within 1e-3 degrees of the edge threshold.  In the target's final (flipped) orientation."""
    from tests import train_data_reference as R
    from moge_amd import train_data as T
    h, w = inst["height"], inst["width"]
    mats = geo["mats"]
    with np.errstate(all="ignore"):
        sx, sy = R.source_coords(mats[9:18], h, w)
        knife = (np.abs(sx - np.floor(sx) - 0.5) < 1e-4) | (np.abs(sy - np.floor(sy) - 0.5) < 1e-4)
        sx, sy = R.source_coords(mats[18:27], h, w)
        knife |= (np.abs(sx - np.rint(sx)) < 1e-4) | (np.abs(sy - np.rint(sy)) < 1e-4)
        _, _, angles = R.normal_map(inst["depth"], inst["intrinsics"], T.EDGE_THRESHOLD, return_angles=True)
        _, _, spread = R.depth_edge(inst["depth"], T.EDGE_KERNEL, T.EDGE_LTOL, return_spread=True)
        raw = (np.abs(angles - T.EDGE_THRESHOLD) < 1e-3).any(-1) | (np.abs(spread - np.float32(T.EDGE_LTOL)) < 1e-5)
        H, W = raw.shape
        ok = np.isfinite(sx) & np.isfinite(sy) & (np.abs(sx) < 1e6) & (np.abs(sy) < 1e6)
        x0, y0 = np.floor(np.where(ok, sx, 0)).astype(np.int64), np.floor(np.where(ok, sy, 0)).astype(np.int64)
        for dy in (0, 1):
            for dx in (0, 1):
                yy, xx = y0 + dy, x0 + dx
                inside = ok & (yy >= 0) & (yy < H) & (xx >= 0) & (xx < W)
                knife |= inside & raw[np.clip(yy, 0, H - 1), np.clip(xx, 0, W - 1)]
    return knife[:, ::-1].copy() if geo["flip"] else knife
