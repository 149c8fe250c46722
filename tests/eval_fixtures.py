"""Inputs of the evaluation-data fixtures (tests/golden/eval_*.npz, written by tools/make_eval_golden.py from the reference's
`EvalDataLoaderPipeline._process_instance`).  A fixture stores a compact recipe; `build_instance` turns it into the raw maps with integer and
float32 elementwise arithmetic, and the stored sha256 checks that the rebuilt maps are the ones the reference warped."""
from __future__ import annotations

import hashlib
import json
import os

import numpy as np

GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CASES = ["nyu", "kitti", "ibims", "eth3d", "invalid"]


def load(name):
    return np.load(os.path.join(GOLDEN_DIR, f"eval_{name}.npz"))


def build_instance(r: dict) -> dict:
    """recipe -> the instance dict of dataloader.py:_load_instance (numpy, raw size).  Recipe keys: H, W, K (3, 3) float32, image_coef (3, 3)
    int (third column: checker shift), depth_grid (gh, gw) float16, nan_mod / inf_mod (int, 0 = none), all_invalid, and optionally seg_x /
    seg_y (block edges), seg_ids (rows, cols) and labels_json."""
    H, W = int(r["H"]), int(r["W"])
    y, x = np.mgrid[0:H, 0:W].astype(np.int64)
    c = np.asarray(r["image_coef"], np.int64)
    image = np.stack([(c[k, 0] * x + c[k, 1] * y + 96 * (((x >> c[k, 2]) + (y >> 3)) & 1)) & 255 for k in range(3)],
                     axis=-1).astype(np.uint8)
    grid = np.asarray(r["depth_grid"]).astype(np.float32)
    gh, gw = grid.shape
    depth = grid[y * gh // H, x * gw // W] * (np.float32(1) + y.astype(np.float32) / np.float32(4 * H))
    if int(r["nan_mod"]):
        depth[(x * 7 + y * 13) % int(r["nan_mod"]) == 0] = np.nan
    if int(r["inf_mod"]):
        depth[(x * 5 + y * 3) % int(r["inf_mod"]) == 0] = np.inf
    if int(r["all_invalid"]):
        depth[:] = np.nan
    inst = {"filename": str(r["name"]), "width": int(r["tgt_W"]), "height": int(r["tgt_H"]), "image": image,
            "depth": np.nan_to_num(depth, nan=1, posinf=1, neginf=1), "depth_mask": np.isfinite(depth), "depth_mask_inf": np.isinf(depth),
            "intrinsics": np.asarray(r["K"], np.float32)}
    if "seg_ids" in r:
        ids = np.asarray(r["seg_ids"])
        ey, ex = np.asarray(r["seg_y"]), np.asarray(r["seg_x"])
        by = np.searchsorted(ey, np.arange(H), side="right") - 1
        bx = np.searchsorted(ex, np.arange(W), side="right") - 1
        inst["segmentation_mask"] = ids[np.clip(by, 0, ids.shape[0] - 1)][:, np.clip(bx, 0, ids.shape[1] - 1)]
        inst["segmentation_labels"] = json.loads(str(r["labels_json"]))
    return inst


def instance_digest(inst: dict) -> str:
    h = hashlib.sha256()
    for k in ("image", "depth", "depth_mask", "segmentation_mask", "intrinsics"):
        if k in inst:
            h.update(k.encode())
            h.update(np.ascontiguousarray(inst[k]).tobytes())
    return h.hexdigest()


RECIPE_KEYS = ("name", "H", "W", "tgt_H", "tgt_W", "K", "image_coef", "depth_grid", "nan_mod", "inf_mod", "all_invalid", "seg_x", "seg_y", "seg_ids",
               "labels_json", "config_json")


def recipe(z) -> dict:
    return {k: z[f"recipe_{k}"] for k in RECIPE_KEYS if f"recipe_{k}" in z.files}


def config(z) -> dict:
    """drop_max_depth, depth_unit, include_segmentation, max_segments, min_seg_area, has_sharp_boundary of the case"""
    return json.loads(str(z["recipe_config_json"]))
