"""Evaluation-metric fixtures (tests/golden/metrics_*.npz, written by tools/make_metrics_golden.py).

A fixture stores a compact RECIPE of its inputs rather than the full-resolution maps:
- a low-entropy gt depth (fp16, piecewise constant);
- the validity mask and the segmentation;
- a per-pixel noise index (uint8 into NOISE_LEVELS);
- the gt / predicted intrinsics.

`build_inputs` turns a recipe into the pred / gt maps with float32 elementwise arithmetic only (IEEE-exact, the same bits on any machine).
The generator feeds the reference exactly these arrays, so the fixture's reference outputs belong to what `build_inputs` returns."""
import json
import os

import numpy as np
import torch

GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CASES = ["a_plugin", "b_ibims", "c_depth_only", "d_moge1"]
NOISE_LEVELS = np.array([0.8, 0.97, 1.03, 1.35], np.float32)        # multiplicative noise of the prediction, one level per pixel (δ1 < 1)
F = np.float32


def load(name):
    return np.load(os.path.join(GOLDEN_DIR, f"metrics_{name}.npz"))


def build_inputs(recipe):
    """recipe: a mapping with depth (H, W) fp16, mask (H, W) bool, noise_idx (H, W) uint8, gt_K / pred_K (3, 3) f32, case (str), and for
    segmented cases seg (H, W) uint8 + labels (JSON).  -> (pred, gt) dicts of numpy arrays (gt without the is_metric / boundary flags)."""
    case = str(recipe["case"])
    depth = np.asarray(recipe["depth"]).astype(F)
    mask = np.asarray(recipe["mask"]).astype(bool)
    K, pK = np.asarray(recipe["gt_K"], F), np.asarray(recipe["pred_K"], F)
    H, W = depth.shape
    u = (np.arange(W, dtype=F) + F(0.5)) / F(W)
    v = (np.arange(H, dtype=F) + F(0.5)) / F(H)
    x = (u[None, :] - K[0, 2]) / K[0, 0] * depth
    y = (v[:, None] - K[1, 2]) / K[1, 1] * depth
    points = np.stack([x, y, depth], -1)
    noise = NOISE_LEVELS[np.asarray(recipe["noise_idx"])]
    pred_points = points * noise[..., None] * F(1.3) + np.array([0.02, -0.01, 0.3], F)
    pz = np.ascontiguousarray(pred_points[..., 2])
    gt = dict(depth=depth, points=points, depth_mask=mask, intrinsics=K)
    if case == "a_plugin":
        pred = dict(points_metric=pred_points, depth_metric=pz, intrinsics=pK)
    elif case == "b_ibims":
        pred = dict(points_scale_invariant=pred_points, depth_scale_invariant=pz, intrinsics=pK)
    elif case == "c_depth_only":
        pred = dict(depth_affine_invariant=pz * F(0.7) + F(0.2), disparity_affine_invariant=F(2.0) / pz + F(0.05))
    elif case == "d_moge1":
        pred = dict(points_scale_invariant=pred_points, depth_scale_invariant=pz)
        gt["depth"] = np.where(mask, depth, F(1.0))                                       # the dataloader's nan_to_num -> 1 with the mask false
        gt["points"] = np.where(mask[..., None], points, F(1.0))
    else:
        raise ValueError(case)
    if "seg" in recipe:
        gt["segmentation_mask"] = np.asarray(recipe["seg"]).astype(np.int64)
        gt["segmentation_labels"] = json.loads(str(recipe["labels"]))
    return pred, gt


def inputs_digest(pred, gt) -> str:
    """sha256 over the rebuilt maps (sorted keys, raw bytes): the generator stores it, so a changed rebuild cannot pass unnoticed"""
    import hashlib
    h = hashlib.sha256()
    for d in (pred, gt):
        for k in sorted(d):
            if isinstance(d[k], np.ndarray):
                h.update(k.encode())
                h.update(np.ascontiguousarray(d[k]).tobytes())
    return h.hexdigest()


def inputs(z, device="cuda"):
    """-> pred, gt dicts as compute_metrics takes them (tensors on `device`, gt with its flags)"""
    pred, gt = build_inputs(z)
    pred = {k: torch.from_numpy(np.ascontiguousarray(v)).to(device) for k, v in pred.items()}
    gt = {k: (torch.from_numpy(np.ascontiguousarray(v)).to(device) if isinstance(v, np.ndarray) else v) for k, v in gt.items()}
    gt["is_metric"], gt["has_sharp_boundary"] = (bool(v) for v in z["flags"])
    return pred, gt


def pred_depth_aligned(z, pred):
    """The reference's pred_depth_aligned (metrics.py:141-220), rebuilt from the fixture's variant parameters: the first depth variant's
    transform of its source (tools/make_metrics_golden.py checks this bit for bit against the reference's misc['pred_depth'])."""
    name = str(z["pda_variant"])
    mode, s, t0 = (float(v) for v in z["variant_params"][json.loads(str(z["variant_names"])).index(name)][:3])
    src = {"depth_metric": "depth_metric", "depth_scale_invariant": "depth_scale_invariant",
           "depth_affine_invariant": "depth_affine_invariant"}[name]
    src = pred.get(src, pred.get("depth_scale_invariant", pred.get("depth_metric")))
    s, t0 = torch.tensor(s, dtype=torch.float32, device=src.device), torch.tensor(t0, dtype=torch.float32, device=src.device)
    if mode == 0:
        return src if name == "depth_metric" else src * s
    return src * s + t0
