"""Golden fixtures of the evaluation metrics (tests/golden/metrics_*.npz) from the reference's unmodified `moge.test.metrics` on the CPU.

    python tools/make_metrics_golden.py          (build machine: needs the reference checkout of oracle/make_golden.py)

The reference imports two utils3d functions that are not vendored; beside oracle.make_golden.install_stubs() this file supplies them:
  * masked_nearest_resize: the convention of csrc/metrics.hip (lr_sample_kernel), restated in numpy below (unpinned);
  * sliding_window_2d: stride-1 windows over the last two dims, (H - k + 1, W - k + 1, k, k).
A fixture stores the compact recipe of its inputs (tests/metrics_fixtures.py: build_inputs turns it into the maps with float32 elementwise
arithmetic), and the reference is run on exactly those maps.  The four cases stay far below a megabyte each."""
from __future__ import annotations

import json
import math
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests.metrics_fixtures import NOISE_LEVELS, build_inputs, inputs_digest, pred_depth_aligned      # noqa: E402


def masked_nearest_resize_np(mask: np.ndarray, size=(64, 64)):
    """mask (H, W) bool -> lr_mask (h, w) bool, rows (h, w) int64, cols (h, w) int64 (csrc/metrics.hip, lr_sample_kernel)."""
    H, W = mask.shape
    h, w = size
    fh, fw = max(1.0, H / h), max(1.0, W / w)
    wh, ww = math.ceil(fh), math.ceil(fw)
    lr_mask = np.zeros((h, w), bool)
    rows = np.zeros((h, w), np.int64)
    cols = np.zeros((h, w), np.int64)
    for i in range(h):
        cy = (i + 0.5) * H / h
        y0 = int(np.rint(cy - fh / 2))
        for j in range(w):
            cx = (j + 0.5) * W / w
            x0 = int(np.rint(cx - fw / 2))
            best_v = best_a = math.inf
            by = bx = -1
            ay, ax = min(max(y0, 0), H - 1), min(max(x0, 0), W - 1)
            for y in range(y0, y0 + wh):
                if y < 0 or y >= H:
                    continue
                for x in range(x0, x0 + ww):
                    if x < 0 or x >= W:
                        continue
                    d = (y + 0.5 - cy) ** 2 + (x + 0.5 - cx) ** 2
                    if d < best_a:
                        best_a, ay, ax = d, y, x
                    if mask[y, x] and d < best_v:
                        best_v, by, bx = d, y, x
            lr_mask[i, j] = by >= 0
            rows[i, j], cols[i, j] = (by, bx) if by >= 0 else (ay, ax)
    return lr_mask, rows, cols


def _stub_masked_nearest_resize(*image, mask, size, return_index=False):
    lm, r, c = masked_nearest_resize_np(mask.cpu().numpy().astype(bool), size)
    rows, cols = torch.from_numpy(r), torch.from_numpy(c)
    out = tuple(im[..., rows, cols, :] if im.dim() == 3 else im[..., rows, cols] for im in image) + (torch.from_numpy(lm),)
    return out + ((rows, cols),) if return_index else out


def _stub_sliding_window_2d(x, window_size, stride=1, dim=(-2, -1)):
    assert stride == 1 and tuple(dim) == (-2, -1)
    return x.unfold(-2, window_size, 1).unfold(-2, window_size, 1)


def install():
    sys.path.insert(0, ROOT)
    from oracle.make_golden import install_stubs
    install_stubs()
    pt = sys.modules["utils3d"].pt
    pt.masked_nearest_resize = _stub_masked_nearest_resize
    pt.sliding_window_2d = _stub_sliding_window_2d


# ------------------------------------------------------------------------------------------------------------------------------------------
# synthetic scenes
# ------------------------------------------------------------------------------------------------------------------------------------------
def recipe(case, H, W, seed, steps=True):
    """A compact scene (tests/metrics_fixtures.py turns it into the full maps): a piecewise-constant gt depth (planes banded in y and x, with
    rectangular depth steps), a validity mask, a per-pixel noise level of the prediction and the intrinsics."""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:H, 0:W]
    depth = 3.0 + np.floor(24 * y / H) / 16 + np.floor(8 * x / W) / 8
    if steps:
        for _ in range(6):
            y0, x0 = rng.integers(0, H - H // 4), rng.integers(0, W - W // 4)
            depth[y0:y0 + rng.integers(H // 8, H // 4), x0:x0 + rng.integers(W // 8, W // 4)] -= np.round(rng.uniform(0.5, 1.5) * 8) / 8
    fx, fy = 0.8 + 0.1 * rng.random(), 0.8 * W / H + 0.1 * rng.random()
    K = np.array([[fx, 0, 0.5], [0, fy, 0.5], [0, 0, 1]], np.float32)
    pK = K.copy()
    pK[0, 0] *= 1.03
    pK[1, 1] *= 0.98
    mask = rng.random((H, W)) > 0.05
    mask[: H // 10, : W // 6] = False
    return dict(case=np.array(case), depth=np.maximum(depth, 0.5).astype(np.float16), mask=mask,
                noise_idx=rng.integers(0, len(NOISE_LEVELS), (H, W)).astype(np.uint8), gt_K=K, pred_K=pK)


def segments(H, W, seed):
    """15-20 segments with arbitrary ids: a grid of blocks, one tiny block (< 10 low-resolution samples), one block in the masked-out corner."""
    rng = np.random.default_rng(seed)
    seg = np.zeros((H, W), np.uint8)                   # 0 = unlabelled
    ids = rng.choice(np.arange(1, 250), 18, replace=False)
    k = 0
    for by in range(4):
        for bx in range(4):
            seg[by * H // 4 + 2:(by + 1) * H // 4 - 2, bx * W // 4 + 2:(bx + 1) * W // 4 - 2] = ids[k]
            k += 1
    seg[H // 10 // 4: H // 10 // 2, W // 6 // 4: W // 6 // 2] = ids[16]          # inside the masked-out corner
    seg[H // 2 - 4:H // 2 + 4, W // 2 - 4:W // 2 + 4] = ids[17]                  # tiny
    labels = {f"seg{i}": int(v) for i, v in enumerate(ids)}
    return seg, labels


def cases():
    """name -> (recipe, is_metric, has_sharp_boundary)"""
    b = recipe("b_ibims", 480, 640, 2)
    seg, labels = segments(480, 640, 2)
    b.update(seg=seg, labels=np.array(json.dumps(labels)))
    return {"a_plugin": (recipe("a_plugin", 240, 320, 1), True, False),
            "b_ibims": (b, False, True),
            "c_depth_only": (recipe("c_depth_only", 240, 320, 3), False, True),
            "d_moge1": (recipe("d_moge1", 187, 251, 4), False, True)}


def to_torch(rec, is_metric, sharp):
    pred, gt = build_inputs(rec)
    pred = {k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in pred.items()}
    gt = {k: (torch.from_numpy(np.ascontiguousarray(v)) if isinstance(v, np.ndarray) else v) for k, v in gt.items()}
    gt["is_metric"], gt["has_sharp_boundary"] = is_metric, sharp
    return pred, gt


def main():
    install()
    from moge.test import metrics as M              # the unmodified reference
    from moge.utils import alignment as RA
    torch.set_grad_enabled(False)
    os.makedirs(GOLDEN, exist_ok=True)
    for name, (rec, is_metric, sharp) in cases().items():
        pred, gt = to_torch(rec, is_metric, sharp)
        metrics, misc = M.compute_metrics(pred, gt, vis=True)
        mask, gd, gp = gt["depth_mask"], gt["depth"], gt["points"]
        lr_mask, (rows, cols) = _stub_masked_nearest_resize(mask=mask, size=(64, 64), return_index=True)
        lr = lambda x: x[rows, cols][lr_mask]                                       # noqa: E731
        store = {}
        # the alignment of every variant, by the same reference functions compute_metrics calls (metrics.py:157 / :184 / :207 / :231 / :250 / :269)
        variants = {}
        if "depth_metric" in pred and gt["is_metric"]:
            variants["depth_metric"] = (0, 1.0, [0, 0, 0])
        pdsi = pred.get("depth_scale_invariant", pred.get("depth_metric"))
        if pdsi is not None:
            g = lr(gd)
            variants["depth_scale_invariant"] = (0, float(RA.align_depth_scale(lr(pdsi), g, 1 / g)), [0, 0, 0])
        pdai = next((pred[k] for k in ("depth_affine_invariant", "depth_scale_invariant", "depth_metric") if k in pred), None)
        if pdai is not None:
            g = lr(gd)
            s, t = RA.align_depth_affine(lr(pdai), g, 1 / g)
            variants["depth_affine_invariant"] = (1, float(s), [float(t), 0, 0])
        pdisp = pred.get("disparity_affine_invariant")
        if pdisp is None and "depth_scale_invariant" in pred:
            pdisp = 1 / pred["depth_scale_invariant"]
        if pdisp is None and "depth_metric" in pred:
            pdisp = 1 / pred["depth_metric"]
        if pdisp is not None:
            s, t = RA.align_affine_lstsq(pdisp[mask], 1 / gd[mask])
            variants["disparity_affine_invariant"] = (3, float(s), [float(t), 0, 0], float(np.float32(1 / gd[mask].max().item())))
        if "points_metric" in pred and gt["is_metric"]:
            g = lr(gp)
            t = RA.align_points_xyz_shift(lr(pred["points_metric"]), g, 1 / g.norm(dim=-1))
            variants["points_metric"] = (2, 1.0, [float(v) for v in t])
        ppsi = pred.get("points_scale_invariant", pred.get("points_metric"))
        if ppsi is not None:
            g = lr(gp)
            variants["points_scale_invariant"] = (0, float(RA.align_points_scale(lr(ppsi), g, 1 / g.norm(dim=-1))), [0, 0, 0])
        ppai = next((pred[k] for k in ("points_affine_invariant", "points_scale_invariant", "points_metric") if k in pred), None)
        if ppai is not None:
            g = lr(gp)
            s, t = RA.align_points_scale_xyz_shift(lr(ppai), g, 1 / g.norm(dim=-1))
            variants["points_affine_invariant"] = (1, float(s), [float(v) for v in t])
        params = {k: [float(v[0]), v[1], *v[2], (v[3] if len(v) > 3 else 0.0)] for k, v in variants.items()}
        # per-radius F1 on the reference's pred_depth_aligned
        pda = misc["pred_depth"]
        f1 = [M.boundary_f1(pda, gd, mask, radius=r) for r in (1, 2, 3)]
        # per segment (metrics.py:292-311), by the reference's functions
        if "segmentation_mask" in gt:
            p = next(pred[k] for k in pred if "points" in k)
            segm = gt["segmentation_mask"]
            seg_lr = segm[rows, cols]
            seg_rows = []
            for key, sid in gt["segmentation_labels"].items():
                vm = (segm == sid) & mask
                vlr = (seg_lr == sid) & lr_mask
                n_lr = int(vlr.sum())
                if n_lr < 10:
                    seg_rows.append([sid, n_lr] + [math.nan] * 7)
                    continue
                gm = gp[vm]
                diam = (gm.max(dim=0).values - gm.min(dim=0).values).max()
                plr, glr = p[rows, cols][vlr], gp[rows, cols][vlr]
                s, t = RA.align_points_scale_xyz_shift(plr, glr, 1 / diam.expand(glr.shape[0]))
                pm = p[vm] * s + t
                seg_rows.append([sid, n_lr, float(diam), float(s), *[float(v) for v in t], M.rel_point_local(pm, gm, diam), M.delta1_point_local(pm, gm, diam)])
            store["segments"] = np.array(seg_rows, np.float64)        # id, lr count, diameter, scale, shift xyz, rel, delta1
        store.update(rec)
        store["inputs_sha256"] = np.array(inputs_digest(*build_inputs(rec)))
        depth_variants = [k for k in params if k.startswith("depth_")]
        store["pda_variant"] = np.array(depth_variants[0] if depth_variants else "")
        store.update(metrics=np.array(json.dumps(metrics)), flags=np.array([is_metric, sharp]),
                     lr_mask=lr_mask.numpy(), lr_index=np.stack([rows.numpy(), cols.numpy()]).astype(np.int32),
                     variant_names=np.array(json.dumps(list(params))), variant_params=np.array(list(params.values()), np.float64),
                     boundary_f1=np.array(f1, np.float64),
                     misc_shapes=np.array(json.dumps({k: list(v.shape) for k, v in misc.items()})))
        if depth_variants:                               # the tests rebuild pred_depth_aligned from the stored variant: it must be the reference's
            assert torch.equal(pred_depth_aligned(store, pred), pda), name
        path = os.path.join(GOLDEN, f"metrics_{name}.npz")
        np.savez_compressed(path, **store)
        print(path, os.path.getsize(path), json.dumps(metrics)[:300])


if __name__ == "__main__":
    main()
