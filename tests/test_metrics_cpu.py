"""CPU: the evaluation-metric fixtures load, the generator's masked_nearest_resize stand-in follows its stated convention on a hand-worked case,
and moge_amd.metrics refuses CPU tensors."""
import json

import numpy as np
import pytest
import torch

from tests.metrics_fixtures import CASES, build_inputs, inputs, inputs_digest, load, pred_depth_aligned
from tools.make_metrics_golden import masked_nearest_resize_np


@pytest.mark.parametrize("name", CASES)
def test_fixture_loads(name):
    z = load(name)
    metrics = json.loads(str(z["metrics"]))
    pred, gt = build_inputs(z)
    assert inputs_digest(pred, gt) == str(z["inputs_sha256"])      # the rebuilt maps are the ones the reference scored
    H, W = gt["depth_mask"].shape
    assert z["lr_mask"].shape == (64, 64) and z["lr_index"].shape == (2, 64, 64)
    assert (z["lr_index"][0] < H).all() and (z["lr_index"][1] < W).all()
    assert json.loads(str(z["variant_names"])) and z["variant_params"].shape[1] == 6
    assert all(np.isfinite(v) for d in metrics.values() for v in d.values())
    if z["flags"][1]:
        pt, _ = inputs(z, device="cpu")
        assert tuple(pred_depth_aligned(z, pt).shape) == (H, W) and "boundary" in metrics


def test_masked_nearest_resize_hand_case():
    # 4 x 6 image to a 2 x 3 grid: fh = fw = 2, window 2 x 2, centres (2i + 1, 2j + 1), top-left rint(centre - 1) = (2i, 2j);
    # every pixel of a window is at distance sqrt(0.5) from the centre, so the first valid pixel in row-major order wins
    mask = np.zeros((4, 6), bool)
    mask[0, 1] = mask[1, 0] = True          # window (0, 0): (0, 1) comes first
    mask[1, 3] = True                       # window (0, 1): only (1, 3)
    mask[3, 5] = True                       # window (1, 2)
    lr_mask, rows, cols = masked_nearest_resize_np(mask, (2, 3))
    assert lr_mask.tolist() == [[True, True, False], [False, False, True]]
    assert (rows[0, 0], cols[0, 0]) == (0, 1) and (rows[0, 1], cols[0, 1]) == (1, 3) and (rows[1, 2], cols[1, 2]) == (3, 5)
    # a 3 x 3 window (fh = 2.5 -> ceil 3) with an odd source size: 5 x 5 to 2 x 2.  Cell 0: centre 1.25, top-left rint(0) = 0, nearest
    # source centre 1.5 -> pixel 1.  Cell 1: centre 3.75, top-left rint(2.5) = 2 (half to even), nearest source centre 3.5 -> pixel 3;
    # with (3, 3) masked out, (3, 4) and (4, 3) tie nearest (0.0625 + 0.5625; (2, 3) and (3, 2) are at 0.0625 + 1.5625), and (3, 4) comes
    # first in row-major window order
    m = np.ones((5, 5), bool)
    lm, r, c = masked_nearest_resize_np(m, (2, 2))
    assert lm.all() and (r[0, 0], c[0, 0]) == (1, 1) and (r[1, 1], c[1, 1]) == (3, 3)
    m[3, 3] = False
    lm, r, c = masked_nearest_resize_np(m, (2, 2))
    assert (r[1, 1], c[1, 1]) == (3, 4)


def test_metrics_reject_cpu_tensors():
    from moge_amd import metrics as M
    z = load("c_depth_only")
    pred, gt = inputs(z, device="cpu")
    with pytest.raises(RuntimeError, match="GPU tensors only"):
        M.compute_metrics(pred, gt)
    with pytest.raises(RuntimeError, match="GPU tensors only"):
        M.rel_depth(torch.ones(4), torch.ones(4))
    with pytest.raises(RuntimeError, match="GPU tensors only"):
        M.masked_nearest_resize(mask=torch.ones(8, 8, dtype=torch.bool), size=(4, 4), return_index=True)


# ---------------------------------------------------------------------------------------------------------------------------------------
# the numpy references of tests/eval_reference.py (what the GPU sweeps compare the kernels with) against the reference's stored results
# ---------------------------------------------------------------------------------------------------------------------------------------
def variant_sources(pred):
    """the tensor each stored variant of a fixture transforms (metrics.py:134-280 fall-back chains)"""
    src = {"depth_metric": pred.get("depth_metric"), "depth_scale_invariant": pred.get("depth_scale_invariant", pred.get("depth_metric")),
           "depth_affine_invariant": next((pred[k] for k in ("depth_affine_invariant", "depth_scale_invariant", "depth_metric") if k in pred), None),
           "points_metric": pred.get("points_metric"), "points_scale_invariant": pred.get("points_scale_invariant", pred.get("points_metric")),
           "points_affine_invariant": next((pred[k] for k in ("points_affine_invariant", "points_scale_invariant", "points_metric") if k in pred), None)}
    if "disparity_affine_invariant" in pred:
        src["disparity_affine_invariant"] = pred["disparity_affine_invariant"]
    else:
        src["disparity_affine_invariant"] = 1 / next(pred[k] for k in ("depth_scale_invariant", "depth_metric") if k in pred)
    return src


@pytest.mark.parametrize("name", CASES)
def test_error_pass_reference_matches_fixture(name):
    from tests.eval_reference import error_pass_ref
    z = load(name)
    pred, gt = inputs(z, device="cpu")
    ref = json.loads(str(z["metrics"]))
    mask = gt["depth_mask"].numpy()
    n = int(mask.sum())
    src = variant_sources(pred)
    for k, prm in zip(json.loads(str(z["variant_names"])), z["variant_params"]):
        dim = 3 if k.startswith("points") else 1
        g = gt["points"] if dim == 3 else gt["depth"]
        s, d1, cnt = error_pass_ref(src[k].numpy(), g.numpy(), mask, prm[None], dim)[0]
        assert cnt == n
        assert abs(s / n - ref[k]["rel"]) <= 1e-5 * abs(ref[k]["rel"]), (k, s / n, ref[k]["rel"])
        assert int(d1) == round(ref[k]["delta1"] * n), (k, d1, ref[k]["delta1"] * n)


@pytest.mark.parametrize("name", ["b_ibims", "c_depth_only", "d_moge1"])
def test_boundary_reference_matches_fixture(name):
    from tests.eval_reference import boundary_counts_ref, boundary_f1_ref
    z = load(name)
    pred, gt = inputs(z, device="cpu")
    pda = pred_depth_aligned(z, pred).numpy()
    for r in (1, 2, 3):
        f1 = boundary_f1_ref(boundary_counts_ref(pda, gt["depth"].numpy(), gt["depth_mask"].numpy(), r))
        assert abs(f1 - z["boundary_f1"][r - 1]) <= 1e-6, (r, f1, z["boundary_f1"][r - 1])


def test_segment_reference_matches_fixture():
    """per stored segment (id, lr count, diameter, scale, shift xyz, rel, delta1; the reference fills the last six for kept segments only):
    the low-resolution count, and for kept segments the diameter and the per-segment error at the reference's own scale and shift"""
    from tests.eval_reference import segment_error_ref, segments_ref
    z = load("b_ibims")
    pred, gt = inputs(z, device="cpu")
    labels = sorted(set(gt["segmentation_labels"].values()))
    seg, mask, gtp = gt["segmentation_mask"].numpy(), gt["depth_mask"].numpy(), gt["points"].numpy()
    got = dict(zip(labels, segments_ref(seg, mask, gtp, labels, z["lr_mask"], z["lr_index"])))
    pp = pred["points_scale_invariant"].numpy()
    kept = 0
    for row in z["segments"]:
        s = got[int(row[0])]
        assert s["lr_count"] == int(row[1]), row
        if row[1] < 10:
            continue
        kept += 1
        assert float(s["diameter"]) == row[2], (row, s["diameter"])
        rel, d1, n = segment_error_ref(seg, mask, pp, gtp, int(row[0]), row[3], row[4:7], s["diameter"])
        assert abs(rel / n - row[7]) <= 1e-5 * abs(row[7]), (row, rel / n)
        assert d1 == round(row[8] * n), (row, d1, row[8] * n)
    assert kept >= 10
