"""GPU: moge_amd.metrics (csrc/metrics.hip) against the reference's compute_metrics through the fixtures of tools/make_metrics_golden.py, the
batched local-points solve against a per-segment loop, and a full evaluation size (2048 x 1365, 100 segments) without a fixture."""
import json
import warnings

import numpy as np
import pytest
import torch

from tests.metrics_fixtures import CASES, inputs, load, pred_depth_aligned

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def M():
    from moge_amd import metrics
    return metrics


@pytest.mark.parametrize("name", CASES)
def test_lr_sampling(M, name):
    z = load(name)
    _, gt = inputs(z)
    lr_mask, (rows, cols) = M.masked_nearest_resize(mask=gt["depth_mask"], size=(64, 64), return_index=True)
    assert np.array_equal(lr_mask.cpu().numpy(), z["lr_mask"])
    assert np.array_equal(rows.cpu().numpy(), z["lr_index"][0]) and np.array_equal(cols.cpu().numpy(), z["lr_index"][1])
    d = gt["depth"]
    assert torch.equal(d[rows, cols], d[torch.from_numpy(z["lr_index"][0]).long().cuda(), torch.from_numpy(z["lr_index"][1]).long().cuda()])


@pytest.mark.parametrize("name", CASES)
def test_error_pass_with_reference_alignment(M, name):
    z = load(name)
    pred, gt = inputs(z)
    ref = json.loads(str(z["metrics"]))
    names = json.loads(str(z["variant_names"]))
    mask = gt["depth_mask"]
    src = {"depth_metric": pred.get("depth_metric"), "depth_scale_invariant": pred.get("depth_scale_invariant", pred.get("depth_metric")),
           "depth_affine_invariant": next((pred[k] for k in ("depth_affine_invariant", "depth_scale_invariant", "depth_metric") if k in pred), None),
           "points_metric": pred.get("points_metric"), "points_scale_invariant": pred.get("points_scale_invariant", pred.get("points_metric")),
           "points_affine_invariant": next((pred[k] for k in ("points_affine_invariant", "points_scale_invariant", "points_metric") if k in pred), None)}
    if "disparity_affine_invariant" in pred:
        src["disparity_affine_invariant"] = pred["disparity_affine_invariant"]
    else:
        src["disparity_affine_invariant"] = 1 / next(pred[k] for k in ("depth_scale_invariant", "depth_metric") if k in pred)
    n = int(mask.sum())
    for k, prm in zip(names, z["variant_params"]):
        g = gt["points"] if k.startswith("points") else gt["depth"]
        out = M.error_pass(src[k], g, mask, torch.tensor(prm, dtype=torch.float32, device="cuda")[None]).cpu().numpy()[0]
        assert out[2] == n
        rel = out[0] / out[2]
        assert abs(rel - ref[k]["rel"]) <= 1e-5 * abs(ref[k]["rel"]), (k, rel, ref[k]["rel"])
        assert int(out[1]) == round(ref[k]["delta1"] * n), (k, int(out[1]), ref[k]["delta1"] * n)


@pytest.mark.parametrize("name", ["b_ibims", "c_depth_only", "d_moge1"])
def test_boundary_f1(M, name):
    z = load(name)
    pred, gt = inputs(z)
    pda = pred_depth_aligned(z, pred)
    for r in (1, 2, 3):
        f1 = M.boundary_f1(pda, gt["depth"], gt["depth_mask"], radius=r)
        assert abs(f1 - z["boundary_f1"][r - 1]) <= 1e-6, (r, f1, z["boundary_f1"][r - 1])


def _close(a, b):
    return abs(a - b) <= max(2e-3 * abs(b), 1e-4)


@pytest.mark.parametrize("name", CASES)
def test_compute_metrics_end_to_end(M, name):
    z = load(name)
    pred, gt = inputs(z)
    ref = json.loads(str(z["metrics"]))
    metrics, misc = M.compute_metrics(pred, gt, vis=True)
    assert list(metrics) == list(ref)
    for k in ref:
        assert list(metrics[k]) == list(ref[k]), k
        for kk, v in ref[k].items():
            assert isinstance(metrics[k][kk], float)
            if k == "fov_x":
                assert abs(metrics[k][kk] - v) <= 1e-4, (k, kk)
            else:
                assert _close(metrics[k][kk], v), (k, kk, metrics[k][kk], v)
    shapes = json.loads(str(z["misc_shapes"]))
    assert list(misc) == list(shapes) and all(list(misc[k].shape) == s for k, s in shapes.items())


def _objective(src, tgt, w, scale, shift):
    return ((src * scale[:, None, None] + shift[:, None, :] - tgt).abs() * w[..., None]).sum(dim=(1, 2))


def test_batched_segments_match_loop(M):
    from moge_amd import alignment as A
    z = load("b_ibims")
    pred, gt = inputs(z)
    mask = gt["depth_mask"]
    lr_mask, lr_index = M.masked_nearest_resize(mask=mask, size=(64, 64), return_index=True)
    p = pred["points_scale_invariant"]
    det = {}
    res = M.local_points(p, gt["points"], mask, gt["segmentation_mask"], gt["segmentation_labels"], lr_mask, lr_index, details=det)
    src, tgt, wt = det["src"], det["tgt"], det["weight"]
    obj_b = _objective(src, tgt, wt, det["scale"], det["shift"])
    ref = z["segments"]
    kept = sorted((r for r in ref if r[1] >= 10), key=lambda r: r[0])     # batch rows follow the sorted labels
    assert src.shape[0] == len(kept)
    scales, shifts = [], []
    for e in range(src.shape[0]):
        n = int((wt[e] > 0).sum())
        s, t = A.align_points_scale_xyz_shift(src[e, :n], tgt[e, :n], wt[e, :n])
        scales.append(s)
        shifts.append(t)
        assert np.isclose(float(det["diameter"][e]), kept[e][2], rtol=0, atol=0)
    obj_l = _objective(src, tgt, wt, torch.stack(scales), torch.stack(shifts))
    assert bool((obj_b <= obj_l * (1 + 1e-5)).all())
    # per-segment metrics of the loop's solution through the same kernel
    seg = gt["segmentation_mask"]
    labels = sorted(set(gt["segmentation_labels"].values()))
    loop = []
    for e, r in enumerate(kept):
        vm = (seg == int(r[0])) & mask
        d = det["diameter"][e]
        pm = p[vm] * scales[e] + shifts[e]
        loop.append({"rel": M.rel_point_local(pm, gt["points"][vm], d), "delta1": M.delta1_point_local(pm, gt["points"][vm], d)})
    ka = M.key_average(loop)
    assert list(res) == ["delta1", "rel"]
    for k in res:
        assert abs(res[k] - ka[k]) <= 1e-5 * max(1.0, abs(ka[k])), (k, res[k], ka[k])
    assert labels


def _full_case(S, seed=0, H=1365, W=2048):
    g = torch.Generator(device="cuda").manual_seed(seed)
    y = torch.arange(H, device="cuda", dtype=torch.float32)[:, None]
    x = torch.arange(W, device="cuda", dtype=torch.float32)[None, :]
    depth = 4.0 + 2.0 * y / H + torch.sin(x / W * 6.0)
    depth = depth + ((x // 256 + y // 256) % 3 == 0).float() * 1.5          # sharp steps
    K = torch.tensor([[0.8, 0, 0.5], [0, 1.2, 0.5], [0, 0, 1]], device="cuda")
    u, v = (x + 0.5) / W, (y + 0.5) / H
    pts = torch.stack([(u - 0.5) / 0.8 * depth, (v - 0.5) / 1.2 * depth, depth], -1)
    mask = torch.rand(H, W, device="cuda", generator=g) > 0.03
    noise = 1 + 0.05 * torch.randn(H, W, 1, device="cuda", generator=g)
    pp = pts * noise * 1.3 + torch.tensor([0.02, -0.01, 0.3], device="cuda")
    side = int(np.ceil(np.sqrt(S)))
    seg = ((y * side // H) * side + (x * side // W)).long() * 7 + 3        # arbitrary ids
    labels = {f"s{i}": int(i * 7 + 3) for i in range(S)}
    pred = {"points_metric": pp, "depth_metric": pp[..., 2].contiguous(), "intrinsics": K * 1.02}
    gt = {"depth": depth.contiguous(), "points": pts.contiguous(), "depth_mask": mask, "intrinsics": K, "segmentation_mask": seg,
          "segmentation_labels": labels, "is_metric": True, "has_sharp_boundary": True}
    return pred, gt


def _count_syncs(fn):
    torch.cuda.synchronize()
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        torch.cuda.set_sync_debug_mode("warn")
        try:
            out = fn()
        finally:
            torch.cuda.set_sync_debug_mode("default")
    return out, [f"{w.filename.split('/')[-1]}:{w.lineno}" for w in rec if "synchroniz" in str(w.message)]


def _values(m):
    return [(k, kk, v) for k, d in m.items() for kk, v in d.items()]


def test_full_eval_size(M):
    pred, gt = _full_case(100)
    m1, _ = M.compute_metrics(pred, gt)
    m2, _ = M.compute_metrics(pred, gt)
    assert set(m1) >= {"depth_metric", "points_affine_invariant", "local_points", "boundary", "fov_x"}
    assert all(np.isfinite(v) for _, _, v in _values(m1))
    assert _values(m1) == _values(m2)                                      # bit-identical
    # a power-of-two scale of pred and gt changes no delta1 or F1 count and no relative error beyond the eps of rel_depth / rel_point (g + 1e-6)
    p2 = {k: (v * 4.0 if k != "intrinsics" else v) for k, v in pred.items()}
    g2 = dict(gt, depth=gt["depth"] * 4.0, points=gt["points"] * 4.0)
    m3, _ = M.compute_metrics(p2, g2)
    for (k, kk, a), (_, _, b) in zip(_values(m1), _values(m3)):
        assert (abs(a - b) <= 1e-5 * abs(a)) if kk == "rel" else (a == b), (k, kk, a, b)
    # the host synchronises as often for 10 segments as for 100 (each counted after one uncounted call: first-use work such as the sync
    # debug mode's own set-up is not part of a call)
    p10, g10 = _full_case(10)
    M.compute_metrics(p10, g10)
    _count_syncs(lambda: None)
    _, n100 = _count_syncs(lambda: M.compute_metrics(pred, gt))
    _, n10 = _count_syncs(lambda: M.compute_metrics(p10, g10))
    assert len(n100) > 0 and len(n10) == len(n100), (n10, n100)
