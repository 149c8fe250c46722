"""GPU: moge_amd.evaluation (csrc/evaldata.hip) against the reference's `EvalDataLoaderPipeline._process_instance` through the fixtures of
tools/make_eval_golden.py, determinism, and the `eval_baseline` command end to end on a generated benchmark directory."""
import hashlib
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from moge_amd import evaluation as E
from tests.eval_fixtures import CASES, build_instance, config, load, recipe

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module", autouse=True)
def _needs_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


def _warp(z):
    inst = build_instance(recipe(z))
    cfg = config(z)
    seg = inst.get("segmentation_mask")
    seg_t = None
    if cfg["include_segmentation"] and seg is not None:
        seg_t = torch.from_numpy(seg.view(np.int16) if seg.dtype == np.uint16 else seg).cuda()
    warped = E.warp_sample(torch.from_numpy(inst["image"]).cuda(), torch.from_numpy(inst["depth"]).cuda(), torch.from_numpy(inst["depth_mask"]).cuda(),
                           inst["intrinsics"], inst["width"], inst["height"], segmentation=seg_t, drop_max_depth=cfg["drop_max_depth"],
                           depth_unit=cfg["depth_unit"])
    meta = {k: v for k, v in inst.items() if k not in ("image", "depth", "depth_mask", "segmentation_mask")}
    out = E.finish_sample(meta, warped, cfg["include_segmentation"], cfg["max_segments"], cfg["min_seg_area"], cfg["depth_unit"],
                          cfg["has_sharp_boundary"])
    torch.cuda.synchronize()
    return inst, warped, out


def _unpack(bits, shape):
    return np.unpackbits(bits)[: int(np.prod(shape))].reshape(shape).astype(bool)


@pytest.fixture(scope="module", params=CASES)
def case(request, _needs_gpu):
    z = load(request.param)
    return (request.param, z) + _warp(z)


def test_lanczos_bytes(case):
    name, z, _, warped, _ = case
    lz = warped["rescaled_image"].cpu().numpy()
    assert lz.shape[:2] == tuple(int(v) for v in z["rescaled_size"])
    assert np.array_equal(lz[:64, :96], z["lanczos_crop"])
    assert hashlib.sha256(np.ascontiguousarray(lz).tobytes()).hexdigest() == str(z["lanczos_sha256"])


def test_masked_nearest_depth(case):
    name, z, inst, warped, _ = case
    h, w = warped["geometry"]["rescaled_size"]
    d, m, _ = E.masked_nearest_resize_distance(torch.from_numpy(inst["depth"]).cuda(), torch.from_numpy(inst["depth_mask"]).cuda(), (h, w),
                                               inst["intrinsics"])
    assert np.array_equal(d.cpu().numpy(), z["mnr_depth"])
    assert np.array_equal(m.cpu().numpy().astype(bool), _unpack(z["mnr_mask"], (h, w)))


def test_remapped_image(case):
    name, z, _, warped, out = case
    got = warped["image_u8"].cpu().numpy()[::2]
    ref = z["image_rows"]
    diff = np.abs(got.astype(np.int16) - ref.astype(np.int16))
    assert diff.max() <= 1 and (diff.any(axis=-1)).mean() <= 1e-3, (diff.max(), diff.any(axis=-1).mean())
    u8 = warped["image_u8"].cpu().numpy()
    assert np.array_equal(out["image"].cpu().numpy(), u8.astype(np.float32).transpose(2, 0, 1) / 255.0)      # numpy's true division, :191


def test_max_depth_mask_depth_points(case):
    name, z, _, warped, out = case
    H, W = out["depth"].shape
    md = warped["max_depth"].cpu().numpy()[0]
    assert np.float32(md).tobytes() == np.float32(z["max_depth"]).tobytes() or (math.isnan(md) and math.isnan(float(z["max_depth"])))
    knife = _unpack(z["knife"], (H, W))
    mask = out["depth_mask"].cpu().numpy()
    ref_mask = _unpack(z["depth_mask"], (H, W))
    assert np.array_equal(mask[~knife], ref_mask[~knife]), int((mask != ref_mask)[~knife].sum())
    ok = ~knife
    depth = out["depth"].cpu().numpy()
    ref = z["depth_rows"]
    sel = ok[::6]
    assert np.all(np.abs(depth[::6][sel] - ref[sel]) <= 1e-6 * np.maximum(np.abs(ref[sel]), 1e-30))
    pts = out["points"].cpu().numpy()[::6, ::6]
    rp = z["points_sub"]
    sel = ok[::6, ::6]
    assert np.all(np.abs(pts[sel] - rp[sel]) <= 1e-6 * np.maximum(np.abs(rp[sel]), 1e-30))


def test_labels_and_label_type(case):
    name, z, _, _, out = case
    ref = json.loads(str(z["segmentation_labels"]))
    got = out.get("segmentation_labels")
    assert got == ref and (got is None or list(got.items()) == list(ref.items()))
    assert out.get("label_type", "") == str(z["label_type"])
    cfg = config(z)
    assert out["is_metric"] == (cfg["depth_unit"] is not None)
    keys = {"filename", "width", "height", "image", "depth", "depth_mask", "depth_mask_inf", "intrinsics", "points", "is_metric", "has_sharp_boundary"}
    assert keys <= set(out)
    for k in ("image", "depth", "depth_mask", "intrinsics", "points"):
        assert out[k].is_cuda


def test_two_runs_same_bits():
    z = load("kitti")
    _, a, oa = _warp(z)
    _, b, ob = _warp(z)
    for k in ("image", "depth", "depth_mask", "points"):
        assert torch.equal(oa[k], ob[k]), k
    assert torch.equal(a["max_depth"], b["max_depth"])
    z = load("ibims")
    _, a, _ = _warp(z)
    _, b, _ = _warp(z)
    assert torch.equal(a["segmentation_hist"], b["segmentation_hist"]) and torch.equal(a["segmentation_mask"], b["segmentation_mask"])


def test_rejects_cpu_tensors():
    with pytest.raises(RuntimeError):
        E.lanczos_resize(torch.zeros((4, 4, 3), dtype=torch.uint8), 2, 2)


# ---------------------------------------------------------------------------------------------------------------------------------------
# end to end: the command on a generated two-benchmark, three-sample directory
# ---------------------------------------------------------------------------------------------------------------------------------------
def _same(a, b):
    """nested dict equality with NaN == NaN"""
    if isinstance(a, dict) or isinstance(b, dict):
        return isinstance(a, dict) and isinstance(b, dict) and list(a) == list(b) and all(_same(a[k], b[k]) for k in a)
    return a == b or (isinstance(a, float) and isinstance(b, float) and math.isnan(a) and math.isnan(b))


def write_benchmark(root, name, n, H, W, with_seg, seed):
    from PIL import Image
    rng = np.random.default_rng(seed)
    d = root / name
    files = []
    for i in range(n):
        f = f"sample_{i}"
        p = d / f
        p.mkdir(parents=True)
        y, x = np.mgrid[0:H, 0:W]
        img = np.stack([(x * (3 + c) + y * (2 + i) + 40 * c) % 256 for c in range(3)], -1).astype(np.uint8)
        Image.fromarray(img).save(p / "image.jpg", quality=95)
        depth = (2.0 + 3.0 * y / H + np.floor(4 * x / W) * 0.5 + rng.uniform(0, 0.01, (H, W))).astype(np.float32)
        depth[rng.random((H, W)) < 0.05] = np.nan
        E.write_depth(p / "depth.png", depth)
        if with_seg:
            seg = (1 + (y * 3 // H) * 4 + (x * 4 // W)).astype(np.uint8)
            E.write_segmentation(p / "segmentation.png", seg, {f"s{k}": k for k in range(1, 13)} | {"sky": 13})
        K = [[0.9 + 0.05 * i, 0, 0.5 + 0.01 * i], [0, 0.9 * W / H, 0.5], [0, 0, 1]]
        (p / "meta.json").write_text(json.dumps({"intrinsics": K}))
        files.append(f)
    (d / ".index.txt").write_text("\n".join(files))
    return str(d)


@pytest.fixture(scope="module")
def bench_dir(tmp_path_factory, _needs_gpu):
    root = tmp_path_factory.mktemp("evalbench")
    cfg = {
        "BenchA": {"path": write_benchmark(root, "A", 3, 120, 160, False, 0), "width": 160, "height": 120, "depth_unit": 1.0},
        # metric: with vis (--dump_pred) and a non-metric benchmark, the reference's compute_metrics reads pred['points_scale_invariant'],
        # which a v2 plugin does not return (metrics.py:256-257; moge_amd.metrics keeps that behaviour)
        "BenchB": {"path": write_benchmark(root, "B", 3, 150, 200, True, 1), "width": 160, "height": 128, "include_segmentation": True,
                   "min_seg_area": 50, "has_sharp_boundary": True, "depth_unit": 1.0},
    }
    (root / "config.json").write_text(json.dumps(cfg))
    from oracle import moge_oracle as O
    mcfg = O.named_configs()["tiny-vits-normal"]
    O.save_checkpoint(str(root / "model.pt"), mcfg, O.synth_state_dict(mcfg, 0, True))
    return root, cfg


def test_eval_baseline_end_to_end(bench_dir):
    root, cfg = bench_dir
    out = root / "out" / "res.json"
    cmd = [sys.executable, "-m", "moge_amd.scripts.cli", "eval_baseline", "--baseline", os.path.join(ROOT, "baselines", "moge_mi355x.py"),
           "--config", str(root / "config.json"), "--output", str(out), "--dump_pred", "--dump_gt", "--pretrained", str(root / "model.pt"),
           "--version", "v2", "--num_tokens", "108"]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    res = json.loads(out.read_text())
    assert list(res) == ["BenchA", "BenchB", "mean"]
    assert "inference_time" in res["BenchA"] and "inference_time" in res["mean"]
    assert "depth_scale_invariant" in res["BenchA"] and "rel" in res["BenchA"]["depth_scale_invariant"]
    assert all(isinstance(v, dict) for k, v in res["BenchB"].items() if k != "inference_time")
    assert _same(E.key_average([res["BenchA"], res["BenchB"]]), res["mean"])
    for b in ("BenchA", "BenchB"):
        for i in range(3):
            d = root / "out" / "res_dump" / b / f"sample_{i}"
            for f in ("pred/image.jpg", "pred/metrics.json", "pred/points.exr", "pred/depth.png", "pred/fov.json", "gt/image.jpg", "gt/points.exr",
                      "gt/depth.png", "gt/mask.png", "gt/info.json"):
                assert (d / f).exists(), d / f

    # every value equals key_average of compute_metrics on the same samples (the inference time aside)
    sys.path.insert(0, os.path.join(ROOT, "baselines"))
    from moge_amd.metrics import compute_metrics
    import importlib.util
    spec = importlib.util.spec_from_file_location("moge_mi355x", os.path.join(ROOT, "baselines", "moge_mi355x.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    baseline = mod.Baseline(108, 9, str(root / "model.pt"), False, "cuda:0", "v2")
    for b, bc in cfg.items():
        ms = []
        with E.EvalDataLoader(**bc) as loader:
            for _ in range(len(loader)):
                s = loader.get()
                m, _ = compute_metrics(baseline.infer_for_evaluation(s["image"]), s)
                ms.append(m)
        ref = E.key_average(ms)
        got = dict(res[b])
        got.pop("inference_time")
        assert _same(json.loads(json.dumps(ref)), got), b
