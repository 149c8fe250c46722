"""CPU: the host half of moge_amd.train_data against the fixtures of the reference's `_process_instance` (tests/golden/train_*.npz), the numpy
references of tests/train_data_reference.py against the same fixtures (which pins them to the reference), and the loader's host logic."""
import json
import random
import warnings

import numpy as np
import pytest
from PIL import Image

from moge_amd import evaluation as E
from moge_amd import train_data as T
from tests import train_data_reference as R
from tests.train_data_fixtures import CASES, build_instance, config, instance_digest, knife_map, load, recipe, warp_kwargs

REL, ABS = 1e-6, 1e-6             # depth / max_depth relative, normal absolute


def _bits(z, key, shape):
    return np.unpackbits(z[key])[:shape[0] * shape[1]].reshape(shape).astype(bool)


@pytest.fixture(scope="module", params=CASES)
def case(request):
    z = load(request.param)
    inst = build_instance(recipe(z))
    assert instance_digest(inst) == str(z["digest"])
    cfg = config(z)
    ref = R.warp_train_sample(inst["image"], inst["depth"], inst["intrinsics"], inst["width"], inst["height"], inst["seed"], **warp_kwargs(cfg))
    return request.param, z, inst, cfg, ref


def test_cases_reach_their_branches():
    sizes = {}
    for name in CASES:
        z = load(name)
        raw = (int(z["recipe_H"]), int(z["recipe_W"]))
        sizes[name] = (tuple(z["image_size"]) != raw, tuple(z["nearest_size"]) != raw)
    assert sizes["upscale"] == (False, False) and sizes["downscale"] == (True, True) and sizes["mild"] == (False, True)
    assert bool(load("flip_yes")["flip"]) and not bool(load("flip_no")["flip"])
    assert bool(load("allnan")["invalid"]) and not any(bool(load(n)["invalid"]) for n in CASES if n != "allnan")
    holes = load("holes")
    shape = (int(holes["recipe_tgt_H"]), int(holes["recipe_tgt_W"]))
    branch = _bits(holes, "bilinear", shape)
    assert 0.2 < branch.mean() < 0.8 and np.isnan(holes["depth"]).any() and np.isinf(holes["depth"]).any()
    assert (holes["depth"][np.isfinite(holes["depth"])] == holes["max_depth"]).any()                 # the clamp cuts
    R_far = load("offcentre")["R"]
    assert np.abs(R_far - np.eye(3)).max() > 0.05
    metric = load("metric")
    shape = (int(metric["recipe_tgt_H"]), int(metric["recipe_tgt_W"]))
    assert bool(metric["is_metric"]) and (_bits(metric, "depth_mask_fin", shape) != ~_bits(metric, "depth_mask_inf", shape)).any()


def test_geometry_reproduces_the_sampled_view(case):
    _, z, inst, cfg, ref = case
    geo = ref["geometry"]
    assert np.abs(geo["tgt_intrinsics"] - z["tgt_intrinsics"]).max() <= 1e-6 and geo["tgt_intrinsics"].dtype == np.float32
    assert np.abs(np.asarray(geo["R"], np.float64) - z["R"]).max() <= 1e-6
    assert geo["flip"] == bool(z["flip"])
    assert geo["image_size"] == tuple(z["image_size"]) and geo["nearest_size"] == tuple(z["nearest_size"])
    assert geo["mats"].shape == (39,) and geo["mats"].dtype == np.float32


def test_knife_edge_pixels_stay_under_the_cap(case):
    _, z, inst, cfg, ref = case
    shape = (inst["height"], inst["width"])
    knife = knife_map(inst, ref["geometry"])
    assert (knife == _bits(z, "knife", shape)).all()
    assert knife.mean() <= 0.01


def test_numpy_references_reproduce_the_reference(case):
    _, z, inst, cfg, ref = case
    shape = (inst["height"], inst["width"])
    keep = ~_bits(z, "knife", shape)
    assert np.abs(ref["image_u8"].astype(int) - z["image"].astype(int)).max() <= 1
    assert ref["invalid"] == bool(z["invalid"])
    assert abs(float(ref["max_depth"]) - float(z["max_depth"])) <= REL * abs(float(z["max_depth"]))
    for key in ("depth_mask_fin", "depth_mask_inf", "bilinear"):
        assert (ref[key] == _bits(z, key, shape))[keep].all(), key
    d, g = ref["depth"][keep], z["depth"][keep]
    assert (np.isnan(d) == np.isnan(g)).all() and (np.isposinf(d) == np.isposinf(g)).all()
    fin = np.isfinite(g) & (g != 0)
    assert (d[g == 0] == 0).all()
    err = np.abs(d[fin] - g[fin]) / np.abs(g[fin])
    print("depth rel", err.max() if err.size else 0.0)
    assert err.size == 0 or err.max() <= REL
    n, gn = ref["normal"][keep], z["normal"][keep]
    assert (np.isnan(n) == np.isnan(gn)).all()
    nerr = np.abs(n - gn)[~np.isnan(gn)]
    print("normal abs", nerr.max() if nerr.size else 0.0)
    assert nerr.size == 0 or nerr.max() <= ABS


def test_normal_sign_and_threshold():
    K = np.array([[0.9, 0, 0.5], [0, 1.2, 0.5], [0, 0, 1]], np.float32)
    normal, mask = R.normal_map(np.full((7, 9), 2.0, np.float32), K)
    assert mask.all() and np.abs(normal - np.array([0, 0, -1], np.float32)).max() < 1e-6            # fronto-parallel: camera-facing, -z
    depth = np.full((7, 9), 2.0, np.float32)
    depth[:, 5:] = 40.0                                                 # a step with faces beyond 88 degrees from the viewing ray: they do not count
    normal, mask, angles = R.normal_map(depth, K, return_angles=True)
    every, _ = R.normal_map(depth, K, edge_threshold=180.0)
    steep = (angles > 88).any(-1)
    assert mask.all() and steep.any() and not steep.all()
    assert (np.abs(normal - every).max(-1) > 1e-3)[steep].all() and (normal == every)[~steep].all()
    lone = np.full((5, 5), np.nan, np.float32)
    lone[2, 2] = 1.0
    normal, mask = R.normal_map(lone, K)
    assert not mask.any() and np.isnan(normal).all()


def test_depth_edge_rule():
    depth = np.full((9, 11), 2.0, np.float32)
    depth[:, 6:] = np.float32(2.0 * np.exp(0.02))
    depth[0, 0], depth[8, 10] = np.nan, np.inf
    eligible, known, spread = R.depth_edge(depth, 5, 0.01, return_spread=True)
    assert eligible[0, 0] == 0 and eligible[8, 10] == 0 and known[0, 0] == 0 and known[8, 10] == 1
    assert (eligible[1:8, 4:8] == 0).all() and (eligible[:, :4] == np.isfinite(depth[:, :4])).all() and (eligible[:8, 8:] == 1).all()
    assert abs(np.nanmax(spread) - 0.02) < 1e-6


def test_all_ones_bilinear_is_exactly_one():
    rng = np.random.default_rng(0)
    ones = np.ones((23, 31), np.float32)
    for _ in range(5):
        M = np.eye(3) + rng.uniform(-0.2, 0.2, (3, 3)) * np.array([[1, 1, 8], [1, 1, 8], [1e-3, 1e-3, 0]])
        sx, sy = R.source_coords(np.linalg.inv(M).astype(np.float32), 40, 50)
        out = R.sample_bilinear(ones, sx, sy)
        interior = (sx >= 0) & (sx <= 30) & (sy >= 0) & (sy <= 22)
        assert interior.sum() > 200 and (out[interior] == np.float32(1)).all()
        assert (out[(sx < -1) | (sy < -1) | (sx > 31) | (sy > 23)] == 0).all()
    f = rng.uniform(0, 1, 200000).astype(np.float32)
    assert ((np.float32(1) - f) + f == np.float32(1)).all()


def test_lanczos4_weights():
    t = np.linspace(0, 1, 257, dtype=np.float32)[:-1]
    w = R.lanczos4_weights(t)
    assert w.dtype == np.float32 and (w[0] == np.eye(8, dtype=np.float32)[3]).all()
    assert np.abs(w.sum(-1) - 1).max() < 1e-6
    assert np.abs(w[1:] - w[1:][::-1, ::-1]).max() < 1e-6                                  # w(t)[i] = w(1 - t)[7 - i]
    x = np.float64(t[64]) + 3 - np.arange(8)                                               # the closed form sinc(x) sinc(x / 4), normalised
    closed = np.sinc(x) * np.sinc(x / 4)
    assert np.abs(w[64] - closed / closed.sum()).max() < 1e-6


def test_nearest_rounds_half_to_even():
    src = np.arange(1, 7, dtype=np.float32).reshape(1, 6)
    sx = np.array([[-0.5, 0.5, 1.5, 2.5, 4.5, 5.5, 5.4999]], np.float32)
    out = R.sample_nearest(src, sx, np.zeros_like(sx))
    assert out.tolist() == [[1, 1, 3, 3, 5, 0, 6]]              # -0.5 -> -0 (inside), 5.5 -> 6 (outside)


@pytest.mark.parametrize("n", [1000, 3000, 131072 + 17])
def test_fallback_boundary_is_the_float64_division(n):
    for count in (n // 1000 - 1, n // 1000, n // 1000 + 1, -(-n // 1000)):
        depth = np.full(n, np.nan, np.float32)
        depth[:max(count, 0)] = 2.0
        out = R.finish(depth, max(count, 0), None, 1000.0, False)
        assert out[3] == bool(np.isfinite(depth).sum() / depth.size < 0.001)


# ---------------------------------------------------------------------------------------------------------------------------------------
# the loader's host logic
# ---------------------------------------------------------------------------------------------------------------------------------------
def _write_dataset(root, name, n, size=(40, 32)):
    d = root / name
    d.mkdir()
    names = []
    rng = np.random.default_rng(len(name))
    for i in range(n):
        s = d / f"s{i}"
        s.mkdir()
        Image.fromarray(rng.integers(0, 255, (size[1], size[0], 3), dtype=np.uint8)).save(s / "image.jpg")
        E.write_depth(s / "depth.png", rng.uniform(1, 4, (size[1], size[0])).astype(np.float32))
        (s / "meta.json").write_text(json.dumps({"intrinsics": [[0.9, 0, 0.5], [0, 1.2, 0.5], [0, 0, 1]]}))
        names.append(f"s{i}")
    (d / ".index.txt").write_text("\n".join(names))
    return str(d)


@pytest.fixture()
def folders(tmp_path):
    a, b = _write_dataset(tmp_path, "alpha", 3), _write_dataset(tmp_path, "beta", 2)
    return {"clamp_max_depth": 1000.0, "fov_range_absolute": [1, 179], "fov_range_relative": [0.6, 0.97], "center_augmentation": 0.5,
            "aspect_ratio_range": [0.5, 2.0], "area_range": [600, 1200],
            "datasets": [{"name": "alpha", "path": a, "weight": 3.0, "label_type": "lidar", "depth_unit": 0.001, "aspect_ratio_range": [1.0, 1.2],
                          "center_augmentation": 0.0, "finite_depth_mask": "only_known"},
                         {"name": "beta", "path": b, "weight": 1.0, "label_type": "synthetic"}]}


def test_loader_size_strategies_and_sampling_order(folders):
    loader = T.TrainDataLoader(folders, batch_size=4, device="cpu")
    assert loader.image_size_strategy == "aspect_area"
    random.seed(5)
    batch = loader.sample_batch()
    random.seed(5)                                          # the reference's calls, in its order
    expect = []
    for _ in range(4):
        name = random.choices(["alpha", "beta"], weights=[3.0, 1.0])[0]
        expect.append((name, random.choice(loader.datasets[name]["filenames"]), random.randint(0, 2 ** 32 - 1)))
    area = random.uniform(600, 1200)
    ranges = [[1.0, 1.2] if e[0] == "alpha" else [0.5, 2.0] for e in expect]                        # the per-dataset override
    aspect = random.uniform(min(r[0] for r in ranges), max(r[1] for r in ranges))
    assert [(i["dataset"], i["filename"], i["seed"]) for i in batch] == expect
    assert {(i["width"], i["height"]) for i in batch} == {(int((area * aspect) ** 0.5), int((area / aspect) ** 0.5))}
    assert [i["label_type"] for i in batch] == ["lidar" if e[0] == "alpha" else "synthetic" for e in expect] and batch[0]["batch_id"] == 1

    fixed = dict(folders, image_sizes=[[48, 36], [32, 32]])
    loader = T.TrainDataLoader(fixed, batch_size=2, device="cpu")
    assert loader.image_size_strategy == "fixed"
    assert {(i["width"], i["height"]) for _ in range(20) for i in loader.sample_batch()} == {(48, 36), (32, 32)}
    bad = {k: v for k, v in folders.items() if k != "area_range"}
    with pytest.raises(ValueError, match="Invalid image size configuration"):
        T.TrainDataLoader(bad, batch_size=2, device="cpu")


def test_loader_overrides_and_invalid_substitution(folders, capsys):
    loader = T.TrainDataLoader(folders, batch_size=2, device="cpu")
    inst = {"dataset": "alpha", "filename": "s0", "path": loader.datasets["alpha"]["path"] + "/s0", "label_type": "lidar"}
    assert loader._setting(inst, "center_augmentation", loader.center_augmentation) == 0.0 and loader._setting(inst, "depth_unit") == 0.001
    assert loader._setting(inst, "finite_depth_mask") == "only_known"
    other = dict(inst, dataset="beta")
    assert loader._setting(other, "center_augmentation", loader.center_augmentation) == 0.5 and loader._setting(other, "depth_unit") is None
    good = loader.load_instance(dict(inst))
    assert good["image"].shape == (32, 40, 3) and good["depth"].shape == (32, 40) and good["depth"].dtype == np.float32 and good["label_type"] == "lidar"
    assert good["intrinsics"].dtype == np.float32
    missing = loader.load_instance(dict(inst, filename="nope", path=loader.datasets["alpha"]["path"] + "/nope"))
    assert "Failed to load instance alpha/nope" in capsys.readouterr().out
    assert missing["label_type"] == "invalid" and missing["image"].shape == (256, 256, 3) and (missing["depth"] == 1).all()
    assert (missing["intrinsics"] == np.array([[1, 0, 0.5], [0, 1, 0.5], [0, 0, 1]], np.float32)).all()
    with pytest.raises(RuntimeError, match="outside"):
        loader.get()


def test_loader_color_augmentation_refuse_and_skip(folders):
    cfg = dict(folders, image_augmentation=["jittering", "dof"])
    cfg["datasets"] = [dict(cfg["datasets"][0], image_augmentation=["shot_noise"]), cfg["datasets"][1]]
    with pytest.raises(NotImplementedError, match=r"dof.*jittering.*shot_noise"):
        T.TrainDataLoader(cfg, batch_size=2, device="cpu")
    with pytest.warns(UserWarning, match="skipped") as rec:
        T.TrainDataLoader(cfg, batch_size=2, device="cpu", color_augmentation="skip")
    assert len(rec) == 1
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        T.TrainDataLoader(folders, batch_size=2, device="cpu")                 # nothing configured: nothing to refuse
    with pytest.raises(ValueError, match="color_augmentation"):
        T.TrainDataLoader(folders, batch_size=2, device="cpu", color_augmentation="apply")


def test_gpu_only_entry():
    import torch
    with pytest.raises(RuntimeError, match="GPU tensors only"):
        T.warp_train_sample(torch.zeros((4, 4, 3), dtype=torch.uint8), torch.ones((4, 4)), np.eye(3, dtype=np.float32), 4, 4, 0, center_augmentation=0.0,
                            fov_range_absolute=[1, 179], fov_range_relative=[0.5, 1.0], clamp_max_depth=1000.0)
