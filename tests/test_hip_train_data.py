"""GPU: moge_amd.train_data.warp_train_sample against the fixtures of the reference's `_process_instance` (tests/golden/train_*.npz), and a
TrainDataLoader batch against the per-instance outputs.  Gates: image within 1 LSB; masks, the invalid flag and the
branch choice equal outside the fixture's knife-edge pixels; depth and max_depth within 1e-6 relative, normals within 1e-6 absolute."""
import json
import random

import numpy as np
import pytest
import torch
from PIL import Image

from moge_amd import evaluation as E
from moge_amd import train_data as T
from tests import train_data_reference as R
from tests.train_data_fixtures import CASES, build_instance, config, instance_digest, knife_map, load, recipe, warp_kwargs

pytestmark = pytest.mark.gpu
REL, ABS = 1e-6, 1e-6


@pytest.fixture(scope="module", autouse=True)
def _needs_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


def _bits(z, key, shape):
    return np.unpackbits(z[key])[:shape[0] * shape[1]].reshape(shape).astype(bool)


def _warp(inst, cfg, **extra):
    return T.warp_train_sample(torch.from_numpy(inst["image"]).cuda(), torch.from_numpy(inst["depth"]).cuda(), inst["intrinsics"], inst["width"], inst["height"],
                               inst["seed"], **warp_kwargs(cfg), **extra)


def _compare(got, want, keep, tag):
    """got: numpy views of a warp; want: dict with image (h, w, 3) u8, depth, normal, depth_mask_fin / _inf, bilinear, invalid, max_depth"""
    lsb = np.abs(got["image_u8"].astype(int) - want["image"].astype(int)).max()
    d, g = got["depth"][keep], want["depth"][keep]
    fin = np.isfinite(g) & (g != 0)
    assert (d[g == 0] == 0).all()
    rel = (np.abs(d[fin] - g[fin]) / np.abs(g[fin])).max() if fin.any() else 0.0
    n, gn = got["normal"][keep], want["normal"][keep]
    nerr = np.abs(n - gn)[~np.isnan(gn)]
    nerr = nerr.max() if nerr.size else 0.0
    md = abs(float(got["max_depth"]) - float(want["max_depth"])) / abs(float(want["max_depth"]))
    print(f"{tag}: image lsb {lsb}, depth rel {rel:.3g}, normal abs {nerr:.3g}, max_depth rel {md:.3g}, excluded {(~keep).sum()}")
    assert lsb <= 1
    assert (got["image"] == (got["image_u8"].astype(np.float32) / np.float32(255)).transpose(2, 0, 1)).all()
    assert bool(got["invalid"]) == bool(want["invalid"])
    for key in ("depth_mask_fin", "depth_mask_inf", "bilinear"):
        assert (got[key] == want[key])[keep].all(), key
    assert (np.isnan(d) == np.isnan(g)).all() and (np.isposinf(d) == np.isposinf(g)).all()
    assert (np.isnan(n) == np.isnan(gn)).all()
    assert rel <= REL and nerr <= ABS and md <= REL


def _host(res):
    keys = ("image", "image_u8", "depth", "depth_mask_fin", "depth_mask_inf", "normal", "bilinear", "invalid", "max_depth", "count")
    out = {k: res[k].cpu().numpy() for k in keys}
    out["invalid"], out["max_depth"], out["count"] = int(out["invalid"][0]), out["max_depth"][0], int(out["count"][0])
    return out


@pytest.mark.parametrize("name", CASES)
def test_warp_matches_the_reference_fixture(name):
    z = load(name)
    inst = build_instance(recipe(z))
    assert instance_digest(inst) == str(z["digest"])
    cfg = config(z)
    res = _warp(inst, cfg)
    geo = res["geometry"]
    assert np.abs(geo["tgt_intrinsics"] - z["tgt_intrinsics"]).max() <= 1e-6 and geo["flip"] == bool(z["flip"])
    assert geo["image_size"] == tuple(z["image_size"]) and geo["nearest_size"] == tuple(z["nearest_size"])
    assert tuple(res["resized_image"].shape[:2]) == geo["image_size"] and tuple(res["nearest_depth"].shape) == geo["nearest_size"]
    shape = (inst["height"], inst["width"])
    want = {"image": z["image"], "depth": z["depth"], "normal": z["normal"], "invalid": z["invalid"], "max_depth": z["max_depth"],
            **{k: _bits(z, k, shape) for k in ("depth_mask_fin", "depth_mask_inf", "bilinear")}}
    got = _host(res)
    _compare(got, want, ~_bits(z, "knife", shape), name)
    assert (got["count"] == 0) == (name == "allnan") and res["depth_mask_fin"].dtype == torch.bool and res["image"].shape == (3,) + shape
    # a second run gives the same bits (integer atomics only)
    again = _host(_warp(inst, cfg))
    for k in ("image_u8", "depth", "normal", "depth_mask_fin", "depth_mask_inf"):
        assert np.array_equal(got[k], again[k], equal_nan=True), k
    assert got["count"] == again["count"] and np.float32(got["max_depth"]).tobytes() == np.float32(again["max_depth"]).tobytes()


def test_warp_writes_only_its_slot_and_follows_the_stream():
    z = load("holes")
    inst, cfg = build_instance(recipe(z)), config(z)
    alone = _host(_warp(inst, cfg))
    out = T.allocate_batch(3, inst["height"], inst["width"], "cuda")
    for v in out.values():
        v.view(torch.uint8).fill_(7)
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        res = _warp(inst, cfg, out=out, slot=1)
    stream.synchronize()
    got = _host(res)
    for k in ("image", "image_u8", "depth", "normal", "depth_mask_fin", "depth_mask_inf", "bilinear"):
        assert np.array_equal(got[k], alone[k], equal_nan=True), k
        assert res[k].data_ptr() == out[k][1].data_ptr()
        assert (out[k][0].view(torch.uint8) == 7).all() and (out[k][2].view(torch.uint8) == 7).all(), k
    assert got["count"] == alone["count"] and int(out["count"][1]) == alone["count"]
    with pytest.raises(ValueError, match="does not fit"):
        _warp(inst, cfg, out=out, slot=3)


def _write_instance(folder, inst):
    folder.mkdir()
    Image.fromarray(inst["image"]).save(folder / "image.jpg", quality=95)
    depth = inst["depth"]
    if np.isnan(depth).all():                       # write_depth needs one finite value for its range; code 0 is NaN
        Image.fromarray(np.zeros(depth.shape, np.uint16)).save(folder / "depth.png", pnginfo=_range_info())
    else:
        E.write_depth(folder / "depth.png", depth)
    (folder / "meta.json").write_text(json.dumps({"intrinsics": inst["intrinsics"].tolist()}))


def _range_info():
    from PIL import PngImagePlugin
    info = PngImagePlugin.PngInfo()
    info.add_text("near", "1.0")
    info.add_text("far", "2.0")
    return info


def test_loader_collates_the_per_instance_outputs(tmp_path):
    names = ["holes", "flip_yes", "allnan"]
    root = tmp_path / "set"
    root.mkdir()
    for n in names:
        _write_instance(root / n, build_instance(recipe(load(n))))
    (root / ".index.txt").write_text("\n".join(names + ["missing"]))
    cfg = {"clamp_max_depth": 1000.0, "fov_range_absolute": [1, 179], "fov_range_relative": [0.6, 0.97], "center_augmentation": 0.5,
           "image_sizes": [[40, 30]], "datasets": [{"name": "set", "path": str(root), "weight": 1.0, "label_type": "synthetic", "depth_unit": 0.5,
                                                    "finite_depth_mask": "only_known"}]}
    random.seed(1)
    expect = T.TrainDataLoader(cfg, batch_size=8, device="cuda").sample_batch()
    assert {i["filename"] for i in expect} == set(names + ["missing"])            # this seed draws every entry at least once
    random.seed(1)
    with T.TrainDataLoader(cfg, batch_size=8, num_load_workers=2, buffer_size=1) as loader:
        batch = loader.get()
    assert sorted(batch) == sorted(["label_type", "is_metric", "info", "image", "depth", "depth_mask_fin", "depth_mask_inf", "normal", "intrinsics"])
    assert batch["image"].shape == (8, 3, 30, 40) and batch["image"].dtype == torch.float32 and batch["image"].is_cuda
    assert batch["depth"].shape == (8, 30, 40) and batch["depth"].dtype == torch.float32 and batch["normal"].shape == (8, 30, 40, 3)
    assert batch["depth_mask_fin"].dtype == batch["depth_mask_inf"].dtype == torch.bool and batch["intrinsics"].shape == (8, 3, 3)
    assert batch["info"] == [{"dataset": "set", "filename": i["filename"]} for i in expect] and batch["is_metric"] == [True] * 8
    assert batch["label_type"] == ["invalid" if i["filename"] in ("allnan", "missing") else "synthetic" for i in expect]
    done = set()
    for b, inst in enumerate(expect):
        if inst["filename"] in done:
            continue
        done.add(inst["filename"])
        if inst["filename"] == "missing":
            image, depth, K = np.zeros((256, 256, 3), np.uint8), np.ones((256, 256), np.float32), np.array([[1, 0, 0.5], [0, 1, 0.5], [0, 0, 1]], np.float32)
        else:
            d = root / inst["filename"]
            image, depth, K = E.read_image(d / "image.jpg"), E.read_depth(d / "depth.png"), np.array(E.read_meta(d / "meta.json")["intrinsics"], np.float32)
        kw = dict(center_augmentation=0.5, fov_range_absolute=[1, 179], fov_range_relative=[0.6, 0.97], clamp_max_depth=1000.0, depth_unit=0.5,
                  finite_depth_mask="only_known")
        one = _host(T.warp_train_sample(torch.from_numpy(image).cuda(), torch.from_numpy(depth).cuda(), K, 40, 30, inst["seed"], **kw))
        for k in ("image", "depth", "normal", "depth_mask_fin", "depth_mask_inf"):
            assert np.array_equal(batch[k][b].cpu().numpy(), one[k], equal_nan=True), (inst["filename"], k)
        ref = R.warp_train_sample(image, depth, K, 40, 30, inst["seed"], **kw)
        assert np.abs(batch["intrinsics"][b].cpu().numpy() - ref["geometry"]["tgt_intrinsics"]).max() == 0
        assert ref["invalid"] == (inst["filename"] == "allnan")                # `missing` is invalid by its load failure, not by the fallback
        knife = knife_map({"depth": depth, "intrinsics": K, "height": 30, "width": 40}, ref["geometry"])
        assert knife.mean() <= 0.01
        want = dict(ref, image=ref["image_u8"])
        _compare(one, want, ~knife, inst["filename"])
