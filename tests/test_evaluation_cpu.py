"""CPU: the host side of moge_amd.evaluation (file formats, key_average, the 3 x 3 geometry against the reference's fixtures) and the
conventions the GPU kernels of csrc/evaldata.hip implement, restated in numpy: Pillow's fixed-point Lanczos and the radix-select quantile."""
import json
import math
import subprocess
import sys

import numpy as np
import pytest
from PIL import Image

from moge_amd import evaluation as E
from tests.eval_fixtures import CASES, build_instance, config, instance_digest, load, recipe
from tests.eval_reference import lanczos_np


# ---------------------------------------------------------------------------------------------------------------------------------------
# file formats
# ---------------------------------------------------------------------------------------------------------------------------------------
def test_depth_png_round_trip(tmp_path):
    rng = np.random.default_rng(0)
    depth = rng.uniform(0.5, 80.0, (37, 53)).astype(np.float32)
    depth[3, 4] = np.nan
    depth[10, 11] = np.inf
    E.write_depth(tmp_path / "depth.png", depth)
    back = E.read_depth(tmp_path / "depth.png")
    assert back.dtype == np.float32 and back.shape == depth.shape
    assert np.isnan(back[3, 4]) and np.isposinf(back[10, 11])
    fin = np.isfinite(depth)
    assert np.isfinite(back[fin]).all()
    assert np.max(np.abs(back[fin] / depth[fin] - 1)) < 1e-4          # 16-bit log code over a 160x range


def test_depth_png_unit_chunk(tmp_path):
    from PIL import PngImagePlugin
    code = np.array([[0, 1, 65534, 65535]], np.uint16)
    info = PngImagePlugin.PngInfo()
    info.add_text("near", "2.0")
    info.add_text("far", "8.0")
    info.add_text("unit", "0.5")
    Image.fromarray(code).save(tmp_path / "d.png", pnginfo=info)
    d = E.read_depth(tmp_path / "d.png")
    assert np.isnan(d[0, 0]) and np.isposinf(d[0, 3])
    assert d[0, 1] == np.float32(1.0) and abs(d[0, 2] - 4.0) < 1e-5


@pytest.mark.parametrize("dtype", [np.uint8, np.uint16])
def test_segmentation_png_round_trip(tmp_path, dtype):
    seg = (np.arange(40 * 30).reshape(30, 40) % (200 if dtype == np.uint8 else 60000)).astype(dtype)
    labels = {"wall": 3, "sky": 0, "chair": int(seg.max())}
    E.write_segmentation(tmp_path / "s.png", seg, labels)
    back, lab = E.read_segmentation(tmp_path / "s.png")
    assert back.dtype == dtype and np.array_equal(back, seg)
    assert lab == labels and list(lab) == list(labels)


# ---------------------------------------------------------------------------------------------------------------------------------------
# key_average
# ---------------------------------------------------------------------------------------------------------------------------------------
def test_key_average_nested_with_nan():
    a = {"b": {"rel": 1.0, "delta1": float("nan")}, "t": 2.0, "only_a": float("nan")}
    b = {"b": {"rel": 3.0, "delta1": 0.5}, "t": 4.0, "c": {"x": {"y": 7.0}}}
    out = E.key_average([a, b])
    assert list(out) == ["b", "c", "only_a", "t"]
    assert list(out["b"]) == ["delta1", "rel"]
    assert out["b"] == {"delta1": 0.5, "rel": 2.0}
    assert out["t"] == 3.0 and out["c"] == {"x": {"y": 7.0}}
    assert math.isnan(out["only_a"])
    assert E.key_average([]) == {}


# ---------------------------------------------------------------------------------------------------------------------------------------
# host geometry against the reference (fixtures of tools/make_eval_golden.py)
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CASES)
def test_fixture_inputs_rebuild(name):
    z = load(name)
    assert instance_digest(build_instance(recipe(z))) == str(z["digest"])


@pytest.mark.parametrize("name", CASES)
def test_host_geometry_matches_reference(name):
    z = load(name)
    inst = build_instance(recipe(z))
    geo = E.warp_geometry(inst["image"].shape[0], inst["image"].shape[1], inst["intrinsics"], inst["width"], inst["height"])
    assert tuple(geo["rescaled_size"]) == tuple(int(v) for v in z["rescaled_size"])
    assert geo["tgt_intrinsics"].dtype == np.float32 and np.array_equal(geo["tgt_intrinsics"], z["tgt_intrinsics"])
    assert np.array_equal(geo["transform"], z["transform"])


def test_off_centre_intrinsics_rotate_the_view():
    z = load("kitti")
    inst = build_instance(recipe(z))
    R = E.warp_geometry(inst["image"].shape[0], inst["image"].shape[1], inst["intrinsics"], inst["width"], inst["height"])["R"]
    assert not np.allclose(R, np.eye(3)) and np.allclose(R @ R.T, np.eye(3), atol=1e-6)


def test_select_segments_order_and_cuts():
    labels = {"a": 1, "sky": 2, "b": 3, "c": 4, "d": 5, "e": 6}
    counts = {1: 10, 2: 99, 3: 30, 4: 10, 5: 30}               # e absent
    # descending counts, stable on ties (b before d, a before c), sky dropped, then max_segments, then min_seg_area
    assert list(E.select_segments(labels, counts, max_segments=4, min_seg_area=10)) == ["b", "d", "a", "c"]
    assert list(E.select_segments(labels, counts, max_segments=3, min_seg_area=11)) == ["b", "d"]


# ---------------------------------------------------------------------------------------------------------------------------------------
# Lanczos: the fixed-point convention of csrc/evaldata.hip, restated (tests/eval_reference.py), against Pillow
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("src,dst", [((13, 17), (5, 7)), ((11, 9), (29, 31)), ((23, 7), (7, 23)), ((40, 33), (40, 11)), ((9, 50), (27, 50)),
                                     ((61, 45), (19, 14))])
def test_lanczos_convention_matches_pillow(src, dst):
    rng = np.random.default_rng(src[0] * 100 + dst[1])
    img = rng.integers(0, 256, src + (3,), dtype=np.uint8)
    img[:, ::3] = 255                                            # hard edges: the fixed-point sums overshoot and clip
    ref = np.array(Image.fromarray(img).resize((dst[1], dst[0]), Image.Resampling.LANCZOS))
    assert np.array_equal(lanczos_np(img, *dst), ref)


# ---------------------------------------------------------------------------------------------------------------------------------------
# quantile: the radix select of csrc/evaldata.hip, restated, against np.nanquantile
# ---------------------------------------------------------------------------------------------------------------------------------------
def _key(v):
    b = v.astype(np.float32).view(np.uint32)
    return np.where(b & 0x80000000, ~b, b | 0x80000000).astype(np.uint32)


def _unkey(k):
    k = np.uint32(k)
    return (np.uint32(k & 0x7FFFFFFF) if k & 0x80000000 else np.uint32(~k)).view(np.float32)


def radix_quantile(depth, mask, q=0.01):
    vals = depth[mask & ~np.isnan(depth)].astype(np.float32)
    n = vals.size
    if n == 0:
        return np.float32(np.nan)
    qf = np.float32(q)
    vi = np.float32(n - 1) * qf                        # numpy's 'linear' virtual index
    above = vi >= np.float32(n - 1)
    ranks = [n - 1, n - 1] if above else [int(np.floor(vi)), int(np.floor(vi)) + 1]
    keys = _key(vals)
    picked = []
    for rank in ranks:
        prefix = 0
        for p in range(4):
            shift = 24 - 8 * p
            sel = keys[(keys >> np.uint32(shift + 8)) == prefix] if p else keys
            hist = np.bincount((sel >> np.uint32(shift)) & 255, minlength=256)
            c = np.cumsum(hist)
            digit = int(np.searchsorted(c, rank, side="right"))
            rank -= int(c[digit - 1]) if digit else 0
            prefix = (prefix << 8) | digit
        picked.append(_unkey(prefix))
    a, b = picked
    prev = -1.0 if above else float(np.floor(vi))
    gamma = np.float32(float(vi) - prev)
    with np.errstate(invalid="ignore"):
        d = np.float32(b - a)
        return np.float32(b - d * (np.float32(1) - gamma)) if gamma >= np.float32(0.5) else np.float32(a + d * gamma)


def _same(a, b):
    return (np.isnan(a) and np.isnan(b)) or np.float32(a).tobytes() == np.float32(b).tobytes()


@pytest.mark.parametrize("case", ["ties", "n1", "n1_inf", "integer_index", "negative", "infs", "random", "empty", "denormal", "n3", "n1000"])
def test_radix_quantile_matches_numpy(case):
    rng = np.random.default_rng(len(case))
    if case == "ties":
        v = np.repeat(np.float32([1.5, 2.0, 2.0, 7.25]), [40, 30, 30, 5])
    elif case == "n1":
        v = np.float32([3.75])
    elif case == "n1_inf":
        v = np.float32([np.inf])
    elif case == "integer_index":                        # n = 101: q (n - 1) = 1 exactly in reals
        v = rng.uniform(1, 2, 101).astype(np.float32)
    elif case == "negative":
        v = rng.normal(0, 3, 777).astype(np.float32)
        v[::5] = -0.0
    elif case == "infs":
        v = np.concatenate([np.full(3, -np.inf), rng.uniform(1, 2, 50), np.full(4, np.inf)]).astype(np.float32)
    elif case == "denormal":
        v = np.float32([1e-45, 0.0, 2e-45, 1e-40] * 30)
    elif case in ("n3", "n1000"):                      # (n - 1) q and n q + (1 - q) - 1 round apart in fp32 at q = 0.01 / 0.999
        v = rng.lognormal(1, 1, int(case[1:])).astype(np.float32)
    elif case == "empty":
        v = np.float32([np.nan, np.nan])
    else:
        v = (rng.lognormal(1, 1, 12345)).astype(np.float32)
    mask = np.ones(v.shape, bool)
    if case == "random":
        mask = rng.random(v.shape) > 0.3
        v[rng.random(v.shape) > 0.9] = np.nan
    for q in (0.0, 0.01, 0.5, 0.999, 1.0):
        with np.errstate(all="ignore"), __import__("warnings").catch_warnings():
            __import__("warnings").simplefilter("ignore")
            ref = np.nanquantile(np.where(mask, v, np.nan), q)
        assert _same(radix_quantile(v, mask, q), ref), (q, radix_quantile(v, mask, q), ref)


# ---------------------------------------------------------------------------------------------------------------------------------------
# command
# ---------------------------------------------------------------------------------------------------------------------------------------
def test_cli_lists_eval_baseline():
    out = subprocess.run([sys.executable, "-m", "moge_amd.scripts.cli", "--help"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    assert "eval_baseline" in out.stdout


def test_eval_baseline_options():
    from click.testing import CliRunner
    from moge_amd.scripts.eval_baseline import main
    out = CliRunner().invoke(main, ["--help"])
    assert out.exit_code == 0
    for opt in ("--baseline", "--config", "--output", "--oracle", "--dump_pred", "--dump_gt"):
        assert opt in out.output


# ---------------------------------------------------------------------------------------------------------------------------------------
# the numpy restatement of remap / quantile cut / unproject (tests/eval_reference.py; what the GPU sweeps compare the kernels with) against
# the reference's stored results, fed the restated Lanczos (checked by sha256) and the reference's stored masked nearest depth and mask
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CASES)
def test_remap_reference_matches_fixture(name):
    import hashlib
    from tests import eval_reference as R
    z = load(name)
    inst = build_instance(recipe(z))
    cfg = config(z)
    geo = E.warp_geometry(inst["image"].shape[0], inst["image"].shape[1], inst["intrinsics"], inst["width"], inst["height"])
    h, w = geo["rescaled_size"]
    OH, OW = inst["height"], inst["width"]
    rescaled = lanczos_np(inst["image"], h, w)
    assert hashlib.sha256(np.ascontiguousarray(rescaled).tobytes()).hexdigest() == str(z["lanczos_sha256"])
    mnr_depth = z["mnr_depth"]
    mnr_mask = np.unpackbits(z["mnr_mask"])[: h * w].reshape(h, w)
    dist = R.distance_ref(mnr_depth, inst["intrinsics"])
    kinv = np.asarray(geo["tgt_intrinsics_inv"], np.float32)
    out = R.remap_ref(rescaled, dist, mnr_mask, None, np.asarray(geo["transform"], np.float32), kinv, OH, OW)

    diff = np.abs(out["image"][::2].astype(np.int16) - z["image_rows"].astype(np.int16))
    assert diff.max() <= 1 and diff.any(axis=-1).mean() <= 1e-3, (diff.max(), diff.any(axis=-1).mean())

    md, mask, depth, count = R.quantile_cut_ref(out["depth"], out["mask"], 0.01, cfg["drop_max_depth"], cfg["depth_unit"])
    assert R.same_bits(md, z["max_depth"]), (md, z["max_depth"])
    mask, depth = mask.reshape(OH, OW), depth.reshape(OH, OW)
    knife = np.unpackbits(z["knife"])[: OH * OW].reshape(OH, OW).astype(bool)
    ref_mask = np.unpackbits(z["depth_mask"])[: OH * OW].reshape(OH, OW).astype(bool)
    depth, mask, pts = R.unproject_ref(depth, mask, kinv, count)
    assert np.array_equal(mask[~knife], ref_mask[~knife]), int((mask != ref_mask)[~knife].sum())
    sel = ~knife[::6]
    ref = z["depth_rows"]
    assert np.all(np.abs(depth[::6][sel] - ref[sel]) <= 1e-6 * np.maximum(np.abs(ref[sel]), 1e-30))
    sel = ~knife[::6, ::6]
    rp = z["points_sub"]
    assert np.all(np.abs(pts[::6, ::6][sel] - rp[sel]) <= 1e-6 * np.maximum(np.abs(rp[sel]), 1e-30))
    assert (str(z["label_type"]) == "invalid") == (count == 0)
