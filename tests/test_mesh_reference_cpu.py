"""CPU: the loop restatement of tests/mesh_reference.py equals `moge_amd.io.build_mesh_from_map` and `moge_amd.io.masked_point_cloud` - integers
exactly, floats bit for bit - on every shape and mask tests/test_hip_mesh.py uses.  It passes without moge_amd.mesh: it exists so the yardstick of
the GPU module does not rest on one implementation.  (The two 256-workgroup shapes run with one map and tri=True only: their Python loops are
the slow part of this module.)"""
import numpy as np
import pytest

import mesh_reference as MR
from moge_amd import io as IO


def scene(H, W, seed=0):
    rng = np.random.default_rng(seed + 31 * H + W)
    points = rng.standard_normal((H, W, 3)).astype(np.float32)
    image = rng.integers(0, 256, size=(H, W, 3), dtype=np.uint8)
    normal = rng.standard_normal((H, W, 3)).astype(np.float32)
    plane = rng.standard_normal((H, W)).astype(np.float32)
    return points, image, normal, plane


def same(got, want):
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert g.shape == w.shape and g.dtype == w.dtype, (g.shape, w.shape, g.dtype, w.dtype)
        assert np.array_equal(g if g.dtype != np.float32 else MR.bits(g), w if w.dtype != np.float32 else MR.bits(w))


@pytest.mark.parametrize("shape", MR.SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_loop_mesh_equals_the_host_function(shape):
    H, W = shape
    points, image, normal, plane = scene(H, W)
    big = shape in MR.SPAN_SHAPES
    maps = [points] if big else [points, image.astype(np.float32) / 255, IO.uv_map(H, W), normal, plane]
    for name, mask in MR.masks(H, W).items():
        for tri in ((True,) if big else (True, False)):
            want = IO.build_mesh_from_map(*maps, mask=mask, tri=tri)
            got = MR.image_mesh(maps, mask=mask, tri=tri)
            assert got[0].dtype == np.int32 and got[0].shape[1] == (3 if tri else 4), name
            same(got, want)
            if name == "checkerboard" or name == "all_false" or min(H, W) == 1:
                assert got[0].shape[0] == 0 and got[1].shape[0] == 0, name


@pytest.mark.parametrize("shape", MR.SMALL_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_loop_point_cloud_equals_the_host_function(shape):
    H, W = shape
    points, image, normal, _ = scene(H, W, seed=1)
    for name, mask in MR.masks(H, W).items():
        if mask is None:
            continue
        for img, nrm in ((image, normal), (None, None), (image.astype(np.float32) / 255, None)):
            want = IO.masked_point_cloud(points, mask, img, nrm)
            got = MR.point_cloud(points, mask, img, nrm)
            for g, w in zip(got, want):
                assert (g is None) == (w is None), name
                if g is not None:
                    same([g], [w])
        if name == "checkerboard":
            assert got[0].shape[0] == (H * W + 1) // 2            # every other pixel is a point although the mesh is empty


def test_masks_cover_the_cases_by_construction():
    m = MR.masks(70, 67)
    assert set(m) == {"none", "all_true", "all_false", "checkerboard", "island_tl", "island_tr", "island_bl", "island_br", "island_on_block_boundary",
                      "alternate_rows", "random_0.5", "random_0.97", "one_false_pixel"}
    isl = np.flatnonzero(m["island_on_block_boundary"].reshape(-1))
    assert isl[0] == MR.BLOCK_PX - 1 and isl[1] == MR.BLOCK_PX and isl.size == 4
    assert "island_on_block_boundary" not in MR.masks(3, 5) and "island_on_block_boundary" in MR.masks(5, 52429)
    assert (~m["one_false_pixel"]).sum() == 1 and m["island_br"][-2:, -2:].all() and m["island_br"].sum() == 4
