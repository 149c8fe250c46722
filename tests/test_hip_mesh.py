"""moge_amd.mesh (csrc/mesh.hip) against the host functions it mirrors, `moge_amd.io.build_mesh_from_map` and `masked_point_cloud`, bit for bit:
integers with array_equal, floats through their int32 bit patterns (in the export-transform test only, NaNs compare equal as NaN: a NaN
times -1 need not keep its sign bit the same way on both machines).  There is no tolerance anywhere in this module.  On the small shapes the
loop restatement of tests/mesh_reference.py (tied to the host functions by tests/test_mesh_reference_cpu.py) is checked as well.

Shapes and masks are those of tests/mesh_reference.py: they sit on the scan's constants, moge_amd.mesh.BLOCK_PX = 1024 pixels per workgroup
(one under, on, over; as long rows and as a near-square) and SCAN_SPAN = 256 workgroup totals per second-level workgroup (256 and 257
workgroups), plus the degenerate 1 x 7 / 7 x 1 / 2 x 2."""
import ctypes as C

import numpy as np
import pytest
import torch

import mesh_reference as MR
from moge_amd import io as IO

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def M():
    import moge_amd.mesh as mesh
    assert (mesh.BLOCK_PX, mesh.SCAN_SPAN) == (MR.BLOCK_PX, MR.SCAN_SPAN)
    return mesh


def scene(H, W, seed=0):
    rng = np.random.default_rng(seed + 31 * H + W)
    return {"points": rng.standard_normal((H, W, 3)).astype(np.float32), "image": rng.integers(0, 256, size=(H, W, 3), dtype=np.uint8),
            "normal": rng.standard_normal((H, W, 3)).astype(np.float32), "plane": rng.standard_normal((H, W)).astype(np.float32)}


def cuda(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def same(got, want, what, nan_equal=False):
    """got: tensors / arrays from the device form, want: numpy arrays of the host form."""
    assert len(got) == len(want), what
    for k, (g, w) in enumerate(zip(got, want)):
        g = g.cpu().numpy() if torch.is_tensor(g) else g
        assert g.shape == w.shape and g.dtype == w.dtype, (what, k, g.shape, w.shape, g.dtype, w.dtype)
        if g.dtype == np.float32:
            if nan_equal:
                nan = np.isnan(w)
                assert np.array_equal(np.isnan(g), nan), (what, k)
                g, w = np.where(nan, np.float32(0), g), np.where(nan, np.float32(0), w)
            g, w = MR.bits(g), MR.bits(w)
        assert np.array_equal(g, w), (what, k, int((g != w).sum()))


@pytest.mark.parametrize("shape", MR.SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_mesh_equals_the_host_function(M, shape):
    """Every mask, tri and quads; maps: points (C = 3), the uint8 image, the generated uv and a 2-D map."""
    H, W = shape
    s = scene(H, W)
    host_maps = [s["points"], s["image"].astype(np.float32) / 255, IO.uv_map(H, W), s["plane"]]
    dev_maps = [cuda(s["points"]), cuda(s["image"]), M.UV, cuda(s["plane"])]
    for name, mask in MR.masks(H, W).items():
        for tri in (True, False):
            want = IO.build_mesh_from_map(*host_maps, mask=mask, tri=tri)
            got = M.build_mesh_from_map(*dev_maps, mask=cuda(mask), tri=tri)
            assert all(t.is_cuda for t in got) and got[0].dtype == torch.int32
            same(got, want, (shape, name, tri))
        if shape in MR.SMALL_SHAPES:
            same(got, MR.image_mesh(host_maps, mask=mask, tri=False), (shape, name, "loops"))


@pytest.mark.parametrize("shape", [(3, 5), (31, 33), (70, 67)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_channel_counts_dtypes_and_views(M, shape):
    H, W = shape
    rng = np.random.default_rng(3)
    mask = rng.random((H, W)) < 0.9
    maps = [rng.standard_normal((H, W, c)).astype(np.float32) for c in (1, 2, 3, 4)] + [rng.standard_normal((H, W)).astype(np.float32)]
    u8 = rng.integers(0, 256, size=(H, W, 3), dtype=np.uint8)
    want = IO.build_mesh_from_map(*maps, u8.astype(np.float32) / 255, IO.uv_map(H, W), mask=mask)
    got = M.build_mesh_from_map(*[cuda(m) for m in maps], cuda(u8), cuda(IO.uv_map(H, W)), mask=cuda(mask))        # uv as one more map
    same(got, want, shape)
    assert [tuple(g.shape[1:]) for g in got[1:]] == [(1,), (2,), (3,), (4,), (1,), (3,), (2,)]
    # non-contiguous views: a channel slice, a strided column slice of a wider map, a transposed mask
    wide = rng.standard_normal((H, 2 * W, 4)).astype(np.float32)
    t = cuda(wide)
    view, col = t[:, ::2, 1:4], t[:, ::2, 0]
    assert not view.is_contiguous() and not col.is_contiguous()
    mt = cuda(np.ascontiguousarray(mask.T)).T
    assert not mt.is_contiguous() or min(H, W) == 1
    same(M.build_mesh_from_map(view, col, mask=mt), IO.build_mesh_from_map(wide[:, ::2, 1:4], wide[:, ::2, 0], mask=mask), (shape, "views"))
    # every value of a uint8 map: x / 255 is the correctly rounded fp32 quotient
    ramp = np.arange(256, dtype=np.uint8).reshape(2, 128)
    f, c = M.build_mesh_from_map(cuda(ramp))
    assert np.array_equal(MR.bits(c.cpu().numpy().reshape(-1)), MR.bits(np.arange(256, dtype=np.float32) / np.float32(255)))


def test_special_values_pass_through_or_stay_out(M):
    H, W = 37, 45
    s = scene(H, W, seed=2)
    rng = np.random.default_rng(4)
    mask = rng.random((H, W)) < 0.8
    base = IO.build_mesh_from_map(s["points"], mask=mask)
    used = np.zeros(H * W, bool)                             # the used pixels, from the host result itself
    quad_ok = mask[:-1, :-1] & mask[:-1, 1:] & mask[1:, :-1] & mask[1:, 1:]
    for di in (0, 1):
        for dj in (0, 1):
            used.reshape(H, W)[di:H - 1 + di, dj:W - 1 + dj] |= quad_ok
    assert used.sum() == base[1].shape[0] and (mask.reshape(-1) & ~used).any()
    pts = s["points"].copy()
    flat = pts.reshape(-1, 3)
    junk = np.array([np.nan, np.inf, -np.inf], dtype=np.float32)
    flat[~used] = junk[rng.integers(0, 3, size=((~used).sum(), 3))]        # masked out, or masked in but in no quad: must not appear
    got = M.build_mesh_from_map(cuda(pts), mask=cuda(mask))
    same(got, base, "junk at unused pixels")
    assert np.isfinite(got[1].cpu().numpy()).all()
    # at used pixels every bit pattern survives: quiet and signalling NaNs with payloads, both infinities, -0.0, denormals
    patterns = np.array([0x7FC00000, 0xFFC00001, 0x7F800001, 0xFFA5A5A5, 0x7F800000, 0xFF800000, 0x80000000, 0x00000001, 0x807FFFFF], dtype=np.uint32)
    raw = pts.view(np.uint32).reshape(-1, 3).copy()
    rows = np.flatnonzero(used)[:: max(1, used.sum() // 40)]
    raw[rows] = patterns[rng.integers(0, len(patterns), size=(rows.size, 3))]
    special = raw.view(np.float32).reshape(H, W, 3)
    want = IO.build_mesh_from_map(special, mask=mask)
    got = M.build_mesh_from_map(cuda(special), mask=cuda(mask))
    same(got, want, "special values at used pixels")
    assert np.isnan(got[1].cpu().numpy()).any()


def test_batch_equals_each_image_alone_and_a_rerun(M):
    H, W = 70, 67
    all_masks = MR.masks(H, W)
    chosen = [all_masks["random_0.5"], all_masks["island_on_block_boundary"], all_masks["random_0.97"]]
    scenes = [scene(H, W, seed=k) for k in range(3)]
    pts = cuda(np.stack([s["points"] for s in scenes]))
    img = cuda(np.stack([s["image"] for s in scenes]))
    pl = cuda(np.stack([s["plane"] for s in scenes]))
    mk = cuda(np.stack(chosen))
    for tri in (True, False):
        batch = M.build_mesh_from_map(pts, img, M.UV, pl, mask=mk, tri=tri)
        again = M.build_mesh_from_map(pts, img, M.UV, pl, mask=mk, tri=tri)
        assert isinstance(batch, list) and len(batch) == 3
        for b in range(3):
            alone = M.build_mesh_from_map(pts[b], img[b], M.UV, pl[b], mask=mk[b], tri=tri)
            want = IO.build_mesh_from_map(scenes[b]["points"], scenes[b]["image"].astype(np.float32) / 255, IO.uv_map(H, W), scenes[b]["plane"], mask=chosen[b], tri=tri)
            same(batch[b], want, ("batch", b, tri))
            same(alone, want, ("alone", b, tri))
            for x, y in zip(batch[b], again[b]):
                assert torch.equal(x, y) if x.dtype == torch.int32 else torch.equal(x.view(torch.int32), y.view(torch.int32))
    # an empty image inside a batch, an all-empty batch, a batch without a mask
    mk2 = mk.clone(); mk2[1] = False
    mixed = M.build_mesh_from_map(pts, mask=mk2)
    assert mixed[1][0].shape == (0, 3) and mixed[1][1].shape == (0, 3)
    same(mixed[2], IO.build_mesh_from_map(scenes[2]["points"], mask=chosen[2]), "after an empty image")
    empty = M.build_mesh_from_map(pts, mask=torch.zeros_like(mk))
    assert all(f.shape == (0, 3) and v.shape == (0, 3) for f, v in empty)
    same(M.build_mesh_from_map(pts)[1], IO.build_mesh_from_map(scenes[1]["points"]), "4-D map without a mask")
    assert M.build_mesh_from_map(pts[:0], mask=mk[:0]) == []


@pytest.mark.parametrize("shape", [(1, 7), (3, 5), (2, 513), (31, 33), (70, 67), (5, 52429)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_masked_point_cloud_equals_the_host_function(M, shape):
    H, W = shape
    s = scene(H, W, seed=5)
    for name, mask in MR.masks(H, W).items():
        if mask is None:
            continue
        for img, nrm in ((s["image"], s["normal"]), (None, None), (s["image"].astype(np.float32) / 255, None)):
            want = IO.masked_point_cloud(s["points"], mask, img, nrm)
            got = M.masked_point_cloud(cuda(s["points"]), cuda(mask), cuda(img), cuda(nrm))
            assert [g is None for g in got] == [w is None for w in want], name
            same([g for g in got if g is not None], [w for w in want if w is not None], (shape, name))
        if name == "checkerboard":
            assert got[0].shape[0] == (H * W + 1) // 2 and M.build_mesh_from_map(cuda(s["points"]), mask=cuda(mask))[1].shape[0] == 0
    both = M.masked_point_cloud(cuda(np.stack([s["points"]] * 2)), cuda(np.stack([mask, ~mask])), cuda(np.stack([s["image"]] * 2)))
    same(both[1][:2], IO.masked_point_cloud(s["points"], ~mask, s["image"])[:2], "batched point cloud")


@pytest.mark.parametrize("shape", [(3, 5), (32, 32), (70, 67)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_export_mesh_equals_the_scripts_float64_expressions(M, shape):
    """scripts/infer.py: vertices * [1, -1, -1], vertex_uvs * [1, -1] + [0, 1], vertex_normals * [1, -1, -1] in float64 on the host, cast to '<f4'
    by the writers.  A few NaNs and -0.0 sit at used pixels."""
    H, W = shape
    s = scene(H, W, seed=6)
    mask = MR.masks(H, W)["random_0.97"]
    s["points"][1, 1] = [np.nan, -0.0, np.inf]
    s["normal"][H // 2, W // 2] = [-0.0, np.nan, 0.0]
    for normal in (s["normal"], None):
        for tri in (True, False):
            maps = [s["points"], s["image"].astype(np.float32) / 255, IO.uv_map(H, W)] + ([normal] if normal is not None else [])
            faces, v, c, uv, *rest = IO.build_mesh_from_map(*maps, mask=mask, tri=tri)
            with np.errstate(invalid="ignore"):
                want = [faces, (v * [1, -1, -1]).astype("<f4"), c, (uv * [1, -1] + [0, 1]).astype("<f4")] + [(r * [1, -1, -1]).astype("<f4") for r in rest]
            got = M.export_mesh(cuda(s["points"]), cuda(s["image"]), cuda(mask), cuda(normal), tri=tri)
            same(got, want, (shape, tri, normal is not None), nan_equal=True)
    batch = M.export_mesh(cuda(s["points"])[None], cuda(s["image"])[None], cuda(mask)[None], None, tri=False)
    assert isinstance(batch, list) and len(batch) == 1
    same(batch[0], want, "batched export", nan_equal=True)


def test_errors(M):
    H, W = 6, 9
    s = scene(H, W)
    p, m = cuda(s["points"]), cuda(np.ones((H, W), bool))
    with pytest.raises(RuntimeError):
        M.build_mesh_from_map(p.cpu(), mask=m.cpu())
    with pytest.raises(RuntimeError):
        M.build_mesh_from_map(p, mask=m.cpu())
    with pytest.raises(RuntimeError):
        M.masked_point_cloud(p.cpu(), m)
    with pytest.raises(RuntimeError):
        M.export_mesh(p, cuda(s["image"]).cpu(), m)
    for bad in (lambda: M.build_mesh_from_map(p, cuda(s["plane"])[:, :5], mask=m),                    # mismatched map
                lambda: M.build_mesh_from_map(p, mask=m[:5]),                                            # mismatched mask
                lambda: M.build_mesh_from_map(torch.zeros(H, W, 5, device="cuda"), mask=m),              # C > 4
                lambda: M.build_mesh_from_map(p.double(), mask=m),                                       # dtypes
                lambda: M.build_mesh_from_map(p.half(), mask=m),
                lambda: M.build_mesh_from_map(p, mask=m.float()),
                lambda: M.build_mesh_from_map(*[p] * 9, mask=m),                                         # more than 8 maps
                lambda: M.build_mesh_from_map(mask=m),
                lambda: M.build_mesh_from_map(p, "xy", mask=m),
                lambda: M.masked_point_cloud(p, None),
                lambda: M.export_mesh(p[..., :2], cuda(s["image"]), m)):
        with pytest.raises(ValueError):
            bad()


def test_fill_with_null_outputs_is_an_error_and_launches_nothing(M):
    from moge_amd import _lib as L
    H, W = 20, 26
    s = scene(H, W)
    pts, mask = cuda(s["points"]), cuda(MR.masks(H, W)["random_0.97"])
    ws = torch.empty(M.workspace_bytes(1, H, W), dtype=torch.uint8, device="cuda")
    counts = torch.empty((1, 2), dtype=torch.int32, device="cuda")
    offsets = torch.empty((1, 2), dtype=torch.int64, device="cuda")
    st = L.stream_ptr(pts.device)
    assert L.lib.moge_image_mesh_count(mask.view(torch.uint8).data_ptr(), 1, H, W, 0, ws.data_ptr(), counts.data_ptr(), offsets.data_ptr(), st) == 0
    V, Q = counts.cpu().tolist()[0]
    want = IO.build_mesh_from_map(s["points"], mask=mask.cpu().numpy())
    assert (V, 2 * Q) == (want[1].shape[0], want[0].shape[0]) and offsets.cpu().tolist() == [[0, 0]]
    out = torch.full((V, 3), -7.0, device="cuda")
    faces = torch.full((2 * Q, 3), -7, dtype=torch.int32, device="cuda")
    arr = (L.MeshMap * 1)()
    arr[0].data, arr[0].out, arr[0].channels, arr[0].dtype = pts.data_ptr(), None, 3, L.MESH_F32
    snapshot = ws.clone()
    assert L.lib.moge_image_mesh_fill(1, H, W, ws.data_ptr(), arr, 1, 1, faces.data_ptr(), offsets.data_ptr(), st) == -1 and b"null" in L.lib.moge_last_error()
    arr[0].out = out.data_ptr()
    assert L.lib.moge_image_mesh_fill(1, H, W, ws.data_ptr(), arr, 1, 1, None, offsets.data_ptr(), st) == -1 and b"null" in L.lib.moge_last_error()
    torch.cuda.synchronize()
    assert (out == -7).all() and (faces == -7).all() and torch.equal(ws, snapshot)           # neither outputs nor the index plane were touched
    assert L.lib.moge_image_mesh_fill(1, H, W, ws.data_ptr(), arr, 1, 1, faces.data_ptr(), offsets.data_ptr(), st) == 0
    same([faces, out], want, "the raw C calls")


def test_model_image_mesh(M, tmp_path):
    from moge_amd.model import import_model_class_by_version
    from oracle import moge_oracle as O
    cfg = O.named_configs()["tiny-vits-normal"]
    path = str(tmp_path / "model.pt")
    O.save_checkpoint(path, cfg, O.synth_state_dict(cfg, 0, True))
    model = import_model_class_by_version("v2").from_pretrained(path).to("cuda").eval()
    assert hasattr(import_model_class_by_version("v1"), "image_mesh")
    imgs = np.random.default_rng(5).integers(0, 256, size=(2, 70, 98, 3), dtype=np.uint8)
    out = model.infer_uint8(torch.from_numpy(imgs), num_tokens=108, use_fp16=False)
    rtol = 1e9               # the synthetic weights' depth is noise: the default threshold leaves no pixel, this one the pixels away from masked-out ones
    got = model.image_mesh(out, torch.from_numpy(imgs), rtol=rtol)
    clean = model.depth_edge_mask(out["depth"], out["mask"], rtol=rtol).cpu().numpy()
    assert len(got) == 2 and all(g[0].shape[0] > 1000 for g in got)
    for b in range(2):
        faces, v, c, uv, n = IO.build_mesh_from_map(out["points"][b].cpu().numpy(), imgs[b].astype(np.float32) / 255, IO.uv_map(70, 98),
                                                    out["normal"][b].cpu().numpy(), mask=clean[b])
        want = [faces, (v * [1, -1, -1]).astype("<f4"), c, (uv * [1, -1] + [0, 1]).astype("<f4"), (n * [1, -1, -1]).astype("<f4")]
        same(got[b], want, ("model", b), nan_equal=True)
    one = model.image_mesh({k: v[0] for k, v in out.items()}, torch.from_numpy(imgs[0]), rtol=rtol)
    same(one, [t.cpu().numpy() for t in got[0]], "unbatched", nan_equal=True)
    with pytest.raises(ValueError):
        model.image_mesh({"mask": out["mask"]}, torch.from_numpy(imgs))
