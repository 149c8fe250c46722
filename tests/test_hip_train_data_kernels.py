"""GPU: every kernel of csrc/traindata.hip against the plain numpy references of tests/train_data_reference.py, at the edges the fixtures of
tests/test_hip_train_data.py miss.  The tolerances are the fixtures': image within 1 LSB, depth relative and normal absolute 1e-6, decisions
equal outside pixels that sit on a decision boundary of the reference."""
import ctypes as C

import numpy as np
import pytest
import torch

from moge_amd import _lib as L
from moge_amd import evaluation as E
from moge_amd import train_data as T
from tests import train_data_reference as R

pytestmark = pytest.mark.gpu

STRIDE = 512 * 256                       # Q_BLOCKS x Q_THREADS: the grid stride of the finish passes
REL, ABS = 1e-6, 1e-6
K0 = np.array([[0.9, 0, 0.47], [0, 1.2, 0.52], [0, 0, 1]], np.float32)
# (H, W): a row, a column, widths and pixel counts that are no multiple of 64 or 256, and more than 131 072 pixels
SHAPES = [(1, 37), (41, 1), (2, 2), (33, 67), (64, 256), (301, 449)]


@pytest.fixture(scope="module", autouse=True)
def _needs_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _depth(shape, seed, kind="mixed"):
    """a smooth surface with a step, NaN and inf pixels at the corners, on the borders and inside"""
    H, W = shape
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:H, 0:W]
    d = (2 + 0.02 * np.sin(x / 7.0) + 0.01 * np.cos(y / 5.0) + 0.0005 * rng.standard_normal(shape)).astype(np.float32)
    d[:, W // 2:] *= np.float32(1.5)
    if kind == "mixed":
        holes = rng.uniform(size=shape)
        d[holes < 0.08] = np.nan
        d[holes > 0.95] = np.inf
        d[0, 0], d[-1, -1] = np.nan, np.inf
        d[0, -1], d[-1, 0] = 3.0, 2.5
    return d


# ---------------------------------------------------------------------------------------------------------------------------------------
# normal map and depth edge
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["mixed", "dense"])
@pytest.mark.parametrize("shape", SHAPES)
def test_normal_map(shape, kind):
    depth = _depth(shape, 1, kind)
    got = T.normal_map(_t(depth), K0).cpu().numpy()
    want, mask, angles = R.normal_map(depth, K0, 88.0, return_angles=True)
    with np.errstate(invalid="ignore"):
        keep = ~(np.abs(angles - 88.0) < 1e-3).any(-1)
    assert keep.mean() >= 0.99
    assert (np.isnan(got).all(-1) == ~mask)[keep].all() and (np.isnan(got).any(-1) == np.isnan(got).all(-1)).all()
    err = np.abs(got - want)[keep & mask]
    print(shape, kind, "normal abs", err.max() if err.size else 0.0, "valid", mask.mean())
    assert err.size == 0 or err.max() <= ABS
    if kind == "dense" and min(shape) > 2:
        assert mask.all()                                                  # corners and borders have one or two faces
    if min(shape) == 1:
        assert not mask.any()                                              # no face without two directions


def test_normal_map_isolated_pixel_plane_sign_and_threshold():
    lone = np.full((9, 11), np.nan, np.float32)
    lone[4, 5] = 2.0
    lone[0, 0], lone[0, 1], lone[1, 0] = 2.0, 2.0, 2.0                   # one face at the corner
    got = T.normal_map(_t(lone), K0).cpu().numpy()
    assert np.isnan(got[4, 5]).all() and np.abs(got[0, 0] - np.array([0, 0, -1])).max() < 1e-6
    want, mask = R.normal_map(lone, K0)
    assert (np.isnan(got).all(-1) == ~mask).all()
    plane = T.normal_map(_t(np.full((6, 7), 3.0, np.float32)), K0).cpu().numpy()
    assert np.abs(plane - np.array([0, 0, -1], np.float32)).max() < 1e-6           # camera-facing: -z for a fronto-parallel plane
    step = np.full((7, 9), 2.0, np.float32)
    step[:, 5:] = 40.0
    for thr in (88.0, 180.0):                                               # the threshold drops the faces across the step
        got = T.normal_map(_t(step), K0, edge_threshold=thr).cpu().numpy()
        want, _ = R.normal_map(step, K0, thr)
        assert np.abs(got - want).max() <= ABS
    assert np.abs(T.normal_map(_t(step), K0, 88.0).cpu().numpy() - T.normal_map(_t(step), K0, 180.0).cpu().numpy()).max() > 1e-3


@pytest.mark.parametrize("ksize", [1, 3, 5])
@pytest.mark.parametrize("shape", SHAPES)
def test_depth_edge(shape, ksize):
    depth = _depth(shape, 2)
    eligible, known = T.depth_edge(_t(depth), ksize, 0.01)
    want, wknown, spread = R.depth_edge(depth, ksize, 0.01, return_spread=True)
    with np.errstate(invalid="ignore"):
        keep = ~(np.abs(spread - np.float32(0.01)) < 1e-5)
    assert keep.mean() >= 0.99
    got = eligible.cpu().numpy()
    assert set(np.unique(got)) <= {0.0, 1.0} and (got == want)[keep].all() and (known.cpu().numpy() == wknown).all()
    assert (got[~np.isfinite(depth)] == 0).all()
    if ksize == 1:
        assert (got == np.isfinite(depth)).all()
    elif min(shape) > 8 and ksize == 5:
        assert 0.005 < (want[np.isfinite(depth)] == 0).mean() < 0.9         # both outcomes occur


def test_depth_edge_isolated_pixel_and_window_reach():
    lone = np.full((9, 11), np.nan, np.float32)
    lone[4, 5] = 2.0
    assert T.depth_edge(_t(lone))[0].cpu().numpy().sum() == 1               # alone in its window: never an edge
    pair = np.full((9, 11), 2.0, np.float32)
    pair[0, 0] = 2.5                                                        # reaches the pixels within two steps of the corner, no further
    got = T.depth_edge(_t(pair))[0].cpu().numpy()
    assert (got[:3, :3] == 0).all() and got[:3, 3:].all() and got[3:, :].all()


# ---------------------------------------------------------------------------------------------------------------------------------------
# warp
# ---------------------------------------------------------------------------------------------------------------------------------------
def _maps(shape, seed):
    H, W = shape
    rng = np.random.default_rng(seed)
    depth = _depth(shape, seed)
    normal, _ = R.normal_map(depth, K0)
    eligible, _ = R.depth_edge(depth)
    image = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    return image, depth, eligible, normal


def _mats(minv_img, minv_near, minv_raw, Rm=None, zr=(0.05, -0.03, 1.0)):
    Rm = np.eye(3) if Rm is None else Rm
    return np.concatenate([np.asarray(m, np.float32).ravel() for m in (minv_img, minv_near, minv_raw, Rm, zr)]).astype(np.float32)


def _run_warp(image, nearest, depth, eligible, normal, mats, oh, ow, flip):
    dev = "cuda"
    out = T.allocate_batch(1, oh, ow, dev)
    ti, tn, td, te, tm = _t(image), _t(nearest), _t(depth), _t(eligible), _t(normal)
    mats = np.ascontiguousarray(mats, np.float32)
    L.check(L.lib.moge_train_warp(_p(ti), image.shape[0], image.shape[1], _p(tn), nearest.shape[0], nearest.shape[1], _p(td), _p(te), _p(tm), depth.shape[0],
                                  depth.shape[1], oh, ow, C.c_void_p(mats.ctypes.data), flip, _p(out["image_u8"]), _p(out["image"]), _p(out["depth"]), _p(out["normal"]),
                                  _p(out["bilinear"]), _p(out["count"]), _stream()))
    return {k: out[k][0].cpu().numpy() for k in ("image_u8", "image", "depth", "normal", "bilinear")}, int(out["count"][0])


def _check_warp(got, count, want, tag):
    img, depth, nrm, branch, wcount = want
    lsb = np.abs(got["image_u8"].astype(int) - img.astype(int)).max()
    fin = np.isfinite(depth) & (depth != 0)
    assert (got["depth"][depth == 0] == 0).all()                            # target pixels outside every source
    rel = (np.abs(got["depth"][fin] - depth[fin]) / np.abs(depth[fin])).max() if fin.any() else 0.0
    ok = ~np.isnan(nrm)
    nerr = np.abs(got["normal"][ok] - nrm[ok]).max() if ok.any() else 0.0
    print(tag, "image lsb", lsb, "depth rel", rel, "normal abs", nerr, "bilinear", branch.mean(), "finite", fin.mean())
    assert lsb <= 1 and (got["image"] == (got["image_u8"].astype(np.float32) / np.float32(255)).transpose(2, 0, 1)).all()
    assert (got["bilinear"] == branch).all()
    assert (np.isnan(got["depth"]) == np.isnan(depth)).all() and (np.isinf(got["depth"]) == np.isinf(depth)).all()
    assert (np.isnan(got["normal"]) == np.isnan(nrm)).all()
    assert rel <= REL and nerr <= ABS and count == wcount


def _homography(rng, src, dst, spread=0.15):
    """target pixel -> source pixel: a scale between the grids, then a random projective disturbance and a shift that pushes taps outside"""
    (sh, sw), (dh, dw) = src, dst
    M = np.array([[sw / dw, 0, 0], [0, sh / dh, 0], [0, 0, 1]])
    M = M @ (np.eye(3) + rng.uniform(-spread, spread, (3, 3)) * np.array([[1, 1, 0.2 * dw], [1, 1, 0.2 * dh], [1 / dw, 1 / dh, 0]]))
    return M.astype(np.float32)


@pytest.mark.parametrize("flip", [0, 1])
@pytest.mark.parametrize("src,dst", [((33, 67), (29, 45)), ((33, 67), (1, 90)), ((33, 67), (75, 1)), ((64, 256), (40, 64)), ((20, 24), (301, 449))])
def test_warp_against_the_numpy_reference(src, dst, flip):
    rng = np.random.default_rng(src[0] * 7 + dst[1] + flip)
    image, depth, eligible, normal = _maps(src, 5)
    near_shape = (max(src[0] * 3 // 4, 1), max(src[1] * 3 // 4, 1))
    nearest = E.masked_nearest_resize(depth, ~np.isnan(depth), near_shape)[0]
    big = (src[0] + 5, src[1] + 9)
    big_image = rng.integers(0, 256, big + (3,), dtype=np.uint8)            # the three source grids have three sizes
    Rm = E.rotation_matrix_from_vectors(np.array([0.2, -0.1, 1.0], np.float32), np.array([0, 0, 1], np.float32))
    mats = _mats(_homography(rng, big, dst), _homography(rng, near_shape, dst), _homography(rng, src, dst), Rm)
    got, count = _run_warp(big_image, nearest, depth, eligible, normal, mats, dst[0], dst[1], flip)
    want = R.warp_maps(big_image, nearest, depth, eligible, normal, mats, dst[0], dst[1], flip)
    _check_warp(got, count, want, f"{src}->{dst} flip {flip}")


@pytest.mark.parametrize("side", ["left", "right", "top", "bottom", "outside", "far"])
def test_warp_taps_outside_the_source(side):
    """A translation that hangs the 8 x 8 Lanczos window and the bilinear taps over one side, or puts the whole target outside"""
    src, dst = (24, 30), (16, 20)
    image, depth, eligible, normal = _maps(src, 9)
    image[:] = 255                                   # a constant image: the constant-0 border shows in every tap that reaches outside
    depth = np.full(src, 2.0, np.float32)
    eligible = np.ones(src, np.float32)
    normal = np.broadcast_to(np.array([0, 0, -1], np.float32), src + (3,)).copy()
    shift = {"left": (-6.3, 2.2), "right": (17.6, 2.2), "top": (3.4, -5.7), "bottom": (3.4, 14.6), "outside": (-200.5, 7.0), "far": (3e9, -3e9)}[side]
    M = np.array([[1, 0, shift[0]], [0, 1, shift[1]], [0, 0, 1]], np.float32)
    mats = _mats(M, M, M)
    got, count = _run_warp(image, depth, depth, eligible, normal, mats, dst[0], dst[1], 0)
    want = R.warp_maps(image, depth, depth, eligible, normal, mats, dst[0], dst[1], 0)
    _check_warp(got, count, want, side)
    if side in ("outside", "far"):
        assert not got["image_u8"].any() and not got["bilinear"].any() and (got["depth"] == 0).all() and (got["normal"] == 0).all()
    else:
        assert 0 < (got["image_u8"] == 255).all(-1).sum() < dst[0] * dst[1] and got["bilinear"].any() and not got["bilinear"].all()


def test_warp_all_ones_eligibility_is_exactly_one_inside():
    src, dst = (40, 52), (61, 83)
    image, depth, _, normal = _maps(src, 3)
    depth = np.full(src, 2.0, np.float32)
    rng = np.random.default_rng(4)
    M = _homography(rng, src, dst, 0.1)
    mats = _mats(M, M, M, zr=(0.0, 0.0, 1.0))
    got, _ = _run_warp(image, depth, depth, np.ones(src, np.float32), normal, mats, dst[0], dst[1], 0)
    sx, sy = R.source_coords(M, dst[0], dst[1])
    inside = (sx >= 0) & (sx <= src[1] - 1) & (sy >= 0) & (sy <= src[0] - 1)
    assert inside.sum() > 1000 and got["bilinear"][inside].all()
    assert np.abs(got["depth"][inside] - 2.0).max() <= 2.0 * REL


def test_warp_nearest_rounds_half_to_even():
    src = (6, 8)
    nearest = (np.arange(48, dtype=np.float32) + 1).reshape(src)
    image = np.zeros(src + (3,), np.uint8)
    zeros = np.zeros(src, np.float32)
    M = np.array([[1, 0, -0.5], [0, 1, 0.5], [0, 0, 1]], np.float32)        # every coordinate lies exactly on a half
    mats = _mats(M, M, M, zr=(0.0, 0.0, 1.0))
    got, _ = _run_warp(image, nearest, np.ones(src, np.float32), zeros, np.zeros(src + (3,), np.float32), mats, 7, 9, 0)
    rx, ry = np.rint(np.arange(9) - 0.5), np.rint(np.arange(7) + 0.5)
    want = np.zeros((7, 9), np.float32)
    for i, y in enumerate(ry):
        for j, x in enumerate(rx):
            if 0 <= x <= 7 and 0 <= y <= 5:
                want[i, j] = nearest[int(y), int(x)]
    assert rx.tolist() == [-0.0, 0, 2, 2, 4, 4, 6, 6, 8] and (got["depth"] == want).all() and not got["bilinear"].any()


# ---------------------------------------------------------------------------------------------------------------------------------------
# finish: fallback, unit, quantile clamp, masks
# ---------------------------------------------------------------------------------------------------------------------------------------
def _finish(depth, count, unit, clamp, only_known):
    n = depth.size
    d = _t(depth.ravel())
    fin, inf = torch.full((n,), 7, dtype=torch.uint8, device="cuda"), torch.full((n,), 7, dtype=torch.uint8, device="cuda")
    ws = torch.empty(E.QUANTILE_WORKSPACE, dtype=torch.int32, device="cuda")
    cnt, invalid = _t(np.array([count], np.int32)), torch.full((1,), 7, dtype=torch.int32, device="cuda")
    L.check(L.lib.moge_train_finish(_p(d), n, _p(cnt), float(unit or 0.0), int(unit is not None), 0.01, float(clamp), int(only_known), _p(ws), _p(fin), _p(inf),
                                    _p(invalid), _stream()))
    return d.cpu().numpy(), fin.cpu().numpy().astype(bool), inf.cpu().numpy().astype(bool), int(invalid[0]), ws[5:6].view(torch.float32).cpu().numpy()[0]


def _values(kind, n, rng):
    if kind == "random":
        return rng.uniform(0.5, 80, n).astype(np.float32)
    if kind == "equal":
        return np.full(n, 3.25, np.float32)
    v = rng.uniform(0.5, 80, n).astype(np.float32)                          # specials: negatives, zeros, inf and NaN among the finite values
    v[::7], v[1::11], v[2::13], v[3::17] = np.inf, np.nan, -1.5, 0.0
    return v


@pytest.mark.parametrize("unit,only_known,clamp", [(None, False, 1000.0), (0.001, True, 1.5)])
@pytest.mark.parametrize("kind", ["random", "equal", "specials"])
@pytest.mark.parametrize("n", [1, 2, 101, 1000, STRIDE - 1, STRIDE + 1, 2 * STRIDE + 17])
def test_finish(n, kind, unit, only_known, clamp):
    rng = np.random.default_rng(n)
    depth = _values(kind, n, rng)
    count = int(np.isfinite(depth).sum())
    got = _finish(depth, count, unit, clamp, only_known)
    want = R.finish(depth, count, unit, clamp, only_known)
    assert got[3] == int(want[3])
    if np.isfinite(want[4]):
        assert abs(got[4] - want[4]) <= REL * abs(want[4])
    else:
        assert np.isnan(got[4]) and np.isnan(want[4])
    assert (got[1] == want[1]).all() and (got[2] == want[2]).all()
    d, g = got[0], want[0]
    assert (np.isnan(d) == np.isnan(g)).all() and (np.isinf(d) == np.isinf(g)).all()
    fin = np.isfinite(g)
    assert not fin.any() or (np.abs(d[fin] - g[fin]) <= REL * np.abs(g[fin])).all()


@pytest.mark.parametrize("finite", [1, 2, 101])
def test_finish_quantile_of_few_finite_values_among_inf(finite):
    n = 5000
    depth = np.full(n, np.inf, np.float32)
    depth[np.random.default_rng(finite).choice(n, finite, replace=False)] = np.linspace(1, 9, finite, dtype=np.float32)
    got = _finish(depth, n, None, 2.0, False)                               # the count says "enough finite": no fallback
    want = R.finish(depth, n, None, 2.0, False)
    assert got[3] == 0 and abs(got[4] - want[4]) <= REL * abs(want[4])
    assert np.array_equal(got[0], want[0]) and got[2].sum() == n - finite and (got[1] == ~got[2]).all()


@pytest.mark.parametrize("n", [1000, 3000, STRIDE + 1017])
def test_finish_fallback_boundary(n):
    """count / n < 0.001 in float64: count = n / 1000 (rounded up) keeps the depth, one less replaces it with ones"""
    edge = -(-n // 1000)
    for count in (edge, edge - 1):
        depth = np.full(n, np.nan, np.float32)
        depth[:count] = 2.0
        got = _finish(depth, count, 0.5, 1000.0, True)
        want = R.finish(depth, count, 0.5, 1000.0, True)
        fallback = count / n < 0.001
        assert fallback == (count == edge - 1) and got[3] == int(fallback) == int(want[3])
        assert np.array_equal(got[0], want[0], equal_nan=True) and (got[1] == want[1]).all() and (got[2] == want[2]).all()
        if fallback:
            assert (got[0] == 0.5).all() and got[1].all() and got[4] == 500.0


# ---------------------------------------------------------------------------------------------------------------------------------------
# bad arguments
# ---------------------------------------------------------------------------------------------------------------------------------------
def test_argument_checks():
    lib, st = L.lib, _stream()
    depth = _t(np.full((4, 5), 2.0, np.float32))
    normal = torch.full((4, 5, 3), 7.0, device="cuda")
    elig = torch.full((4, 5), 7.0, device="cuda")
    image = torch.zeros((4, 5, 3), dtype=torch.uint8, device="cuda")
    out = T.allocate_batch(1, 4, 5, "cuda")
    for v in out.values():
        v.view(torch.uint8).fill_(7)

    def fails(code, text):
        assert code == -1 and text in lib.moge_last_error().decode()

    fails(lib.moge_train_normal_map(None, 4, 5, 0.9, 1.2, 0.5, 0.5, 88.0, _p(normal), st), "null")
    fails(lib.moge_train_normal_map(_p(depth), 0, 5, 0.9, 1.2, 0.5, 0.5, 88.0, _p(normal), st), "empty")
    fails(lib.moge_train_normal_map(_p(depth), 4, -1, 0.9, 1.2, 0.5, 0.5, 88.0, _p(normal), st), "empty")
    fails(lib.moge_train_normal_map(_p(depth), 4, 5, 0.0, 1.2, 0.5, 0.5, 88.0, _p(normal), st), "focal")
    fails(lib.moge_train_normal_map(_p(depth), 4, 5, 0.9, 1.2, 0.5, 0.5, 0.0, _p(normal), st), "threshold")
    fails(lib.moge_train_depth_edge(_p(depth), 4, 5, 5, 0.01, None, None, st), "null")
    fails(lib.moge_train_depth_edge(_p(depth), 4, 0, 5, 0.01, _p(elig), None, st), "empty")
    fails(lib.moge_train_depth_edge(_p(depth), 4, 5, 4, 0.01, _p(elig), None, st), "kernel size")
    fails(lib.moge_train_depth_edge(_p(depth), 4, 5, 17, 0.01, _p(elig), None, st), "kernel size")

    eye = np.eye(3, dtype=np.float32)
    good = _mats(eye, eye, eye)

    def warp(mats=good, img=image, ih=4, oh=4, count=out["count"]):
        mats = np.ascontiguousarray(mats, np.float32)
        return lib.moge_train_warp(_p(img), ih, 5, _p(depth), 4, 5, _p(depth), _p(depth), _p(normal), 4, 5, oh, 5, C.c_void_p(mats.ctypes.data), 0, _p(out["image_u8"]),
                                   _p(out["image"]), _p(out["depth"]), _p(out["normal"]), None, _p(count), st)

    fails(warp(img=None), "null")
    fails(warp(count=None), "null")
    fails(warp(ih=0), "empty")
    fails(warp(oh=-3), "empty")
    singular = np.array([[1, 2, 3], [2, 4, 6], [0, 0, 1]], np.float32)
    for slot in range(3):
        mats = [eye, eye, eye]
        mats[slot] = singular
        fails(warp(mats=_mats(*mats)), "singular")
    fails(warp(mats=_mats(eye, eye * np.float32(np.nan), eye)), "singular")
    fails(lib.moge_train_warp(_p(image), 4, 5, _p(depth), 4, 5, _p(depth), _p(depth), _p(normal), 4, 5, 4, 5, None, 0, _p(out["image_u8"]), _p(out["image"]),
                              _p(out["depth"]), _p(out["normal"]), None, _p(out["count"]), st), "null")

    ws = out["workspace"][0]
    fin, inf = out["depth_mask_fin"][0], out["depth_mask_inf"][0]
    fails(lib.moge_train_finish(None, 20, _p(out["count"]), 0.0, 0, 0.01, 1000.0, 0, _p(ws), _p(fin), _p(inf), _p(out["invalid"]), st), "null")
    fails(lib.moge_train_finish(_p(out["depth"]), 0, _p(out["count"]), 0.0, 0, 0.01, 1000.0, 0, _p(ws), _p(fin), _p(inf), _p(out["invalid"]), st), "n < 1")
    fails(lib.moge_train_finish(_p(out["depth"]), 20, _p(out["count"]), 0.0, 0, 1.5, 1000.0, 0, _p(ws), _p(fin), _p(inf), _p(out["invalid"]), st), "q outside")
    torch.cuda.synchronize()
    for k, v in out.items():                                                # nothing was launched: no output changed
        assert (v.view(torch.uint8) == 7).all(), k
    assert (normal == 7).all() and (elig == 7).all()
    assert lib.moge_train_warp(_p(image), 4, 5, _p(depth), 4, 5, _p(depth), _p(depth), _p(normal.fill_(0)), 4, 5, 4, 5, C.c_void_p(good.ctypes.data), 0,
                               _p(out["image_u8"]), _p(out["image"]), _p(out["depth"]), _p(out["normal"]), None, _p(out["count"]), st) == 0      # NULL branch map is allowed
    torch.cuda.synchronize()
    assert int(out["count"][0]) == 20
