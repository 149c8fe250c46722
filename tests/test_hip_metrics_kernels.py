"""GPU: the kernels of csrc/metrics.hip against the plain numpy references of tests/eval_reference.py, at the sizes and values the fixtures of
tests/test_hip_metrics.py never reach: grid-stride tails around the fixed 256 x 256 grid, every transform mode and K up to 8, empty masks,
NaN / signed zeros / negatives, boundary tiles that are not multiples of 16 and maps too small for an interior, per-pixel interleaved
segments, and 1 and 512 segment labels."""

import numpy as np
import pytest
import torch

from moge_amd import evaluation as E
from tests import eval_reference as R

pytestmark = pytest.mark.gpu

STRIDE = 256 * 256                      # MOGE_METRICS_PARTIALS workgroups x 256 threads: the grid stride of the error pass / masked max


@pytest.fixture(scope="module")
def M():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from moge_amd import metrics
    return metrics


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _close(got, ref, tol=1e-12):
    return abs(got - ref) <= tol * max(abs(ref), 1e-300)


# ---------------------------------------------------------------------------------------------------------------------------------------
# error pass
# ---------------------------------------------------------------------------------------------------------------------------------------
def _error_inputs(n, dim, seed, empty=False):
    rng = np.random.default_rng(seed)
    shape = (n,) if dim == 1 else (n, 3)
    gt = rng.uniform(0.5, 20.0, shape).astype(np.float32)
    if dim == 3:
        gt[:, :2] = rng.uniform(-10, 10, (n, 2)).astype(np.float32)
    noise = rng.choice(np.float32([0.7, 0.79, 0.8, 0.95, 1.0, 1.05, 1.249, 1.25, 1.26, 1.6]), shape)
    pred = (gt * noise).astype(np.float32)
    if n > 4:
        pred.reshape(-1)[:: 97] = 0.0                     # q = 0: g / q = inf in delta1
        pred.reshape(-1)[1:: 89] *= -1                    # sign flips
    mask = np.zeros(n, bool) if empty else rng.random(n) < 0.7
    if n and not empty:
        mask[-1] = True                                   # the last element of the grid-stride tail
    return pred, gt, mask


def _params(dim, K, seed):
    rng = np.random.default_rng(seed)
    modes = [0, 1, 2, 3] if dim == 1 else [0, 1, 2]
    rows = []
    for k in range(K):
        mode = modes[k % len(modes)]
        s = np.float32(rng.uniform(0.6, 1.4))
        t = rng.uniform(-0.5, 0.5, 3).astype(np.float32)
        c = np.float32(1 / 15.0) if mode == 3 else np.float32(0)          # mode 3: clamp_min(., 1 / max gt) clamps the small disparities
        rows.append([mode, s, *t, c])
    return np.array(rows, np.float32)


@pytest.mark.parametrize("dim", [1, 3])
@pytest.mark.parametrize("n", [1, 255, 256, 257, STRIDE - 1, STRIDE, STRIDE + 1, 1365 * 2048])
def test_error_pass_sweep(M, dim, n):
    pred, gt, mask = _error_inputs(n, dim, seed=n + dim)
    if dim == 1:
        pred = np.where(np.arange(n) % 3 == 0, np.float32(1) / np.where(pred == 0, np.float32(1), pred), pred).astype(np.float32)   # disparity-like
    for K in (1, 8):
        params = _params(dim, K, seed=K)
        got = M.error_pass(_t(pred), _t(gt), _t(mask), _t(params)).cpu().numpy()
        ref = R.error_pass_ref(pred, gt, mask, params, dim)
        for k in range(K):
            assert got[k, 2] == ref[k, 2] and got[k, 1] == ref[k, 1], (K, k, got[k], ref[k])
            assert _close(got[k, 0], ref[k, 0]), (K, k, got[k, 0], ref[k, 0])


@pytest.mark.parametrize("dim", [1, 3])
def test_error_pass_empty_mask(M, dim):
    pred, gt, mask = _error_inputs(STRIDE + 3, dim, seed=5, empty=True)
    got = M.error_pass(_t(pred), _t(gt), _t(mask), _t(_params(dim, 8, 0))).cpu().numpy()
    assert np.array_equal(got, np.zeros((8, 3)))


def test_error_pass_mode3_clamp(M):
    """every value below the clamp: q = 1 / c exactly"""
    n = 1000
    gt = np.full(n, 4.0, np.float32)
    pred = np.linspace(-1, 0.01, n).astype(np.float32)
    params = np.array([[3, 1.0, 0.0, 0, 0, 0.25], [3, 2.0, 0.125, 0, 0, 0.25]], np.float32)
    got = M.error_pass(_t(pred), _t(gt), _t(np.ones(n, bool)), _t(params)).cpu().numpy()
    ref = R.error_pass_ref(pred, gt, np.ones(n, bool), params, 1)
    assert np.array_equal(got[:, 1:], ref[:, 1:]) and ref[0, 1] == n
    assert all(_close(got[k, 0], ref[k, 0]) for k in range(2))


# ---------------------------------------------------------------------------------------------------------------------------------------
# masked max: -inf when empty, NaN when any masked value is NaN (either sign, as torch.max), +0.0 above -0.0
# ---------------------------------------------------------------------------------------------------------------------------------------
NEG_NAN = np.uint32(0xFFC00000).view(np.float32)


def _mm_case(name, n):
    rng = np.random.default_rng(len(name) + n)
    x = rng.uniform(-5, 5, n).astype(np.float32)
    mask = rng.random(n) < 0.5
    if name == "empty":
        mask[:] = False
    elif name == "nan":
        x[n // 3] = np.nan
        mask[n // 3] = True
    elif name == "neg_nan":
        x[n - 1] = NEG_NAN
        mask[n - 1] = True
    elif name == "nan_unmasked":
        x[n // 2] = np.nan
        x[n // 2 + 1 if n > 1 else 0] = NEG_NAN
        mask[n // 2] = False
        mask[n // 2 + 1 if n > 1 else 0] = False
    elif name == "all_negative":
        x = -np.abs(x) - np.float32(1e-3)
    elif name == "signed_zeros":
        x[:] = np.float32(-0.0)
        mask[:] = True
        x[n - 1] = 0.0 if n > 1 else x[n - 1]
    elif name == "neg_zero_only":
        x = np.where(mask, np.float32(-0.0), np.float32(7.0)).astype(np.float32)
        mask[0] = True
        x[0] = np.float32(-0.0)
    elif name == "last_only":
        mask[:] = False
        mask[n - 1] = True
        x[n - 1] = np.float32(-3.5)
    return x, mask


@pytest.mark.parametrize("n", [1, 257, STRIDE + 1])
@pytest.mark.parametrize("name", ["empty", "nan", "neg_nan", "nan_unmasked", "all_negative", "signed_zeros", "neg_zero_only", "last_only", "random"])
def test_masked_max(M, name, n):
    x, mask = _mm_case(name, n)
    got = M.masked_max(_t(x), _t(mask)).cpu().numpy()
    ref = R.masked_max_ref(x, mask)
    assert R.same_bits(got, ref), (name, n, got, ref)
    if name == "empty":
        assert got == -np.inf
    if name in ("nan", "neg_nan"):
        assert np.isnan(got)


# ---------------------------------------------------------------------------------------------------------------------------------------
# boundary counts
# ---------------------------------------------------------------------------------------------------------------------------------------
SIZES = [1, 2, 6, 7, 15, 16, 17, 33, 100]
HW = [(h, w) for h in SIZES for w in SIZES if (h * 7 + w * 3) % 4 == 0 or h == w or 1 in (h, w)]


def _boundary_maps(H, W, kind, seed):
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:H, 0:W]
    gt = (2.0 + (x * 3 // max(W, 1)) * 0.4 + (y * 2 // max(H, 1)) * 0.3).astype(np.float32) * rng.choice(np.float32([1, 1.03, 1.12, 1.3]), (H, W))
    pred = (gt * rng.choice(np.float32([0.9, 1.0, 1.06, 1.2]), (H, W))).astype(np.float32)
    mask = rng.random((H, W)) < 0.85
    if kind == "specials":
        pred.reshape(-1)[:: 5] = 0.0
        pred.reshape(-1)[1:: 7] *= -1
        pred.reshape(-1)[2:: 11] = np.nan
        gt.reshape(-1)[3:: 13] = 0.0
        gt.reshape(-1)[4:: 17] *= -1
    elif kind == "no_mask":
        mask[:] = False
    elif kind == "constant":
        pred[:] = 3.0
        gt[:] = 3.0
    return pred.astype(np.float32), gt.astype(np.float32), mask


@pytest.mark.parametrize("kind", ["random", "specials", "no_mask", "constant"])
def test_boundary_counts_sweep(M, kind):
    for H, W in HW:
        pred, gt, mask = _boundary_maps(H, W, kind, H * 131 + W)
        got = M.boundary_counts(_t(pred), _t(gt), _t(mask)).cpu().numpy()
        for r in (1, 2, 3):
            ref = R.boundary_counts_ref(pred, gt, mask, r)
            assert np.array_equal(got[r - 1], ref), (kind, H, W, r, got[r - 1], ref)
            if kind == "random" and (H, W) in ((33, 100), (100, 17)):
                f1 = M.boundary_f1(_t(pred), _t(gt), _t(mask), radius=r)
                assert _close(f1, R.boundary_f1_ref(ref)), (H, W, r)
        if kind in ("no_mask", "constant") or min(H, W) <= 2:          # nothing valid / no ratio above 1 / no interior for any radius
            assert not got.any(), (kind, H, W)


def test_boundary_f1_large(M):
    """a 1365 x 2048 map: counts far above one tile's 16-bit halves, F1 from the counts"""
    pred, gt, mask = _boundary_maps(1365, 2048, "random", 7)
    got = M.boundary_counts(_t(pred), _t(gt), _t(mask)).cpu().numpy()
    for r in (1, 2, 3):
        ref = R.boundary_counts_ref(pred, gt, mask, r)
        assert np.array_equal(got[r - 1], ref), r
        assert _close(M.boundary_f1(_t(pred), _t(gt), _t(mask), radius=r), R.boundary_f1_ref(ref))


# ---------------------------------------------------------------------------------------------------------------------------------------
# low-resolution sampling (masked nearest resize) against the float64 numpy restatement
# ---------------------------------------------------------------------------------------------------------------------------------------
def _lr_ref(mask, size):
    H, W = mask.shape
    flat, valid = E.masked_nearest_resize(np.arange(H * W).reshape(H, W), mask, size)
    return valid, flat // W, flat % W


@pytest.mark.parametrize("src,size", [((480, 640), (64, 64)), ((64, 64), (64, 64)), ((40, 50), (64, 64)), ((1365, 2048), (64, 64)),
                                      ((97, 211), (64, 64)), ((100, 30), (7, 13)), ((5, 5), (2, 2))])
@pytest.mark.parametrize("kind", ["random", "all_invalid", "single", "sparse"])
def test_lr_sample(M, src, size, kind):
    rng = np.random.default_rng(src[0] + size[1])
    mask = rng.random(src) < 0.6
    if kind == "all_invalid":
        mask[:] = False
    elif kind == "single":
        mask[:] = False
        mask[src[0] // 3, src[1] - 1] = True
    elif kind == "sparse":                    # few valid pixels: equidistant ties inside windows are common
        mask = rng.random(src) < 0.05
    lr_mask, (rows, cols) = M.masked_nearest_resize(mask=_t(mask), size=size, return_index=True)
    valid, r_rows, r_cols = _lr_ref(mask, size)
    assert np.array_equal(lr_mask.cpu().numpy(), valid)
    assert np.array_equal(rows.cpu().numpy(), r_rows) and np.array_equal(cols.cpu().numpy(), r_cols)


# ---------------------------------------------------------------------------------------------------------------------------------------
# local points: segment statistics, packing and per-segment error
# ---------------------------------------------------------------------------------------------------------------------------------------
def _seg_case(kind, seed=0):
    rng = np.random.default_rng(seed)
    H, W = (240, 320) if kind != "u512" else (480, 640)
    y, x = np.mgrid[0:H, 0:W]
    depth = (3.0 + y / H + np.sin(x / W * 5)).astype(np.float32)
    u = ((x + 0.5) / W).astype(np.float32)
    v = ((y + 0.5) / H).astype(np.float32)
    gt = np.stack([(u - np.float32(0.5)) / np.float32(0.8) * depth, (v - np.float32(0.5)) / np.float32(1.1) * depth, depth], -1).astype(np.float32)
    pred = (gt * rng.uniform(0.9, 1.1, (H, W, 1)).astype(np.float32) * np.float32(1.3) + np.float32(0.05)).astype(np.float32)
    mask = rng.random((H, W)) < 0.9
    if kind == "interleaved":                 # per-pixel random labels from 40 ids: every wave holds many segments
        ids = np.arange(40) * 3 + 1
        seg = rng.choice(ids, (H, W))
        labels = {f"s{i}": int(i) for i in ids}
    elif kind == "blocks":
        seg = (y // 40) * 8 + (x // 40) + 100
        labels = {f"s{i}": int(i) for i in np.unique(seg)}
    elif kind == "signed":                    # negative coordinates only, and -0.0 / +0.0 in x
        seg = (y // 60) * 4 + (x // 80)
        gt[..., 0] = -np.abs(gt[..., 0])
        gt[:, : W // 2, 1] = np.float32(-0.0)
        gt[:, W // 2:, 1] = np.float32(0.0)
        gt[y % 7 == 0, 0] = np.float32(-0.0)
        labels = {f"s{i}": int(i) for i in np.unique(seg)}
    elif kind == "absent":                    # labels absent from the map, and map ids absent from the labels
        seg = (y // 60) * 4 + (x // 80) + 10
        labels = {f"s{i}": int(i) for i in list(range(10, 26, 2)) + [1000, 3, 77]}
    elif kind == "u1":
        seg = np.where(x < W // 2, 5, 9)
        labels = {"only": 5}
    elif kind == "u512":                      # 512 labels with skewed sizes, interleaved per pixel: some kept, most not
        p = 1.0 / np.arange(1, 513) ** 1.2
        seg = rng.choice(np.arange(512) * 2 + 7, (H, W), p=p / p.sum())
        labels = {f"s{i}": int(v) for i, v in enumerate(np.arange(512) * 2 + 7)}
    else:
        raise ValueError(kind)
    return pred, gt, mask, seg.astype(np.int64), labels


@pytest.mark.parametrize("kind", ["interleaved", "blocks", "signed", "absent", "u1", "u512"])
def test_segment_stats_pack_error(M, kind):
    pred, gt, mask, seg, labels = _seg_case(kind)
    H, W = mask.shape
    uniq = sorted(set(labels.values()))
    U = len(uniq)
    lr_mask, lr_index = M.masked_nearest_resize(mask=_t(mask), size=(64, 64), return_index=True)
    lr_m, lr_i = lr_mask.cpu().numpy(), np.stack([lr_index[0].cpu().numpy(), lr_index[1].cpu().numpy()])
    ref = R.segments_ref(seg, mask, gt, uniq, lr_m, lr_i)

    # statistics through the C entry: bbox keys, low-resolution counts, diameters
    seg32 = _t(seg.astype(np.int32))
    bbox = torch.empty(U * 6, dtype=torch.int32, device="cuda")
    lr_count = torch.empty(U, dtype=torch.int32, device="cuda")
    diameter = torch.empty(U, dtype=torch.float32, device="cuda")
    labels_t = _t(np.array(uniq, np.int32))
    index = _t(lr_i.astype(np.int32))
    p = M.L.ptr
    m8, gt_t, lr8 = _t(mask.view(np.uint8)), _t(gt), _t(lr_m.view(np.uint8))            # held until the kernels have run
    M.L.check(M.L.lib.moge_metrics_segment_stats(p(seg32), p(m8), p(gt_t), H, W, p(lr8), p(index), 64, 64, p(labels_t), U, p(bbox), p(lr_count),
                                                 p(diameter), M.L.stream_ptr(seg32.device)))
    bbox, lr_count, diameter = bbox.cpu().numpy().reshape(U, 6), lr_count.cpu().numpy(), diameter.cpu().numpy()
    for u, s in enumerate(ref):
        assert np.array_equal(bbox[u], s["bbox"]), (kind, u, bbox[u], s["bbox"])
        assert lr_count[u] == s["lr_count"], (kind, u)
        assert R.same_bits(diameter[u], s["diameter"]), (kind, u, diameter[u], s["diameter"])

    # packing and the batched solve through local_points
    det = {}
    res = M.local_points(_t(pred), _t(gt), _t(mask), _t(seg), labels, lr_mask, lr_index, details=det)
    kept = [u for u in range(U) if ref[u]["lr_count"] >= 10]
    if not kept:
        assert res == {} and not det
        return
    src, tgt, wt = det["src"].cpu().numpy(), det["tgt"].cpu().numpy(), det["weight"].cpu().numpy()
    n_max = max(ref[u]["lr_count"] for u in kept)
    assert src.shape == (len(kept), n_max, 3)
    pf, gf = pred.reshape(-1, 3), gt.reshape(-1, 3)
    for e, u in enumerate(kept):
        flat, k = ref[u]["lr_flat"], ref[u]["lr_count"]
        assert np.array_equal(src[e, :k], pf[flat]) and np.array_equal(tgt[e, :k], gf[flat]), (kind, e)
        assert np.all(wt[e, :k] == np.float32(1) / ref[u]["diameter"]) and not wt[e, k:].any()
        assert not src[e, k:].any() and not tgt[e, k:].any()

    # per-segment error at a chosen scale / shift per kept segment
    rng = np.random.default_rng(3)
    E_ = len(kept)
    scale = rng.uniform(0.6, 0.9, E_).astype(np.float32)
    shift = rng.uniform(-0.1, 0.1, (E_, 3)).astype(np.float32)
    row = [-1] * U
    for e, u in enumerate(kept):
        row[u] = e
    out = M._segment_error(seg32, _t(mask), _t(pred), _t(gt), labels_t, U, _t(np.array(row, np.int32)), _t(np.array(kept, np.int32)),
                           _t(scale), _t(shift), _t(diameter)).cpu().numpy()
    for e, u in enumerate(kept):
        rel, d1, n = R.segment_error_ref(seg, mask, pred, gt, uniq[u], scale[e], shift[e], diameter[u])
        assert out[e, 2] == n and out[e, 1] == d1, (kind, e, out[e], (rel, d1, n))
        assert _close(out[e, 0], rel), (kind, e, out[e, 0], rel)
