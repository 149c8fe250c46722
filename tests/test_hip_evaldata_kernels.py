"""GPU: the kernels of csrc/evaldata.hip against Pillow, np.nanquantile, np.bincount and the plain numpy references of tests/eval_reference.py,
at the shapes and values the five fixtures of tests/test_hip_evaluation.py never reach: Lanczos up / down / one axis / identity / 1-pixel /
extreme ratios / clipping content, 16-bit labels at and above 32768, homographies that leave the source, the radix-select quantile at the
grid-stride boundaries with every q and adversarial values, and the argument checks of the C entries."""
import ctypes as C

import numpy as np
import pytest
import torch
from PIL import Image

from moge_amd import _lib as L
from moge_amd import evaluation as E
from tests import eval_reference as R

pytestmark = pytest.mark.gpu

QSTRIDE = 512 * 256                      # EV_BLOCKS x EV_THREADS: the grid stride of the quantile passes


@pytest.fixture(scope="module", autouse=True)
def _needs_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _p(t):
    return C.c_void_p(t.data_ptr())


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


# ---------------------------------------------------------------------------------------------------------------------------------------
# Lanczos: equal bytes to Pillow
# ---------------------------------------------------------------------------------------------------------------------------------------
def _image(shape, seed, kind):
    rng = np.random.default_rng(seed)
    img = rng.integers(0, 256, shape + (3,), dtype=np.uint8)
    if kind == "checker":                         # 0 / 255 hard edges: the fixed-point sums overshoot and clip on both sides
        y, x = np.mgrid[0:shape[0], 0:shape[1]]
        img[:] = (255 * (((x // 2) + (y // 3)) & 1)).astype(np.uint8)[..., None]
        img[..., 1] = 255 - img[..., 1]
    return img


LANCZOS = [((30, 40), (30, 40)),                 # identity (a copy)
           ((50, 80), (50, 33)), ((50, 80), (50, 161)),          # W only
           ((80, 50), (21, 50)), ((80, 50), (203, 50)),          # H only
           ((40, 60), (60, 90)),                 # up x1.5
           ((13, 11), (91, 77)),                 # up x7
           ((64, 48), (1, 1)), ((40, 50), (1, 37)), ((40, 50), (29, 1)), ((1, 1), (5, 7)), ((1, 300), (1, 7)),
           ((97, 211), (13, 389)),               # primes, down in H and up in W
           ((2000, 9), (3, 9)), ((7, 3000), (7, 2)),              # extreme ratios: ksize in the thousands, host row window
           ((4032, 6048), (427, 640))]


@pytest.mark.parametrize("kind", ["random", "checker"])
@pytest.mark.parametrize("src,dst", LANCZOS)
def test_lanczos_matches_pillow(src, dst, kind):
    if src == (4032, 6048) and kind == "checker":
        pytest.skip("one large case is enough")
    img = _image(src, src[0] * 7 + dst[1], kind)
    ref = np.array(Image.fromarray(img).resize((dst[1], dst[0]), Image.Resampling.LANCZOS))
    got = E.lanczos_resize(_t(img), *dst).cpu().numpy()
    assert got.shape == ref.shape and np.array_equal(got, ref), (src, dst, kind, int((got != ref).sum()))


# ---------------------------------------------------------------------------------------------------------------------------------------
# nearest resize of label maps (cv2 INTER_NEAREST rule)
# ---------------------------------------------------------------------------------------------------------------------------------------
IDS = np.array([0, 255, 256, 32767, 32768, 65535], np.uint16)


@pytest.mark.parametrize("dtype", [np.uint8, np.uint16])
@pytest.mark.parametrize("src,dst", [((30, 40), (30, 40)), ((30, 40), (90, 120)), ((30, 40), (10, 8)), ((37, 53), (100, 71)), ((100, 71), (37, 53)),
                                     ((1, 1), (5, 9)), ((40, 50), (1, 1)), ((1, 50), (7, 3)), ((1008, 1512), (341, 512))])
def test_resize_nearest(src, dst, dtype):
    rng = np.random.default_rng(src[0] + dst[1])
    seg = rng.choice(IDS if dtype == np.uint16 else IDS[:2], src).astype(dtype)
    seg[:, ::5] = rng.integers(0, np.iinfo(dtype).max + 1, (src[0], len(range(0, src[1], 5))), dtype=np.int64).astype(dtype)
    dev = _t(seg.view(np.int16) if dtype == np.uint16 else seg)             # 16-bit labels travel as int16 bits, as in the loader
    got = E.resize_nearest(dev, dst).cpu().numpy()
    if dtype == np.uint16:
        got = got.view(np.uint16)
    assert np.array_equal(got, R.resize_nearest_ref(seg, *dst))


# ---------------------------------------------------------------------------------------------------------------------------------------
# masked nearest resize + distance
# ---------------------------------------------------------------------------------------------------------------------------------------
K0 = np.array([[0.9, 0, 0.47], [0, 1.2, 0.55], [0, 0, 1]], np.float32)


@pytest.mark.parametrize("src,dst", [((240, 320), (240, 320)), ((240, 320), (80, 120)), ((100, 150), (37, 61)), ((60, 80), (150, 190)),
                                     ((1008, 1512), (341, 512)), ((9, 9), (2, 2)), ((5, 7), (1, 1))])
@pytest.mark.parametrize("kind", ["random", "all_invalid", "single", "ties"])
def test_masked_nearest_distance(src, dst, kind):
    rng = np.random.default_rng(src[1] + dst[0])
    depth = rng.uniform(0.5, 30, src).astype(np.float32)
    mask = rng.random(src) < 0.7
    if kind == "all_invalid":
        mask[:] = False
    elif kind == "single":
        mask[:] = False
        mask[src[0] - 1, src[1] // 2] = True
    elif kind == "ties":                          # one valid pixel per 2 x 2 block corner pair: equidistant candidates in even windows
        mask[:] = False
        mask[::2, ::2] = True
        mask[1::2, 1::2] = True
    d, m, dist = E.masked_nearest_resize_distance(_t(depth), _t(mask), dst, K0)
    ref_d, ref_m = E.masked_nearest_resize(depth, mask, dst)
    assert np.array_equal(m.cpu().numpy().astype(bool), ref_m)
    assert np.array_equal(d.cpu().numpy(), ref_d)
    assert R.same_bits(dist.cpu().numpy(), R.distance_ref(ref_d, K0))


# ---------------------------------------------------------------------------------------------------------------------------------------
# remap
# ---------------------------------------------------------------------------------------------------------------------------------------
TGT_K = np.array([[1.1, 0, 0.5], [0, 1.4, 0.5], [0, 0, 1]], np.float32)
HOMOGRAPHIES = {
    "identity": np.eye(3, dtype=np.float32),
    "off_centre": np.array([[0.9, 0.02, 0.07], [-0.01, 1.05, -0.03], [0.01, 0.02, 1.0]], np.float32),
    "partly_outside": np.array([[1.3, 0.1, -0.2], [-0.05, 1.2, -0.15], [0.05, -0.04, 1.0]], np.float32),
}


def _remap(image, distance, mask, seg, T, OH, OW):
    h, w = mask.shape
    kinv = np.linalg.inv(TGT_K).astype(np.float32)
    mats, mats_p = E._host_f32(np.concatenate([T.ravel(), kinv.ravel()]))
    out = {"image": torch.empty((OH, OW, 3), dtype=torch.uint8, device="cuda"), "chw": torch.empty((3, OH, OW), device="cuda"),
           "depth": torch.empty((OH, OW), device="cuda"), "mask": torch.empty((OH, OW), dtype=torch.uint8, device="cuda")}
    seg_t = None
    if seg is not None:
        seg_t = _t(seg.view(np.int16) if seg.dtype == np.uint16 else seg)
        out["seg"] = torch.empty((OH, OW), dtype=torch.int32, device="cuda")
        out["hist"] = torch.empty(E.SEG_BINS, dtype=torch.int32, device="cuda")
    ins = [_t(image), _t(distance), _t(mask.astype(np.uint8))]             # held until the kernel has run
    rc = L.lib.moge_eval_remap(_p(ins[0]), _p(ins[1]), _p(ins[2]), None if seg_t is None else _p(seg_t),
                               0 if seg is None else seg.itemsize, h, w, OH, OW, mats_p, _p(out["image"]), _p(out["chw"]), _p(out["depth"]),
                               _p(out["mask"]), None if seg is None else _p(out["seg"]), None if seg is None else _p(out["hist"]), _stream())
    L.check(rc)
    torch.cuda.synchronize()
    del mats, ins
    return {k: v.cpu().numpy() for k, v in out.items()}, kinv


@pytest.mark.parametrize("seg_dtype", [None, np.uint8, np.uint16])
@pytest.mark.parametrize("name", list(HOMOGRAPHIES))
@pytest.mark.parametrize("src,dst", [((240, 320), (240, 320)), ((386, 1333), (375, 750)), ((50, 70), (123, 97))])
def test_remap(src, dst, name, seg_dtype):
    rng = np.random.default_rng(src[0] + dst[0] + len(name))
    image = rng.integers(0, 256, src + (3,), dtype=np.uint8)
    image[::4] = 255
    distance = rng.uniform(0.5, 50, src).astype(np.float32)
    mask = rng.random(src) < 0.8
    seg = None
    if seg_dtype is not None:
        seg = rng.choice(IDS if seg_dtype == np.uint16 else IDS[:2], src).astype(seg_dtype)
        seg[::3] = rng.integers(0, np.iinfo(seg_dtype).max + 1, seg[::3].shape, dtype=np.int64).astype(seg_dtype)
    T = HOMOGRAPHIES[name]
    got, kinv = _remap(image, distance, mask, seg, T, *dst)
    ref = R.remap_ref(image, distance, mask, seg, T, kinv, *dst)
    diff = np.abs(got["image"].astype(np.int16) - ref["image"].astype(np.int16))
    assert diff.max() <= 1 and diff.any(axis=-1).mean() <= 1e-3, (diff.max(), diff.any(axis=-1).mean())
    assert np.array_equal(got["chw"], got["image"].astype(np.float32).transpose(2, 0, 1) / np.float32(255))
    assert np.array_equal(got["mask"].astype(bool), ref["mask"])
    assert R.same_bits(got["depth"], ref["depth"])
    if name == "partly_outside":
        assert not ref["mask"].all() and ref["mask"].any()
    if seg is not None:
        assert np.array_equal(got["seg"], ref["seg"])
        assert np.array_equal(got["hist"], np.bincount(got["seg"].ravel(), minlength=E.SEG_BINS))
        if seg_dtype == np.uint16:
            assert got["hist"][32768:].sum() > 0


# ---------------------------------------------------------------------------------------------------------------------------------------
# quantile cut: exact np.nanquantile at any q, then mask / nan_to_num / unit, through the C entry
# ---------------------------------------------------------------------------------------------------------------------------------------
def _quantile(depth, mask, q, drop, unit):
    d, m = _t(depth), _t(mask.astype(np.uint8))
    ws = torch.empty(E.QUANTILE_WORKSPACE, dtype=torch.int32, device="cuda")
    count = torch.empty(1, dtype=torch.int32, device="cuda")
    L.check(L.lib.moge_eval_quantile_cut(_p(d), _p(m), depth.size, float(q), float(drop), float(unit or 0.0), int(unit is not None), _p(ws),
                                         _p(count), _stream()))
    return ws[5:6].view(torch.float32).cpu().numpy()[0], m.cpu().numpy().astype(bool), d.cpu().numpy(), int(count.item())


def _values(kind, n, rng):
    if kind == "random":
        v = rng.lognormal(1, 1, n)
    elif kind == "equal":
        v = np.full(n, 2.5)
    elif kind == "digits":                        # few distinct values whose keys differ in every byte, heavily duplicated
        v = rng.choice(np.float32([1.0, np.nextafter(np.float32(1), np.float32(2)), 1.0039062, 2.0, 256.0, 0.5, 3e-39, 1e30]), n)
    elif kind == "specials":
        v = rng.choice(np.float32([-np.inf, -7.5, -1.0, -0.0, 0.0, 1e-45, 0.25, 3.0, np.inf, np.nan,
                                   np.uint32(0xFFC00000).view(np.float32)]), n)
    else:
        raise ValueError(kind)
    return np.asarray(v, np.float32)


@pytest.mark.parametrize("kind", ["random", "equal", "digits", "specials"])
@pytest.mark.parametrize("n", [1, 255, QSTRIDE - 1, QSTRIDE, QSTRIDE + 1, 3 * QSTRIDE + 17])
def test_quantile_cut(n, kind):
    rng = np.random.default_rng(n + len(kind))
    depth = _values(kind, n, rng)
    for valid in ("none", "one", "one_neg_zero", "two", "some", "all"):
        mask = np.zeros(n, bool)
        depth_v = depth
        if valid == "one":
            mask[n - 1] = True
        elif valid == "one_neg_zero":             # n = 1 takes the last element with gamma = 1: b - d (1 - gamma) keeps the sign of -0.0
            depth_v = depth.copy()
            depth_v[n // 2] = np.float32(-0.0)
            mask[n // 2] = True
        elif valid == "two" and n >= 2:
            mask[[0, n - 1]] = True
        elif valid == "some":
            mask = rng.random(n) < 0.6
        elif valid == "all":
            mask[:] = True
        for q in (0.0, 0.01, 0.5, 0.999, 1.0):
            drop, unit = ((1.0, None), (3.0, 0.5))[int(q * 1000) % 2]
            md, m, d, count = _quantile(depth_v, mask, q, drop, unit)
            r_md, r_m, r_d, r_count = R.quantile_cut_ref(depth_v, mask, q, drop, unit)
            assert R.same_bits(md, r_md), (n, kind, valid, q, md, r_md)
            assert np.array_equal(m, r_m) and count == r_count, (n, kind, valid, q)
            assert np.array_equal(d.view(np.uint32), r_d.view(np.uint32)), (n, kind, valid, q)


# ---------------------------------------------------------------------------------------------------------------------------------------
# unproject, with and without the empty-mask fallback
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("count", [0, 5])
def test_unproject(count):
    rng = np.random.default_rng(count)
    OH, OW = 123, 97
    depth = rng.uniform(0.1, 40, (OH, OW)).astype(np.float32)
    mask = rng.random((OH, OW)) < 0.5
    kinv = np.linalg.inv(TGT_K).astype(np.float32)
    d, m = _t(depth), _t(mask.astype(np.uint8))
    pts = torch.empty((OH, OW, 3), device="cuda")
    buf, kp = E._host_f32(kinv)
    cnt = _t(np.array([count], np.int32))
    L.check(L.lib.moge_eval_unproject(_p(d), _p(m), OH, OW, kp, _p(cnt), _p(pts), _stream()))
    torch.cuda.synchronize()
    r_d, r_m, r_p = R.unproject_ref(depth, mask, kinv, count)
    assert np.array_equal(d.cpu().numpy(), r_d) and np.array_equal(m.cpu().numpy().astype(bool), r_m)
    assert R.same_bits(pts.cpu().numpy(), r_p)
    del buf


# ---------------------------------------------------------------------------------------------------------------------------------------
# argument checks: rejected before any launch
# ---------------------------------------------------------------------------------------------------------------------------------------
def test_argument_checks():
    d, m = torch.ones(64, device="cuda"), torch.ones(64, dtype=torch.uint8, device="cuda")
    ws = torch.zeros(E.QUANTILE_WORKSPACE, dtype=torch.int32, device="cuda")
    count = torch.zeros(1, dtype=torch.int32, device="cuda")
    for q in (-0.01, 1.01, float("nan"), float("inf")):
        assert L.lib.moge_eval_quantile_cut(_p(d), _p(m), 64, q, 1.0, 0.0, 0, _p(ws), _p(count), _stream()) == -1, q
    for n in (0, -5):
        assert L.lib.moge_eval_quantile_cut(_p(d), _p(m), n, 0.5, 1.0, 0.0, 0, _p(ws), _p(count), _stream()) == -1, n
    src, dst = torch.zeros(64, dtype=torch.uint8, device="cuda"), torch.zeros(64, dtype=torch.uint8, device="cuda")
    for size in (0, 3, 4):
        assert L.lib.moge_eval_resize_nearest(_p(src), size, 4, 4, 2, 2, _p(dst), _stream()) == -1, size
    torch.cuda.synchronize()
    assert not ws.any() and not count.any() and not dst.any()          # nothing ran
