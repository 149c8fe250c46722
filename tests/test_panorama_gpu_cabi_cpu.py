"""CPU: the panorama entry points of the C ABI (include/moge_hip.h, csrc/panorama.hip) are exported and bound, the workspace size is the documented
arithmetic, bad arguments come back as MOGE_ERR_INVALID with a message before anything touches a GPU, and the host refactor that gives the GPU
tests a value for every stage - `moge_amd.panorama.merge_system` followed by scipy's lsmr - reproduces `merge_panorama_depth` bit for bit.  No GPU
call is made here: every C call below either is pure arithmetic or is rejected by the argument checks."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
NAMES = ["moge_pano_split", "moge_pano_merge_workspace", "moge_pano_system", "moge_pano_lsmr", "moge_pano_resize_bilinear", "moge_pano_resize_nearest",
         "moge_pano_log", "moge_pano_finish", "moge_test_pano_apply"]
INVALID = -1


def last_error(L):
    return (L.lib.moge_last_error() or b"").decode()


def documented_bytes(width, height, n, span, state_doubles):
    N = width * height
    M = N + (height - 1) * width + (height - 1) + N
    P = -(-M // span)
    return 8 * (M + 3 * N + 3 * P + state_doubles) + 5 * n * N


def test_symbols_are_declared_exported_and_bound():
    from moge_amd import _lib as L
    hdr = open(os.path.join(ROOT, "include", "moge_hip.h")).read()
    for name in NAMES:
        assert re.search(r"\bint\s+" + name + r"\s*\(", hdr), name
        assert name in L.EXPORTS and getattr(L.lib, name).argtypes is not None, name
    assert L.lib.moge_abi_version() == 5                                   # purely additive
    for macro, value in (("MOGE_PANO_MAX_VIEWS", L.PANO_MAX_VIEWS), ("MOGE_PANO_SPAN", L.PANO_SPAN), ("MOGE_PANO_STATE_DOUBLES", L.PANO_STATE_DOUBLES)):
        assert int(re.search(r"#define\s+" + macro + r"\s+(\d+)", hdr).group(1)) == value, macro
    assert re.search(r"#define\s+MOGE_PANO_MAX_PIXELS\s+\(1 << 29\)", hdr) and L.PANO_MAX_PIXELS == 1 << 29
    import moge_amd.panorama_gpu as G
    assert (G.MAX_VIEWS, G.SPAN, G.LAUNCHES_PER_ITERATION) == (16, 1024, 6)
    assert "panorama.hip" in __import__("moge_amd.build", fromlist=["SOURCES"]).SOURCES


def test_workspace_is_the_documented_arithmetic():
    from moge_amd import _lib as L
    import moge_amd.panorama_gpu as G
    n = C.c_int64(-1)
    for w, h, views in ((72, 36, 12), (264, 132, 12), (1920, 960, 12), (2, 2, 1), (1, 1, 0), (150, 1, 12), (513, 77, 16), (72, 36, 0)):
        assert L.lib.moge_pano_merge_workspace(w, h, views, C.byref(n)) == 0
        assert n.value == documented_bytes(w, h, views, L.PANO_SPAN, L.PANO_STATE_DOUBLES) == G.workspace_bytes(w, h, views), (w, h, views)
    assert G.system_rows(72, 36) == 2 * 2592 + 35 * 72 + 35 == 7739
    assert documented_bytes(72, 36, 12, 1024, 64) == 8 * (7739 + 3 * 2592 + 3 * 8 + 64) + 5 * 12 * 2592
    assert G.system_rows(1920, 960) == 2 * 1843200 + 959 * 1920 + 959 == 5528639                            # the finest system of the CLI's merge: 5.5 M rows, zero rows included


def test_bad_arguments_are_rejected_with_a_message():
    from moge_amd import _lib as L
    lib = L.lib
    n = C.c_int64(7)
    buf = (C.c_int64 * 64)()
    p = C.addressof(buf)                     # host scratch stands in for device memory: nothing is launched, so nothing dereferences it
    assert lib.moge_pano_merge_workspace(8, 4, 1, None) == INVALID and "null" in last_error(L)
    for w, h in ((0, 4), (4, 0), (-3, 4), (32768, 32768), (2 ** 31 - 1, 2), (1 << 29, 2)):
        assert lib.moge_pano_merge_workspace(w, h, 1, C.byref(n)) == INVALID, (w, h)
        assert n.value == 0 and "2^29" in last_error(L)
        # the same sizes through the working calls: rejected by the size check, which comes before any pointer is looked at
        assert lib.moge_pano_system(w, h, None, None, 1, 4, 4, None, None, None, None, None, None, None) == INVALID and "moge_pano_system" in last_error(L)
        assert lib.moge_pano_lsmr(w, h, None, None, None, 1e-5, 1e-5, 1e8, 0, 32, None, None, None, None) == INVALID and "moge_pano_lsmr" in last_error(L)
        assert lib.moge_test_pano_apply(w, h, None, 0, None, None, None) == INVALID and "moge_test_pano_apply" in last_error(L)
        assert lib.moge_pano_finish(p, p, h, w, p, None) == INVALID and "moge_pano_finish" in last_error(L)
        assert lib.moge_pano_resize_bilinear(p, h, w, 4, 4, p, None) == INVALID and lib.moge_pano_resize_bilinear(p, 4, 4, h, w, p, None) == INVALID
        assert lib.moge_pano_resize_nearest(p, h, w, 4, 4, p, None) == INVALID and lib.moge_pano_resize_nearest(p, 4, 4, h, w, p, None) == INVALID
        assert lib.moge_pano_split(p, 1, h, w, p, p, 1, 8, p, None) == INVALID and "moge_pano_split" in last_error(L)
    for views in (-1, 17):
        assert lib.moge_pano_merge_workspace(8, 4, views, C.byref(n)) == INVALID and "views" in last_error(L)
    for views in (0, 17):
        assert lib.moge_pano_system(8, 4, p, p, views, 4, 4, p, p, p, p, p, p, None) == INVALID and "views" in last_error(L)
        assert lib.moge_pano_split(p, 1, 4, 8, p, p, views, 8, p, None) == INVALID and "views" in last_error(L)
    assert lib.moge_pano_system(8, 4, p, p, 1, 0, 4, p, p, p, p, p, p, None) == INVALID and "view sizes" in last_error(L)
    assert lib.moge_pano_split(p, 1, 4, 8, p, p, 1, 0, p, None) == INVALID and "resolution" in last_error(L)

    # good sizes, null pointers
    def system(**kw):
        a = dict(distance=p, masks=p, E=p, K=p, ws=p, b=p, rows=p, seen=p)
        a.update(kw)
        return lib.moge_pano_system(8, 4, a["distance"], a["masks"], 1, 4, 4, a["E"], a["K"], a["ws"], a["b"], a["rows"], a["seen"], None)
    for k in ("distance", "masks", "E", "K", "ws", "b", "rows", "seen"):
        assert system(**{k: None}) == INVALID and "null" in last_error(L), k

    def solve(b=p, rows=p, ws=p, x=p, info=p, atol=1e-5, conlim=1e8, maxiter=0, poll=32):
        return lib.moge_pano_lsmr(8, 4, b, rows, None, atol, 1e-5, conlim, maxiter, poll, ws, x, info, None)
    for k in ("b", "rows", "ws", "x", "info"):
        assert solve(**{k: None}) == INVALID and "null" in last_error(L), k
    assert solve(poll=0) == INVALID and "poll" in last_error(L)
    assert solve(maxiter=-1) == INVALID and "maxiter" in last_error(L)
    assert solve(atol=-1.0) == INVALID and solve(atol=float("nan")) == INVALID and solve(conlim=-1.0) == INVALID and "atol" in last_error(L)
    assert lib.moge_pano_split(None, 1, 4, 8, p, p, 1, 8, p, None) == INVALID and "null" in last_error(L)
    assert lib.moge_pano_split(p, 1, 4, 8, None, p, 1, 8, p, None) == INVALID and lib.moge_pano_split(p, 1, 4, 8, p, p, 1, 8, None, None) == INVALID
    assert lib.moge_pano_resize_bilinear(None, 4, 4, 8, 8, p, None) == INVALID and lib.moge_pano_resize_bilinear(p, 4, 4, 8, 8, None, None) == INVALID
    assert lib.moge_pano_resize_nearest(None, 4, 4, 8, 8, p, None) == INVALID and lib.moge_pano_resize_nearest(p, 4, 4, 8, 8, None, None) == INVALID
    assert lib.moge_pano_log(None, 4, p, None) == INVALID and lib.moge_pano_log(p, 4, None, None) == INVALID and "null" in last_error(L)
    assert lib.moge_pano_log(p, -1, p, None) == INVALID and "2^29" in last_error(L)
    assert lib.moge_pano_finish(p, None, 4, 8, p, None) == INVALID and "null" in last_error(L)
    assert lib.moge_pano_finish(None, p, 4, 8, None, None) == INVALID and "nothing to write" in last_error(L)
    assert lib.moge_test_pano_apply(8, 4, None, 0, p, p, None) == INVALID and "null" in last_error(L)
    assert lib.moge_test_pano_apply(8, 4, p, 2, p, p, None) == INVALID and "transpose" in last_error(L)


def test_python_surface_refuses_cpu_tensors_and_bad_shapes():
    import torch
    import moge_amd.panorama_gpu as G
    from moge_amd.panorama import get_panorama_cameras
    E, Ks = get_panorama_cameras()
    d, m = torch.ones(12, 8, 8), torch.ones(12, 8, 8, dtype=torch.bool)
    with pytest.raises(RuntimeError, match="GPU tensors only"):
        G.merge_panorama_depth(16, 8, d, m, E, Ks)
    with pytest.raises(RuntimeError, match="GPU tensors only"):
        G.merge_system(16, 8, d, m, E, Ks)
    with pytest.raises(RuntimeError, match="GPU tensors only"):
        G.split_panorama_image(torch.zeros(8, 16, 3, dtype=torch.uint8), E, Ks, 8)
    with pytest.raises(RuntimeError, match="GPU tensors only"):
        G.infer_panorama(None, torch.zeros(8, 16, 3, dtype=torch.uint8))
    with pytest.raises(ValueError, match="n == 0"):
        G.merge_panorama_depth(16, 8, [], [], [], [])
    with pytest.raises(ValueError):
        G.merge_panorama_depth(16, 8, np.ones((12, 8, 8), np.float32), m, E, Ks)


@pytest.mark.parametrize("width,height,res", [(72, 36, 24), (264, 132, 40)])
def test_merge_system_then_lsmr_is_merge_panorama_depth_bit_for_bit(width, height, res):
    """The refactor changes no result: the helper plus the solve, written out here, give the bits of the public function (one level at 72 x 36;
    at 264 x 132 the coarse-to-fine start runs, and the fine level's system is the one `merge_system(264, 132, ...)` returns)."""
    from scipy.sparse.linalg import lsmr
    import make_panorama_golden as MG
    from moge_amd import panorama as P
    E, Ks, dist, masks = MG.merge_inputs(P, res, seed=width)
    want, want_seen = P.merge_panorama_depth(width, height, dist, masks, E, Ks)
    x0 = None
    if max(width, height) > 256:
        *_, A, b = P.merge_system(width // 2, height // 2, dist, masks, E, Ks)
        coarse = np.exp(lsmr(A, b, atol=1e-5, btol=1e-5)[0]).reshape(height // 2, width // 2).astype(np.float32)
        x0 = np.log(P._resize_bilinear(coarse, height, width)).reshape(-1).astype(np.float64)
    bx, by, bl, rx, ry, rl, seen, A, b = P.merge_system(width, height, dist, masks, E, Ks)
    assert bx.shape == bl.shape == (height, width) and by.shape == (height - 1, width) and seen.shape == (height, width)
    assert rx.shape == rl.shape == (width * height,) and ry.shape == ((height - 1) * width,)
    n_rows = int(rx.sum() + ry.sum() + ry[np.arange(height - 1) * width].sum() + rl.sum())
    assert A.shape == (n_rows, width * height) and b.shape == (n_rows,) and A.dtype == b.dtype == np.float64
    got = np.exp(lsmr(A, b, atol=1e-5, btol=1e-5, x0=x0)[0]).reshape(height, width).astype(np.float32)
    assert np.array_equal(got, want) and np.array_equal(seen, want_seen)
