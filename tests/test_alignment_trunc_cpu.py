"""CPU: the numpy restatement of the truncated alignment objective (tests/alignment_trunc_reference.py) against the reference's own results
(tests/golden/align_trunc_*.npz, tools/make_alignment_trunc_golden.py), the kernel's one-pass objective (sweep_objective) against direct
summation, and the host-side argument checks of moge_amd.alignment that need no GPU."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from tests import alignment_trunc_reference as R

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
OBJ_TOL = 1e-5
ONE_D = ["align_trunc_small", "align_trunc_exact", "align_trunc_zero", "align_trunc_huge", "align_trunc_many", "align_trunc_clamp"]
EXACT = ["align_trunc_exact", "align_trunc_zero", "align_trunc_clamp"]


def load(name):
    return dict(np.load(os.path.join(GOLD, name + ".npz")))


def flipped(g):
    return R.keys(g["x"], g["y"], g["w"], float(g["trunc"]))


@pytest.mark.parametrize("sweep", [False, True])
@pytest.mark.parametrize("name", ONE_D)
def test_align_trunc_golden(name, sweep):
    g = load(name)
    trunc = float(g["trunc"])
    a, loss, idx = R.align_trunc(g["x"], g["y"], g["w"], trunc, sweep=sweep)
    xs, ys, ws = flipped(g)[:3]
    ref_obj = R.objective(g["a"], xs, ys, ws, trunc)
    assert np.all(R.objective(a, xs, ys, ws, trunc) <= ref_obj * (1 + OBJ_TOL) + 1e-12)
    assert np.allclose(loss, g["loss"], rtol=1e-5, atol=1e-6)
    if name in EXACT:
        assert np.array_equal(idx, g["index"])
        assert np.array_equal(a.view(np.uint32), g["a"].view(np.uint32))


def test_fixture_coverage():
    """The fixtures reach what they are meant to: ties at the last element, an empty row, dozens of extrema, clamped w x."""
    g = load("align_trunc_exact")
    xs, ys, ws, wx, wy, A, B, C = flipped(g)
    for r in (6, 7):                                     # duplicated (x, y, w): the reference kept the last copy of the winning ratio
        same = np.nonzero(A[r] == A[r][g["index"][r]])[0]
        assert len(same) > 1 and g["index"][r] == same[-1]
    assert g["index"][8] == 0                            # no weight, no extremum: element 0
    g = load("align_trunc_many")
    xs, ys, ws, wx, wy, A, B, C = flipped(g)
    assert min(R.extrema(A[r], B[r], C[r], wx[r]).sum() for r in range(len(A))) >= 12
    g = load("align_trunc_clamp")
    xs, ys, ws, wx, wy, A, B, C = flipped(g)
    assert ((wx > 0) & (wx < R.EPS) & (xs >= R.EPS)).sum() > 50


@pytest.mark.parametrize("name", ONE_D)
def test_sweep_matches_direct_objective(name):
    """The closed form at every candidate equals the objective summed directly over the row."""
    g = load(name)
    trunc = float(g["trunc"])
    xs, ys, ws, wx, wy, A, B, C = flipped(g)
    for r in range(len(A)):
        f = R.sweep_objective(xs[r], ys[r], ws[r], wx[r], wy[r], A[r], B[r], C[r], trunc)
        d = R.objective(A[r], xs[r][None], ys[r][None], ws[r][None], trunc) if trunc > 0 else np.zeros(len(A[r]))
        scale = max(1.0, float(np.abs(d).max()))
        assert np.allclose(f, d, rtol=1e-5, atol=1e-5 * scale), (name, r)


def test_huge_trunc_is_the_weighted_median():
    g = load("align_trunc_huge")
    xs, ys, ws = flipped(g)[:3]
    l1 = lambda a: (ws * np.abs(np.asarray(a, np.float32)[:, None] * xs - ys)).sum(-1)     # noqa: E731
    cand = ys / np.maximum(xs, np.float32(R.EPS))
    best = np.min([(ws * np.abs(cand[:, [j]] * xs - ys)).sum(-1) for j in range(xs.shape[1])], axis=0)
    assert np.allclose(l1(g["a"]), best, rtol=1e-5)
    assert np.allclose(g["loss"], best, rtol=1e-5)


@pytest.mark.parametrize("name", ["align_trunc_solvers_6", "align_trunc_solvers_24"])
def test_affine_solvers_golden(name):
    g = load(name)
    trunc = float(g["trunc"])
    P, G, W = g["pred"], g["gt"], g["w"]

    def obj(s, sh, src, tgt, w):                          # the truncated objective of a (scale, shift) over a batch
        r = np.abs(np.asarray(s, np.float32)[..., None, None] * src + np.asarray(sh, np.float32)[..., None, :] - tgt) * w[..., None]
        return np.minimum(r, np.float32(trunc)).astype(np.float64).sum((-2, -1))

    s, sh = R.depth_affine(P[..., 2], G[..., 2], W, trunc)
    mine = obj(s, np.stack([0 * sh, 0 * sh, sh], -1), P * [0, 0, 1], G * [0, 0, 1], W)
    ref = obj(g["depth_affine_scale"], np.stack([0 * sh, 0 * sh, g["depth_affine_shift"]], -1), P * [0, 0, 1], G * [0, 0, 1], W)
    assert np.all(mine <= ref * (1 + OBJ_TOL) + 1e-9)
    for key, xyz in (("points_scale_z_shift", False), ("points_scale_xyz_shift", True)):
        s, sh = R.points_affine(P, G, W, trunc, xyz)
        assert np.all(obj(s, sh, P, G, W) <= obj(g[key + "_scale"], g[key + "_shift"], P, G, W) * (1 + OBJ_TOL) + 1e-9), key
        assert np.allclose(s, g[key + "_scale"], rtol=2e-3), key


def test_trunc_must_be_scalar():
    from moge_amd import alignment as A
    x = torch.ones(3, 50)
    with pytest.raises(ValueError, match="scalar"):
        A.align_trunc(x, x, x, torch.full((3, 50), 0.2))
    with pytest.raises(NotImplementedError, match="align_trunc"):        # align() stays untruncated-only
        A.align(x, x, x, 0.5)
    with pytest.raises(ValueError, match="scalar"):
        A.align_points_scale_xyz_shift(torch.ones(2, 5, 3), torch.ones(2, 5, 3), torch.ones(2, 5), torch.tensor([0.1, 0.2]))
    assert A._trunc_value(torch.tensor(0.25)) == 0.25 and A._trunc_value(torch.tensor([0.5])) == 0.5 and A._trunc_value(1) == 1.0


def test_row_limit_and_workspace():
    from moge_amd import _lib as L
    b = C.c_int64(-1)
    assert L.lib.moge_align_trunc_workspace(15361, 10, C.byref(b)) != 0
    assert b"15360" in L.lib.moge_last_error()
    assert L.lib.moge_align_trunc_workspace(0, 10, C.byref(b)) != 0
    for n, rows, staged in ((108, 10 ** 5, False), (432, 10 ** 5, False), (1728, 10 ** 4, False), (6912, 3, True), (15360, 10 ** 5, True)):
        assert L.lib.moge_align_trunc_workspace(n, rows, C.byref(b)) == 0
        assert (b.value > 0) == staged, n
        if staged:                                        # one slot per workgroup in flight, not one per row
            per_row = b.value // min(rows, 256)
            assert b.value == per_row * min(rows, 256) and per_row < 128 * n
