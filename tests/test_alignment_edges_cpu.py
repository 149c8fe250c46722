"""CPU: what tests/test_hip_alignment_edges.py rests on.
  - tests/alignment_fixtures.trunc_plan / trunc_layout_bytes restate the launch-form choice of csrc/alignment.hip: held to the path table and, through
    moge_align_trunc_workspace (which loads without a GPU), to the C++ layout byte for byte.
  - On the dyadic rows of the GPU sweep the reference's direct sums (sweep=False) and the kernel's closed form (sweep=True) give the same index and the
    same float64 loss: the exact-equality gate is fair to the kernel.  The rows hold what the gate is there for: extrema that tie for the smallest
    objective (n >= 22) and TR_DIRECT elements (n >= 171).
  - The float64 prefix sums AO.align decides with are exact on those rows (math.fsum of the same prefix), so the summation order cannot matter."""
import ctypes as C
import math

import numpy as np
import pytest

from oracle import alignment_oracle as AO
from tests import alignment_fixtures as AF
from tests import alignment_trunc_reference as R


def test_trunc_plan_reproduces_the_path_table():
    first, seen = [], set()
    for ne in range(1, AF.ALIGN_MAX_N + 1):
        plan = AF.trunc_plan(ne)
        if plan not in seen:
            seen.add(plan)
            first.append((ne,) + plan)
    assert first == AF.TRUNC_TABLE
    # every first length and the one before it are in the sweep
    for ne, _, _ in AF.TRUNC_TABLE:
        assert ne in AF.TRUNC_EDGES and (ne == 1 or ne - 1 in AF.TRUNC_EDGES)
    assert AF.trunc_plan(10923)[1] == 1 << 16          # event ids fill the whole unsigned short


def test_layout_matches_the_library():
    """moge_align_trunc_workspace is 0 on the LDS paths and layout bytes * min(rows, 256 slots) on the staged path."""
    from moge_amd import _lib as L
    b = C.c_int64(-1)
    staged = 0
    for n in AF.TRUNC_EDGES:
        path, np_ = AF.trunc_plan(n)
        for rows in (1, 256, 257):
            assert L.lib.moge_align_trunc_workspace(n, rows, C.byref(b)) == 0
            want = AF.trunc_layout_bytes(n, np_) * min(rows, AF.TRUNC_SLOTS) if path == 2 else 0
            assert b.value == want, (n, rows, path, b.value, want)
        staged += path == 2
    assert staged == 8
    # the 572 / 573 edge (path 0 -> 1) does not show in the workspace; it is the layout's arithmetic against the LDS budget
    assert AF.trunc_layout_bytes(572, 2048) * 4 == AF.TRUNC_LDS_BYTES and AF.trunc_layout_bytes(573, 2048) * 4 > AF.TRUNC_LDS_BYTES
    assert AF.trunc_layout_bytes(2288, 8192) <= AF.TRUNC_LDS_BYTES < AF.trunc_layout_bytes(2289, 8192)


def test_dyadic_generators():
    x, y, w = AF.dyadic_rows(7, 4000, 1)
    for v in (x, y, w):
        assert v.dtype == np.float32
    m, e = np.frexp(np.abs(x[x != 0]))
    assert np.all(m == 0.5) and set(np.unique(e - 1)) == {-1, 0, 1, 2}
    assert 0.03 < (x == 0).mean() < 0.07 and 0.2 < (x < 0).mean() / (x != 0).mean() < 0.3
    assert np.all(y * 8 == np.round(y * 8)) and np.abs(y).max() <= 6.0
    assert set(np.unique(w)) == {0.0, 2.0 ** -30, 0.25, 0.5, 1.0, 2.0}
    reg, zero, direct = AF.classes(x, y, w)
    assert direct.sum() > 300 and np.all(w[direct] == np.float32(2.0 ** -30))
    src, tgt, pw = AF.dyadic_points(3, 64, 3, 2)
    assert src.shape == tgt.shape == (3, 64, 3) and pw.shape == (3, 64)
    diff = (src[:, :, None] - src[:, None]).astype(np.float64)              # anchor subtraction: exact, and again a signed power of two or 0
    assert np.array_equal(diff, src[:, :, None].astype(np.float64) - src[:, None].astype(np.float64))
    m, _ = np.frexp(np.abs(diff[diff != 0]))
    assert np.all(m == 0.5)
    assert np.all((pw > 0).any(1)) and np.all((pw == 0).any(1))


@pytest.mark.parametrize("n,trunc", AF.TRUNC_CASES)
def test_direct_sums_equal_the_closed_form(n, trunc):
    c = AF.trunc_case(n, trunc)
    a, loss, index = R.align_trunc(c["x"], c["y"], c["w"], trunc, sweep=True)
    assert np.array_equal(index, c["index"]), (index, c["index"])
    assert np.array_equal(loss, c["loss"])                                   # float64, bit for bit
    assert np.array_equal(a.view(np.uint32), c["a"].view(np.uint32))
    direct = int(AF.classes(c["x"], c["y"], c["w"])[2].sum())
    if n >= 171:
        assert direct >= 1
    if 22 <= n <= AF.TRUNC_MANY_MAX_N:                                       # above: the tie count would cost the (extrema, n) block a second time
        ties = AF.minimum_ties(c["x"], c["y"], c["w"], trunc)
        assert max(ties) >= 2, ties
        assert any(t >= 2 and c["index"][r] > 0 for r, t in enumerate(ties))


def test_long_rows_tie_too():
    """n > 5462 (trunc 4.0 only): the winning ratio is shared by many elements, all of them extrema with the same objective; the last one wins."""
    for n in (10922, 10923, 15360):
        c = AF.trunc_case(n, 4.0)
        xs, ys, ws, wx, wy, A, B, Cc = R.keys(c["x"], c["y"], c["w"], 4.0)
        for r in range(len(A)):
            same = np.nonzero(A[r] == c["a"][r])[0]
            ext = R.extrema(A[r], B[r], Cc[r], wx[r])
            assert len(same) >= 2 and ext[same].all() and c["index"][r] == same[-1]


@pytest.mark.parametrize("n", AF.L1_EDGES)
def test_l1_prefix_sums_are_exact(n):
    c = AF.l1_case(n, "dyadic")
    x, y, w = c["x"], c["y"], c["w"]
    s = np.sign(x)
    ratio = (y * s) / np.maximum(x * s, np.float32(1e-7))
    for r in range(x.shape[0]):
        order = np.argsort(ratio[r], kind="stable")
        wx = (x[r] * s[r] * w[r])[order]
        cum = np.cumsum(wx, dtype=np.float64)
        pos = int(np.nonzero(order == c["index"][r])[0][0])
        for p in {pos, max(pos - 1, 0), n - 1}:
            assert cum[p] == math.fsum(float(v) for v in wx[:p + 1])
        total = cum[-1]
        assert 2 * cum[pos] - total >= 0 and (pos == 0 or 2 * cum[pos - 1] - total < 0)
        terms = (w[r] * np.abs(c["a"][r] * x[r] * s[r] - y[r] * s[r])).astype(np.float32)
        assert c["loss"][r] == np.float32(math.fsum(float(v) for v in terms))
