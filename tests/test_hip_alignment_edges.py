"""GPU: every kernel of csrc/alignment.hip at the row lengths where its launch form, its padding or its striding changes, against the plain numpy
references (oracle/alignment_oracle.py, tests/alignment_trunc_reference.py with direct sums) on exactly representable data
(tests/alignment_fixtures.py: every ratio, clipping edge, product and float64 sum is exact, so the summation order cannot matter and a tie is a real
tie).  The gate is EQUALITY: the reference's index, the reference's `a` bit for bit (uint32), loss == float32(reference's float64 loss).  That it is
fair to the kernel's closed-form objective is shown on the CPU (tests/test_alignment_edges_cpu.py).  Output buffers handed to the C ABI are filled
with NaN (int32: -7) and carry guard entries behind the last row, which must come back untouched.

Cases, as run on an MI355X (158 passed, 5.1 s for the module, numpy references included; slowest case 0.7 s; profiles/alignment_edges_tests.log):
  align_trunc_kernel     53 (row length, trunc) cases over the 28 lengths of TRUNC_EDGES (trunc 0.75: many extrema, 4.0: few; 0.75 up to 5462), 7 / 5 / 1 rows
                         on the packed path and 3 elsewhere, one 259-row case at the first staged length, 64 single-element random rows: 111 launches, 508 rows
  align_l1_kernel        18 lengths of L1_EDGES x (dyadic, random), five special rows at n = 5 and 1025, 64 random rows at n = 1 and 2: 40 launches, 246 rows
  anchored entries       6 (n, d, mask) cases x (l1, trunc 0.75, trunc 4.0), six anchors each: 18 launches, 108 rows
  align_select_kernel    rows 0, 1, 255, 256, 257, 1000 and four one-lane cases, batch 3 with an empty element: 10 launches
  align_lstsq_kernel     8 lengths x (weighted, unweighted) x (dyadic: bit equality; random: one float32 ulp), 3 rows each: 32 launches, 96 rows
  solvers                align_depth_affine, align_points_scale_z_shift, align_points_scale_xyz_shift at n = 1, 2, 9, 64, with and without trunc, B = 3: 24 calls
Worst error / bound of the two toleranced gates (`pytest -s` prints the table of the run at hand):
  random-family l1 loss (bound 1e-5 relative with a floor of 1e-3, the gate of test_align_l1_matches_oracle_bitwise_on_distinct_ratios): < 0.00005 of the bound in all
      54 rows (with the residual rounded as the reference rounds it the float32 terms are the oracle's; before that fix 1.64 at n = 1)
  random-family lstsq (bound 2^-23 |ref|: the final float32 rounding; float64 sums against np.longdouble; conditioning det / (n sum u^2) >= 0.1 asserted): 0.474

Out of scope: NaN and infinite inputs (the kernels map a NaN ratio to +inf, numpy sorts NaN after +inf: the two orders are not comparable element
for element) and align_depth_affine_irls (not mirrored).  EXPERIMENTS.md R7.3 has the table of the six one-line kernel mutations (dropped index
tie-break of the sort, reversed tie rule of the truncated solve, `<` for `<=` in the right-derivative search and in the row selection, `>` for `>=`
in the weighted median, swapped signs of the clipped count) and the cases that caught each."""
import numpy as np
import pytest
import torch

from oracle import alignment_oracle as AO
from tests import alignment_fixtures as AF
from tests import alignment_trunc_reference as R

pytestmark = pytest.mark.gpu

F = np.float32
EPS = 1e-7
GUARD = 4
COUNT = {}
WORST = {}


@pytest.fixture(scope="module")
def A():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from moge_amd import alignment
    yield alignment
    print("\ncomparisons per kernel:")
    for k in sorted(COUNT):
        print(f"  {k:24s} {COUNT[k][0]:5d} launches, {COUNT[k][1]:6d} rows")
    print("worst error / bound of the toleranced gates:")
    for k in sorted(WORST):
        print(f"  {k:24s} {WORST[k]:.4f}")


# ------------------------------------------------------------------------------------------------------------------ calling the C ABI
def dev(a):
    return torch.from_numpy(np.array(a)).cuda()                  # a copy: the shared references are read-only


def _outs(rows):
    a = torch.full((rows + GUARD,), float("nan"), device="cuda")
    return a, a.clone(), torch.full((rows + GUARD,), -7, device="cuda", dtype=torch.int32)


def _back(outs, rows, what):
    a, loss, index = (o.cpu().numpy() for o in outs)
    assert np.isnan(a[rows:]).all() and np.isnan(loss[rows:]).all() and np.all(index[rows:] == -7), ("wrote past the last row", what)
    return a[:rows], loss[:rows], index[:rows]


def run_trunc(A, x, y, w, trunc):
    from moge_amd import _lib as L
    rows, n = x.shape
    xd, yd, wd = dev(x), dev(y), dev(w)
    ws = A._trunc_workspace(n, rows, xd.device)
    outs = _outs(rows)
    L.check(L.lib.moge_align_trunc(L.ptr(xd), L.ptr(yd), L.ptr(wd), rows, n, trunc, EPS, L.ptr(ws), *(L.ptr(o) for o in outs), L.stream_ptr(xd.device)))
    return _back(outs, rows, ("align_trunc", rows, n, trunc))


def run_l1(x, y, w):
    from moge_amd import _lib as L
    rows, n = x.shape
    xd, yd, wd = dev(x), dev(y), dev(w)
    outs = _outs(rows)
    L.check(L.lib.moge_align_l1(L.ptr(xd), L.ptr(yd), L.ptr(wd), rows, n, EPS, *(L.ptr(o) for o in outs), L.stream_ptr(xd.device)))
    return _back(outs, rows, ("align_l1", rows, n))


def run_anchored(A, src, tgt, w, mask, rb, rk, trunc):
    from moge_amd import _lib as L
    _, n, d = src.shape
    rows = len(rb)
    sd, td, wd, rbd, rkd = dev(src), dev(tgt), dev(w), dev(np.asarray(rb, np.int32)), dev(np.asarray(rk, np.int32))
    outs = _outs(rows)
    st = L.stream_ptr(sd.device)
    if trunc is None:
        L.check(L.lib.moge_align_l1_anchored(L.ptr(sd), L.ptr(td), L.ptr(wd), n, d, mask, L.ptr(rbd), L.ptr(rkd), rows, EPS, *(L.ptr(o) for o in outs), st))
    else:
        ws = A._trunc_workspace(n * d, rows, sd.device)
        L.check(L.lib.moge_align_trunc_anchored(L.ptr(sd), L.ptr(td), L.ptr(wd), n, d, mask, L.ptr(rbd), L.ptr(rkd), rows, trunc, EPS, L.ptr(ws),
                                                *(L.ptr(o) for o in outs), st))
    return _back(outs, rows, ("anchored", n, d, mask, trunc))


def same(kernel, got, ref, what):
    """index equal, `a` equal as bits, loss == float32(reference loss); prints what it compares first."""
    (a, loss, index), (ra, rloss, rindex) = got, ref
    ra, rloss, rindex = np.asarray(ra, F), np.asarray(rloss).astype(F), np.asarray(rindex, np.int64)
    c = COUNT.setdefault(kernel, [0, 0])
    c[0], c[1] = c[0] + 1, c[1] + len(ra)
    bad = np.nonzero((index != rindex) | (a.view(np.uint32) != ra.view(np.uint32)) | (loss.view(np.uint32) != rloss.view(np.uint32)))[0]
    head = slice(0, 8)
    print(f"{kernel} {what}: {len(ra)} rows, index {index[head].tolist()} ref {rindex[head].tolist()}, a {a[head].tolist()} ref {ra[head].tolist()}, "
          f"loss {loss[head].tolist()} ref {rloss[head].tolist()}; rows that differ: {bad.tolist()}")
    assert np.array_equal(index, rindex), (kernel, what, "index", bad.tolist(), index[bad].tolist(), rindex[bad].tolist())
    assert np.array_equal(a.view(np.uint32), ra.view(np.uint32)), (kernel, what, "a", bad.tolist(), a[bad].tolist(), ra[bad].tolist())
    assert np.array_equal(loss.view(np.uint32), rloss.view(np.uint32)), (kernel, what, "loss", bad.tolist(), loss[bad].tolist(), rloss[bad].tolist())


# ------------------------------------------------------------------------------------------------------------------ (a) align_trunc_kernel
@pytest.mark.parametrize("n,trunc", AF.TRUNC_CASES)
def test_align_trunc_edges(A, n, trunc):
    """Every first / last row length of a (path, NP) pair.  Path 0 packs four rows per workgroup: 7 rows leave one tail slot, 5 rows three, 1 row three
    in the only workgroup; a tail slot repeats the last row and must write nothing (guard entries)."""
    c = AF.trunc_case(n, trunc)
    path, np_ = AF.trunc_plan(n)
    ref = (c["a"], c["loss"], c["index"])
    same("align_trunc", run_trunc(A, c["x"], c["y"], c["w"], trunc), ref, f"n={n} trunc={trunc} path={path} NP={np_}")
    if path == 0:
        for rows in (5, 1):
            same("align_trunc", run_trunc(A, c["x"][:rows], c["y"][:rows], c["w"][:rows], trunc), tuple(v[:rows] for v in ref),
                 f"n={n} trunc={trunc} path=0 first {rows} rows alone")


def test_align_trunc_scratch_slots_reused(A):
    """259 rows at the first staged length: 256 scratch slots, rows 256 .. 258 run second in slots 0 .. 2.  The reference solves rows 0, 255 .. 258;
    every row must name an element whose ratio is the returned `a` and return the objective at it, and two runs must give the same bits."""
    n, rows, trunc = 2289, 259, 0.75
    assert AF.trunc_plan(n) == (2, 8192) and AF.trunc_plan(n - 1)[0] == 1
    x, y, w = AF.dyadic_rows(rows, n, 99)
    got = run_trunc(A, x, y, w, trunc)
    again = run_trunc(A, x, y, w, trunc)
    sel = [0, 255, 256, 257, 258]
    same("align_trunc", tuple(v[sel] for v in got), R.align_trunc(x[sel], y[sel], w[sel], trunc, sweep=False), f"n={n} rows {sel} of {rows}")
    a, loss, index = got
    xs, ys, ws, _, _, Ak, _, _ = R.keys(x, y, w, trunc)
    print(f"all {rows} rows: index range {index.min()} .. {index.max()}, distinct a {len(np.unique(a))}")
    assert index.min() >= 0 and index.max() < n
    assert np.array_equal(Ak[np.arange(rows), index].view(np.uint32), a.view(np.uint32))
    assert np.array_equal(R.objective(a, xs, ys, ws, trunc).astype(F), loss)
    for u, v in zip(got, again):
        assert np.array_equal(u.view(np.uint32), v.view(np.uint32))


# ------------------------------------------------------------------------------------------------------------------ (b) align_l1_kernel
@pytest.mark.parametrize("n", AF.L1_EDGES)
def test_align_l1_edges_dyadic(A, n):
    """NP = max(1024, pow2 >= n), NP / 1024 consecutive sorted positions per thread: around every doubling, heavy ties."""
    c = AF.l1_case(n, "dyadic")
    same("align_l1", run_l1(c["x"], c["y"], c["w"]), (c["a"], c["loss"], c["index"]), f"n={n} dyadic")


@pytest.mark.parametrize("n", AF.L1_EDGES)
def test_align_l1_edges_random(A, n):
    """The random family and the gate of test_align_l1_matches_oracle_bitwise_on_distinct_ratios: index and a equal, loss within 1e-5."""
    c = AF.l1_case(n, "random")
    a, loss, index = run_l1(c["x"], c["y"], c["w"])
    err = np.abs(loss.astype(np.float64) - c["loss"]) / np.maximum(np.abs(c["loss"].astype(np.float64)), 1e-3)
    cnt = COUNT.setdefault("align_l1 (random)", [0, 0])
    cnt[0], cnt[1] = cnt[0] + 1, cnt[1] + len(a)
    WORST["l1 random loss"] = max(WORST.get("l1 random loss", 0.0), float(err.max()) / 1e-5)
    print(f"align_l1 n={n} random: index {index.tolist()} ref {c['index'].tolist()}, a {a.tolist()} ref {c['a'].tolist()}, loss error / bound {err.max() / 1e-5:.4f}")
    assert np.array_equal(index, c["index"])
    assert np.array_equal(a, c["a"])
    assert float(err.max()) <= 1e-5


@pytest.mark.parametrize("n", [5, 1025])
def test_align_l1_special_rows(A, n):
    x, y, w = (np.repeat(v, 5, 0).copy() for v in AF.dyadic_rows(1, n, 40 + n, tiny=0.0))
    x[0] = 0                                                     # all x zero: every ratio is (+-)0, nothing has weight: the first element
    w[1] = 0                                                     # all w zero: the derivative is 0 everywhere, the smallest ratio, first index among equals
    k = n // 2 + 1
    w[2] = 0; w[2, k] = 0.5; x[2, k] = -2.0                      # one positive weight only (x < 0: the sign flip)
    x[3] = np.where(x[3] == 0, 1, x[3]); y[3] = 1.5 * x[3]       # all ratios equal: the sort must keep the index order, the median is found by weight alone
    x[4] = np.where(np.arange(n) % 3 == 0, -1, 1); y[4] = x[4] * (n - np.arange(n)) * 0.5      # strictly descending ratios: the sort reverses the row
    x, y, w = (v.astype(F) for v in (x, y, w))
    ref = AO.align(x, y, w)
    assert ref[2][0] == 0 and ref[0][1] == ((y * np.sign(x)) / np.maximum(np.abs(x), F(EPS)))[1].min() and ref[2][2] == k and ref[0][3] == 1.5
    same("align_l1", run_l1(x, y, w), ref, f"n={n} special rows (x = 0, w = 0, one weight, equal ratios, descending)")


@pytest.mark.parametrize("n", [1, 2])
def test_loss_terms_round_as_the_reference(A, n):
    """Random rows of one or two elements: the loss is one float32 term w |a x - y|, or the float64 sum of two (one addition: no order), so it must be
    the reference's bits although the data is not exact.  The element that is fit exactly leaves pure rounding noise: a x is rounded to float before
    y is subtracted (two torch ops in the reference), and a kernel that fuses the two into an fma returns noise of another size (it did: at n = 1 the
    1e-5 gate of the random family was missed by 1.64x before align_residual)."""
    x, y, w = AF.random_rows(64, n, 77 + n)
    assert np.abs(x).min() > 1e-4
    same("align_l1", run_l1(x, y, w), AO.align(x, y, w), f"n={n} random, single terms")
    if n == 1:            # (two elements: both candidates often cost trunc + noise, and direct sums and closed form may split that near-tie differently)
        same("align_trunc", run_trunc(A, x, y, w, 0.5), R.align_trunc(x, y, w, 0.5, sweep=False), f"n={n} trunc=0.5 random, single terms")


# ------------------------------------------------------------------------------------------------------------------ (c) anchored entries
ANCHORED = [(7, 3, 0b111), (191, 3, 0b100), (763, 3, 0b111), (572, 1, 0b1), (573, 1, 0b1), (342, 3, 0b100)]      # NE = 21, 573, 2289, 572, 573, 1026


@pytest.mark.parametrize("trunc", [None, 0.75, 4.0])
@pytest.mark.parametrize("n,d,mask", ANCHORED)
def test_anchored_entries(A, n, d, mask, trunc):
    """moge_align_l1_anchored / moge_align_trunc_anchored form the residual row while loading (sample minus anchor in the masked components); the
    reference forms it in numpy as AO._anchored and R._anchor do and solves the plain row."""
    src, tgt, w = AF.dyadic_points(2, n, d, 100 * n + d)
    rng = np.random.default_rng(n)
    rb = np.array([0, 1, 0, 1, 0, 1])
    rk = np.array([0, n - 1, np.nonzero(w[0] == 0)[0][0], rng.integers(n), rng.integers(n), rng.integers(n)])
    assert w[0, rk[2]] == 0 and set(rb) == {0, 1}
    m = np.array([(mask >> c) & 1 for c in range(d)], F)
    xs = (src[rb] - (src[rb, rk] * m)[:, None, :]).reshape(len(rb), -1)
    ys = (tgt[rb] - (tgt[rb, rk] * m)[:, None, :]).reshape(len(rb), -1)
    ws = np.repeat(w[rb], d, axis=1)
    ref = AO.align(xs, ys, ws) if trunc is None else R.align_trunc(xs, ys, ws, trunc, sweep=False)
    kernel = "l1_anchored" if trunc is None else "trunc_anchored"
    same(kernel, run_anchored(A, src, tgt, w, mask, rb, rk, trunc), ref, f"n={n} d={d} mask={mask:03b} NE={n * d} trunc={trunc} anchors {rk.tolist()}")


# ------------------------------------------------------------------------------------------------------------------ (d) align_select_kernel
def run_select(loss, rb, batch):
    from moge_amd import _lib as L
    rows = len(rb)
    ld, rbd = dev(np.asarray(loss, F) if rows else np.zeros(1, F)), dev(np.asarray(rb, np.int32) if rows else np.zeros(1, np.int32))
    mn = torch.full((batch + GUARD,), float("nan"), device="cuda")
    mr = torch.full((batch + GUARD,), -7, device="cuda", dtype=torch.int32)
    L.check(L.lib.moge_align_select(L.ptr(ld), L.ptr(rbd), rows, batch, L.ptr(mn), L.ptr(mr), L.stream_ptr(ld.device)))
    mn, mr = mn.cpu().numpy(), mr.cpu().numpy()
    assert np.isnan(mn[batch:]).all() and np.all(mr[batch:] == -7)
    return mn[:batch], mr[:batch]


def check_select(loss, rb, batch, what):
    rmin, rrow = AO.scatter_min(batch, rb, loss) if len(rb) else (np.full(batch, np.inf, F), np.full(batch, -1))
    mn, mr = run_select(loss, rb, batch)
    c = COUNT.setdefault("align_select", [0, 0])
    c[0], c[1] = c[0] + 1, c[1] + len(rb)
    print(f"align_select {what}: min {mn.tolist()} ref {rmin.tolist()}, row {mr.tolist()} ref {rrow.tolist()}")
    assert np.array_equal(mn, rmin) and np.array_equal(mr, rrow)
    return mn, mr


VALUES = np.array([0.25, 0.375, 0.5, 0.75, 1.0, 1.5, 2.0, 3.0], F)


@pytest.mark.parametrize("rows", [1, 255, 256, 257, 1000])
def test_align_select(A, rows):
    """Rows stride by 256; eight loss values, so every batch element has many exact ties: the LAST row with the minimum comes back.  Batch element 1
    has no row: (+inf, -1)."""
    rng = np.random.default_rng(rows)
    loss = VALUES[rng.integers(0, 8, rows)]
    rb = rng.choice([0, 2], rows)
    mn, mr = check_select(loss, rb, 3, f"rows={rows}")
    assert mn[1] == np.inf and mr[1] == -1
    if rows >= 255:
        for b in (0, 2):
            assert (loss[rb == b] == mn[b]).sum() >= 2               # a real tie


def test_align_select_one_lane_and_no_rows(A):
    """All rows of batch element 2 in one 256-stride lane (row ids 5 mod 256): the strided pass alone decides, ties to the later row."""
    rng = np.random.default_rng(7)
    lane = np.array([5, 261, 517, 773])
    for vals, want in (([0.5, 0.5, 0.5, 0.5], 773), ([1.0, 0.5, 0.5, 1.0], 517), ([0.25, 0.5, 0.5, 1.0], 5), ([1.0, 2.0, 3.0, 0.75], 773)):
        loss = VALUES[rng.integers(0, 8, 1000)]
        rb = np.zeros(1000, np.int64)
        rb[lane] = 2
        loss[lane] = vals
        mn, mr = check_select(loss, rb, 3, f"lane 5 of batch 2 holds {vals}")
        assert mr[2] == want and mr[1] == -1
    mn, mr = check_select(np.zeros(0, F), np.zeros(0, np.int64), 3, "no rows at all")
    assert np.all(mn == np.inf) and np.all(mr == -1)


# ------------------------------------------------------------------------------------------------------------------ (e) align_lstsq_kernel
def run_lstsq(x, y, w):
    from moge_amd import _lib as L
    rows, n = x.shape
    xd, yd, wd = dev(x), dev(y), None if w is None else dev(w)
    a = torch.full((rows + GUARD,), float("nan"), device="cuda")
    b = a.clone()
    L.check(L.lib.moge_align_lstsq(L.ptr(xd), L.ptr(yd), L.ptr(wd), rows, n, L.ptr(a), L.ptr(b), L.stream_ptr(xd.device)))
    a, b = a.cpu().numpy(), b.cpu().numpy()
    assert np.isnan(a[rows:]).all() and np.isnan(b[rows:]).all()
    return a[:rows], b[:rows]


def lstsq_reference(x, y, w, dtype):
    """The kernel's normal equations from the same float32 u = sqrt(w) x, v = sqrt(w) y, summed in `dtype`.  -> a, b, det / (n sum u^2)"""
    ws = np.ones_like(x) if w is None else np.sqrt(w)
    u, v = (ws * x).astype(F).astype(dtype), (ws * y).astype(F).astype(dtype)
    n = dtype(x.shape[-1])
    suu, su, suv, sv = (u * u).sum(-1), u.sum(-1), (u * v).sum(-1), v.sum(-1)
    det = suu * n - su * su
    return (suv * n - su * sv) / det, (suu * sv - su * suv) / det, det / (n * suu)


LSTSQ_N = [2, 63, 64, 65, 1023, 1024, 1025, 4097]


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("n", LSTSQ_N)
def test_align_lstsq_dyadic(A, n, weighted):
    """x, y multiples of 1/4 in [-4, 4], w in {0, 0.25, 1, 2.25, 4} (exact square roots): the four sums, the determinant and both numerators are exact
    in float64 in any order, so a and b are the reference's bits."""
    rng = np.random.default_rng(n)
    x = (rng.integers(-16, 17, (3, n)) / 4).astype(F)
    y = (rng.integers(-16, 17, (3, n)) / 4).astype(F)
    w = rng.choice(np.array([0, 0.25, 1, 2.25, 4], F), (3, n)) if weighted else None
    x[:, 0], x[:, 1] = 1.0, -2.0                                  # two distinct u at least: det > 0
    if weighted:
        w[:, :2] = 1.0
    ra, rb, cond = lstsq_reference(x, y, w, np.float64)
    assert np.all(cond > 0)
    a, b = run_lstsq(x, y, w)
    c = COUNT.setdefault("align_lstsq", [0, 0])
    c[0], c[1] = c[0] + 1, c[1] + 3
    print(f"align_lstsq dyadic n={n} weighted={weighted}: a {a.tolist()} ref {ra.astype(F).tolist()}, b {b.tolist()} ref {rb.astype(F).tolist()}")
    assert np.array_equal(a.view(np.uint32), ra.astype(F).view(np.uint32))
    assert np.array_equal(b.view(np.uint32), rb.astype(F).view(np.uint32))


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("n", LSTSQ_N)
def test_align_lstsq_random(A, n, weighted):
    """|got - ref| <= 2^-23 |ref|: the final rounding to float32 (2^-24) and float64 summation error that is negligible at this conditioning
    (det / (n sum u^2) >= 0.1 is asserted on the inputs)."""
    rng = np.random.default_rng(1000 + n)
    x = rng.normal(0, 1, (3, n)).astype(F)
    if n == 2:
        x[:, 1] = -x[:, 0] * F(0.75)                              # two samples: keep them well apart
    y = (F(1.3) * x + F(0.2) + F(0.1) * rng.normal(0, 1, (3, n))).astype(F)
    w = rng.uniform(0.1, 1, (3, n)).astype(F) if weighted else None
    ra, rb, cond = lstsq_reference(x, y, w, np.longdouble)
    assert float(cond.min()) >= 0.1, cond
    a, b = run_lstsq(x, y, w)
    bound = 2.0 ** -23
    ea = np.abs(a.astype(np.longdouble) - ra) / (bound * np.abs(ra))
    eb = np.abs(b.astype(np.longdouble) - rb) / (bound * np.abs(rb))
    worst = float(max(ea.max(), eb.max()))
    c = COUNT.setdefault("align_lstsq (random)", [0, 0])
    c[0], c[1] = c[0] + 1, c[1] + 3
    WORST["lstsq random"] = max(WORST.get("lstsq random", 0.0), worst)
    print(f"align_lstsq random n={n} weighted={weighted}: a {a.tolist()}, b {b.tolist()}, conditioning {float(cond.min()):.3f}, error / bound {worst:.4f}")
    assert worst <= 1.0


# ------------------------------------------------------------------------------------------------------------------ (f) the solvers, small
def solver_points(n, d, seed):
    """B = 3: element 0 as generated, element 1 with exactly one positive weight, element 2 with all weights equal."""
    src, tgt, w = AF.dyadic_points(3, n, d, seed)
    w[1] = 0
    w[1, n - 1] = 0.5
    w[2] = 1.0
    return src, tgt, w


def bits(kernel, got, ref, what):
    c = COUNT.setdefault(kernel, [0, 0])
    c[0], c[1] = c[0] + 1, c[1] + 3
    for name, g, r in zip(("scale", "shift"), got, ref):
        g, r = g.detach().cpu().numpy(), np.asarray(r, F)
        print(f"{kernel} {what}: {name} {g.tolist()} ref {r.tolist()}")
        assert g.shape == r.shape and np.array_equal(g.view(np.uint32), r.view(np.uint32)), (kernel, what, name)


@pytest.mark.parametrize("trunc", [None, 0.75])
@pytest.mark.parametrize("n", [1, 2, 9, 64])
def test_solvers_small(A, n, trunc):
    """Anchor search + row selection + the recomputation from the two selected samples: scale and shift are the reference's bits (n = 1: a single
    anchor whose own residuals are all zero)."""
    src, tgt, w = solver_points(n, 3, 10 + n)
    sd, td, wd = dev(src), dev(tgt), dev(w)
    ref = AO.align_depth_affine(src[..., 2], tgt[..., 2], w) if trunc is None else R.depth_affine(src[..., 2], tgt[..., 2], w, trunc)
    bits("align_depth_affine", A.align_depth_affine(sd[..., 2].contiguous(), td[..., 2].contiguous(), wd, trunc), ref, f"n={n} trunc={trunc}")
    for name, xyz in (("align_points_scale_z_shift", False), ("align_points_scale_xyz_shift", True)):
        ref = getattr(AO, name)(src, tgt, w) if trunc is None else R.points_affine(src, tgt, w, trunc, xyz)
        bits(name, getattr(A, name)(sd, td, wd, trunc), ref, f"n={n} trunc={trunc}")
