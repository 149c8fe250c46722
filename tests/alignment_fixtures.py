"""Deterministic inputs shared by tests/test_alignment_edges_cpu.py and tests/test_hip_alignment_edges.py, and the Python restatement of how
csrc/alignment.hip chooses a launch form from the row length.  Nothing here needs a GPU.

Exactly representable ("dyadic") data: x and w are signed powers of two (or zero), y small dyadic numbers.  Every ratio y / x, every clipping edge
(w y -+ trunc) / (w x), every product w x, w y, every term w |a x - y| is then exact in float32, and every sum of them needs far fewer than 53 bits
(granularity >= 2^-34, magnitude < 2^18), so it is exact in float64 in ANY order.  A kernel and a reference that implement the same decision must then
return the same index and the same bits: no tolerance, and a tie is a real tie.  The one inexact operation is the division by eps = float32(1e-7) where
a clamp binds (x == 0: 0 / eps = 0 exactly; w x < eps: the B / C edges of a TR_DIRECT element); it is one correctly rounded float32 division on both
sides.

The path table of align_trunc_kernel (trunc_plan / trunc_layout of csrc/alignment.hip, restated below), first row length NE of every (path, NP):

    NE      path                                              NP (sorted events)
    1       0  four one-wave rows per workgroup, LDS          64
    22 / 43 / 86 / 171 / 342       0                          128 / 256 / 512 / 1024 / 2048
    573     1  one 1024-thread workgroup per row, LDS         2048
    683 / 1366                     1                          4096 / 8192
    2289    2  global scratch, 256 slots                      8192
    2731 / 5462 / 10923            2                          16384 / 32768 / 65536
"""
import functools

import numpy as np

from oracle import alignment_oracle as AO
from tests import alignment_trunc_reference as R

F = np.float32

# ---- csrc/alignment.hip: TruncLayout, trunc_layout, trunc_plan --------------------------------------------------------------------------------------
TRUNC_LDS_BYTES = 160 * 1024 - 1024          # dynamic LDS of one workgroup
TRUNC_SMALL_TPR, TRUNC_SMALL_RPW = 64, 4     # path 0: one wave per row, four rows per workgroup
TRUNC_THREADS = 1024                         # paths 1 and 2: one 1024-thread workgroup per row
TRUNC_SLOTS = 256                            # path 2: workgroups in flight, one scratch slot each
ALIGN_MAX_N = 15360

# first NE of every (path, NP), as the issue tabulates it; tests/test_alignment_edges_cpu.py holds trunc_plan to it
TRUNC_TABLE = [(1, 0, 64), (22, 0, 128), (43, 0, 256), (86, 0, 512), (171, 0, 1024), (342, 0, 2048), (573, 1, 2048), (683, 1, 4096), (1366, 1, 8192),
               (2289, 2, 8192), (2731, 2, 16384), (5462, 2, 32768), (10923, 2, 65536)]

TRUNC_EDGES = [1, 2, 3, 21, 22, 42, 43, 85, 86, 170, 171, 341, 342, 572, 573, 682, 683, 1365, 1366, 2288, 2289, 2730, 2731, 5461, 5462, 10922, 10923, 15360]
L1_EDGES = [1, 2, 3, 63, 64, 65, 1023, 1024, 1025, 2047, 2048, 2049, 4096, 4097, 8192, 8193, 15359, 15360]
TRUNCS = [0.75, 4.0]                         # many extrema / few
TRUNC_MANY_MAX_N = 5462                      # above it trunc = 0.75 is left out: the reference's (extrema, n) block stays below ~200 MB per row
TRUNC_CASES = [(n, t) for n in TRUNC_EDGES for t in TRUNCS if t == 4.0 or n <= TRUNC_MANY_MAX_N]


def _al(b):
    return (b + 15) & ~15


def trunc_layout_bytes(ne, np_):
    """One row's workspace: float64 prefix [NP + 1], float64 objective [NE], float32 keys [NP], float32 A / wx / wy [NE] each, uint16 event ids [NP],
    class bytes [NE]; every section rounded up to 16 bytes."""
    return _al((np_ + 1) * 8) + _al(ne * 8) + _al(np_ * 4) + 3 * _al(ne * 4) + _al(np_ * 2) + _al(ne)


def trunc_plan(ne):
    """-> (path, NP).  NP = pow2 >= 3 NE with a floor of 64 on path 0 (one event per lane at least) and of 1024 on paths 1 and 2."""
    np_ = 1
    while np_ < 3 * ne:
        np_ <<= 1
    small = max(np_, TRUNC_SMALL_TPR)
    if trunc_layout_bytes(ne, small) * TRUNC_SMALL_RPW <= TRUNC_LDS_BYTES:
        return 0, small
    big = max(np_, TRUNC_THREADS)
    return (1 if trunc_layout_bytes(ne, big) <= TRUNC_LDS_BYTES else 2), big


def trunc_rows(n):
    """Rows of the sweep: 7 on path 0 (four rows per workgroup: the second workgroup has three live slots and one tail slot, which repeats row 6
    and must write nothing; the GPU test also runs the first 5 rows alone, one live slot and three tail slots), 3 on paths 1 and 2."""
    return 7 if trunc_plan(n)[0] == 0 else 3


# ---- data -------------------------------------------------------------------------------------------------------------------------------------------
def dyadic_rows(rows, n, seed, tiny=0.02):
    """x = +-2^k (k in -1..2, a quarter negative, 5 % zeros), y = j / 2 + 0.75 x (integer j in [-6, 6]: the skew keeps the weighted median off 0),
    w = 2^k (k in -2..1, 10 % zeros); a `tiny` fraction of w is 2^-30, so that w x < eps with x >= eps: the kernel's TR_DIRECT class."""
    rng = np.random.default_rng(seed)
    x = np.ldexp(1.0, rng.integers(-1, 3, (rows, n)))
    x *= np.where(rng.random((rows, n)) < 0.25, -1.0, 1.0)
    x[rng.random((rows, n)) < 0.05] = 0.0
    y = rng.integers(-6, 7, (rows, n)) / 2 + 0.75 * x
    w = np.ldexp(1.0, rng.integers(-2, 2, (rows, n)))
    w[rng.random((rows, n)) < 0.10] = 0.0
    w[rng.random((rows, n)) < tiny] = 2.0 ** -30
    return x.astype(F), y.astype(F), w.astype(F)


def dyadic_points(B, n, d, seed, tiny=0.02):
    """src / tgt (B, n, d), w (B, n) for the anchored solvers.  Per (batch, component) src takes the three values {-h, 0, h} (h in 0.5, 1, 2): the
    difference of two of them is 0, +-h or +-2h, again a signed power of two, so a residual row (sample minus anchor, or the sample itself where the
    component is not anchored) is data of the dyadic_rows kind and every ratio stays exact.  tgt = j / 2 + 0.75 src.  w as in dyadic_rows; every
    batch element keeps a sample with weight > 0 and, from n = 3 on, one with weight 0."""
    rng = np.random.default_rng(seed)
    h = np.ldexp(1.0, rng.integers(-1, 2, (B, 1, d)))
    src = h * rng.integers(-1, 2, (B, n, d))
    tgt = rng.integers(-6, 7, (B, n, d)) / 2 + 0.75 * src
    w = np.ldexp(1.0, rng.integers(-2, 2, (B, n)))
    w[rng.random((B, n)) < 0.10] = 0.0
    w[rng.random((B, n)) < tiny] = 2.0 ** -30
    w[:, 0] = np.where(w[:, 0] > 0, w[:, 0], 1.0)
    if n >= 3:
        w[:, n // 2] = np.where((w == 0).any(1), w[:, n // 2], 0.0)
    return src.astype(F), tgt.astype(F), w.astype(F)


def random_rows(rows, n, seed):
    """The family of test_align_l1_matches_oracle_bitwise_on_distinct_ratios: distinct ratios, no ties."""
    rng = np.random.default_rng(seed)
    return (rng.normal(0, 1, (rows, n)).astype(F), rng.normal(0, 1, (rows, n)).astype(F), rng.uniform(0.1, 1, (rows, n)).astype(F))


def _frozen(d):
    for v in d.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return d


# ---- references, computed once per process and shared by the CPU and the GPU module -------------------------------------------------------------------
def trunc_seed(n):
    return 7000 + n


@functools.lru_cache(maxsize=None)
def trunc_case(n, trunc):
    """dyadic rows of length n and the reference's solution (direct sums, sweep=False): x, y, w, a, loss (float64), index."""
    x, y, w = dyadic_rows(trunc_rows(n), n, trunc_seed(n))
    a, loss, index = R.align_trunc(x, y, w, trunc, sweep=False)
    return _frozen(dict(x=x, y=y, w=w, a=a, loss=loss, index=index))


@functools.lru_cache(maxsize=None)
def l1_case(n, family):
    """family "dyadic" or "random": 3 rows of length n and AO.align's a, loss, index."""
    x, y, w = dyadic_rows(3, n, 3000 + n) if family == "dyadic" else random_rows(3, n, 5000 + n)
    a, loss, index = AO.align(x, y, w)
    return _frozen(dict(x=x, y=y, w=w, a=a, loss=loss, index=index))


def classes(x, y, w, eps=R.EPS):
    """The kernel's element classes on sign-flipped rows: regular (x >= eps and w x >= eps), zero (w == 0 or x == 0), direct (the rest)."""
    xs = np.abs(np.asarray(x, F))
    wx = np.asarray(w, F) * xs
    reg = (xs >= F(eps)) & (wx >= F(eps))
    zero = (np.asarray(w) == 0) | (xs == 0)
    return reg, zero, ~reg & ~zero


def minimum_ties(x, y, w, trunc):
    """Per row: how many extrema attain the smallest objective (direct float64 sums).  > 1: the tie rule decides the answer."""
    xs, ys, ws, wx, wy, A, B, C = R.keys(x, y, w, trunc)
    out = []
    for r in range(xs.shape[0]):
        ext = np.nonzero(R.extrema(A[r], B[r], C[r], wx[r]))[0]
        vals = R.objective(A[r][ext], xs[r][None], ys[r][None], ws[r][None], trunc)
        out.append(int((vals == vals.min()).sum()))
    return out
