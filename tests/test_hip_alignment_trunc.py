"""GPU: the truncated alignment objective of moge_amd.alignment (align_trunc_kernel, csrc/alignment.hip) against the reference's own results
(tests/golden/align_trunc_*.npz, tools/make_alignment_trunc_golden.py) and against properties the fixtures cannot show.

Gates (as tests/test_hip_alignment.py): objective at the returned solution <= the reference's * (1 + 1e-5); solutions within 2e-3 relative,
5x that for shifts; loss within 1e-4 relative; same index and bits on the exactly representable fixtures; the reference's gradients where the
same two samples were selected."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from tests import alignment_trunc_reference as R

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
OBJ_TOL, SOL_TOL = 1e-5, 2e-3
ONE_D = ["align_trunc_small", "align_trunc_exact", "align_trunc_zero", "align_trunc_huge", "align_trunc_many", "align_trunc_clamp"]
EXACT = ["align_trunc_exact", "align_trunc_zero", "align_trunc_clamp"]


@pytest.fixture(scope="module")
def A():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from moge_amd import alignment
    return alignment


def load(name):
    return dict(np.load(os.path.join(GOLD, name + ".npz")))


def dev(a, grad=False):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda().requires_grad_(grad)


def np_(t):
    return t.detach().cpu().numpy()


def close(a, b, tol, what):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    err = np.abs(a - b) / np.maximum(np.abs(b), 1e-3)
    assert float(err.max()) <= tol, (what, a, b)


def obj1(a, x, y, w, trunc):
    return R.objective(a, x, y, w, trunc)


def obj_points(scale, shift, src, tgt, w, trunc):
    r = np.abs(np.asarray(scale, np.float32)[..., None, None] * src + np.asarray(shift, np.float32)[..., None, :] - tgt) * w[..., None]
    return np.minimum(r, np.float32(trunc)).astype(np.float64).sum((-2, -1))


@pytest.mark.parametrize("name", ONE_D)
def test_align_golden(A, name):
    g = load(name)
    trunc = float(g["trunc"])
    a, loss, index = (np_(v) for v in A.align_trunc(dev(g["x"]), dev(g["y"]), dev(g["w"]), trunc))
    ref = obj1(g["a"], g["x"], g["y"], g["w"], trunc)
    assert np.all(obj1(a, g["x"], g["y"], g["w"], trunc) <= ref * (1 + OBJ_TOL) + 1e-12)
    close(a, g["a"], SOL_TOL, "a")
    assert np.allclose(loss, g["loss"], rtol=1e-4, atol=1e-7)
    if name in EXACT:
        assert np.array_equal(index, g["index"])
        assert np.array_equal(a.view(np.uint32), g["a"].view(np.uint32))


@pytest.mark.parametrize("name", ["align_trunc_solvers_6", "align_trunc_solvers_24"])
def test_solvers_golden(A, name):
    g = load(name)
    trunc = float(g["trunc"])
    P, G, W = g["pred"], g["gt"], g["w"]
    Pd, Gd, Wd = dev(P), dev(G), dev(W)
    z = np.zeros_like(W[..., 0])

    s = np_(A.align_depth_scale(Pd[..., 2], Gd[..., 2], Wd, trunc))
    assert np.all(obj1(s, P[..., 2], G[..., 2], W, trunc) <= obj1(g["depth_scale"], P[..., 2], G[..., 2], W, trunc) * (1 + OBJ_TOL) + 1e-9)
    close(s, g["depth_scale"], SOL_TOL, "depth_scale")
    s = np_(A.align_points_scale(Pd, Gd, Wd, trunc))
    assert np.all(obj_points(s, np.zeros((len(s), 3)), P, G, W, trunc) <= obj_points(g["points_scale"], np.zeros((len(s), 3)), P, G, W, trunc) * (1 + OBJ_TOL) + 1e-9)
    close(s, g["points_scale"], SOL_TOL, "points_scale")
    for key in ("points_z_shift", "points_xyz_shift"):
        sh = np_(getattr(A, "align_" + key)(Pd, Gd, Wd, trunc))
        one = np.ones(len(sh), np.float32)
        assert np.all(obj_points(one, sh, P, G, W, trunc) <= obj_points(one, g[key], P, G, W, trunc) * (1 + OBJ_TOL) + 1e-9), key
        close(sh, g[key], 5 * SOL_TOL, key)

    affine = {"depth_affine": lambda p, q: A.align_depth_affine(p[..., 2], q[..., 2], Wd, trunc),
              "points_scale_z_shift": lambda p, q: A.align_points_scale_z_shift(p, q, Wd, trunc),
              "points_scale_xyz_shift": lambda p, q: A.align_points_scale_xyz_shift(p, q, Wd, trunc)}
    for key, fn in affine.items():
        p, q = dev(P, True), dev(G, True)
        s, sh = fn(p, q)
        gp, gq = torch.autograd.grad(s.sum() + sh.sum(), (p, q))
        s, sh = np_(s), np_(sh)
        if key == "depth_affine":
            mine = obj_points(s, np.stack([z, z, sh], -1), P * [0, 0, 1], G * [0, 0, 1], W, trunc)
            ref = obj_points(g[key + "_scale"], np.stack([z, z, g[key + "_shift"]], -1), P * [0, 0, 1], G * [0, 0, 1], W, trunc)
        else:
            mine, ref = obj_points(s, sh, P, G, W, trunc), obj_points(g[key + "_scale"], g[key + "_shift"], P, G, W, trunc)
        assert np.all(mine <= ref * (1 + OBJ_TOL) + 1e-9), key
        close(s, g[key + "_scale"], SOL_TOL, key)
        close(sh, g[key + "_shift"], 5 * SOL_TOL, key)
        # gradients reach the two selected samples: where the solution is the reference's to rounding, so is the gradient
        gp, gq = np_(gp), np_(gq)
        same = np.abs(s - g[key + "_scale"]) <= 1e-6 * np.abs(g[key + "_scale"]) + 1e-7
        assert same.sum() >= len(s) // 2, key
        for b in np.nonzero(same)[0]:
            assert np.allclose(gp[b], g[key + "_grad_src"][b], rtol=1e-4, atol=1e-5), (key, b)
            assert np.allclose(gq[b], g[key + "_grad_tgt"][b], rtol=1e-4, atol=1e-5), (key, b)


def test_global_row_golden_and_determinism(A):
    g = load("align_trunc_global_48")
    trunc = float(g["trunc"])
    P, G, W = g["pred"], g["gt"], g["w"]
    runs = []
    for _ in range(2):
        p, q = dev(P, True), dev(G, True)
        s, sh = A.align_points_scale_z_shift(p, q, dev(W), trunc)
        gp, gq = torch.autograd.grad(s.sum() + sh.sum(), (p, q))
        runs.append([np_(v) for v in (s, sh, gp, gq)])
    for u, v in zip(*runs):
        assert np.array_equal(u.view(np.uint32), v.view(np.uint32))
    s, sh, gp, gq = runs[0]
    key = "points_scale_z_shift"
    assert np.all(obj_points(s, sh, P, G, W, trunc) <= obj_points(g[key + "_scale"], g[key + "_shift"], P, G, W, trunc) * (1 + OBJ_TOL) + 1e-9)
    close(s, g[key + "_scale"], SOL_TOL, "scale")
    close(sh, g[key + "_shift"], 5 * SOL_TOL, "shift")
    if abs(float(s[0] - g[key + "_scale"][0])) <= 1e-6 * abs(float(g[key + "_scale"][0])):
        assert np.allclose(gp, g[key + "_grad_src"], rtol=1e-4, atol=1e-5)
        assert np.allclose(gq, g[key + "_grad_tgt"], rtol=1e-4, atol=1e-5)


def test_huge_trunc_is_untruncated(A):
    g = torch.Generator(device="cuda").manual_seed(1)
    x = torch.randn(64, 900, device="cuda", generator=g)
    y = 0.7 * x + 0.3 * torch.randn(64, 900, device="cuda", generator=g)
    w = torch.rand(64, 900, device="cuda", generator=g)
    at, lt, _ = A.align_trunc(x, y, w, 1e9)
    a0, l0, _ = A.align(x, y, w)
    l1 = lambda a: (w * (a[:, None] * x - y).abs()).double().sum(-1)     # noqa: E731
    assert torch.allclose(l1(at), l1(a0), rtol=1e-5)
    assert torch.allclose(lt.double(), l0.double(), rtol=1e-5)


def _row_data(rows, n, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    x = torch.randn(rows, n, device="cuda", generator=g)
    y = 1.3 * x + 0.05 * torch.randn(rows, n, device="cuda", generator=g)
    y += (torch.rand(rows, n, device="cuda", generator=g) < 0.3) * 5 * torch.randn(rows, n, device="cuda", generator=g)
    w = torch.rand(rows, n, device="cuda", generator=g)
    return x, y, w


@pytest.mark.parametrize("n", [108, 432, 1728, 6912])          # across the row-length paths: packed small rows, one row per workgroup in LDS, staged
def test_row_alone_equals_row_in_batch(A, n):
    rows = 10 ** 4 if n <= 1728 else 600
    x, y, w = _row_data(rows, n, n)
    a, loss, idx = A.align_trunc(x, y, w, 0.2)
    for r in (0, rows // 2 + 1, rows - 1):
        a1, l1, i1 = A.align_trunc(x[r:r + 1], y[r:r + 1], w[r:r + 1], 0.2)
        assert int(i1) == int(idx[r]) and float(a1) == float(a[r]) and float(l1) == float(loss[r])
    a2, l2, i2 = A.align_trunc(x, y, w, 0.2)                          # and two runs give the same bits
    assert torch.equal(a, a2) and torch.equal(loss, l2) and torch.equal(idx, i2)
    sub = slice(0, 3)                                           # against the numpy restatement on a few rows
    ra, rl, ri = R.align_trunc(np_(x[sub]), np_(y[sub]), np_(w[sub]), 0.2)
    xs, ys, ws = (np_(v[sub]) for v in (x, y, w))
    assert np.all(obj1(np_(a[sub]), xs, ys, ws, 0.2) <= obj1(ra, xs, ys, ws, 0.2) * (1 + OBJ_TOL) + 1e-9)


@pytest.mark.parametrize("n,d,mask", [(36, 3, 0b111), (144, 3, 0b100), (576, 3, 0b111), (2304, 3, 0b100), (700, 1, 0b1)])
def test_anchored_row_alone_equals_row_in_batch(A, n, d, mask):
    from moge_amd import _lib as L
    g = torch.Generator(device="cuda").manual_seed(n)
    B = 4
    src = torch.randn(B, n, d, device="cuda", generator=g)
    tgt = 0.8 * src + 0.1 + 0.05 * torch.randn(B, n, d, device="cuda", generator=g)
    w = torch.rand(B, n, device="cuda", generator=g)
    rows = 10 ** 4 if n * d <= 1728 else 1000
    rb = torch.randint(0, B, (rows,), device="cuda", generator=g, dtype=torch.int32)
    rk = torch.randint(0, n, (rows,), device="cuda", generator=g, dtype=torch.int32)

    def solve(rb, rk):
        m = rb.numel()
        out = [torch.empty(m, device="cuda"), torch.empty(m, device="cuda"), torch.empty(m, device="cuda", dtype=torch.int32)]
        ws = A._trunc_workspace(n * d, m, src.device)
        L.check(L.lib.moge_align_trunc_anchored(L.ptr(src), L.ptr(tgt), L.ptr(w), n, d, mask, L.ptr(rb), L.ptr(rk), m, 0.1, 1e-7, L.ptr(ws), *(L.ptr(o) for o in out),
                                                L.stream_ptr(src.device)))
        return out

    batch = solve(rb, rk)
    for r in (0, rows - 1):
        one = solve(rb[r:r + 1].contiguous(), rk[r:r + 1].contiguous())
        for u, v in zip(one, batch):
            assert torch.equal(u[0], v[r])
    again = solve(rb, rk)
    assert all(torch.equal(u, v) for u, v in zip(again, batch))


def test_equivariance_and_permutation(A):
    g = load("align_trunc_solvers_24")
    trunc = float(g["trunc"])
    P, G, W = dev(g["pred"]), dev(g["gt"]), dev(g["w"])
    s0, sh0 = A.align_points_scale_xyz_shift(P, G, W, trunc)
    for f in (2.0, 0.5, 3.0):                                   # target and trunc scaled by f: the scale follows
        s1, sh1 = A.align_points_scale_xyz_shift(P, G * f, W, trunc * f)
        assert torch.allclose(s1, s0 * f, rtol=1e-5) and torch.allclose(sh1, sh0 * f, rtol=1e-4, atol=1e-5)
    perm = torch.randperm(P.shape[1], generator=torch.Generator().manual_seed(0)).cuda()
    s2, sh2 = A.align_points_scale_xyz_shift(P[:, perm], G[:, perm], W[:, perm], trunc)
    assert torch.allclose(s2, s0, rtol=1e-6) and torch.allclose(sh2, sh0, rtol=1e-5, atol=1e-6)


def test_exact_recovery_with_outlier_majority(A):
    """60 % of the weight on gross outliers: the truncated optimum is the true transform, the weighted median is not."""
    rng = np.random.default_rng(7)
    n = 576                                                     # dyadic grid: the true transform is exact in float32
    pred = np.stack([rng.integers(-32, 33, n), rng.integers(-24, 25, n), rng.integers(16, 129, n)], -1).astype(np.float32) / 16
    gt = (pred * np.float32(1.5) + np.array([0, 0, 0.25], np.float32)).astype(np.float32)
    bad = rng.permutation(n)[: int(0.6 * n)]
    pred[bad] += (rng.choice([-1, 1], (len(bad), 3)) * rng.integers(80, 800, (len(bad), 3)) / 16).astype(np.float32)
    w = np.ones(n, np.float32)
    P, G, W = dev(pred[None]), dev(gt[None]), dev(w[None])
    s, sh = A.align_points_scale_z_shift(P, G, W, 0.01)
    assert float(s) == 1.5 and np_(sh).tolist() == [[0.0, 0.0, 0.25]]
    s_l1, _ = A.align_points_scale_z_shift(P, G, W)
    assert abs(float(s_l1) - 1.5) > 1e-2


def test_errors(A):
    x = torch.rand(3, 50, device="cuda")
    with pytest.raises(ValueError, match="scalar"):
        A.align_trunc(x, x, x, torch.full((3, 50), 0.2))
    with pytest.raises(ValueError, match="scalar"):
        A.align_depth_affine(x, x, x, torch.full((3,), 0.2, device="cuda"))
    with pytest.raises(RuntimeError, match="GPU"):
        A.align_trunc(x.cpu(), x.cpu(), x.cpu(), 0.5)
    with pytest.raises(RuntimeError, match="GPU"):
        A.align_points_scale_xyz_shift(torch.rand(1, 4, 3), torch.rand(1, 4, 3), torch.rand(1, 4), 0.5)
    long = torch.rand(1, 15361, device="cuda")
    with pytest.raises(Exception, match="15360"):
        A.align_trunc(long, long, long, 0.5)
    with pytest.raises(Exception, match="15360"):
        A.align_points_scale_xyz_shift(torch.rand(1, 5121, 3, device="cuda"), torch.rand(1, 5121, 3, device="cuda"), torch.rand(1, 5121, device="cuda"), 0.5)
    with pytest.raises(ValueError, match="weight > 0"):
        A.align_points_scale_z_shift(torch.rand(1, 4, 3, device="cuda"), torch.rand(1, 4, 3, device="cuda"), torch.zeros(1, 4, device="cuda"), 0.5)
    # align() itself keeps its untruncated-only contract and names the truncated entry point
    with pytest.raises(NotImplementedError, match="align_trunc"):
        A.align(x, x, x, 0.5)
    # a one-element tensor is a scalar
    a0, _, _ = A.align_trunc(x, x * 2, x, 0.5)
    a1, _, _ = A.align_trunc(x, x * 2, x, torch.tensor(0.5))
    assert torch.equal(a0, a1)
