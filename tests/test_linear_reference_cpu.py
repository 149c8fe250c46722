"""CPU: the float64 references of tests/linear_reference.py are the right ones (torch's float64 autograd of F.linear), their bounds hold an honest
fp32 emulation that tiles and splits in another order than the kernels, and each of a list of injected faults - what csrc/linear_grad.hip could get
wrong at a tile edge - lands OUTSIDE a bound on the inputs chosen here.  No GPU."""
import numpy as np
import pytest
import torch

import linear_reference as LR
from linear_reference import to_storage

PRECS = [0, 1]
SHAPES = [(1, 8, 8), (33, 72, 136), (129, 136, 264), (257, 64, 72)]           # (M, K, N)


def rounded(v, prec):
    """fp32 -> storage type -> float64: the kernel's single rounding of a result."""
    return to_storage(np.asarray(v, dtype=np.float32), prec)


def inside(got, ref_bound):
    ref, bound = ref_bound
    return bool((np.abs(got - ref) <= bound).all())


@pytest.mark.parametrize("M,K,N", SHAPES)
def test_references_agree_with_torch_float64_autograd(M, K, N):
    c = LR.case(M, K, N, "random", 0)
    x, w, b = (torch.tensor(c[n], dtype=torch.float64, requires_grad=True) for n in ("x", "w", "b"))
    y = torch.nn.functional.linear(x, w, b)
    y.backward(torch.tensor(c["dy"], dtype=torch.float64))
    for name, t in (("y", y.detach()), ("dx", x.grad), ("dw", w.grad), ("db", b.grad)):
        ref = c["ref"][name][0]
        assert ref.shape == tuple(t.shape) and np.abs(ref - t.numpy()).max() <= 1e-12 * max(1.0, np.abs(ref).max()), name
        assert (c["ref"][name][1] > 0).all(), name
    assert "db" not in LR.linear(c["x"], c["w"], None, c["dy"], 0)


def emulate(c, prec, kt=48, splits=3):
    """fp32 arithmetic in another order than the kernels': contraction tiles of `kt`, the weight gradient and the bias gradient as `splits` fp32
    partials over M added afterwards, one rounding to the storage type at the end."""
    x, w, b, dy = (c[n].astype(np.float32) for n in ("x", "w", "b", "dy"))

    def tiled(a, bt):                                  # a (I, C) . bt (J, C)^T with fp32 partial sums per tile of C
        acc = np.zeros((a.shape[0], bt.shape[0]), dtype=np.float32)
        for k0 in range(0, a.shape[1], kt):
            acc = acc + a[:, k0:k0 + kt] @ bt[:, k0:k0 + kt].T
        return acc

    M = x.shape[0]
    edges = np.linspace(0, M, splits + 1).astype(int)
    dw, db = np.zeros((w.shape[0], x.shape[1]), dtype=np.float32), np.zeros(w.shape[0], dtype=np.float32)
    for m0, m1 in zip(edges[:-1], edges[1:]):
        dw = dw + tiled(np.ascontiguousarray(dy[m0:m1].T), np.ascontiguousarray(x[m0:m1].T))
        db = db + dy[m0:m1].sum(0, dtype=np.float32)
    return {"y": rounded(tiled(x, w) + b, prec), "dx": rounded(tiled(dy, np.ascontiguousarray(w.T)), prec), "dw": rounded(dw, prec), "db": rounded(db, prec)}


@pytest.mark.parametrize("prec", PRECS, ids=["fp32", "fp16"])
@pytest.mark.parametrize("family", ["random", "offset"])
@pytest.mark.parametrize("M,K,N", SHAPES + [(1025, 72, 136)])
def test_an_honest_fp32_emulation_stays_inside_every_bound(M, K, N, family, prec):
    c = LR.case(M, K, N, family, prec)
    got = emulate(c, prec)
    for name in ("y", "dx", "dw", "db"):
        ref, bound = c["ref"][name]
        frac = float((np.abs(got[name] - ref) / bound).max())
        print(f"emulation M{M} K{K} N{N} {family} prec{prec} {name}: worst error / bound = {frac:.3f}")
        assert frac <= 1.0, name


def cancelling_case(prec, M=512, K=64, N=72):
    """The weight gradient as two partials over M that nearly cancel: dy = +1 on the first half of the rows, -1 (both plus noise) on the second, x
    positive.  Each partial is ~ M / 2 times the sum it leaves, so a rounding of the PARTIALS to fp16 is far more than the rounding of the sum."""
    rng = np.random.default_rng(7)
    x = to_storage(1.0 + 0.25 * rng.standard_normal((M, K)), prec)
    dy = to_storage(np.where(np.arange(M)[:, None] < M // 2, 1.0, -1.0) + 0.05 * rng.standard_normal((M, N)), prec)
    w = to_storage(rng.standard_normal((N, K)) / 8.0, prec)
    b = to_storage(rng.standard_normal(N), prec)
    return dict(x=x, w=w, b=b, dy=dy, ref=LR.linear(x, w, b, dy, prec))


@pytest.mark.parametrize("prec", PRECS, ids=["fp32", "fp16"])
def test_injected_faults_land_outside_the_bounds(prec):
    ch = 8 if prec == 1 else 4
    M, K, N = 129, 136, 136                             # N = K: the transposed weight of the dgrad fault has the right shape
    for family in ("random", "offset"):
        c = LR.case(M, K, N, family, prec)
        x, w, b, dy = (c[n].astype(np.float64) for n in ("x", "w", "b", "dy"))
        ref = c["ref"]
        good = {"y": x @ w.T + b, "dx": dy @ w, "dw": dy.T @ x, "db": dy.sum(0)}
        for name in good:                               # the exact value, rounded once, is inside: the faults below are what moves it out
            assert inside(rounded(good[name], prec), ref[name]), name
        faults = {
            "the last K chunk dropped": ("y", x[:, :-ch] @ w[:, :-ch].T + b),
            "the last N chunk dropped in dgrad": ("dx", dy[:, :-ch] @ w[:-ch]),
            "a clamped tail row counted in dW": ("dw", good["dw"] + np.outer(dy[-1], x[-1])),
            "a clamped tail row counted in db": ("db", good["db"] + dy[-1]),
            "W indexed [k][n] for [n][k] in dgrad": ("dx", dy @ w.T),
            "bias added twice": ("y", good["y"] + b),
            "bias missing": ("y", x @ w.T),
        }
        for what, (name, value) in faults.items():
            assert not inside(rounded(value, prec), ref[name]), (what, family)
    # a partial of the split rounded to fp16 (in either storage type: the partials are fp32 in both)
    c = cancelling_case(prec)
    x, dy = c["x"], c["dy"]
    h = x.shape[0] // 2
    parts = [dy[:h].T @ x[:h], dy[h:].T @ x[h:]]
    assert inside(rounded(parts[0].astype(np.float32).astype(np.float64) + parts[1].astype(np.float32).astype(np.float64), prec), c["ref"]["dw"])
    faulty = rounded(to_storage(parts[0], 1) + to_storage(parts[1], 1), prec)
    ref, bound = c["ref"]["dw"]
    frac = float((np.abs(faulty - ref) / bound).max())
    print(f"partials rounded to fp16, prec{prec}: worst error / bound = {frac:.2f}")
    assert frac > 1.0
