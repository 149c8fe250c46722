"""float64 references, with per-element error bounds, of the trainable Linear (moge_amd.linear, csrc/linear_grad.hip), written
from the definitions and not from the kernels, on inputs ALREADY rounded to the storage type:

    Y = X W^T + b        dX = dY W        dW = dY^T X        db[n] = sum_m dY[m][n]

tests/test_linear_reference_cpu.py checks them against torch's float64 autograd of F.linear, holds an honest fp32 emulation inside every bound and a
list of injected faults outside.  tests/test_hip_linear.py compares element by element: |got - ref| <= bound(element).

The bounds follow tests/core_reference.py (its H16, SUB16, C_EPI and store are used here): u = 2^-24, h = 2^-11,
    e_Y  = (K + C_EPI) u (|b| + sum_k |x w|)       e_dX = (N + C_EPI) u sum_n |dy w|
    e_dW = (M + C_EPI) u sum_m |dy x|              e_db = (M + C_EPI) u sum_m |dy|
and an fp16 store adds h (|ref| + e) + 2^-25.  (n - 1) u is Higham's bound for a sum of n terms in ANY order (Accuracy and Stability of Numerical
Algorithms, section 4.2), so it covers every tiling and the split of M in the weight gradient, whose partials stay fp32: a second pass that summed
partials ROUNDED TO FP16 would be a kernel bug, not a term to add here.  C_EPI = 2: the bias addition and one spare for the final fp32 rounding.
It is rigorous for the fp32 MFMA (a k-ordered fmaf chain, one rounding per step); an fp16 x fp16 product is exact in fp32, and - core_reference's
ASSUMPTION, stated again - the internal adds of the fp16 MFMA (v_mfma_f32_32x32x16_f16), which the kernel guide does not document, are taken to be no
worse than correctly rounded fp32 additions in some order.  The column sums of db add fp16 values converted exactly to fp32."""
import functools

import numpy as np

import core_reference as CR
from core_reference import C_EPI, H16, SUB16, store, to_storage          # noqa: F401  (re-exported for the tests)
from tail_reference import U32


def linear(x, w, b, dy, prec):
    """x (M, K), w (N, K), b (N,) or None, dy (M, N): float64 values of the storage type -> {name: (ref, bound)} for y, dx, dw, db (db with b only)."""
    x, w, dy = CR.f64(x), CR.f64(w), CR.f64(dy)
    M, K = x.shape
    N = w.shape[0]
    bb = np.zeros(N) if b is None else CR.f64(b)
    out = {}
    y = x @ w.T + bb
    out["y"] = (y, store(y, (K + C_EPI) * U32 * (np.abs(bb) + np.abs(x) @ np.abs(w).T), prec))
    dx = dy @ w
    out["dx"] = (dx, store(dx, (N + C_EPI) * U32 * (np.abs(dy) @ np.abs(w)), prec))
    dw = dy.T @ x
    out["dw"] = (dw, store(dw, (M + C_EPI) * U32 * (np.abs(dy).T @ np.abs(x)), prec))
    if b is not None:
        db = dy.sum(0)
        out["db"] = (db, store(db, (M + C_EPI) * U32 * np.abs(dy).sum(0), prec))
    return out


def inputs(M, K, N, family, seed=0):
    """x, w, bias from core_reference.gemm_inputs (random / offset) and an incoming gradient dy ~ N(0, 1) (offset: + 0.25, so that the sums over M
    do not cancel): float32."""
    x, w, b = CR.gemm_inputs(M, N, K, family, seed)
    dy = np.random.default_rng([seed + 1, M, N, K]).standard_normal((M, N)) + (0.25 if family == "offset" else 0.0)
    return x, w, b, dy.astype(np.float32)


SWEEP_M = (1, 31, 32, 33, 127, 128, 129, 257)


def sweep_kn(prec):
    """(K, N) pairs that cross the 128 x 128 tile and the K tile (64 fp16 / 32 fp32 elements) in every dimension once."""
    c = CR.chunk(prec)
    return ((c, c), (64, 72), (72, 136), (128, 128), (136, 264))


LARGE = (1370, 384, 1536)            # a ViT-S block's fc1 at 37 x 37 patches
SPLIT = (2049, 72, 136)              # two tiles of dW and 33 (fp16) / 65 (fp32) K tiles over M: the split of M engages, with every tail


@functools.lru_cache(maxsize=None)
def case(M, K, N, family, prec):
    """The seeded inputs as float32 arrays of storage-type values and the reference of every product; built once, never modified."""
    x, w, b, dy = (to_storage(t, prec) for t in inputs(M, K, N, family))
    return dict(x=x.astype(np.float32), w=w.astype(np.float32), b=b.astype(np.float32), dy=dy.astype(np.float32), ref=linear(x, w, b, dy, prec))
