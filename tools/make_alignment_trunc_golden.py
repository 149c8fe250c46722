"""Golden fixtures of the truncated alignment objective (tests/golden/align_trunc_*.npz) from the reference's unmodified
`moge/utils/alignment.py`, run on the CPU.

    python tools/make_alignment_trunc_golden.py          (build machine: needs the reference checkout of oracle/make_golden.py)

Each fixture holds the inputs, `trunc` and the reference's results: `a`, `loss`, `index` of `align`, or scale / shift of the solvers.  For the
affine solvers it also holds the reference's gradients of scale.sum() + shift.sum() with respect to the source and target points."""
from __future__ import annotations

import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle.make_golden import GOLDEN_DIR, install_stubs                 # noqa: E402
from oracle.make_golden_alignment import scene                           # noqa: E402

t = torch.from_numpy


def save(name, **arrays):
    np.savez(os.path.join(GOLDEN_DIR, name + ".npz"), **arrays)
    print(name, {k: v.shape for k, v in arrays.items()})


def one_d(A, name, x, y, w, trunc):
    a, loss, idx = A.align(t(x), t(y), t(w), trunc)
    save(name, x=x, y=y, w=w, trunc=np.float64(trunc), a=a.numpy(), loss=loss.numpy(), index=idx.numpy())


def solvers(A, name, pred, gt, w, trunc):
    out = dict(pred=pred, gt=gt, w=w, trunc=np.float64(trunc))
    W = t(w)
    P, G = t(pred), t(gt)
    out["depth_scale"] = A.align_depth_scale(P[..., 2], G[..., 2], W, trunc).numpy()
    out["points_scale"] = A.align_points_scale(P, G, W, trunc).numpy()
    out["points_z_shift"] = A.align_points_z_shift(P, G, W, trunc).numpy()
    out["points_xyz_shift"] = A.align_points_xyz_shift(P, G, W, trunc).numpy()
    affine = {"depth_affine": lambda p, g: A.align_depth_affine(p[..., 2], g[..., 2], W, trunc),
              "points_scale_z_shift": lambda p, g: A.align_points_scale_z_shift(p, g, W, trunc),
              "points_scale_xyz_shift": lambda p, g: A.align_points_scale_xyz_shift(p, g, W, trunc)}
    for key, fn in affine.items():
        P, G = t(pred).requires_grad_(), t(gt).requires_grad_()
        s, sh = fn(P, G)
        gp, gg = torch.autograd.grad(s.sum() + sh.sum(), (P, G))
        out[key + "_scale"], out[key + "_shift"] = s.detach().numpy(), sh.detach().numpy()
        out[key + "_grad_src"], out[key + "_grad_tgt"] = gp.numpy(), gg.numpy()
    save(name, **out)


def global_row(A, name, pred, gt, w, trunc):
    P, G = t(pred).requires_grad_(), t(gt).requires_grad_()
    s, sh = A.align_points_scale_z_shift(P, G, t(w), trunc)
    gp, gg = torch.autograd.grad(s.sum() + sh.sum(), (P, G))
    save(name, pred=pred, gt=gt, w=w, trunc=np.float64(trunc), points_scale_z_shift_scale=s.detach().numpy(),
         points_scale_z_shift_shift=sh.detach().numpy(), points_scale_z_shift_grad_src=gp.numpy(), points_scale_z_shift_grad_tgt=gg.numpy())


def main():
    install_stubs()
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    from moge.utils import alignment as A          # the reference
    os.makedirs(GOLDEN_DIR, exist_ok=True)
    rng = np.random.default_rng(20261016)

    # ---- the 1-D solve ------------------------------------------------------------------------------------------------------------------
    # small: zeros in x (sign 0) and in w, a few gross outliers
    x = rng.normal(0, 1, (7, 33)).astype(np.float32)
    x[:, ::11] = 0
    y = (1.7 * x + rng.normal(0, 0.1, x.shape)).astype(np.float32)
    y[:, 3::8] += rng.normal(0, 4, y[:, 3::8].shape).astype(np.float32)
    w = rng.uniform(0, 2, x.shape).astype(np.float32)
    w[:, 5] = 0
    one_d(A, "align_trunc_small", x, y, w, 0.5)

    # exactly representable: x in {1, 2, 4}, integer ratios and weights -> every sum and every residual is exact, the index is pinned.
    # Rows 0-5 random; rows 6-7 repeat one (x, y, w) at several elements (duplicate ratios: the tie goes to the last); row 8 has no weight
    x = rng.choice(np.array([1, 2, 4], np.float32), (9, 40))
    y = (x * rng.integers(-6, 7, (9, 40))).astype(np.float32)
    w = rng.integers(0, 4, (9, 40)).astype(np.float32)
    for r in (6, 7):
        dup = rng.choice(40, 6, replace=False)
        x[r, dup], y[r, dup], w[r, dup] = 2, 2 * (r - 3), 3
    w[8] = 0
    one_d(A, "align_trunc_exact", x, y, w, 4.0)
    one_d(A, "align_trunc_zero", x, y, w, 0.0)                     # trunc = 0: a constant objective, every extremum ties

    # nothing clipped: the truncated solve is the weighted median
    x = rng.normal(0, 1, (4, 200)).astype(np.float32)
    y = (0.8 * x + rng.normal(0, 0.2, x.shape)).astype(np.float32)
    w = rng.uniform(0.1, 1, x.shape).astype(np.float32)
    one_d(A, "align_trunc_huge", x, y, w, 1e6)

    # dozens of extrema: a long noisy row with a small trunc
    pred, gt, wt = scene(rng, 2, 576, outliers=0.3)
    one_d(A, "align_trunc_many", pred.reshape(2, -1), gt.reshape(2, -1), np.repeat(wt, 3, axis=-1), 0.002)

    # w x below eps although x is not: B and C clamp w x (not x); the objective is added directly for these elements
    x = rng.integers(1, 5, (6, 48)).astype(np.float32)
    y = (x * rng.integers(-5, 6, (6, 48))).astype(np.float32)
    w = (rng.integers(0, 4, (6, 48)) * 2.0 ** -27).astype(np.float32)               # dyadic: the float32 sums stay exact
    one_d(A, "align_trunc_clamp", x, y, w, 2.0 ** -22)

    # ---- all eight solvers on scene() data with outliers: 6^2 and 24^2 samples (the local loss's patches), one 48^2 global-loss row ----
    pred, gt, wt = scene(rng, 4, 36, outliers=0.3)
    solvers(A, "align_trunc_solvers_6", pred, gt, wt, 0.05)
    pred, gt, wt = scene(rng, 2, 576, outliers=0.3)
    solvers(A, "align_trunc_solvers_24", pred, gt, wt, 0.1)
    pred, gt, wt = scene(rng, 1, 2304, outliers=0.3)
    global_row(A, "align_trunc_global_48", pred, gt, wt, 1.0)


if __name__ == "__main__":
    sys.exit(main())
