"""Plain numpy restatement of the truncated alignment objective (reference `moge/utils/alignment.py:91-144`), written from its formulas.

    min_a  sum_i min(trunc, w_i |a x_i - y_i|)      per row, trunc one scalar

Steps, as the reference decides them:
  1. flip signs so that x >= 0; wx = w x, wy = w y; candidates A = y / max(x, eps), edges B = (wy - trunc) / max(wx, eps),
     C = (wy + trunc) / max(wx, eps) (B and C clamp wx, A clamps x), all in float32;
  2. left derivative L(a) = 2 sum_{A_i < a} wx_i - sum_{B_i < a} wx_i - sum_{C_i < a} wx_i, right derivative R(a) the same with <=;
     element i is an extremum iff L(A_i) < 0 <= R(A_i); a row without one has element 0 as its only extremum;
  3. the objective at each extremum, summed over the whole row;
  4. the smallest objective wins, an exact tie goes to the largest element index (scatter_min's last write);
  5. the affine solvers solve one anchored row per sample with weight > 0, keep the best anchor (ties: the last) and recompute scale and
     shift from the two selected samples.

`align_trunc` is that decision with float64 sums (the reference sums in float32; the two can split a near-tie differently, so tests compare
objective values tightly and indices only on exactly representable data).  `sweep_objective` is the kernel's way to get step 3 at every
candidate in one pass (csrc/alignment.hip, align_trunc_kernel): the objective is piecewise linear with its kinks at A, B and C, so it is a
prefix sum over the 3n edges in sorted order.  Nothing here needs a GPU."""
from __future__ import annotations

import numpy as np

F = np.float32
EPS = 1e-7


def keys(x, y, w, trunc, eps=EPS):
    """Step 1 on (rows, n) float32 -> x, y (sign-flipped), w, wx, wy, A, B, C."""
    x, y, w = (np.asarray(v, F) for v in (x, y, w))
    s = np.sign(x).astype(F)
    x, y = x * s, y * s
    wx, wy = w * x, w * y
    e, t = F(eps), F(trunc)
    with np.errstate(all="ignore"):
        A = y / np.maximum(x, e)
        B = (wy - t) / np.maximum(wx, e)
        C = (wy + t) / np.maximum(wx, e)
    return x, y, w, wx, wy, A, B, C


def derivatives(A, B, C, wx):
    """Step 2 for one row: L and R at every candidate A_i (float64 sums)."""
    wx = wx.astype(np.float64)

    def below(K, side):
        order = np.argsort(K, kind="stable")
        q = np.concatenate([[0.0], np.cumsum(wx[order])])
        return q[np.searchsorted(K[order], A, side=side)]

    left = 2 * below(A, "left") - below(B, "left") - below(C, "left")
    right = 2 * below(A, "right") - below(B, "right") - below(C, "right")
    return left, right


def extrema(A, B, C, wx):
    left, right = derivatives(A, B, C, wx)
    ext = (left < 0) & (right >= 0)
    if not ext.any():
        ext[0] = True
    return ext


def objective(a, x, y, w, trunc):
    """Step 3, directly: sum_i min(trunc, |a x_i - y_i| w_i), float32 terms summed in float64.  a (...,), x, y, w (..., n)."""
    a = np.asarray(a, F)[..., None]
    with np.errstate(all="ignore"):
        r = np.minimum(np.abs(a * np.asarray(x, F) - np.asarray(y, F)) * np.asarray(w, F), F(trunc))
    return r.astype(np.float64).sum(-1)


def sweep_objective(x, y, w, wx, wy, A, B, C, trunc, eps=EPS):
    """Step 3 at every candidate of one row in one pass over the sorted edges (the kernel's closed form, float64):
        f(a) = trunc * #clipped(a) + sum_{edges e < a} c_e + a * sum_{edges e < a} s_e
    s: A +2wx, B -wx, C -wx;  c: A -2wy, B +wy, C +wy;  #clipped = #regular - #{B < a} + #{C < a}.  Only "regular" elements (x >= eps and
    wx >= eps: the edges are the true kinks) enter it; elements with w = 0 or x = 0 add 0; the others are added directly.  trunc <= 0 makes
    the objective a constant: 0 at every candidate."""
    n = len(A)
    if trunc <= 0:
        return np.zeros(n)
    reg = (x >= F(eps)) & (wx >= F(eps))
    zero = (w == 0) | (x == 0)
    direct = ~reg & ~zero
    wxd, wyd = np.where(reg, wx, 0).astype(np.float64), np.where(reg, wy, 0).astype(np.float64)
    kind = np.repeat([[0, 1, 2]], n, 0).ravel()
    elem = np.repeat(np.arange(n), 3)
    key = np.stack([A, B, C], -1).ravel()
    s = np.where(kind == 0, 2 * wxd[elem], -wxd[elem])
    c = np.where(kind == 0, -2 * wyd[elem], wyd[elem])
    cnt = np.where(kind == 1, -1.0, np.where(kind == 2, 1.0, 0.0)) * reg[elem]
    order = np.lexsort((np.arange(3 * n), key))
    pos = np.empty(3 * n, np.int64)
    pos[order] = np.arange(3 * n)
    ex = [np.concatenate([[0.0], np.cumsum(v[order])[:-1]]) for v in (s, c, cnt)]
    at = pos[3 * np.arange(n)]                                        # sorted position of each element's A edge
    a = A.astype(np.float64)
    f = float(trunc) * (reg.sum() + ex[2][at]) + ex[1][at] + a * ex[0][at]
    if direct.any():
        f = f + objective(A, x[direct][None], y[direct][None], w[direct][None], trunc)
    return f


def align_trunc(x, y, w, trunc, eps=EPS, sweep=False):
    """(rows, n) -> a (rows,) float32, loss (rows,) float64, index (rows,) int64.  sweep=True takes the objective at the extrema from
    sweep_objective (the kernel's algorithm) instead of summing it directly (the reference's)."""
    x, y, w = np.broadcast_arrays(*(np.asarray(v, F) for v in (x, y, w)))
    x, y, w = (v.reshape(-1, v.shape[-1]) for v in (x, y, w))
    xs, ys, ws, wx, wy, A, B, C = keys(x, y, w, trunc, eps)
    rows = xs.shape[0]
    a_out, loss_out, idx_out = np.zeros(rows, F), np.zeros(rows), np.zeros(rows, np.int64)
    for r in range(rows):
        ext = np.nonzero(extrema(A[r], B[r], C[r], wx[r]))[0]
        if sweep:
            vals = sweep_objective(xs[r], ys[r], ws[r], wx[r], wy[r], A[r], B[r], C[r], trunc, eps)[ext]
        else:
            vals = objective(A[r][ext], xs[r][None], ys[r][None], ws[r][None], trunc)
        best = ext[np.nonzero(vals == vals.min())[0][-1]]             # ties: the last element
        a_out[r] = A[r][best]
        loss_out[r] = objective(A[r][best], xs[r], ys[r], ws[r], trunc)
        idx_out[r] = best
    return a_out, loss_out, idx_out


# ---------------------------------------------------------------------------------------------------------------------------------------
# the anchored solvers (alignment.py:163-212, :246-299, :302-354)
# ---------------------------------------------------------------------------------------------------------------------------------------
def _anchor(src, tgt, w, mask, trunc, sweep=False):
    """src / tgt (B, n, d), w (B, n): per batch element the best anchor k and the solution element i2 in [0, n d)."""
    Bn, n, d = src.shape
    m = np.array(mask, F)
    ks, i2s = np.zeros(Bn, np.int64), np.zeros(Bn, np.int64)
    for b in range(Bn):
        anchors = np.nonzero(w[b] > 0)[0]
        xs = (src[b][None] - src[b][anchors][:, None] * m).reshape(len(anchors), -1)
        ys = (tgt[b][None] - tgt[b][anchors][:, None] * m).reshape(len(anchors), -1)
        ww = np.repeat(w[b], d)[None].repeat(len(anchors), 0)
        _, loss, idx = align_trunc(xs, ys, ww, trunc, sweep=sweep)
        loss = loss.astype(F)                                         # the kernels hand float32 losses to the anchor choice
        j = np.nonzero(loss == loss.min())[0][-1]
        ks[b], i2s[b] = anchors[j], idx[j]
    return ks, i2s


def depth_affine(src, tgt, w, trunc, sweep=False):
    src, tgt, w = (np.asarray(v, F) for v in (src, tgt, w))
    k, i2 = _anchor(src[..., None], tgt[..., None], w, [1], trunc, sweep)
    r = np.arange(len(k))
    s1, t1, s2, t2 = src[r, k], tgt[r, k], src[r, i2], tgt[r, i2]
    scale = (t2 - t1) / np.where(s2 != s1, s2 - s1, F(1e-7))
    return scale, t1 - scale * s1


def points_affine(src, tgt, w, trunc, xyz_shift: bool, sweep=False):
    src, tgt, w = (np.asarray(v, F) for v in (src, tgt, w))
    m = np.array([1, 1, 1] if xyz_shift else [0, 0, 1], F)
    k, i2 = _anchor(src, tgt, w, m, trunc, sweep)
    r = np.arange(len(k))
    sa, ta = src * m, tgt * m
    i1 = k * 3 + i2 % 3
    s1, t1 = sa.reshape(len(k), -1)[r, i1], ta.reshape(len(k), -1)[r, i1]
    s2, t2 = src.reshape(len(k), -1)[r, i2], tgt.reshape(len(k), -1)[r, i2]
    scale = (t2 - t1) / np.where(s2 != s1, s2 - s1, F(1))
    return scale, ta[r, k] - scale[:, None] * sa[r, k]
