"""float64 references, with per-element error bounds, of the trainable bilinear resize and the narrow 1x1 conv (moge_amd.resample,
csrc/resample_grad.hip), written from the definitions and not from the kernels or from torch, on inputs ALREADY rounded to the
storage type.

Resize, one axis with n_in input and n_out output samples and scale sigma (n_in / n_out where a size is given, 1 / scale_factor for a module):

    s(o) = max(sigma (o + 0.5) - 0.5, 0)    i0 = min(floor s, n_in - 1)    i1 = min(i0 + 1, n_in - 1)    l1 = s - i0    l0 = 1 - l1
    y[b,o,p,c] = sum_{a,a'} la^H(o) la'^W(p) x[b, ia^H(o), ia'^W(p), c]                dx = the transpose of that map applied to dy

axis_matrix() turns the definition of an axis into the (n_out, n_in) matrix A with A[o, i0] += l0, A[o, i1] += l1 (both on the last sample where
i0 = i1), so y = A_H x A_W^T and dx = A_H^T dy A_W.  tests/test_resample_reference_cpu.py checks them against torch's float64 autograd, holds an fp32
emulation of the kernels' order inside every bound and a list of injected faults outside.  tests/test_hip_resample.py compares element by element:
|got - ref| <= bound.

The bounds, stated before the first GPU run.  u = 2^-24, h = 2^-11.
  sum     (4 + 2) u sum |l l' x|.  The forward as written is v = fma(l1H, bot, l0H top), top = fma(l1W, x01, l0W x00): the x00 term passes l0W = 1 - l1W
          (one rounding; l1 = s - i0 is exact), a product, an fma, l0H, a product, an fma - six roundings, every other term fewer.
  coord   delta_H |dy/ds_H| + delta_W |dy/ds_W|, delta = K_COORD u (s + 1), K_COORD = 3: the coordinate function rounds o + 0.5 (exact below 2^23,
          counted), the fma, and sigma itself to fp32 on its way into the call.  |dy/ds_H| = |sum_a' la'^W (x[i1H, ia'W] - x[i0H, ia'W])| from the four taps in
          float64.  The map is continuous and piecewise linear in s, so a computed s on the other side of an integer - where floor s flips - moves y by
          at most delta times the larger of the two slopes: where s +- delta crosses an integer, the slope of BOTH intervals is taken (the larger
          magnitude).  17 -> 3 has such a point: s(1) = 8 exactly.
  dx      the same two terms per contributing output, summed over the contributing outputs: (4 + 2) u sum |w w' dy| and
          sum (delta_H |dw/ds_H| w' + w delta_W |dw'/ds_W|) |dy|, with |dw/ds| = 1 for a tap of either interval and 0 where both taps are one sample.
          The gradient kernel's chain is longer than six roundings where more than two outputs per axis contribute (rows outer: wH, an fma per row;
          columns inner: wW, an fma per column - n_H + n_W + 2 for the first term, 10 at x2).  The issue sets (4 + 2); it is kept, and Higham's
          worst case would need every one of those roundings at its full u with one sign.
  store   fp16 adds h (|ref| + e) + 2^-25, as convt_reference.
Narrow conv: linear_reference.linear's forms as they are, on the M = B H W pixels as rows (K = Cin, N = Cout):
    e_y = (Cin + 2) u (|b| + sum |x| |w|)    e_dx = (Cout + 2) u sum |dy| |w|    e_dw = (M + 2) u sum |x| |dy|    e_db = (M + 2) u sum |dy|
plus the same store term; (n - 1) u covers any order, so the quad sum of the forward, the row lanes of the weight gradient and its slabs (fp32
partials, added in slab order) are inside.

The kernels' own constants, named so that the shapes below can be seen to cross them: CHUNK = 16 bytes of channels per thread where the layout allows;
the narrow conv's forward takes 64 pixels per workgroup (a quad of lanes each), its weight gradient slabs of at least SLAB pixels, MAX_SLABS at the most."""
import functools

import numpy as np

import core_reference as CR
import linear_reference as LR
from core_reference import H16, SUB16, store, to_storage          # noqa: F401  (re-exported for the tests)
from tail_reference import U32

C_SUM = 4 + 2
K_COORD = 3
SLAB, MAX_SLABS = 512, 1024
FWD_PIXELS = 64


def taps(n_in, n_out, sigma=None):
    """The definition: (s, i0, i1, l0, l1) of every output sample, float64."""
    sigma = n_in / n_out if sigma is None else sigma
    s = np.maximum(sigma * (np.arange(n_out) + 0.5) - 0.5, 0.0)
    i0 = np.minimum(np.floor(s), n_in - 1).astype(np.int64)
    i1 = np.minimum(i0 + 1, n_in - 1)
    l1 = s - i0
    return s, i0, i1, 1.0 - l1, l1


def axis_matrix(n_in, n_out, sigma=None):
    """A (n_out, n_in) with y = A x along the axis."""
    _, i0, i1, l0, l1 = taps(n_in, n_out, sigma)
    A = np.zeros((n_out, n_in))
    o = np.arange(n_out)
    np.add.at(A, (o, i0), l0)
    np.add.at(A, (o, i1), l1)
    return A


def first_table(n_in, n_out, sigma=None):
    """first[r] = min{o : i0(o) >= r}, r = 0 ... n_in (first[n_in] = n_out): the gather table of the gradient."""
    i0 = taps(n_in, n_out, sigma)[1]
    return np.array([int(np.searchsorted(i0, r, side="left")) for r in range(n_in + 1)])


def coord_slack(n_in, n_out, sigma=None):
    """(delta (n_out,), D (n_out, n_in)): the coordinate's error bound and the slope matrix of the coordinate term - dy/ds = D x where s stays inside one
    interval; D is returned as the two candidates (interval of s - delta, interval of s + delta), which differ where s +- delta crosses an integer."""
    s = taps(n_in, n_out, sigma)[0]
    delta = K_COORD * U32 * (s + 1.0)
    Ds = []
    for side in (np.maximum(s - delta, 0.0), s + delta):
        j0 = np.minimum(np.floor(side), n_in - 1).astype(np.int64)
        j1 = np.minimum(j0 + 1, n_in - 1)
        D = np.zeros((n_out, n_in))
        o = np.arange(n_out)
        np.add.at(D, (o, j0), -1.0)
        np.add.at(D, (o, j1), 1.0)
        Ds.append(D)
    return delta, Ds


def _apply(AH, t, AW):
    return np.einsum("oi,bijc,pj->bopc", AH, t, AW)


def resize(x, size, dy, prec, scales=None):
    """x (B, Hin, Win, C), dy (B, Hout, Wout, C), size = (Hout, Wout): float64 values of the storage type -> {"y": (ref, bound), "dx": (ref, bound)};
    scales = (sigma_H, sigma_W), by default the quotients of the sizes."""
    x, dy = CR.f64(x), CR.f64(dy)
    (_, Hin, Win, _), (Hout, Wout) = x.shape, size
    sh, sw = scales or (None, None)
    AH, AW = axis_matrix(Hin, Hout, sh), axis_matrix(Win, Wout, sw)
    (dH, DH), (dW, DW) = coord_slack(Hin, Hout, sh), coord_slack(Win, Wout, sw)
    y = _apply(AH, x, AW)
    e = C_SUM * U32 * _apply(AH, np.abs(x), AW)
    e = e + dH[None, :, None, None] * np.maximum(*(np.abs(_apply(D, x, AW)) for D in DH)) + dW[None, None, :, None] * np.maximum(*(np.abs(_apply(AH, x, D)) for D in DW))
    dx = _apply(AH.T, dy, AW.T)
    ady = np.abs(dy)
    aDH, aDW = np.maximum(np.abs(DH[0]), np.abs(DH[1])), np.maximum(np.abs(DW[0]), np.abs(DW[1]))
    g = C_SUM * U32 * _apply(AH.T, ady, AW.T) + _apply(aDH.T, dH[None, :, None, None] * ady, AW.T) + _apply(AH.T, dW[None, None, :, None] * ady, aDW.T)
    return {"y": (y, store(y, e, prec)), "dx": (dx, store(dx, g, prec))}


conv1x1n = LR.linear               # x (M, Cin), w (Cout, Cin), b (Cout,) or None, dy (M, Cout) -> {name: (ref, bound)} for y, dx, dw, db


# ---- the sweeps --------------------------------------------------------------------------------------------------------------------------------
SWEEP_B = 2                        # a tap, or a gradient range, must not reach into the next image
X2 = (((3, 4), (6, 8)), ((33, 18), (66, 36)))       # run by size and by scale_factor = 2: the same bits
RESIZE = (((1, 1), (1, 1)), ((1, 1), (2, 2)), ((1, 5), (1, 10)), ((5, 1), (10, 1)), ((2, 2), (4, 4)), X2[0], X2[1], ((7, 5), (16, 9)), ((16, 9), (7, 5)),
          ((17, 17), (3, 3)), ((9, 16), (9, 16)), ((5, 7), (4, 23)), ((40, 40), (37, 37)))
IDENTITY = ((9, 16), (9, 16))
EMPTY_ROWS = {((16, 9), (7, 5)): 2, ((17, 17), (3, 3)): 12}      # input rows that receive nothing


def resize_channels(prec):
    """Scalar accesses at 1 and 3, one 16-byte chunk, five (fp16) / ten (fp32) chunks at 40."""
    return (1, 3, CR.chunk(prec), 40)


def slabs_of(M):
    """The documented rule (include/moge_hip.h) -> (slabs, pixels per slab)."""
    per = -(-M // max(1, min(-(-M // SLAB), MAX_SLABS)))
    return -(-M // per), per


RAGGED_M = 1300                    # 3 slabs of 434 pixels, the last one 432
CONV_M = (1, 17, 128, 129, RAGGED_M)


def conv_channels(prec):
    """(Cin, Cout): one chunk to one channel, the two exits of the heads, a chunk count that is no multiple of the quad with an odd Cout, the limits."""
    return ((CR.chunk(prec), 1), (32, 3), (32, 1), (72, 7), (256, 8))


def resize_inputs(B, Hin, Win, Hout, Wout, C, seed=0):
    """x and dy ~ N(0, 1) plus a ramp over the pixel's row and column (so that a tap or a gradient taken from the wrong pixel, or the H and W weights
    swapped, moves the result) and an offset per channel: float32."""
    rng = np.random.default_rng([seed, B, Hin, Win, Hout, Wout, C])

    def field(H, W):
        ramp = 0.5 * np.arange(H)[:, None] - 0.1875 * np.arange(W)[None, :]
        return (rng.standard_normal((B, H, W, C)) + ramp[None, :, :, None] + 0.25 * np.arange(C)[None, None, None, :] / C).astype(np.float32)

    return field(Hin, Win), field(Hout, Wout)


@functools.lru_cache(maxsize=None)
def resize_case(B, Hin, Win, Hout, Wout, C, prec):
    """The seeded inputs as float32 arrays of storage-type values and the reference; built once, never modified."""
    x, dy = (to_storage(t, prec) for t in resize_inputs(B, Hin, Win, Hout, Wout, C))
    return dict(x=x.astype(np.float32), dy=dy.astype(np.float32), ref=resize(x, (Hout, Wout), dy, prec))


@functools.lru_cache(maxsize=None)
def conv_case(M, Cin, Cout, family, prec):
    """linear_reference's seeded inputs (x (M, Cin), w (Cout, Cin), b, dy (M, Cout)) and the reference of every product."""
    x, w, b, dy = (to_storage(t, prec) for t in LR.inputs(M, Cin, Cout, family))
    return dict(x=x.astype(np.float32), w=w.astype(np.float32), b=b.astype(np.float32), dy=dy.astype(np.float32), ref=conv1x1n(x, w, b, dy, prec))
