"""float64 references, with per-element error bounds, of the trainable 3x3 convolution (moge_amd.conv, csrc/conv_grad.hip),
written from the definitions and not from the kernels, on inputs ALREADY rounded to the storage type.  With c(i, n) = min(max(i, 0), n - 1):

    y [b,p,q,o]     = bias[o] + sum_{s,t in -1..1} sum_i x[b, c(p+s,H), c(q+t,W), i] w[o,i,s+1,t+1]
    dx[b,P,Q,i]     = sum over the (p, s) with c(p+s,H) = P and the (q, t) with c(q+t,W) = Q of sum_o dy[b,p,q,o] w[o,i,s+1,t+1]
    dw[o,i,s+1,t+1] = sum_{b,p,q} dy[b,p,q,o] x[b, c(p+s,H), c(q+t,W), i]          db[o] = sum_{b,p,q} dy[b,p,q,o]

tests/test_conv_reference_cpu.py checks them against torch's float64 autograd of F.conv2d(F.pad(x, (1, 1, 1, 1), 'replicate'), w, b), holds an honest
fp32 emulation inside every bound and a list of injected faults outside.  tests/test_hip_conv.py compares element by element: |got - ref| <= bound.

The bounds follow tests/linear_reference.py and tests/core_reference.py (conv3x3, store, C_EPI are used here): u = 2^-24, h = 2^-11,
    e_y  = (9 Cin + C_EPI) u (|b| + core(|x|, |w|))            e_dx = (9 Cout + C_EPI) u [the dx formula on |dy|, |w|]
    e_dw = (B H W + C_EPI) u [the dw formula on |dy|, |x|]     e_db = (B H W + C_EPI) u sum |dy|
and an fp16 store adds h (|ref| + e) + 2^-25.  (n - 1) u is Higham's bound for a sum of n terms in ANY order, so it covers every tiling, the order of
the 9 + 16 steps of the input gradient and the split of the pixels in the weight gradient, whose partials stay fp32.  Every dx element is a sum of
exactly 9 Cout products (three (p, s) per axis at every P, border or not), every y element of 9 Cin.  The fp16 MFMA's internal adds are taken to be no
worse than correctly rounded fp32 additions in some order (core_reference's ASSUMPTION).

The kernels' own constants, named here so that the shapes below can be seen to cross them: pixels are tiled in ONE dimension, PIXEL_TILE = 128
consecutive indices of the flat (b, p, q) order (no second pixel-tile dimension, so no extra shapes around one); output channels in tiles of 128; the
contraction in K tiles of 64 fp16 / 32 fp32 elements - channels in the forward and the input gradient, pixels in the weight gradient, whose split keeps
at least MIN_KTILES of them and aims at FILL workgroups, MAX_SPLIT at the most; db in slabs of at least DB_ROWS pixels."""
import functools

import numpy as np

import core_reference as CR
from core_reference import C_EPI, U32, conv3x3, conv3x3_core, conv_inputs, store, to_storage          # noqa: F401  (re-exported for the tests)

PIXEL_TILE, CHANNEL_TILE = 128, 128
FILL, MIN_KTILES, MAX_SPLIT = 512, 8, 64
DB_ROWS, DB_MAX = 4096, 256


def k_tile(prec):
    return 8 * CR.chunk(prec)


def clamped(n, s):
    return np.clip(np.arange(n) + s, 0, n - 1)


def axis_pairs(n):
    """The (p, s) of one axis by the index P they reach: {P: [(p, s), ...]} - three at every P."""
    out = {P: [] for P in range(n)}
    for p in range(n):
        for s in (-1, 0, 1):
            out[min(max(p + s, 0), n - 1)].append((p, s))
    return out


def dgrad_core(dy, w):
    """dy (B,H,W,Cout), w (Cout,Cin,3,3) float64 -> (B,H,W,Cin): every (p, q, s, t) adds dy[p,q] w[s,t] to the pixel (c(p+s), c(q+t)) it read."""
    B, H, W, _ = dy.shape
    dx = np.zeros((B, H, W, w.shape[1]))
    for s in (-1, 0, 1):
        for t in (-1, 0, 1):
            np.add.at(dx, (slice(None), clamped(H, s)[:, None], clamped(W, t)[None, :]), dy @ w[:, :, s + 1, t + 1])
    return dx


def wgrad_core(dy, x):
    """dy (B,H,W,Cout), x (B,H,W,Cin) float64 -> (Cout,Cin,3,3)."""
    _, H, W, _ = dy.shape
    dw = np.zeros((dy.shape[-1], x.shape[-1], 3, 3))
    for s in (-1, 0, 1):
        for t in (-1, 0, 1):
            dw[:, :, s + 1, t + 1] = np.einsum("bpqo,bpqi->oi", dy, x[:, clamped(H, s)][:, :, clamped(W, t)])
    return dw


def conv(x, w, b, dy, prec):
    """x (B,H,W,Cin), w (Cout,Cin,3,3), b (Cout,) or None, dy (B,H,W,Cout): float64 values of the storage type -> {name: (ref, bound)} for y, dx, dw,
    db (db with b only)."""
    x, w, dy = CR.f64(x), CR.f64(w), CR.f64(dy)
    B, H, W, Cin = x.shape
    Cout = w.shape[0]
    bb = np.zeros(Cout) if b is None else CR.f64(b)
    out = {}
    y, e_y, _ = conv3x3(x, w, bb, prec)
    out["y"] = (y, e_y)
    dx = dgrad_core(dy, w)
    out["dx"] = (dx, store(dx, (9 * Cout + C_EPI) * U32 * dgrad_core(np.abs(dy), np.abs(w)), prec))
    dw = wgrad_core(dy, x)
    out["dw"] = (dw, store(dw, (B * H * W + C_EPI) * U32 * wgrad_core(np.abs(dy), np.abs(x)), prec))
    if b is not None:
        db = dy.sum((0, 1, 2))
        out["db"] = (db, store(db, (B * H * W + C_EPI) * U32 * np.abs(dy).sum((0, 1, 2)), prec))
    return out


FAMILIES = CR.CONV_FAMILIES            # random, coded, offset


def inputs(B, H, W, Cin, Cout, family, seed=0):
    """x, w, bias from core_reference.conv_inputs and an incoming gradient dy ~ N(0, 1); coded: dy carries conv_inputs' ramp as well, so that a gradient
    tap taken from the wrong pixel moves the result; offset: dy + 0.25, so that the long sums over the pixels do not cancel.  float32."""
    x, w, b = conv_inputs(B, H, W, Cin, Cout, family, seed)
    dy = np.random.default_rng([seed + 1, B, H, W, Cin, Cout]).standard_normal((B, H, W, Cout))
    if family == "coded":
        dy = dy + (0.25 * np.arange(H)[:, None] + 0.03125 * np.arange(W)[None, :])[None, :, :, None]
    elif family == "offset":
        dy = dy + 0.25
    return x, w, b, dy.astype(np.float32)


HW = CR.CONV_HW                        # (1,1) (1,17) (2,2) (17,1) (15,16) (16,17) (33,18): every border case, one pixel, one row, one column
SWEEP_B = 2                            # a tap must not cross into the next image; 2 H W = 2 ... 1188 pixels cross PIXEL_TILE up to nine times


def sweep_channels(prec):
    """(Cin, Cout) pairs that cross the K tile (64 fp16 / 32 fp32) and the 128 tile in both roles (Cin is the output width of the input gradient)."""
    c = CR.chunk(prec)
    return ((c, c), (32, 64), (72, 136), (136, 72))


LARGE = (1, 96, 128, 64, 64)           # (B, H, W, Cin, Cout)
SPLIT = (2, 45, 47, 72, 136)           # 4230 pixels = 67 fp16 / 133 fp32 K tiles over 18 tiles of dw: the split engages, its last part ragged


def split_of(pixels, Cin, Cout, prec):
    """The documented rule (include/moge_hip.h) -> (parts, K tiles per part): as many splits of the pixels as bring the 9 ceil(Cin / 128) ceil(Cout / 128)
    tiles of dw to FILL workgroups, each keeping at least MIN_KTILES K tiles, MAX_SPLIT at the most; the parts are equal counts of K tiles, the last takes
    what is left, and only parts that have work are counted."""
    tiles = 9 * -(-Cin // CHANNEL_TILE) * -(-Cout // CHANNEL_TILE)
    ktiles = -(-pixels // k_tile(prec))
    if not ktiles:
        return 1, 1
    per = -(-ktiles // max(1, min(FILL // tiles, ktiles // MIN_KTILES, MAX_SPLIT)))
    return -(-ktiles // per), per


def expected_split(pixels, Cin, Cout, prec):
    return split_of(pixels, Cin, Cout, prec)[0]


def expected_workspace(B, H, W, Cin, Cout, prec):
    """(forward bytes, backward bytes): the repacked weight; behind it the fp32 partials of dw and those of db, each rounded up to 16 bytes."""
    up = lambda n: -(-n // 16) * 16                    # noqa: E731
    pixels = B * H * W
    fwd = up(9 * Cin * Cout * (2 if prec == 1 else 4))
    slabs = max(1, min(-(-pixels // DB_ROWS), DB_MAX))
    return fwd, fwd + 4 * expected_split(pixels, Cin, Cout, prec) * 9 * Cin * Cout + up(4 * slabs * Cout)


@functools.lru_cache(maxsize=None)
def case(B, H, W, Cin, Cout, family, prec):
    """The seeded inputs as float32 arrays of storage-type values and the reference of every product; built once, never modified."""
    x, w, b, dy = (to_storage(t, prec) for t in inputs(B, H, W, Cin, Cout, family))
    return dict(x=x.astype(np.float32), w=w.astype(np.float32), b=b.astype(np.float32), dy=dy.astype(np.float32), ref=conv(x, w, b, dy, prec))
