"""float64 references, with per-element error bounds, of the trainable ConvTranspose2d(kernel 2, stride 2) (moge_amd.convt, csrc/convt_grad.hip,
DESIGN.md section 22), written from the definitions and not from the kernels, on inputs ALREADY rounded to the storage type.  x (B,H,W,Cin),
w (Cin,Cout,2,2), y and dy (B,2H,2W,Cout), taps i, j in {0, 1}:

    y [b, 2p+i, 2q+j, o] = bias[o] + sum_c x[b,p,q,c] w[c,o,i,j]
    dx[b,p,q,c]          = sum_{i,j} sum_o dy[b, 2p+i, 2q+j, o] w[c,o,i,j]
    dw[c,o,i,j]          = sum_{b,p,q} x[b,p,q,c] dy[b, 2p+i, 2q+j, o]           db[o] = sum over the 4 B H W pixels of dy[., ., ., o]

tests/test_convt_reference_cpu.py checks them against torch's float64 autograd of F.conv_transpose2d(x, w, b, stride=2), holds an honest fp32 emulation
inside every bound and a list of injected faults outside.  tests/test_hip_convt.py compares element by element: |got - ref| <= bound.

The bounds follow tests/conv_reference.py and tests/core_reference.py (convt2x2, store, C_EPI are used here): u = 2^-24, h = 2^-11,
    e_y  = (Cin + C_EPI) u (|b| + sum |x| |w|)                 e_dx = (4 Cout + C_EPI) u [the dx formula on |dy|, |w|]
    e_dw = (B H W + C_EPI) u [the dw formula on |dy|, |x|]     e_db = (4 B H W + C_EPI) u sum |dy|
and an fp16 store adds h (|ref| + e) + 2^-25.  (n - 1) u is Higham's bound for a sum of n terms in ANY order, so it covers every tiling, the order of
the four taps of the input gradient inside one accumulator and the split of the pixels in the weight gradient, whose partials stay fp32.  Every dx
element is a sum of exactly 4 Cout products, every y element of Cin, every dw element of B H W.

The kernels' own constants, named here so that the shapes below can be seen to cross them: low-resolution pixels are tiled in ONE dimension,
PIXEL_TILE = 128 consecutive indices of the flat (b, p, q) order; columns (the 4 Cout (tap, o) pairs of the forward, Cin of the input gradient) in
tiles of 128; the contraction in K tiles of 64 fp16 / 32 fp32 elements - Cin in the forward, the 4 Cout (tap, o) pairs in the input gradient, pixels in
the weight gradient, whose split keeps at least MIN_KTILES of them and aims at FILL workgroups, MAX_SPLIT at the most; db in slabs of at least DB_ROWS
high-resolution pixels."""
import functools

import numpy as np

import core_reference as CR
from core_reference import C_EPI, U32, conv_inputs, convt2x2, store, to_storage          # noqa: F401  (re-exported for the tests)

PIXEL_TILE, CHANNEL_TILE = 128, 128
FILL, MIN_KTILES, MAX_SPLIT = 512, 8, 64
DB_ROWS, DB_MAX = 512, 256


def k_tile(prec):
    return 8 * CR.chunk(prec)


def taps_of(dy):
    """dy (B,2H,2W,Cout) -> (B,H,W,2,2,Cout): [b,p,q,i,j] = dy[b, 2p+i, 2q+j]."""
    B, H2, W2, Cout = dy.shape
    return dy.reshape(B, H2 // 2, 2, W2 // 2, 2, Cout).transpose(0, 1, 3, 2, 4, 5)


def dgrad_core(dy, w):
    """dy (B,2H,2W,Cout), w (Cin,Cout,2,2) float64 -> (B,H,W,Cin)."""
    return np.einsum("bpqijo,coij->bpqc", taps_of(dy), w)


def wgrad_core(dy, x):
    """dy (B,2H,2W,Cout), x (B,H,W,Cin) float64 -> (Cin,Cout,2,2)."""
    return np.einsum("bpqc,bpqijo->coij", x, taps_of(dy))


def convt(x, w, b, dy, prec):
    """x (B,H,W,Cin), w (Cin,Cout,2,2), b (Cout,) or None, dy (B,2H,2W,Cout): float64 values of the storage type -> {name: (ref, bound)} for y, dx,
    dw, db (db with b only)."""
    x, w, dy = CR.f64(x), CR.f64(w), CR.f64(dy)
    B, H, W, Cin = x.shape
    Cout = w.shape[1]
    bb = np.zeros(Cout) if b is None else CR.f64(b)
    out = {}
    y, e_y, _ = convt2x2(x, w, bb, prec)
    out["y"] = (y, e_y)
    dx = dgrad_core(dy, w)
    out["dx"] = (dx, store(dx, (4 * Cout + C_EPI) * U32 * dgrad_core(np.abs(dy), np.abs(w)), prec))
    dw = wgrad_core(dy, x)
    out["dw"] = (dw, store(dw, (B * H * W + C_EPI) * U32 * wgrad_core(np.abs(dy), np.abs(x)), prec))
    if b is not None:
        db = dy.sum((0, 1, 2))
        out["db"] = (db, store(db, (4 * B * H * W + C_EPI) * U32 * np.abs(dy).sum((0, 1, 2)), prec))
    return out


FAMILIES = CR.CONV_FAMILIES            # random, coded, offset


def inputs(B, H, W, Cin, Cout, family, seed=0):
    """x, w, bias from core_reference.conv_inputs (transposed) and an incoming gradient dy ~ N(0, 1) on the (2H, 2W) grid; coded: dy carries the ramp
    of the high-resolution pixel as well, so that a gradient tap taken from the wrong pixel moves the result; offset: dy + 0.25, so that the long sums
    over the pixels do not cancel.  conv_inputs draws the four taps of w independently: they differ, as a tap swap would otherwise be invisible (the
    reference model initialises the four taps equal).  float32."""
    x, w, b = conv_inputs(B, H, W, Cin, Cout, family, seed, transposed=True)
    dy = np.random.default_rng([seed + 1, B, H, W, Cin, Cout]).standard_normal((B, 2 * H, 2 * W, Cout))
    if family == "coded":
        dy = dy + (0.25 * np.arange(2 * H)[:, None] + 0.03125 * np.arange(2 * W)[None, :])[None, :, :, None]
    elif family == "offset":
        dy = dy + 0.25
    return x, w, b, dy.astype(np.float32)


HW = ((1, 1), (1, 17), (17, 1), (2, 2), (15, 16), (16, 17), (33, 18))      # one pixel, one row, one column; rows that end inside a 128-pixel tile
SWEEP_B = 2                            # a tap must not land in the next image; 2 H W = 2 ... 1188 pixels cross PIXEL_TILE up to nine times


def sweep_channels(prec):
    """(Cin, Cout): all four taps inside one 128-column tile of the forward at Cout = 32 (and at the chunk), taps that straddle column tiles at
    Cout = 72 and 136, ragged K tiles in every product (Cin = 72, 136 in the forward; 4 Cout = 288, 544 in the input gradient)."""
    c = CR.chunk(prec)
    return ((c, c), (32, 64), (72, 136), (136, 72))


ROWS = (1, 3, 300, 64, 32)             # (B, H, W, Cin, Cout): an image row of 300 pixels spans three 128-pixel tiles, no tile edge on a row end; S = 1 (fp16), 3 (fp32)
SPLIT = (2, 45, 47, 72, 136)           # 4230 pixels = 67 fp16 / 133 fp32 K tiles over 8 tiles of dw: S = 8 (7 x 9 + 4) in fp16, S = 15 (14 x 9 + 7) in fp32
SPLIT_S = {0: 15, 1: 8}                # the S the rule gives at SPLIT, by precision (see test_convt_reference_cpu.py)


def split_of(pixels, Cin, Cout, prec):
    """The documented rule (include/moge_hip.h) -> (parts, K tiles per part): as many splits of the low-resolution pixels as bring the
    4 ceil(Cin / 128) ceil(Cout / 128) tiles of dw to FILL workgroups, each keeping at least MIN_KTILES K tiles, MAX_SPLIT at the most; the parts are
    equal counts of K tiles, the last takes what is left, and only parts that have work are counted."""
    tiles = 4 * -(-Cin // CHANNEL_TILE) * -(-Cout // CHANNEL_TILE)
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
    fwd = up(4 * Cin * Cout * (2 if prec == 1 else 4))
    slabs = max(1, min(-(-4 * pixels // DB_ROWS), DB_MAX))
    return fwd, fwd + 4 * expected_split(pixels, Cin, Cout, prec) * 4 * Cin * Cout + up(4 * slabs * Cout)


@functools.lru_cache(maxsize=None)
def case(B, H, W, Cin, Cout, family, prec):
    """The seeded inputs as float32 arrays of storage-type values and the reference of every product; built once, never modified."""
    x, w, b, dy = (to_storage(t, prec) for t in inputs(B, H, W, Cin, Cout, family))
    return dict(x=x.astype(np.float32), w=w.astype(np.float32), b=b.astype(np.float32), dy=dy.astype(np.float32), ref=convt(x, w, b, dy, prec))
