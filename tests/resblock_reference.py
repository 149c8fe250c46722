"""float64 references, with per-element error bounds, of the fused residual-block convs (moge_amd.resblock, csrc/conv_grad.hip's FUSE / RELU flavours,
DESIGN.md section 24), built on tests/conv_reference.py and written from the definitions, on inputs ALREADY rounded to the storage type.  With conv,
dgrad, wgrad of conv_reference and, element by element on the stored value,

    relu(v) = v > 0 ? v : 0        mask(v) = v > 0 ? 1 : 0        (a positive subnormal passes, -0 and +0 give 0, a NaN gives 0)

    y  = b + conv(relu(x), w) + res                       res (B,H,W,Cout) or None
    dx = mask(x) . dgrad(dy, w) + add                     add (B,H,W,Cin) or None; the mask SELECTS: an inf under a masked element gives 0
    dw = wgrad(dy, relu(x))        db = sum of dy over the pixels

The bounds, stated before the first GPU run and derived, not tuned: u = 2^-24, store and C_EPI as in conv_reference,
    e_y  = store((9 Cin  + C_EPI + 1) u (|b| + |res| + conv(|relu x|, |w|)))
    e_dx = store((9 Cout + C_EPI + 1) u (mask . dgrad(|dy|, |w|) + |add|))
    e_dw, e_db = conv_reference's on relu(x)                                    (each with the underflow term below)
The + 1 is the one extra fp32 addition of res / add into the accumulator before the single rounding; it stays in the bound where the operand is None.
ReLU and the mask are exact (a comparison and a select), so they add no error of their own.

Underflow.  The input family below puts the smallest fp32 subnormal into x, which conv_reference's family never does, and "n u |sum|" is a bound on
ROUNDING only: a product like dy . 2^-149 is not a float32 at all, so a dw element of the one-pixel image whose only live terms are such products
(its exact value is ~ 0.7 . 2^-149, its bound 4 u of that) cannot be met by ANY fp32 arithmetic - the honest CPU emulation fails it as well.  Every
fp32 bound here therefore carries, beside u per operation, the smallest NORMAL float32 per operation: each of the n + C_EPI (+ 1) products and
additions may lose less than TINY32 = 2^-126 to underflow, whether the hardware rounds into the subnormals or flushes them.  That is (n + C) 2^-126
<= 1e-34 absolute at these shapes, a property of the number format and not of the kernels; it is nothing beside any element whose terms are normal
numbers.  The fp16 bounds are the issue's as stated: 2^-24 times a weight is a normal float32, and the store's 2^-25 is already there.

tests/test_resblock_reference_cpu.py checks these against torch's float64 autograd, holds an honest fp32 emulation inside every bound and a list of
injected faults outside; tests/test_hip_resblock.py compares the kernels element by element: |got - ref| <= bound.

The input family is conv_reference.inputs with x modified, per the generator's seed: 1/8 of its elements +0, 1/8 -0, 1/16 plus or minus the smallest
subnormal of the storage type (2^-24 fp16, 2^-149 fp32); res and add ~ N(0, 1)."""
import functools

import numpy as np

import conv_reference as VR
from conv_reference import C_EPI, U32, conv3x3_core, dgrad_core, store, to_storage, wgrad_core          # noqa: F401  (re-exported for the tests)

TINY32 = 2.0 ** -126                   # the smallest normal float32: what one fp32 operation can lose to underflow


def tiny(prec):
    return TINY32 if prec == 0 else 0.0
SUBNORMAL = {0: 2.0 ** -149, 1: 2.0 ** -24}
NAMES = ("y", "dx", "dw", "db")


def relu(v):
    return np.where(v > 0, v, 0.0)


def mask(v):
    return (v > 0).astype(np.float64)


def worst(got, ref_bound):
    """max |got - ref| / bound"""
    ref, bound = ref_bound
    return float((np.abs(got - ref) / bound).max())


def cores(x, w, dy):
    """The sums of relu_conv that do not depend on b, res and add - the expensive part, shared by the references with and without res / add."""
    x, w, dy = (np.asarray(t, dtype=np.float64) for t in (x, w, dy))
    rx = relu(x)
    return dict(y=conv3x3_core(rx, w), y_abs=conv3x3_core(np.abs(rx), np.abs(w)), g=dgrad_core(dy, w), g_abs=dgrad_core(np.abs(dy), np.abs(w)), dw=wgrad_core(dy, rx),
                dw_abs=wgrad_core(np.abs(dy), np.abs(rx)))


def relu_conv(x, w, b, dy, res, add, prec, core=None):
    """x (B,H,W,Cin), w (Cout,Cin,3,3), b (Cout,) or None, dy (B,H,W,Cout), res (B,H,W,Cout) or None, add (B,H,W,Cin) or None: float64 values of the
    storage type -> {name: (ref, bound)} for y, dx, dw, db (db with b only), and "unmasked": dgrad(dy, w) before the mask.  core: cores(x, w, dy)."""
    x, w, dy = (np.asarray(t, dtype=np.float64) for t in (x, w, dy))
    B, H, W, Cin = x.shape
    Cout = w.shape[0]
    k = core or cores(x, w, dy)
    bb = np.zeros(Cout) if b is None else np.asarray(b, dtype=np.float64)
    rr = np.zeros((B, H, W, Cout)) if res is None else np.asarray(res, dtype=np.float64)
    aa = np.zeros((B, H, W, Cin)) if add is None else np.asarray(add, dtype=np.float64)
    out = {}
    y = bb + k["y"] + rr
    out["y"] = (y, store(y, (9 * Cin + C_EPI + 1) * (U32 * (np.abs(bb) + np.abs(rr) + k["y_abs"]) + tiny(prec)), prec))
    dx = np.where(x > 0, k["g"], 0.0) + aa              # a select: an infinite g under a masked element gives 0
    out["dx"] = (dx, store(dx, (9 * Cout + C_EPI + 1) * (U32 * (np.where(x > 0, k["g_abs"], 0.0) + np.abs(aa)) + tiny(prec)), prec))
    out["unmasked"] = k["g"]
    out["dw"] = (k["dw"], store(k["dw"], (B * H * W + C_EPI) * (U32 * k["dw_abs"] + tiny(prec)), prec))
    if b is not None:
        db = dy.sum((0, 1, 2))
        out["db"] = (db, store(db, (B * H * W + C_EPI) * (U32 * np.abs(dy).sum((0, 1, 2)) + tiny(prec)), prec))
    return out


def block(x, w1, b1, w2, b2, dy):
    """The whole block in float64, nothing rounded between the stages: h = conv1(relu x), y = x + conv2(relu h), and the gradients of (x, w1, b1, w2,
    b2) for the incoming dy -> dict of arrays.  (The GPU test judges each stage with relu_conv on the device's own stored h and dh instead.)"""
    x, w1, b1, w2, b2, dy = (np.asarray(t, dtype=np.float64) for t in (x, w1, b1, w2, b2, dy))
    h = b1 + conv3x3_core(relu(x), w1)
    y = x + b2 + conv3x3_core(relu(h), w2)
    dh = mask(h) * dgrad_core(dy, w2)
    dx = dy + mask(x) * dgrad_core(dh, w1)
    return dict(h=h, y=y, dh=dh, dx=dx, dw2=wgrad_core(dy, relu(h)), db2=dy.sum((0, 1, 2)), dw1=wgrad_core(dh, relu(x)), db1=dh.sum((0, 1, 2)))


def special_x(x, prec, key):
    """x with 1/8 of its elements +0, 1/8 -0 and 1/16 plus or minus the smallest subnormal of the storage type, chosen by the generator of `key`."""
    rng = np.random.default_rng(key)
    r, sign = rng.random(x.shape), np.where(rng.random(x.shape) < 0.5, -1.0, 1.0)
    x = np.array(x, dtype=np.float64)
    x[r < 0.125] = 0.0
    x[(r >= 0.125) & (r < 0.25)] = -0.0
    sub = (r >= 0.25) & (r < 0.3125)
    x[sub] = (sign * SUBNORMAL[prec])[sub]
    return x


def inputs(B, H, W, Cin, Cout, family, prec, seed=0):
    """conv_reference.inputs' x, w, b, dy with x through special_x, and res (B,H,W,Cout), add (B,H,W,Cin) ~ N(0, 1): float64 values of the storage
    type (2^-149 is a float32, 2^-24 a float16, so the rounding keeps them)."""
    x, w, b, dy = VR.inputs(B, H, W, Cin, Cout, family, seed)
    rng = np.random.default_rng([seed + 3, B, H, W, Cin, Cout])
    res, add = rng.standard_normal((B, H, W, Cout)), rng.standard_normal((B, H, W, Cin))
    x = special_x(to_storage(x, prec), prec, [seed + 2, B, H, W, Cin, Cout])
    return (x,) + tuple(to_storage(t, prec) for t in (w, b, dy, res, add))


@functools.lru_cache(maxsize=None)
def case(B, H, W, Cin, Cout, family, prec):
    """The seeded inputs (float64 arrays of storage-type values; x keeps its -0 and subnormals) and the references with and without res / add; built
    once, never modified."""
    x, w, b, dy, res, add = inputs(B, H, W, Cin, Cout, family, prec)
    k = cores(x, w, dy)
    return dict(x=x, w=w, b=b, dy=dy, res=res, add=add, ref=relu_conv(x, w, b, dy, res, add, prec, k), ref_plain=relu_conv(x, w, b, dy, None, None, prec, k))
