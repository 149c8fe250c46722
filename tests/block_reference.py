"""float64 references, with per-element error bounds, of the rest of a trainable DINOv2 block (moge_amd.block, csrc/block_grad.hip, DESIGN.md section
20), written from the definitions and not from the kernels, on inputs ALREADY rounded to their storage types:

    layer_norm      mu = mean(x), var = mean((x - mu)^2), rstd = 1 / sqrt(var + eps), xh = (x - mu) rstd, n = xh w + b
                    g = dn w, dx = rstd (g - mean(g) - xh mean(g xh)), dw = sum_m dn xh, db = sum_m dn
    gelu            y = 0.5 x (1 + erf(x / sqrt 2)) = x Phi(x),   dx = dy (Phi(x) + x phi(x))
    scale_residual  y = x + r gamma,   dx = dy,   dr = dy gamma,   dgamma = sum_m dy r
    fused           x1 = x + r gamma, n = layer_norm(x1);   dx = dx1 + layer_norm_backward(dn), dr = dx gamma, dgamma = sum_m dx r

tests/test_block_reference_cpu.py checks them against torch's float64 autograd, holds an honest fp32 emulation inside every bound and a list of
injected faults outside.  tests/test_hip_block.py compares element by element: |got - ref| <= bound(element).

How the bounds are derived
--------------------------
u = 2^-24 (U32), h = 2^-11.  First-order propagation of ONE fp32 rounding per operation (an fma is one operation); a sum of n terms in ANY order has
Higham's (n - 1) u sum |terms| (Accuracy and Stability of Numerical Algorithms, section 4.2), which covers the lane-then-butterfly row sums over C and
the slab-then-reducer column sums over M, whose partials stay fp32.  `store` (core_reference) adds the fp16 store, h (|ref| + e) + 2^-25.  C_EPI = 2
spare roundings per sum, as in core_reference.  ASSUMPTIONS on the device math library, stated with their constants: sqrtf and the fp32 division are
within 1 ulp (2 u each; they are correctly rounded in the default build), erff and expf within K_ULP = 4 ulp (8 u relative), the constant
core_reference.activate uses for gelu_erf.

layer_norm forward, one row (A = mean |x|, d = x - mu, D2 = mean d^2 = var):
  e_mu   = (C + C_EPI) u A                                   the sum over C, 1 / C, the product
  e_d    = e_mu + u |d|                                      the subtraction
  e_var  = (C + C_EPI + 4) u var + e_mu^2                    the fma chain over C of d^2, 1 / C and the product; the 2 u var of the roundings of d;
                                                             a common shift delta of every d moves sum d^2 by EXACTLY C delta^2, because sum d = 0 - this
                                                             is what the two-pass form buys, and what a one-pass E[x^2] - mu^2 does not have
  rho    = e_var / (2 (var + eps)) + 5 u                     relative error of rstd: the fma that adds eps (1), sqrt (2), the division (2)
  e_xh   = rstd e_d + |xh| (rho + u)
  e_n    = |w| e_xh + u (|xh w| + |n|)                       one fma (a separate product and sum would stay inside: u |xh w| + u |n|)
layer_norm backward, one row, from the stored x and the COMPUTED (mean, rstd) - so xh carries e_xh:
  g = dn w: u |g|.   m1 = mean(g): e_m1 = (C + C_EPI) u mean |g|.   m2 = mean(g xh): e_m2 = (C + C_EPI + 1) u mean |g xh| + mean(|g| e_xh)
  e_in   = e_m1 + |m2| e_xh + |xh| e_m2 + 3 u (|g| + |m1| + |xh m2|)          g - m1 - xh m2: g's own rounding, the subtraction, the fma
  e_dx   = rstd e_in + |dx| (rho + u)
  e_dw   = (M + C_EPI) u sum_m |dn xh| + sum_m |dn| e_xh,      e_db = (M + C_EPI) u sum_m |dn|
gelu: forward u (6 |x| + 4 |y|) - core_reference.activate's derivation with an exact argument.  Backward, G = Phi + x phi:
  e_Phi  = 4.5 u + 2 u Phi          erff to 4 ulp of a value <= 1 (8 u) and its argument's rounding (u), halved; 1 + erf rounds once (u (1 + erf) = 2 u Phi)
  e_phi  = (x^2 / 2 + 10) u phi     the argument -x^2 / 2 rounds once (relative u, which exp turns into x^2 / 2 u); expf 8 u; the constant and its product 2 u
  e_G    = |x| e_phi + e_Phi + u (|x phi| + |G|),      e_dx = |dy| e_G + u |dx|
scale_residual: e_y = u (|r gamma| + |y|) (one fma; a separate product and sum stay inside), e_dr = u |dr|, e_dgamma = (M + C_EPI) u sum_m |dy r|.
fused: x1 as scale_residual.  The LayerNorm part reads x1 AS STORED, so its reference takes the stored x1 as its input: on the CPU the exact x1 rounded
once, on the GPU the x1 the kernel returned (which has just been held to its own bound).  dx = dx1 + dx_ln: e_dx = e_dx_ln + u |dx|;
dr = dx gamma with dx before its rounding: e_dr = |gamma| e_dx + u |dr|;  e_dgamma = (M + C_EPI) u sum_m |dx r| + sum_m |r| e_dx.
A gradient that is absent (None) is a zero."""
import functools
import math

import numpy as np
import torch

import core_reference as CR
from core_reference import C_EPI, H16, SUB16, chunk, gelu, gemm_inputs, store, to_storage          # noqa: F401  (re-exported for the tests)
from tail_reference import K_ULP, U32

SQRT_ULP = DIV_ULP = 1.0           # ASSUMPTION: sqrtf and the fp32 division within 1 ulp
EPS = 1e-5                         # nn.LayerNorm's default
ROWS_PER_WG, SLAB, MAX_SLABS, MAX_C = 4, 32, 512, 2048        # the kernels' edges (csrc/block_grad.hip): the sweep below straddles them


def f64(x):
    return np.asarray(x, dtype=np.float64)


def fraction(got, ref_bound):
    """Worst |got - ref| / bound; an element whose bound is zero (a value that is passed through, a sum over nothing) must be exact."""
    ref, bound = ref_bound
    err = np.abs(f64(got) - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        fr = np.where(bound > 0, err / bound, np.where(err == 0, 0.0, np.inf))
    return float(fr.max()) if fr.size else 0.0


def _ln_forward(x, w, b, eps):
    """-> values and pre-store bounds of one LayerNorm over the last axis of x (M, C)."""
    C = x.shape[1]
    mu = x.mean(1, keepdims=True)
    d = x - mu
    var = (d * d).mean(1, keepdims=True)
    rstd = 1.0 / np.sqrt(var + eps)
    xh = d * rstd
    n = xh * w + b
    e_mu = (C + C_EPI) * U32 * np.abs(x).mean(1, keepdims=True)
    e_d = e_mu + U32 * np.abs(d)
    e_var = (C + C_EPI + 4) * U32 * var + e_mu ** 2
    rho = e_var / (2.0 * (var + eps)) + (1 + 2 * SQRT_ULP + 2 * DIV_ULP) * U32
    e_xh = rstd * e_d + np.abs(xh) * (rho + U32)
    e_n = np.abs(w) * e_xh + U32 * (np.abs(xh * w) + np.abs(n))
    return dict(mu=mu, rstd=rstd, xh=xh, n=n, e_mu=e_mu, rho=rho, e_xh=e_xh, e_n=e_n)


def _ln_backward(f, w, dn):
    """-> dx, dw, db and their pre-store bounds from _ln_forward's row quantities."""
    M, C = dn.shape
    xh, rstd, e_xh, rho = f["xh"], f["rstd"], f["e_xh"], f["rho"]
    g = dn * w
    m1 = g.mean(1, keepdims=True)
    m2 = (g * xh).mean(1, keepdims=True)
    dx = rstd * (g - m1 - xh * m2)
    e_m1 = (C + C_EPI) * U32 * np.abs(g).mean(1, keepdims=True)
    e_m2 = (C + C_EPI + 1) * U32 * np.abs(g * xh).mean(1, keepdims=True) + (np.abs(g) * e_xh).mean(1, keepdims=True)
    e_in = e_m1 + np.abs(m2) * e_xh + np.abs(xh) * e_m2 + 3 * U32 * (np.abs(g) + np.abs(m1) + np.abs(xh * m2))
    e_dx = rstd * e_in + np.abs(dx) * (rho + U32)
    dw = (dn * xh).sum(0)
    e_dw = (M + C_EPI) * U32 * np.abs(dn * xh).sum(0) + (np.abs(dn) * e_xh).sum(0)
    db = dn.sum(0)
    e_db = (M + C_EPI) * U32 * np.abs(dn).sum(0)
    return dx, e_dx, dw, e_dw, db, e_db


def layer_norm(x, w, b, dn, px, pn, eps=EPS):
    """x (M, C), w, b (C,) of storage px, dn (M, C) of storage pn: float64 values -> {name: (ref, bound)} for n, mean, rstd, dx, dw, db."""
    x, w, b, dn = f64(x), f64(w), f64(b), f64(dn)
    f = _ln_forward(x, w, b, eps)
    dx, e_dx, dw, e_dw, db, e_db = _ln_backward(f, w, dn)
    return {"n": (f["n"], store(f["n"], f["e_n"], pn)), "mean": (f["mu"][:, 0], f["e_mu"][:, 0]), "rstd": (f["rstd"][:, 0], (f["rstd"] * f["rho"])[:, 0]),
            "dx": (dx, store(dx, e_dx, px)), "dw": (dw, store(dw, e_dw, px)), "db": (db, store(db, e_db, px))}


def gelu_pair(x, dy, prec):
    """x, dy (M, C) of one storage type -> {name: (ref, bound)} for y, dx."""
    x, dy = f64(x), f64(dy)
    y = gelu(x)
    e_y = U32 * (6 * np.abs(x) + 4 * np.abs(y))
    t = torch.from_numpy(np.ascontiguousarray(x))
    Phi = (0.5 * (1.0 + torch.erf(t / math.sqrt(2.0)))).numpy()
    phi = np.exp(-0.5 * x * x) / math.sqrt(2.0 * math.pi)
    G = Phi + x * phi
    e_Phi = (0.5 * (2 * K_ULP + 1) + 2 * Phi) * U32
    e_phi = (0.5 * x * x + 2 * K_ULP + 2) * U32 * phi
    e_G = np.abs(x) * e_phi + e_Phi + U32 * (np.abs(x * phi) + np.abs(G))
    dx = dy * G
    return {"y": (y, store(y, e_y, prec)), "dx": (dx, store(dx, np.abs(dy) * e_G + U32 * np.abs(dx), prec))}


def scale_residual(x, r, gamma, dy, px, pr):
    """x, dy (M, C) and gamma (C,) of storage px, r of storage pr -> {name: (ref, bound)} for y, dr, dgamma (the gradient of x is dy itself)."""
    x, r, gamma, dy = f64(x), f64(r), f64(gamma), f64(dy)
    M = x.shape[0]
    y = x + r * gamma
    dr = dy * gamma
    dg = (dy * r).sum(0)
    return {"y": (y, store(y, U32 * (np.abs(r * gamma) + np.abs(y)), px)), "dr": (dr, store(dr, U32 * np.abs(dr), pr)),
            "dgamma": (dg, store(dg, (M + C_EPI) * U32 * np.abs(dy * r).sum(0), px))}


def fused(x, r, gamma, w, b, dx1, dn, px, pr, pn, x1=None, eps=EPS):
    """The fused pair.  x1: the stored x1 the LayerNorm part reads (None: the exact one rounded once to px); dx1 or dn None: a zero.
    -> {name: (ref, bound)} for x1, n, mean, rstd, dx, dr, dgamma, dw, db."""
    x, r, gamma, w, b = f64(x), f64(r), f64(gamma), f64(w), f64(b)
    M = x.shape[0]
    sr = scale_residual(x, r, gamma, np.zeros_like(x), px, pr)
    x1 = to_storage(sr["y"][0], px) if x1 is None else f64(x1)
    f = _ln_forward(x1, w, b, eps)
    out = {"x1": sr["y"], "n": (f["n"], store(f["n"], f["e_n"], pn)), "mean": (f["mu"][:, 0], f["e_mu"][:, 0]), "rstd": (f["rstd"][:, 0], (f["rstd"] * f["rho"])[:, 0])}
    zero = np.zeros_like(x)
    if dn is None:
        dxl, e_dxl, dw, e_dw, db, e_db = zero, zero, np.zeros_like(w), np.zeros_like(w), np.zeros_like(w), np.zeros_like(w)
    else:
        dxl, e_dxl, dw, e_dw, db, e_db = _ln_backward(f, w, f64(dn))
    dx = dxl + (zero if dx1 is None else f64(dx1))
    e_dx = e_dxl + (U32 * np.abs(dx) if dx1 is not None and dn is not None else 0.0)
    dr = dx * gamma
    dg = (dx * r).sum(0)
    out.update({"dx": (dx, store(dx, e_dx, px)), "dr": (dr, store(dr, np.abs(gamma) * e_dx + U32 * np.abs(dr), pr)),
                "dgamma": (dg, store(dg, (M + C_EPI) * U32 * np.abs(dx * r).sum(0) + (np.abs(r) * e_dx).sum(0), px)),
                "dw": (dw, store(dw, e_dw, px)), "db": (db, store(db, e_db, px))})
    return out


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# seeded input families (float32; the callers round them with to_storage): random, and offset - rows with mean about 8 and spread about 1, which a
# one-pass variance does not survive; every incoming gradient + 0.25 there, so that the sums over M do not cancel
# ---------------------------------------------------------------------------------------------------------------------------------------------------
FAMILIES = ("random", "offset")


def inputs(M, C, family, seed=0):
    assert family in FAMILIES
    rng = np.random.default_rng([seed, M, C, FAMILIES.index(family)])
    off, goff = (8.0, 0.25) if family == "offset" else (0.0, 0.0)
    t = dict(x=rng.standard_normal((M, C)) + off, r=rng.standard_normal((M, C)), gamma=0.25 + rng.random(C), w=1.0 + 0.25 * rng.standard_normal(C),
             b=0.25 * rng.standard_normal(C), dn=rng.standard_normal((M, C)) + goff, dx1=rng.standard_normal((M, C)) + goff,
             h=1.5 * rng.standard_normal((M, C)) + (0.5 if family == "offset" else 0.0))
    return {k: v.astype(np.float32) for k, v in t.items()}


PAIRS_LN = ((0, 0), (1, 1), (0, 1))                      # (px, pn)
TRIPLES_SR = ((0, 0), (1, 1), (0, 1))                    # (px, pr); gamma has px
FUSED = ((0, 0, 0), (0, 0, 1), (0, 1, 0), (0, 1, 1), (1, 1, 1))       # (px, pr, pn)


def slab_rows(M):
    return SLAB * max(1, -(-M // (SLAB * MAX_SLABS)))


SWEEP_M = (1, ROWS_PER_WG - 1, ROWS_PER_WG, ROWS_PER_WG + 1, SLAB - 1, SLAB, SLAB + 1, 2 * SLAB + 1)
CAP_M = SLAB * MAX_SLABS + SLAB + 5                      # past the slab-count cap: slabs of 64 rows, 257 of them and a tail of 37 rows
assert slab_rows(CAP_M) == 2 * SLAB and CAP_M % slab_rows(CAP_M) not in (0, slab_rows(CAP_M) - 1)


def sweep_c(unit=8):
    """One chunk, 63 / 64 / 65 chunks (a wave's lanes and its neighbours), 384 and 1024.  A lane's chunk is 8 elements in every storage type (fp32: two
    16-byte accesses), so that every dtype combination sums a row in the same order."""
    return (unit, 63 * unit, 64 * unit, 65 * unit, 384, 1024)


def sweep_shapes(unit=8):
    """Every M of the sweep with one chunk and with 65 chunks; every C of the sweep with M = 5 and M = SLAB + 1; the slab-count cap with one chunk and
    with 17 (the rows and the columns are walked by independent loops: the cap adds nothing at a C the small M have covered, and a float64 reference
    of CAP_M x 1024 is not a few seconds' work); the widest built row at M = 5."""
    shapes = [(M, C) for M in SWEEP_M for C in (unit, 65 * unit)] + [(M, C) for M in (5, SLAB + 1) for C in sweep_c(unit)]
    shapes += [(CAP_M, unit), (CAP_M, 17 * unit), (5, MAX_C)]
    return sorted(set(shapes))


def _st(t, names_precs):
    return {n: to_storage(t[n], p) for n, p in names_precs}


@functools.lru_cache(maxsize=None)
def case_norm(M, C, family, px, pn):
    s = _st(inputs(M, C, family), (("x", px), ("w", px), ("b", px), ("dn", pn)))
    return dict({k: v.astype(np.float32) for k, v in s.items()}, ref=layer_norm(s["x"], s["w"], s["b"], s["dn"], px, pn))


@functools.lru_cache(maxsize=None)
def case_gelu(M, C, family, prec):
    t = inputs(M, C, family)
    s = {"x": to_storage(t["h"], prec), "dy": to_storage(t["dn"], prec)}
    return dict({k: v.astype(np.float32) for k, v in s.items()}, ref=gelu_pair(s["x"], s["dy"], prec))


@functools.lru_cache(maxsize=None)
def case_sr(M, C, family, px, pr):
    s = _st(inputs(M, C, family), (("x", px), ("r", pr), ("gamma", px), ("dx1", px)))
    return dict({k: v.astype(np.float32) for k, v in s.items()}, ref=scale_residual(s["x"], s["r"], s["gamma"], s["dx1"], px, pr))


@functools.lru_cache(maxsize=None)
def case_fused(M, C, family, px, pr, pn):
    """The inputs only: the reference of the LayerNorm part wants the stored x1 (fused())."""
    s = _st(inputs(M, C, family), (("x", px), ("r", pr), ("gamma", px), ("w", px), ("b", px), ("dn", pn), ("dx1", px)))
    return {k: v.astype(np.float32) for k, v in s.items()}
