"""float64 references, with per-element error bounds, for the matrix-core kernels: GEMM (csrc/gemm.hip, csrc/gemm_pp.hip), the 3x3 conv, its x2
resampler form and ConvTranspose2d (csrc/conv_pp.hip and the generic path of gemm.hip), attention forward (csrc/attention_pp.hip, csrc/attention.hip) and
the LayerNorm statistics the latency-regime GEMM finalises itself (gemm_glds_kernel, GemmArgs::ln_mr_out).

Every reference is written from the definition of the operation, not from the kernel, on inputs ALREADY rounded to the storage type
(tail_reference.to_storage), and is checked on the CPU against an independent torch float64 formulation in tests/test_core_reference_cpu.py, which also
holds an honest float64 emulation of each kernel inside the bound and a list of injected faults outside it.  tests/test_hip_core_kernels.py compares
element by element: |got - ref| <= bound(element).

How the bounds are derived
--------------------------
u = 2^-24 (unit roundoff of fp32), h = 2^-11 (of fp16), 2^-25 = half the spacing of the fp16 subnormals.

Dot products (GEMM, conv, ConvTranspose2d):  y = act(sum_k a_k w_k + bias).
  e_pre = (n + C_EPI) u (|bias| + sum_k |a_k w_k|)
n = number of products; (n - 1) u is Higham's bound for a sum of n terms in ANY order (Accuracy and Stability of Numerical Algorithms, section 4.2), so it
holds for every tiling, K split and slab order of the kernels.  It is rigorous for the fp32 MFMA, which the kernel guide documents as a k-ordered fmaf
chain: one rounding per step, product and addition together, n roundings in all.  An fp16 x fp16 product is exact in fp32.  The guide does not document
the internal summation of the fp16 MFMA (v_mfma_f32_16x16x32_f16 / 32x32x16): ASSUMPTION - its adds are no worse than correctly rounded fp32 additions
in some order.  (A truncating adder would need 2 (n + C_EPI) u; nothing measured asks for it - the observed fractions are in the docstring of
tests/test_hip_core_kernels.py.)  C_EPI = 2: the bias addition of epilogue4 (gemm.hip) / the conv epilogues,
and one spare for the final fp32 rounding of the value itself.  K is zero-padded to the 16-byte chunk by the test entry: exact.
Through the activation:
  ReLU           keeps e_pre
  GELU, fp16     gelu_fast (common.h; gemm.hip and gemm_pp.hip use it for fp16 storage): 1.13 e_pre + 1e-5.  1.13 >= max |gelu'| = 1.1290; 1e-5 is the fit +
                 evaluation allowance of tests/test_hip_gemm_pp.py::test_fast_gelu_matches_erf_gelu, established there for |x| <= 12.5 (asserted here: 12)
  GELU, fp32     gelu_erf = 0.5 x (1 + erff(x / sqrt 2)) (gemm.hip epilogue4, TT<float>): 1.13 e_pre + 6 u |x| + 4 u |gelu|.  erff to K_ULP = 4 ulp of a value
                 <= 1 is 8 u absolute, times 0.5 |x| = 4 u |x|; the two roundings of the argument move erf by at most 2 u max(z erf'(z)) < u, times 0.5 |x|;
                 1 + erf rounds once (u (1 + erf), times 0.5 |x| = u |gelu|), the two products round once each (2 u |gelu|): 4.5 u |x| + 3 u |gelu| in all.
fp16 store: + h (|ref| + e) + 2^-25.

3x3 conv: replicate padding = index clamping; n = 9 Cin.  relu_in is exact.
x2 resampler (up2): the DEFINITION is F.interpolate(scale 2, bilinear, align_corners False) followed by the replicate-padded 3x3 conv at the high
resolution.  The kernel runs it as four low-resolution 3x3 phase convs whose weights combine the 9 taps with the interpolation weights in fp32 and are rounded
ONCE to the storage type (pack_phase_conv_kernel).  CHOSEN: the reference keeps the definition with the caller's fp32 weights, and the weight rounding is BOUNDED,
  e_pre = (9 Cin + C_EPI + 10) u A + [fp16: h A],   A = |bias| + conv3x3(|w|; up2(|x|)) >= sum |Weff x|  (triangle inequality on the combination)
10 u: each combined weight is a 9-term fp32 sum of one-rounding products (the interpolation factors .75 .25 and their products are exact).
conv_up2_phase() is the other choice - the four phase convs with the combined weights rounded by the reference itself (float64 combination, one rounding;
the kernel's fp32 combination can land on the other side of an fp16 tie, which that form does not bound) - kept to MEASURE the two against each other
(test_hip_core_kernels.py prints both fractions; EXPERIMENTS.md records them) and to check the phase algebra on the CPU.
ConvTranspose2d k2 s2: y[2i+dy, 2j+dx, co] = bias[co] + sum_ci x[i, j, ci] w[ci, co, dy, dx]; n = Cin.

Attention forward:  o_i = sum_j p_ij v_j,  p_ij = exp(s_ij - m_i) / l_i,  s = q k^T / 8,  m_i = max_j s_ij,  l_i = sum_j exp(s_ij - m_i) >= 1.
A relative error eps_ij of the j-th weight that enters numerator AND denominator moves o_id by p_ij eps_ij (v_jd - o_id), first order and exact in
|v_jd - o_id| (no triangle inequality):
  e_id = sum_j p_ij eps_ij |v_jd - o_id|                                   weights
       + [fp16] h sum_j p_ij |v_jd| + 2^-25 (sum_j |v_jd| + N |o_id|) / l_i   see (b), (c)
       + (N + ntiles + 8) u (sum_j p_ij |v_jd| + |o_id|)                    fp32 sums of the numerator (P V chain) and of l, see (d)
       + [fp16] h |o_id| + 2^-25                                           the store
  eps_ij = expm1(ds_ij) + K_ULP 2^-23 [+ h, fp16: P rounded to fp16],       K_ULP 2^-23: v_exp_f32 / exp2f
  ds_ij  = [fp16: h, fp32: 0] a_ij + 2 u a_ij + 68 u (a_ij + max_j |s_ij|) [+ fp16: 2^-25 ln 2 sum_d |k_jd|],      a_ij = sum_d |q_id k_jd| / 8
What reading the two kernels changed in that model:
 (a) the scale.  Both kernels take q' = q log2(e) / 8 from the QKV epilogue (the test entry: fp32 product with the fp32 constant, then the conversion to the
     storage type): h a_ij in fp16 (+ the subnormal term for tiny q'), 2 u a_ij in fp32 (the constant's and the product's roundings); nothing is scaled after
     the dot product.  The fp16 kernel starts the K Q^T MFMA chain from -m (the deferred max), the fp32 kernel subtracts m afterwards: 64 products and the
     max enter one fp32 sum either way, 68 u (a_ij + |m|), |m| <= max_j |s_ij| for the true and for any stale max (m_stale is a score of an earlier tile).
 (b) attention_pp.hip forms l from the fp16-ROUNDED P in the hot loop (row sums on the matrix pipe: numerator and denominator share the rounding, which is what
     the (v - o) form needs) but from the UNROUNDED fp32 P in exact_block - the first tile, the masked last tile, the first tile of the second key range of
     attn_pp16ks_kernel and every tile that trips the overflow guard.  There the rounding of P is in the numerator only: + h sum_j p_ij |v_jd|, taken over ALL
     keys so that the bound does not depend on which tiles a dispatch runs exactly.  N <= 64 is one exact tile: the term is what those cases need.
 (c) P is formed against a stale max that is at most the true max, so every row sum is >= l_i >= 1 and P can fall into the fp16 subnormals (absolute 2^-25 per
     weight): shared weights move o by |v_jd - o_id|, numerator-only ones by |v_jd|; |v_jd| + |o_id| covers both.
 (d) ntiles = ceil(N / 64): the exact path rescales O and l by alpha once per exact tile (every tile in attention.hip); + 8: the combine of the key-split kernel
     (two exp2, two products, one sum), 1 / l and the final product.  l's own summation error N u l moves o by N u |o_id|.
 (e) fp32 (attention.hip): true running max, P stays fp32 (no h, no 2^-25 terms), l from the same P as the numerator.
expm1 instead of the first-order ds keeps the second order of large score errors (a dominant key with a_ij ~ 100 has ds ~ 0.05).

LN statistics of the fused finalize.  The producer epilogue writes (sum, sum of squares) of every 32-column group of the updated row: quad sums (depth 2 / 3
with the squares' product and fma), two shuffles, one add: |part1 - exact| <= 5 u sum_group |x|, |part2 - exact| <= 6 u sum_group x^2.  (mean, rstd) are then
tail_reference.ln_finalize's formula on those partials, with its bound (NP = N / 32 partials, any order).  The third check needs no partials at all: the moments of the
returned stream with every element its own partial (NP = N: Higham's any-order bound for the whole row, one more rounding for the squares inside its + 3).
"""
import functools
import math

import numpy as np
import torch

import tail_reference as TR
from tail_reference import K_ULP, U32, to_storage          # noqa: F401  (to_storage: re-exported for the tests)

H16 = 2.0 ** -11
SUB16 = 2.0 ** -25
C_EPI = 2
GELU_SLOPE = 1.13
GELU_FAST_FIT = 1e-5
GELU_FAST_RANGE = 12.0


def f64(x):
    return np.asarray(x, dtype=np.float64)


def store(ref, e, prec):
    return e + H16 * (np.abs(ref) + e) + SUB16 if prec == 1 else e


def gelu(x):
    return 0.5 * x * (1.0 + torch.erf(torch.from_numpy(np.ascontiguousarray(x)) / math.sqrt(2.0)).numpy())


def activate(pre, e, act, prec):
    """act 0 none, 1 ReLU, 2 GELU: (value, bound before the store)."""
    if act == 0:
        return pre, e
    if act == 1:
        return np.maximum(pre, 0.0), e
    ref = gelu(pre)
    if prec == 1:
        assert np.abs(pre).max() <= GELU_FAST_RANGE, "gelu_fast's fit allowance is established for |x| <= 12.5"
        return ref, GELU_SLOPE * e + GELU_FAST_FIT
    return ref, GELU_SLOPE * e + U32 * (6 * np.abs(pre) + 4 * np.abs(ref))


def finish(pre, mag, n, act, prec, extra=0.0):
    e = (n + C_EPI) * U32 * mag + extra
    ref, e = activate(pre, e, act, prec)
    return ref, store(ref, e, prec), pre


def gemm(A, W, bias, act, prec):
    """act(A W^T + bias): A (M,K), W (N,K) float64 already rounded to storage, bias (N) fp32 values or None -> (ref, bound, pre-activation)."""
    A, W = f64(A), f64(W)
    b = np.zeros(W.shape[0]) if bias is None else f64(bias)
    return finish(A @ W.T + b, np.abs(A) @ np.abs(W).T + np.abs(b), A.shape[1], act, prec)


def conv3x3_core(x, w):
    """Replicate-padded (index-clamped) 3x3 cross-correlation: x (B,H,W,Cin), w (Cout,Cin,3,3) float64 -> (B,H,W,Cout)."""
    B, H, W, _ = x.shape
    out = np.zeros((B, H, W, w.shape[0]))
    for dy in range(3):
        yy = np.clip(np.arange(H) + dy - 1, 0, H - 1)
        for dx in range(3):
            xx = np.clip(np.arange(W) + dx - 1, 0, W - 1)
            out += x[:, yy][:, :, xx] @ w[:, :, dy, dx].T
    return out


def conv3x3(x, w, bias, prec, relu_in=False, act=0):
    """x (B,H,W,Cin), w (Cout,Cin,3,3) float64 already rounded to storage, bias (Cout) -> (ref, bound, pre-activation)."""
    x, w, b = f64(x), f64(w), f64(bias)
    if relu_in:
        x = np.maximum(x, 0.0)
    return finish(conv3x3_core(x, w) + b, conv3x3_core(np.abs(x), np.abs(w)) + np.abs(b), 9 * x.shape[-1], act, prec)


def up2_axis(n):
    """Source taps of F.interpolate(scale_factor=2, mode='bilinear', align_corners=False) along one axis: (i0, i1, l1) per destination index."""
    src = np.maximum((np.arange(2 * n) + 0.5) / 2.0 - 0.5, 0.0)
    i0 = np.minimum(np.floor(src).astype(np.int64), n - 1)
    i1 = np.minimum(i0 + 1, n - 1)
    return i0, i1, src - i0


def up2(x):
    """Bilinear x2 of x (B,H,W,C) float64 (the weights .25 / .75 and their products are exact)."""
    y0, y1, ly = up2_axis(x.shape[1])
    x0, x1, lx = up2_axis(x.shape[2])
    rows = x[:, y0] * (1 - ly)[None, :, None, None] + x[:, y1] * ly[None, :, None, None]
    return rows[:, :, x0] * (1 - lx)[None, None, :, None] + rows[:, :, x1] * lx[None, None, :, None]


def conv_up2(x, w, bias, prec):
    """conv3x3(bilinear x2 (x)) + bias at the high resolution: x (B,H,W,Cin) rounded to storage, w (Cout,Cin,3,3) the caller's fp32 weights (the kernel rounds the
    COMBINED phase weights, bounded here) -> (ref (B,2H,2W,Cout), bound, pre)."""
    x, w, b = f64(x), f64(w), f64(bias)
    pre = conv3x3_core(up2(x), w) + b
    mag = conv3x3_core(up2(np.abs(x)), np.abs(w)) + np.abs(b)
    return finish(pre, mag, 9 * x.shape[-1] + 10, 0, prec, extra=H16 * mag if prec == 1 else 0.0)


UP2_R = np.array([[[.75, .25, 0.], [.25, .75, 0.], [0., .75, .25]], [[.25, .75, 0.], [0., .75, .25], [0., .25, .75]]])      # R[parity][dy][a]


def phase_weights(w, prec):
    """The four low-resolution 3x3 kernels of the x2 resampler, (py,px,Cout,3,3,Cin): float64 combination of the fp32 weights, rounded once to storage."""
    weff = np.einsum("oiyx,pya,qxb->pqoabi", f64(w), UP2_R, UP2_R)
    return to_storage(weff, prec) if prec == 1 else weff.astype(np.float32).astype(np.float64)


def conv_up2_phase(x, w, bias, prec, weff=None):
    """The same operation as four phase convs with the reference's own rounded combined weights: (ref, bound); the bound has no weight-rounding term."""
    x, b = f64(x), f64(bias)
    B, H, W, Cin = x.shape
    weff = phase_weights(w, prec) if weff is None else weff
    Cout = weff.shape[2]
    pre, mag = np.zeros((B, 2 * H, 2 * W, Cout)), np.zeros((B, 2 * H, 2 * W, Cout))
    for py in range(2):
        for px in range(2):
            wp = weff[py, px].transpose(0, 3, 1, 2)                # (Cout,Cin,3,3)
            pre[:, py::2, px::2] = conv3x3_core(x, wp) + b
            mag[:, py::2, px::2] = conv3x3_core(np.abs(x), np.abs(wp)) + np.abs(b)
    ref, bound, _ = finish(pre, mag, 9 * Cin, 0, prec)
    return ref, bound


def convt2x2(x, w, bias, prec):
    """ConvTranspose2d(k 2, s 2): x (B,H,W,Cin), w (Cin,Cout,2,2) float64 already rounded to storage -> (ref (B,2H,2W,Cout), bound, pre)."""
    x, w, b = f64(x), f64(w), f64(bias)
    B, H, W, Cin = x.shape
    Cout = w.shape[1]
    pre = np.einsum("bhwc,coyx->bhywxo", x, w).reshape(B, 2 * H, 2 * W, Cout) + b
    mag = np.einsum("bhwc,coyx->bhywxo", np.abs(x), np.abs(w)).reshape(B, 2 * H, 2 * W, Cout) + np.abs(b)
    return finish(pre, mag, Cin, 0, prec)


def attention(q, k, v, prec):
    """softmax(q k^T / 8) v: q, k, v (B,nh,N,64) already rounded to storage (numpy or torch) -> (ref, bound) as float64 numpy (B,N,nh 64)."""
    q, k, v = (torch.as_tensor(np.asarray(t, dtype=np.float64)) if not torch.is_tensor(t) else t.double() for t in (q, k, v))
    B, nh, N, hd = q.shape
    ntiles = (N + 63) // 64
    ref, bound = torch.empty(B, N, nh, hd, dtype=torch.float64), torch.empty(B, N, nh, hd, dtype=torch.float64)
    rows = max(1, (1 << 22) // (N * hd))
    for b in range(B):
        for h in range(nh):
            Q, Kk, V = q[b, h], k[b, h], v[b, h]
            s = Q @ Kk.T / 8.0
            a = Q.abs() @ Kk.abs().T / 8.0
            m = s.max(1, keepdim=True).values
            p = torch.exp(s - m)
            l = p.sum(1, keepdim=True)
            p = p / l
            o = p @ V
            smax = s.abs().max(1, keepdim=True).values
            ds = (2 + 68) * U32 * a + 68 * U32 * smax
            if prec == 1:
                ds = ds + H16 * a + SUB16 * math.log(2.0) * Kk.abs().sum(1)[None, :]
            w = (p * (torch.expm1(ds) + K_ULP * 2.0 ** -23 + (H16 if prec == 1 else 0.0))).float()
            del s, a, ds
            # the O(N^2 64) term in float32 (a bound needs no more: its own rounding, 3e-7 relative at N = 3601, is covered by the factor below)
            e = torch.empty(N, hd, dtype=torch.float32)
            V32, o32 = V.float(), o.float()
            for r0 in range(0, N, rows):
                r1 = min(N, r0 + rows)
                e[r0:r1] = (w[r0:r1, :, None] * (V32[None, :, :] - o32[r0:r1, None, :]).abs()).sum(1)
            e = e.double() * (1 + 1e-5) + 4 * U32 * (w.double() @ (V.abs() + o.abs().max()))           # (... and the float32 rounding of v - o itself)
            pv = p @ V.abs()
            e = e + (N + ntiles + 8) * U32 * (pv + o.abs())
            if prec == 1:
                e = e + H16 * pv + SUB16 * (V.abs().sum(0)[None, :] + N * o.abs()) / l
                e = e + H16 * o.abs() + SUB16
            ref[b, :, h], bound[b, :, h] = o, e
    return ref.reshape(B, N, nh * hd).numpy(), bound.reshape(B, N, nh * hd).numpy()


def ln_partials(x, group=32):
    """(sum, sum of squares) of every `group` columns of x (rows, N) float64 -> part (rows, N / group, 2) and the bound of the producer epilogue's fp32 tree."""
    x = f64(x)
    g = x.reshape(x.shape[0], x.shape[1] // group, group)
    part = np.stack([g.sum(-1), (g * g).sum(-1)], -1)
    bound = np.stack([5 * U32 * np.abs(g).sum(-1), 6 * U32 * (g * g).sum(-1)], -1)
    return part, bound


def ln_stats(part, D):
    """(mean, rstd) (rows, 2) of the finalize formula on the given partials and its bound (tail_reference.ln_finalize)."""
    mean, e_mean, rstd, e_rstd = TR.ln_finalize(part, D)
    return np.stack([mean, rstd], -1), np.stack([e_mean, e_rstd], -1)


def ln_stats_of_stream(x):
    """The same from the stream itself (rows, N): every element its own partial."""
    x = f64(x)
    return ln_stats(np.stack([x, x * x], -1), x.shape[1])


# ---------------------------------------------------------------------------------------------------------------------
# seeded input families (CPU, float32; the callers round them with to_storage)
# ---------------------------------------------------------------------------------------------------------------------
def gemm_inputs(M, N, K, family, seed=0):
    """random: A ~ N(0,1), W ~ N(0,1) / sqrt(K), |bias| >= 0.25.  offset: both with a common positive mean (A + 0.5, (W + 0.125) / sqrt(K): sums that do not
    cancel, sqrt(K) / 16 on average) and bias >= 2, so that a ReLU cannot hide a column whose bias is missing (sum and bias both negative); the
    pre-activation stays below the 12 of the GELU allowance up to K = 1024."""
    rng = np.random.default_rng([seed, M, N, K])
    A, W, r = rng.standard_normal((M, K)), rng.standard_normal((N, K)), rng.standard_normal(N)
    bias = np.sign(r) * (0.25 + np.abs(r))
    if family == "offset":
        A, W, bias = A + 0.5, W + 0.125, 2.0 + 0.5 * np.abs(r)
    else:
        assert family == "random"
    return A.astype(np.float32), (W / math.sqrt(K)).astype(np.float32), bias.astype(np.float32)


def conv_inputs(B, H, W, Cin, Cout, family, seed=0, transposed=False):
    """x (B,H,W,Cin), w (Cout,Cin,3,3) (transposed: (Cin,Cout,2,2)), bias.  coded: x plus the ramp 0.25 y + 0.03125 x (exact in fp16) in every channel: a tap
    taken from the wrong pixel shifts the result.  offset: |x| + 0.5 (every activation positive: a ReLU prologue cannot turn the one product a fault drops
    into an exact zero, which at a 1 x 1 image is the only one there is), w with a positive mean, bias positive."""
    rng = np.random.default_rng([seed, B, H, W, Cin, Cout])
    x = rng.standard_normal((B, H, W, Cin))
    w = rng.standard_normal((Cin, Cout, 2, 2) if transposed else (Cout, Cin, 3, 3))
    r = rng.standard_normal(Cout)
    if family == "coded":
        x = x + (0.25 * np.arange(H)[:, None] + 0.03125 * np.arange(W)[None, :])[None, :, :, None]
    elif family == "offset":
        x, w = np.abs(x) + 0.5, w + 0.25
    else:
        assert family == "random"
    bias = np.sign(r) * (0.25 + np.abs(r))
    if family == "offset":
        bias = np.abs(bias)
    return x.astype(np.float32), (w / math.sqrt(Cin * (1 if transposed else 9))).astype(np.float32), bias.astype(np.float32)


def attention_inputs(B, nh, N, family, seed=0):
    """random: q ~ 1.5 N(0,1), k, v ~ N(0,1), one spiked value row (N // 2) and, from N > 80, one dominant key (N // 2 + 3 aligned with query 5).
    offset: the same with v + 3 (the normalisation 1 / l becomes visible in every output).  neg_scores: q + 8 e_0, k - 8 e_0 without the dominant key: every
    real score is near -8, so a key the kernel should not see (score 0) outweighs the whole row."""
    g = torch.Generator().manual_seed(1000 * seed + N)
    q, k, v = (torch.randn(B, nh, N, 64, generator=g) for _ in range(3))
    q = q * 1.5
    v[:, :, N // 2] += 5.0
    if family == "neg_scores":
        q[..., 0] += 8.0
        k[..., 0] -= 8.0
    else:
        if N > 80:
            k[:, :, N // 2 + 3] = q[:, :, 5] * 6.0
        if family == "offset":
            v = v + 3.0
        else:
            assert family == "random"
    return q.numpy(), k.numpy(), v.numpy()


# ---------------------------------------------------------------------------------------------------------------------
# the sweep: shapes that straddle each tile, shared by the CPU power tests and the GPU tests; every case is built once (lru_cache) and never modified
# ---------------------------------------------------------------------------------------------------------------------
GEMM_M = (1, 63, 64, 65, 127, 129, 257)
GEMM_N = (4, 32, 36, 64, 68, 128, 132, 256, 260)
FAMILIES = ("random", "offset")


def chunk(prec):
    """Elements per 16-byte chunk of the storage type: the K granularity of the kernels (TT<T>::CH)."""
    return 8 if prec == 1 else 4


def gemm_ks(prec):
    return (chunk(prec), 40, 64, 72, 128, 1024)


def gemm_cases(prec):
    """(M, N, K, act, family): every (N, K) pair with two M of the list, rotated so that every kernel of launch_gemm (by N: 128 x 32, 128 x 64, 128 x 128; a K
    that is no multiple of 64 elements (fp32: 32) keeps the generic kernel, the others open the direct-to-LDS kernels from N > 64, N % 256 == 0 with M >= 256 the
    ping-pong kernels) sees a row tail, several row blocks, a column tail where it allows one, one K slab and several.  Plus one K = 4096."""
    out = []
    for i, N in enumerate(GEMM_N):
        for j, K in enumerate(gemm_ks(prec)):
            ms = {GEMM_M[(i + j) % 7], GEMM_M[(i + j + 3) % 7]}
            if N == 256:
                ms.add(257)                       # the only M of the list the ping-pong kernels take
            for t, M in enumerate(sorted(ms)):
                out.append((M, N, K, (i + j + t) % 3, FAMILIES[(i + t) % 2]))
    out.append((65, 132, 4096, 0, "random"))
    out.append((257, 256, 4096, 1, "random"))
    return out


@functools.lru_cache(maxsize=None)
def gemm_case(M, N, K, act, family, prec):
    A, W, bias = gemm_inputs(M, N, K, family)
    ref, bound, pre = gemm(to_storage(A, prec), to_storage(W, prec), bias, act, prec)
    return dict(A=A, W=W, bias=bias, ref=ref, bound=bound, pre=pre)


CONV_HW = ((1, 1), (1, 17), (2, 2), (17, 1), (15, 16), (16, 17), (33, 18))
# Cin 32: the generic kernel in both precisions; Cin % 64 == 0: conv_pp in fp16 - 64 / 128 output columns per workgroup (Cout 64 / a multiple of 128), one halo buffer (Cin 64) or two
CONV_CH = ((32, 32), (32, 64), (32, 68), (64, 64), (64, 128), (128, 64), (128, 128), (192, 256))
CONV_FAMILIES = ("random", "coded", "offset")


def conv_cases():
    """(B, H, W, Cin, Cout, relu_in, act, family): every (H, W) with every channel pair; B = 2 at (2, 2) and (15, 16)."""
    out = []
    for i, (H, W) in enumerate(CONV_HW):
        for j, (Cin, Cout) in enumerate(CONV_CH):
            out.append((2 if (H, W) in ((2, 2), (15, 16)) else 1, H, W, Cin, Cout, (i + j) % 2, ((i + j) // 2) % 2, CONV_FAMILIES[(i + 2 * j) % 3]))
    return out


@functools.lru_cache(maxsize=None)
def conv_case(B, H, W, Cin, Cout, relu_in, act, family, prec):
    x, w, bias = conv_inputs(B, H, W, Cin, Cout, family)
    ref, bound, pre = conv3x3(to_storage(x, prec), to_storage(w, prec), bias, prec, bool(relu_in), act)
    return dict(x=x, w=w, bias=bias, ref=ref, bound=bound, pre=pre)


UP2_CASES = [(B, H, W, Cin, Cout, fam) for (Cin, Cout) in ((64, 32), (128, 64))
             for (B, H, W, fam) in ((1, 1, 1, "random"), (2, 2, 3, "coded"), (1, 16, 16, "offset"), (1, 17, 9, "coded"))]


@functools.lru_cache(maxsize=None)
def up2_case(B, H, W, Cin, Cout, family, prec):
    x, w, bias = conv_inputs(B, H, W, Cin, Cout, family)
    xs = to_storage(x, prec)
    ref, bound, _ = conv_up2(xs, w, bias, prec)
    ref_p, bound_p = conv_up2_phase(xs, w, bias, prec)
    return dict(x=x, w=w, bias=bias, ref=ref, bound=bound, ref_phase=ref_p, bound_phase=bound_p)


CONVT_CASES = [(B, H, W, 128, Cout, fam) for Cout in (64, 128) for (B, H, W, fam) in ((1, 1, 1, "random"), (2, 1, 9, "offset"), (1, 6, 9, "random"), (1, 17, 16, "offset"))]


@functools.lru_cache(maxsize=None)
def convt_case(B, H, W, Cin, Cout, family, prec):
    x, w, bias = conv_inputs(B, H, W, Cin, Cout, family, transposed=True)
    ref, bound, _ = convt2x2(to_storage(x, prec), to_storage(w, prec), bias, prec)
    return dict(x=x, w=w, bias=bias, ref=ref, bound=bound)


ATTN_N = (1, 15, 16, 17, 63, 64, 65, 127, 128, 129, 255, 256, 257)
ATTN_SMALL = [(B, nh, N) for (B, nh) in ((1, 1), (2, 3)) for N in ATTN_N]
ATTN_LARGE = [(1, 2, 1370), (1, 1, 3601)]
ATTN_FAMILIES = ("random", "offset", "neg_scores")


@functools.lru_cache(maxsize=None)
def attention_case(B, nh, N, family, prec):
    """q, k, v as float32 arrays of storage-type values, and the float64 reference with its bound."""
    q, k, v = (to_storage(t, prec) for t in attention_inputs(B, nh, N, family))
    ref, bound = attention(q, k, v, prec)
    return dict(q=q.astype(np.float32), k=k.astype(np.float32), v=v.astype(np.float32), ref=ref, bound=bound)


FUSED_LN_CASES = [(M, N, K) for M in (1, 63, 64, 65, 129, 300) for N in (128, 384, 1024) for K in (64, 1024)]
