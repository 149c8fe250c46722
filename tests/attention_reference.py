"""float64 reference of the trainable attention (moge_amd.attention, csrc/attention_grad.hip), written from the formulas and not
from the kernels: per (batch, head), with S = Q K^T / 8,

    lse = log sum_j exp(S_ij)      P = exp(S - lse)      O = P V
    D = rowsum(dO o O)             dV = P^T dO           dS = P o (dO V^T - D) / 8       dQ = dS K       dK = dS^T Q

reference() is that and nothing else.  attention_grad() is the same arithmetic with a per-element error bound beside every tensor, on inputs ALREADY
rounded to the storage type, in the style of core_reference.attention and linear_reference.linear.  tests/test_attention_reference_cpu.py checks both
against torch's float64 autograd of F.scaled_dot_product_attention, holds an honest float64 emulation of the four kernels inside every bound and a list
of injected faults outside.  tests/test_hip_attention_grad.py compares element by element: |got - ref| <= bound(element).

How the bounds are derived
--------------------------
u = 2^-24 (U32, unit roundoff of fp32), h = 2^-11 (H16, of fp16), 2^-25 (SUB16) = half the spacing of the fp16 subnormals, K_ULP 2^-23 = 2 K_ULP u the
relative error allowed to exp2f / log2f (tail_reference.K_ULP ulp).  (n - 1) u is Higham's bound for a sum of n terms in ANY order (Accuracy and
Stability of Numerical Algorithms, section 4.2): it covers the order of the tiles, the split of a row between the two lane halves, and the different
summation orders of the two backward kernels, which recompute the same P and dS with the roles of lane and register exchanged.  It is rigorous for the
fp32 MFMA, which the kernel guide documents as a k-ordered fmaf chain (one rounding per step, product and addition together); an fp16 x fp16 product
is exact in fp32, and - core_reference's ASSUMPTION, stated again - the internal adds of the fp16 MFMA (v_mfma_f32_32x32x16_f16), which the guide does
not document, are taken to be no worse than correctly rounded fp32 additions in some order.  Where a count below is one more than the roundings named,
the spare one pays for the second-order products of the others (64 u * 64 u << u).  FLUSH = 2^-126: an fp32 operation may flush a subnormal operand or
result; every gradient bound carries (N + 64) FLUSH (1 + max |input|), which nothing but a row of probabilities below 1e-38 can reach.

Notation, per (batch, head): s_ij = sum_d q_id k_jd / 8, a_ij = sum_d |q_id k_jd| / 8, m_i = max_j s_ij, l_i = sum_j exp(s_ij - m_i) >= 1, p_ij =
exp(s_ij - m_i) / l_i, smax_i = max_j |s_ij|, nt = ceil(N / 64) key tiles.

Scores (all three kernels).  The chain over head_dim is 64 MFMA products on the UNSCALED q as stored: |chain - sum q k| <= 64 u sum |q k|.  No h a_ij
term, unlike the infer() kernels whose q is pre-scaled in storage.  The forward then multiplies by the fp32 constant AG_SCALE2 = fl(log2 e) / 8 (relative
error u, the 1/8 exact) with one rounding (`sc[h][r] *= AG_SCALE2`): in natural-log units
    ds_ij = 65 u a_ij + 2 u |s_ij|.

Forward (attn_fwd_kernel).  A true running max; p~ = exp2f(t - m_new) with the subtraction rounded (u |s_ij - m~| <= u (|s_ij| + smax_i) for any
running max m~) and exp2f's K_ULP:
    eps_ij = expm1(ds_ij + u (|s_ij| + smax_i)) + K_ULP 2^-23.
expm1 keeps the second order of a dominant key (a_ij ~ 100).  The fp32 p~ enters `psum` (l) AND, in fp32, the P V product: a relative error delta_j
shared by numerator and denominator moves o_id by sum_j p_ij delta_j (v_jd - o_id) / (1 + sum_j p_ij delta_j) exactly.  With w_ij = p_ij eps_ij,
W_i = sum_j w_ij and Cauchy-Schwarz (so that no N x N x 64 array is needed and nothing is bounded across the cancellation v - o by a triangle inequality),
    sum_j w_ij |v_jd - o_id| <= sqrt(W_i sum_j w_ij (v_jd - o_id)^2) = sqrt(W_i ((w v^2)_id - 2 o_id (w v)_id + o_id^2 W_i)),   divided by 1 - W_i.
alpha = exp2f(m_run - m_new) multiplies O and l alike, once per 64-key tile: its own error cancels in O / l; the two products round (nt each).  l is
summed from the UNROUNDED fp32 p~ (32 of a tile's 64 keys per lane half, `l_run * alpha + psum`, one add across the halves); then 1 / l and the product,
each rounded once (the build has no fast-math: the division is correctly rounded):
    e_o = sqrt(...) / (1 - W_i) + (N + 2 nt + 4) u (sum_j p_ij |v_jd| + |o_id|)
        + [fp16] h sum_j p_ij |v_jd| + 2^-25 sum_j |v_jd| / l_i                       P rounded to fp16 (ag_pack) in the numerator ONLY, in every tile
        + [fp16] h (|o_id| + e) + 2^-25                                               the store (core_reference.store)
The fp16 P is formed against a running max that is at most the true one, so a weight can fall into the fp16 subnormals: 2^-25 absolute, which the
final 1 / l_i (l_i taken against the true max, >= 1) scales.  core_reference.attention's o-bound is not reused: it allows the h a_ij of a pre-scaled q,
the 2^-25 N |o| of a rounded P in the denominator and the key-split combine, none of which this kernel has.

lse = (m_run + log2f(l_tot)) AG_LN2.  log sum_j exp(s_ij + delta_j) - log sum_j exp(s_ij) <= -log1p(-W_i) (the max cancels exactly, whichever score is
taken for it); l's sum (N u, any order), the nt rescales by alpha (2 roundings and exp2f's K_ULP each; the rounded differences m_run - m_new telescope
to at most 2 smax_i), log2f at K_ULP on |log l_i|, the addition on |m_i| + |log l_i|, the constant AG_LN2 and its product on |lse_i|:
    e_lse = -log1p(-W_i) + (N + 2 nt + 2 K_ULP nt) u + 2 u smax_i + 2 K_ULP u |log l_i| + u (|m_i| + |log l_i|) + 2 u |lse_i|.

D (attn_delta_kernel): a 64-term fmaf chain on the O the forward STORED; the reference's D uses the exact O:
    e_D,i = sum_d |dO_id| e_o,id + 65 u sum_d |dO_id| (|o_id| + e_o,id).
e_o is the forward's own bound, fp16 store included, so a D taken from the unstored fp32 O is inside as well: the bound does not demand the rounding.
d_from_out() bounds the delta kernel ALONE, against rowsum(dO o O_returned): 65 u sum_d |dO_id O_id|.

P in the backward (attn_bwd_kv_kernel, attn_bwd_q_kernel): exp2f(fmaf(chain, AG_SCALE2, -fl(lse AG_LOG2E))), NOT self-normalised, so the whole error
of the stored lse shows.  Chain 64 u a_ij, the constant u |s_ij|, the fmaf's single rounding u |s_ij - lse_i|, `rl * AG_LOG2E` (constant and product)
2 u |lse_i|:
    eps'_ij = expm1(65 u a_ij + u |s_ij| + u |s_ij - lse_i| + 2 u |lse_i| + e_lse,i) + K_ULP 2^-23,      e_P,ij = p_ij eps'_ij + FLUSH
    [fp16, ag_pack]  e_P16,ij = e_P,ij + h (p_ij + e_P,ij) + 2^-25.
P of padded rows (queries in the dk / dv kernel, keys in the dq kernel) is forced to 0: exact, no term.

dV_jd = sum_i p_ij dO_id (N products on the matrix pipe, the padded ones exactly 0):
    e_dV = sum_i e_P[16],ij |dO_id| + (N + 2) u sum_i (p_ij + e_P[16],ij) |dO_id|, then the store.

dS_ij = p_ij (dP_ij - D_i), dP_ij = sum_d dO_id v_jd a 64-product chain (b_ij = sum_d |dO_id v_jd|), the subtraction and the product rounded once each.
|dP_ij - D_i| is taken exactly, element by element: no triangle inequality across the cancellation.
    e_dS,ij = e_P,ij |dP_ij - D_i| + (p_ij + e_P,ij) (65 u b_ij + e_D,i + 2 u |dP_ij - D_i|)  [+ fp16, ag_pack: h (|dS_ij| + e) + 2^-25].

dQ_id = sum_j dS_ij k_jd / 8, dK_jd = sum_i dS_ij q_id / 8 (N products; `* 0.125f` is exact, the spare rounding of N + 2 is its allowance):
    e_dQ = (sum_j e_dS,ij |k_jd| + (N + 2) u sum_j (|dS_ij| + e_dS,ij) |k_jd|) / 8, then the store; dK the same with q over i.
"""
import functools

import numpy as np
import torch

from core_reference import H16, SUB16, store
from tail_reference import K_ULP, U32, to_storage

FLUSH = 2.0 ** -126
EXP_ULP = K_ULP * 2.0 ** -23
NAMES = ("o", "lse", "D", "dq", "dk", "dv")


def reference(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, do: torch.Tensor) -> dict:
    """q, k, v, do (B, nh, N, 64) of any float dtype -> float64 CPU tensors o, dq, dk, dv (B, nh, N, 64) and lse (B, nh, N).  One (batch, head)
    at a time, so that N = 3601 needs one N x N matrix at a time."""
    q, k, v, do = (t.detach().to("cpu", torch.float64) for t in (q, k, v, do))
    B, nh, N, _ = q.shape
    res = {name: torch.empty_like(q) for name in ("o", "dq", "dk", "dv")}
    res["lse"] = torch.empty(B, nh, N, dtype=torch.float64)
    for b in range(B):
        for h in range(nh):
            Q, K, V, dO = q[b, h], k[b, h], v[b, h], do[b, h]
            S = Q @ K.T / 8.0
            m = S.max(dim=1, keepdim=True).values
            lse = m + torch.log(torch.exp(S - m).sum(dim=1, keepdim=True))
            P = torch.exp(S - lse)
            O = P @ V
            D = (dO * O).sum(dim=1, keepdim=True)
            dS = P * (dO @ V.T - D) / 8.0
            res["o"][b, h], res["lse"][b, h] = O, lse[:, 0]
            res["dv"][b, h], res["dq"][b, h], res["dk"][b, h] = P.T @ dO, dS @ K, dS.T @ Q
    return res


def _f64(t):
    return t.detach().to("cpu", torch.float64).numpy() if torch.is_tensor(t) else np.asarray(t, dtype=np.float64)


def attention_grad(q, k, v, do, prec) -> dict:
    """q, k, v, do (B, nh, N, 64), values of the storage type (prec 1 = fp16; numpy or torch) -> {name: (ref, bound)} as float64 numpy arrays for
    o, dq, dk, dv (B, nh, N, 64) and lse, D (B, nh, N).  The module docstring derives every term."""
    q, k, v, do = (_f64(t) for t in (q, k, v, do))
    B, nh, N, hd = q.shape
    assert hd == 64
    nt = (N + 63) // 64
    floor = (N + 64) * FLUSH * (1.0 + max(float(np.abs(t).max()) for t in (q, k, v, do)))
    out = {n: (np.empty((B, nh, N, hd)), np.empty((B, nh, N, hd))) for n in ("o", "dq", "dk", "dv")}
    out.update({n: (np.empty((B, nh, N)), np.empty((B, nh, N))) for n in ("lse", "D")})
    for b in range(B):
        for h in range(nh):
            Q, K, V, dO = q[b, h], k[b, h], v[b, h], do[b, h]
            aQ, aK, aV, adO = np.abs(Q), np.abs(K), np.abs(V), np.abs(dO)
            S = Q @ K.T / 8.0
            aS = np.abs(S)
            a = aQ @ aK.T / 8.0
            m = S.max(1, keepdims=True)
            p = np.exp(S - m)
            l = p.sum(1, keepdims=True)
            p = p / l
            logl = np.log(l)
            lse = m + logl
            smax = aS.max(1, keepdims=True)
            o = p @ V
            # ---- forward
            w = p * (np.expm1(65 * U32 * a + 2 * U32 * aS + U32 * (aS + smax)) + EXP_ULP)
            W = w.sum(1, keepdims=True)
            assert float(W.max()) < 0.5
            wv2 = w @ (V * V)
            var = wv2 - 2.0 * o * (w @ V) + o * o * W
            var = np.maximum(var, 0.0) + 1e-14 * (wv2 + o * o * W)             # the float64 rounding of the cancellation above
            pv = p @ aV
            e_o = np.sqrt(W * var) / (1.0 - W) + (N + 2 * nt + 4) * U32 * (pv + np.abs(o))
            if prec == 1:
                e_o = e_o + H16 * pv + SUB16 * aV.sum(0)[None, :] / l
            e_o = store(o, e_o, prec)
            e_lse = (-np.log1p(-W) + (N + 2 * nt + 2 * K_ULP * nt) * U32 + 2 * U32 * smax + 2 * K_ULP * U32 * np.abs(logl) + U32 * (np.abs(m) + np.abs(logl))
                     + 2 * U32 * np.abs(lse))
            # ---- D
            D = (dO * o).sum(1, keepdims=True)
            e_D = (adO * e_o).sum(1, keepdims=True) + 65 * U32 * (adO * (np.abs(o) + e_o)).sum(1, keepdims=True)
            # ---- P, dV
            e_P = p * (np.expm1(65 * U32 * a + U32 * aS + U32 * np.abs(S - lse) + 2 * U32 * np.abs(lse) + e_lse) + EXP_ULP) + FLUSH
            del w, a, aS
            e_P16 = e_P + H16 * (p + e_P) + SUB16 if prec == 1 else e_P
            dv = p.T @ dO
            e_dv = e_P16.T @ adO + (N + 2) * U32 * ((p + e_P16).T @ adO)
            del e_P16
            # ---- dS, dQ, dK
            T = dO @ V.T - D
            dS = p * T
            aT = np.abs(T)
            e_dS = e_P * aT + (p + e_P) * (65 * U32 * (adO @ aV.T) + e_D + 2 * U32 * aT)
            del T, aT, e_P
            if prec == 1:
                e_dS = e_dS + H16 * (np.abs(dS) + e_dS) + SUB16
            dq = dS @ K / 8.0
            e_dq = (e_dS @ aK + (N + 2) * U32 * ((np.abs(dS) + e_dS) @ aK)) / 8.0
            dk = dS.T @ Q / 8.0
            e_dk = (e_dS.T @ aQ + (N + 2) * U32 * ((np.abs(dS) + e_dS).T @ aQ)) / 8.0
            del dS, e_dS
            for name, ref, e in (("o", o, e_o), ("lse", lse[:, 0], e_lse[:, 0]), ("D", D[:, 0], e_D[:, 0])):
                out[name][0][b, h], out[name][1][b, h] = ref, e
            for name, ref, e in (("dq", dq, e_dq), ("dk", dk, e_dk), ("dv", dv, e_dv)):
                out[name][0][b, h], out[name][1][b, h] = ref, store(ref, e + floor, prec)
    return out


def d_from_out(out, do):
    """The delta kernel alone: rowsum(dO o O) of the O the forward RETURNED, out and do (B, nh, N, 64) storage values -> (ref, bound) (B, nh, N)."""
    out, do = _f64(out), _f64(do)
    return (out * do).sum(-1), 65 * U32 * np.abs(out * do).sum(-1)


# ---------------------------------------------------------------------------------------------------------------------
# seeded input families (float32; the callers round them with to_storage) and the sweep, shared by the CPU power tests and the GPU tests
# ---------------------------------------------------------------------------------------------------------------------
FAMILIES = ("random", "offset", "neg_scores", "saturated")
EDGES = (1, 2, 31, 32, 33, 63, 64, 65, 127, 128, 129, 200, 257)
SWEEP_N = tuple(sorted(EDGES + (95, 96, 97, 255, 256)))         # a third 32-query tile (fp32), a half-full second 64-query tile (fp16), two full workgroups
SMALL = [(B, nh, N) for (B, nh) in ((1, 1), (2, 3)) for N in SWEEP_N]
LARGE = [(1, 2, 1370), (1, 1, 3601)]


def inputs(B, nh, N, family):
    """q, k, v, do (B, nh, N, 64) float32.
    random: q ~ 1.5 N(0,1), k, v, do ~ N(0,1), one spiked value row (N // 2: a transposed or permuted key order cannot pass), one spiked gradient row
    (N // 3: nor a permuted query order) and, from N > 80, one dominant key (N // 2 + 3, aligned with query 5: a_ij ~ 100).
    offset: the same with v + 3 and do + 0.25: D is large and dP - D cancels, so an error in D or in 1 / l shows in every element.
    neg_scores: q + 8 e_0, k - 8 e_0, no dominant key: every real score is near -8, so a padded key or query that is not masked (score 0 against a zero
    row) outweighs the whole row.
    saturated: q x 12 (no dominant key): score differences of tens of units, most probabilities exactly 0 in fp32 - the rescale across key tiles in the
    forward and exp(S - lse) in the backward."""
    assert family in FAMILIES
    g = torch.Generator().manual_seed(N)
    q, k, v, do = (torch.randn(B, nh, N, 64, generator=g) for _ in range(4))
    q = q * (1.5 * 8 if family == "saturated" else 1.5)
    v[:, :, N // 2] += 5.0
    do[:, :, N // 3] += 5.0
    if family == "neg_scores":
        q[..., 0] += 8.0
        k[..., 0] -= 8.0
    elif family != "saturated" and N > 80:
        k[:, :, N // 2 + 3] = q[:, :, 5] * 6.0
    if family == "offset":
        v, do = v + 3.0, do + 0.25
    return q, k, v, do


@functools.lru_cache(maxsize=None)
def case(B, nh, N, family, prec):
    """The seeded inputs as float32 arrays of storage-type values (`inputs`, a tuple q, k, v, do) and {name: (ref, bound)}; built once, shared by
    every test that asks for the same case, never modified."""
    x = tuple(to_storage(t.numpy(), prec) for t in inputs(B, nh, N, family))
    return dict(inputs=tuple(t.astype(np.float32) for t in x), ref=attention_grad(*x, prec))
