"""float64 references, with per-element error bounds, for the fused GEMM epilogues a ViT block and the neck entrance run (csrc/gemm.hip epilogue4 /
epilogue_tile32 / epilogue_pair16, csrc/gemm_pp.hip pp_epilogue16): the residual update with the LayerNorm-fold producer outputs (EPI_RESID, EPK_RESID /
EPK_RESID16), the LN-fold consumer (GemmArgs::ln_mr: fc1, EPK_GELU_LN), the row-major QKV scatter with and without the fold (EPI_QKV, EPK_QKV / EPK_QKV_LN),
the neck's 1x1 with the uv term (EPK_UV) and ConvTranspose2d as a GEMM (EPI_CONVT, EPK_CONVT).  core_reference covers the plain stores (bias, none / ReLU /
GELU); this module builds on its finish / activate / store, on its ln_partials / ln_stats and on entrance_reference.linspace32.

Every reference is written from the definition of the operation, on inputs ALREADY rounded to the storage type (tail_reference.to_storage), and returns
(ref, bound) per element.  tests/test_epilogue_reference_cpu.py ties each to an independent torch float64 formulation, holds an honest fp32 emulation of
each epilogue inside the bound and a list of injected faults outside it; tests/test_hip_epilogue_kernels.py compares element by element on the GPU.

How the bounds are derived
--------------------------
u = 2^-24.  acc = sum_k a_k w_k is the MFMA chain: |acc^ - acc| <= K u S, S = sum_k |a_k w_k| (Higham's (n - 1) u for a sum of n terms in ANY order, one more
for the first product of the fp32 chain; core_reference's docstring has the fp16 MFMA assumption).  After the chain every fp32 operation of common.h adds one
rounding u |its result|, and every partial result is no larger than the magnitude sum of the whole expression, so an epilogue with r operations after the
chain is bounded by (K + r) u (magnitude sum).  Counted from common.h:
  resid          x + resid_term(gamma, acc, bias) = x + fmaf(gamma, acc, gamma * bias): the product gamma * bias, the fma, the addition: r = 3, and one
                 spare for the value itself as in core_reference (C_EPI): (K + 4) u (|x| + |gamma| (S + |bias|)) - the bound test_gemm_fused_ln_finalize has used
                 since R18.  fp16 stream (EPK_RESID16, epilogue4's `!g.xres` branch, resid16_quad): x is an fp16 number, the sum is rounded ONCE to fp16: store(., 1).
  ln_consumer    ln_fold_term = fmaf(rstd, fmaf(-mean, c, acc), bias): r = 2 = C_EPI, magnitude |rstd| (S + |mean c|) + |bias|: core_reference.finish with n = K.
  qkv            acc + bias: r = 1 (finish with n = K gives the spare), or the consumer's form with the fold.  q: q_scaled = fp32(v * qscale), made opaque so
                 that it is never fused with the conversion: e_q = qscale e + u |q|, as entrance_reference.qkv.  k, v: nothing more.
  uv_store       uv_term_add(acc + bias, wu, u, wv, v) = fmaf(wu, u, fmaf(wv, v, acc + bias)): r = 3 -> finish with n = K + 1; u(x), v(y) are torch.linspace in
                 fp32 (linspace_at), which the reference takes from entrance_reference.linspace32 (one fused multiply-add per element).  The compiler may leave
                 start + step * i unfused: the product then rounds on its own, u |step i| <= u |u1 - u0| <= 2 ulp32(max |u|), and the sum once more: 3 ulp32(max |u|)
                 per coordinate, times |wu| / |wv| - tail_reference's and entrance_reference's 3 ulp.
  convt          acc + bias4[n]: r = 1; the pixel shuffle moves values, it does not round.
  convt, uv out  epilogue4's EPI_CONVT branch with uv_in = 0 writes `v += wu * u + wv * vv` in plain C++: two products, their sum, the addition (or fewer, where
                 the compiler contracts): r = 1 + 4 -> finish with n = K + 3, + the linspace term over 2 pixW / 2 pixH steps.
then core_reference.activate (ReLU keeps the bound, GELU: its slope and the gelu_fast / erff allowances) and core_reference.store for fp16 storage.
No constant here was fitted to what a GPU returned; the observed fractions are in the docstring of tests/test_hip_epilogue_kernels.py.

The producer outputs of `resid` are checked against the RETURNED stream, not against the reference: x16 must equal fp16(returned xres) bit for bit, ln_part must
be within core_reference.ln_partials(returned stream) (fp16 stream: the statistics are taken from the ROUNDED row, which is the returned stream).

EPI_CONVT with the uv term at the OUTPUT pixel (GemmArgs::uv_in == 0) on the GEMM path: no model_*.hip call site sets it - model_v1.hip is the only caller that
gives an EPI_CONVT GEMM a uv term, and it sets uv_in = 1 (entrance_reference.convt_uv_in); the v2 decoder's uv terms run in conv_pp.hip.  gemm_pp_eligible
refuses `EPI_CONVT && uv.wu`, so only epilogue4 carries the branch: convt_uv_out below is its reference, with one small latency-kernel case in the sweep.

Input families
--------------
core_reference.gemm_inputs (random / offset) plus per-flavour vectors with floors that keep a fault larger than the bound: |bias|, |gamma|, |c|, |mean| >= 0.25,
rstd in [0.5, 2], |wu|, |wv| >= 1; the u and v ranges differ from each other and are not symmetric (a swap of the two, or an index taken from the other end,
moves every element).  The LN-consumer families halve W and keep |mean c| <= 0.75 so that |pre| <= 12 (gelu_fast's allowance; core_reference.activate asserts it).

The sweep (PP_* / LAT_* below) holds the smallest shapes at which each form can go wrong; cases are built once (lru_cache) and never modified.
"""
import functools

import numpy as np

import core_reference as CR
import entrance_reference as ER
import tail_reference as TR
from core_reference import f64
from tail_reference import U32, to_storage

LOG2E_8 = 0.125 * 1.4426950408889634
UV_RANGE = (-0.75, 0.875, -0.4375, 0.625)           # u0, u1, v0, v1: exact in fp32, asymmetric, u and v different


def acc_mag(A, W):
    A, W = f64(A), f64(W)
    return A @ W.T, np.abs(A) @ np.abs(W).T


# ---------------------------------------------------------------------------------------------------------------------
# references
# ---------------------------------------------------------------------------------------------------------------------
def resid(x, A, W, bias, gamma, prec_stream):
    """x + gamma (A W^T + bias): x (M,N) already rounded to the stream's type (prec_stream 1: the fp16 stream, updated with one rounding) -> (ref, bound)."""
    acc, mag = acc_mag(A, W)
    x, b, g = f64(x), f64(bias), f64(gamma)
    ref = x + g * (acc + b)
    e = (A.shape[1] + 4) * U32 * (np.abs(x) + np.abs(g) * (mag + np.abs(b)))
    return ref, CR.store(ref, e, prec_stream)


def fold_pre(A, W, bias, c, mr):
    """rstd (A W^T - mean c) + bias and its magnitude sum: mr (M,2) = (mean, rstd)."""
    acc, mag = acc_mag(A, W)
    b, c, mr = f64(bias), f64(c), f64(mr)
    mean, rstd = mr[:, :1], mr[:, 1:2]
    return rstd * (acc - mean * c) + b, np.abs(rstd) * (mag + np.abs(mean * c)) + np.abs(b)


def ln_consumer(A, W, bias, c, mr, act, prec):
    """act(rstd (A W^T - mean c) + bias), act 0 none / 2 GELU -> (ref, bound)."""
    pre, mag = fold_pre(A, W, bias, c, mr)
    ref, bound, _ = CR.finish(pre, mag, A.shape[1], act, prec)
    return ref, bound


def qkv_rowmajor(A, W, bias, B, Ntok, nh, qscale, prec, mr=None, c=None):
    """q (times qscale), k, v as (B,nh,Ntok,64) (attention.py: qkv(x).reshape(B, N, 3, nh, hd).permute(2, 0, 3, 1, 4)), with the LN fold when mr / c are given:
    dict name -> (ref, bound)."""
    if mr is None:
        acc, mag = acc_mag(A, W)
        pre, mag = acc + f64(bias), mag + np.abs(f64(bias))
    else:
        pre, mag = fold_pre(A, W, bias, c, mr)
    e = (A.shape[1] + CR.C_EPI) * U32 * mag

    def heads(t):
        return t.reshape(B, Ntok, 3, nh, 64).transpose(2, 0, 3, 1, 4)

    val, e = heads(pre), heads(e)
    qs = float(np.float32(qscale))
    q = val[0] * qs
    out = {"q": (q, e[0] * qs + U32 * np.abs(q)), "k": (val[1], e[1]), "v": (val[2], e[2])}
    return {k: (np.ascontiguousarray(r), np.ascontiguousarray(CR.store(r, b, prec))) for k, (r, b) in out.items()}


def uv_planes(uv_range, B, pixH, pixW):
    """u(x), v(y) of every GEMM row m = (b pixH + y) pixW + x, (M,1) each, and the linspace allowance per unit weight of each."""
    u0, u1, v0, v1 = uv_range
    u, v = ER.linspace32(u0, u1, pixW), ER.linspace32(v0, v1, pixH)
    uu = np.broadcast_to(u[None, None, :], (B, pixH, pixW)).reshape(-1, 1)
    vv = np.broadcast_to(v[None, :, None], (B, pixH, pixW)).reshape(-1, 1)
    return uu, vv, 3 * TR.ulp32(max(abs(u0), abs(u1))), 3 * TR.ulp32(max(abs(v0), abs(v1)))


def uv_store(A, W, bias, wu, wv, uv_range, B, pixH, pixW, act, prec):
    """act(A W^T + bias + wu u(x) + wv v(y)), u / v = torch.linspace in fp32 over the pixel columns / rows (v2.py: the uv planes through the 1x1) -> (ref, bound)."""
    acc, mag = acc_mag(A, W)
    b, wu, wv = f64(bias), f64(wu), f64(wv)
    uu, vv, lu, lv = uv_planes(uv_range, B, pixH, pixW)
    pre = acc + b + wu * uu + wv * vv
    mag = mag + np.abs(b) + np.abs(wu * uu) + np.abs(wv * vv)
    ref, bound, _ = CR.finish(pre, mag, A.shape[1] + 1, act, prec, extra=np.abs(wu) * lu + np.abs(wv) * lv)
    return ref, bound


def pixel_shuffle(t, B, pixH, pixW, Cout):
    """GEMM layout (B pixH pixW, 4 Cout), column n = (dy 2 + dx) Cout + co -> (B, 2 pixH, 2 pixW, Cout)."""
    return np.ascontiguousarray(t.reshape(B, pixH, pixW, 2, 2, Cout).transpose(0, 1, 3, 2, 4, 5).reshape(B, 2 * pixH, 2 * pixW, Cout))


def convt(A, W, bias4, B, pixH, pixW, Cout, prec):
    """ConvTranspose2d(k 2, s 2) as the GEMM sees it (the GEMM-side view of core_reference.convt2x2): y[b, 2 i + dy, 2 j + dx, co] = bias4[n] + sum_ci
    A[(b, i, j), ci] W[n, ci], n = (dy 2 + dx) Cout + co -> (ref, bound) (B, 2 pixH, 2 pixW, Cout)."""
    acc, mag = acc_mag(A, W)
    b = f64(bias4)
    ref, bound, _ = CR.finish(acc + b, mag + np.abs(b), A.shape[1], 0, prec)
    return pixel_shuffle(ref, B, pixH, pixW, Cout), pixel_shuffle(bound, B, pixH, pixW, Cout)


def convt_uv_out(A, W, bias4, wu, wv, uv_range, B, pixH, pixW, Cout, prec):
    """The same with the uv term at the OUTPUT pixel: + wu[co] u(2 j + dx) + wv[co] v(2 i + dy), u / v linspace over 2 pixW / 2 pixH steps -> (ref, bound)."""
    acc, mag = acc_mag(A, W)
    b, wu, wv = f64(bias4), f64(wu), f64(wv)
    uu, vv, lu, lv = uv_planes(uv_range, B, 2 * pixH, 2 * pixW)
    term = lambda w, p: (w[None, None, None, :] * p.reshape(B, 2 * pixH, 2 * pixW, 1))                    # noqa: E731
    pre = pixel_shuffle(acc + b, B, pixH, pixW, Cout) + term(wu, uu) + term(wv, vv)
    mag = pixel_shuffle(mag + np.abs(b), B, pixH, pixW, Cout) + np.abs(term(wu, uu)) + np.abs(term(wv, vv))
    ref, bound, _ = CR.finish(pre, mag, A.shape[1] + 3, 0, prec, extra=(np.abs(wu) * lu + np.abs(wv) * lv)[None, None, None, :])
    return ref, bound


# ---------------------------------------------------------------------------------------------------------------------
# seeded input families: core_reference.gemm_inputs plus the per-flavour vectors (float32; the callers round A, W and the fp16 stream with to_storage)
# ---------------------------------------------------------------------------------------------------------------------
def floored(r, floor, scale=1.0, cap=None):
    m = floor + scale * np.abs(r)
    return np.sign(r) * (m if cap is None else np.minimum(m, cap))


def epilogue_inputs(M, N, K, family, seed=0, ln=False):
    """A, W, bias of core_reference.gemm_inputs (ln: W halved, see the module docstring) and gamma, c (N), mr (M,2) = (mean, rstd), wu, wv (N), x (M,N): rows
    with a mean of their own, as a residual stream has."""
    A, W, bias = CR.gemm_inputs(M, N, K, family, seed)
    if ln:
        W = (W * np.float32(0.5)).astype(np.float32)
    rng = np.random.default_rng([seed, M, N, K, 7])
    r = rng.standard_normal((6, N))
    mean = floored(rng.standard_normal(M), 0.25, 0.25, cap=0.5)
    rstd = rng.uniform(0.5, 2.0, M)
    x = rng.standard_normal((M, N)) * 3.0 + rng.standard_normal((M, 1))
    out = dict(A=A, W=W, bias=bias, gamma=floored(r[0], 0.25), c=floored(r[1], 0.25, 0.5, cap=1.5), mr=np.stack([mean, rstd], -1),
               wu=floored(r[2], 1.0), wv=floored(r[3], 1.0), x=x)
    return {k: np.ascontiguousarray(v, dtype=np.float32) for k, v in out.items()}


# ---------------------------------------------------------------------------------------------------------------------
# the sweep, shared by the CPU power tests and the GPU tests
# ---------------------------------------------------------------------------------------------------------------------
FAMILIES = CR.FAMILIES

# ---- ping-pong kernels (fp16; gemm_pp_eligible: N % 256 == 0, K % 64 == 0, M >= 256).  K: PP_KS[kern][i % 2] - the persistent kernel falls back below K = 192
PP_KS = {0: (64, 128), 2: (192, 256)}
# (nh, B, Ntok): M = 256, 258, 393, 257, 400 and 513 (one past a second row tile); Ntok 128 / 129: the single wrap of `t0 += 8` at its smallest; 131, 200: an image
# boundary that is no multiple of 8 rows into a tile; nh = 8: heads across column tiles
PP_QKV = [(4, 2, 128), (4, 2, 129), (4, 3, 131), (4, 1, 257), (4, 2, 200), (4, 3, 171), (8, 2, 129)]
# (B, pixH, pixW): pixW = 8 (the wrap lands on the same px), 9 .. 15, pixH = 1 (every wrap crosses an image), one image of one row
PP_GRIDS = [(1, 32, 8), (1, 33, 8), (1, 29, 9), (1, 18, 15), (17, 1, 16), (5, 5, 11), (1, 1, 300)]
PP_CONVT = [(Cout,) + g for Cout in (64, 128) for g in PP_GRIDS] + [(64, 1, 57, 9)]                      # (1, 57, 9): M = 513
PP_UV = [(N,) + g for N in (256, 512) for g in PP_GRIDS] + [(256, 2, 129, 1), (256, 257, 1, 1), (512, 3, 1, 86), (256, 1, 57, 9)]
PP_RESID = [(M, N) for N in (256, 512) for M in (257, 513)]
PP_GELU_LN = [(257, 256), (257, 512)]

# ---- latency kernels (fp16 and fp32): gemm_kernel 128 x 32 / 128 x 64 / 128 x 128 by N, gemm_glds_kernel from N > 64 when K is a whole number of 128-byte slabs
LAT_M = (1, 63, 65, 129, 257)


def lat_ks(prec):
    """chunk and 40 keep gemm_kernel (no whole slab); 64 and 128 open gemm_glds_kernel from N > 64 (fp32: one slab is 32 elements)."""
    return (CR.chunk(prec), 40, 64, 128)


LAT_QKV = [(nh, B, Ntok) for nh in (1, 2) for (B, Ntok) in ((1, 1), (3, 1), (2, 63), (1, 65), (3, 43), (1, 257))]
LAT_COUT = (4, 8, 12, 16, 20, 32, 36, 64)          # quadrant changes inside a 32-column tile; column tails at N = 48, 80, 144
LAT_GRIDS = [(1, 1, 1), (2, 1, 5), (1, 5, 1), (2, 3, 5), (1, 6, 9), (1, 17, 16)]
LAT_CONVT = [(Cout,) + LAT_GRIDS[(i + j) % 6] for i, Cout in enumerate(LAT_COUT) for j in (0, 2, 3)]
LAT_UV_N = (4, 36, 64, 132, 256)
LAT_UV_GRIDS = [(2, 5, 1), (2, 1, 6), (2, 1, 1), (2, 3, 4), (2, 3, 5), (2, 6, 9), (2, 17, 16)]              # pixW = 1, pixH = 1, even and odd widths and heights
LAT_UV = [(N,) + LAT_UV_GRIDS[(2 * i + j) % 7] + ((i + j) % 2,) for i, N in enumerate(LAT_UV_N) for j in (0, 1, 3, 5)]          # (N, B, pixH, pixW, act)
LAT_RESID_N = (4, 36, 68, 132, 260)                 # without producer outputs, fp32 stream (the fp16 stream takes the producer branch: refused at these N)
LAT_PRODUCER_N = (32, 64, 128, 256, 384)            # whole column tiles: with producer outputs, and the fp16 stream
LAT_LN_N = (36, 68, 132, 256)
LAT_CONVT_UV_OUT = (8, 2, 3, 5)                     # (Cout, B, pixH, pixW): N = 32, the one case of the branch no call site sets


def lat_mk(Ns, prec):
    """(M, N, K): every (N, K) pair with one M of LAT_M, rotated so that every N sees four different M and every K all five."""
    return [(LAT_M[(2 * i + j) % 5], N, K) for i, N in enumerate(Ns) for j, K in enumerate(lat_ks(prec))]


def rot_k(i, prec):
    return lat_ks(prec)[i % 4]


def rot_family(i):
    return FAMILIES[i % 2]


@functools.lru_cache(maxsize=None)
def resid_case(M, N, K, family, prec, half_stream):
    """prec: the storage type of A and W; half_stream: the residual stream is fp16 (prec 1 only)."""
    c = epilogue_inputs(M, N, K, family)
    xs = to_storage(c["x"], 1 if half_stream else 0)
    c["ref"], c["bound"] = resid(xs, to_storage(c["A"], prec), to_storage(c["W"], prec), c["bias"], c["gamma"], 1 if half_stream else 0)
    return c


@functools.lru_cache(maxsize=None)
def ln_case(M, N, K, family, prec, act):
    c = epilogue_inputs(M, N, K, family, ln=True)
    c["ref"], c["bound"] = ln_consumer(to_storage(c["A"], prec), to_storage(c["W"], prec), c["bias"], c["c"], c["mr"], act, prec)
    return c


@functools.lru_cache(maxsize=None)
def qkv_case(nh, B, Ntok, K, family, prec, fold):
    c = epilogue_inputs(B * Ntok, 3 * nh * 64, K, family, ln=bool(fold))
    c["out"] = qkv_rowmajor(to_storage(c["A"], prec), to_storage(c["W"], prec), c["bias"], B, Ntok, nh, LOG2E_8, prec,
                            mr=c["mr"] if fold else None, c=c["c"] if fold else None)
    return c


@functools.lru_cache(maxsize=None)
def uv_case(N, B, pixH, pixW, K, family, prec, act):
    c = epilogue_inputs(B * pixH * pixW, N, K, family)
    c["ref"], c["bound"] = uv_store(to_storage(c["A"], prec), to_storage(c["W"], prec), c["bias"], c["wu"], c["wv"], UV_RANGE, B, pixH, pixW, act, prec)
    return c


@functools.lru_cache(maxsize=None)
def convt_case(Cout, B, pixH, pixW, K, family, prec, uv_out=False):
    """bias4 differs by quadrant (a GEMM-side freedom the model's packing does not use: it replicates the bias) so that a quadrant's bias taken for another shows."""
    c = epilogue_inputs(B * pixH * pixW, 4 * Cout, K, family)
    A, W = to_storage(c["A"], prec), to_storage(c["W"], prec)
    if uv_out:
        c["wu"], c["wv"] = c["wu"][:Cout].copy(), c["wv"][:Cout].copy()
        c["ref"], c["bound"] = convt_uv_out(A, W, c["bias"], c["wu"], c["wv"], UV_RANGE, B, pixH, pixW, Cout, prec)
    else:
        c["ref"], c["bound"] = convt(A, W, c["bias"], B, pixH, pixW, Cout, prec)
    return c


# The cases as lists; `kern` is None for a latency-kernel case (every latency pin of the GPU module runs it) and 0 / 2 for a ping-pong case (PP_KERN).
def resid_sweep(prec):
    """(kern, M, N, K, family, half_stream, producer outputs).  The producer outputs and the fp16 stream exist in fp16 storage only."""
    out = [(None, M, N, K, rot_family(i), False, False) for i, (M, N, K) in enumerate(lat_mk(LAT_RESID_N, prec))]
    if prec == 1:
        for i, (M, N, K) in enumerate(lat_mk(LAT_PRODUCER_N, 1)):
            out += [(None, M, N, K, rot_family(i), False, True), (None, M, N, K, rot_family(i), True, True)]
        for i, (M, N) in enumerate(PP_RESID):
            out += [(kern, M, N, PP_KS[kern][i % 2], rot_family(i), hs, True) for kern in (0, 2) for hs in (False, True)]
    return out


def ln_sweep(prec):
    """(kern, M, N, K, family, act)"""
    out = [(None, M, N, K, rot_family(i), (0, 2)[(i // 4 + i) % 2]) for i, (M, N, K) in enumerate(lat_mk(LAT_LN_N, prec))]
    if prec == 1:
        out += [(kern, M, N, PP_KS[kern][i % 2], rot_family(i), 2) for i, (M, N) in enumerate(PP_GELU_LN) for kern in (0, 2)]
    return out


def qkv_sweep(prec):
    """(kern, nh, B, Ntok, K, family, fold)"""
    out = [(None, nh, B, Ntok, rot_k(i, prec), rot_family(i), fold) for i, (nh, B, Ntok) in enumerate(LAT_QKV) for fold in (0, 1)]
    if prec == 1:
        out += [(kern, nh, B, Ntok, PP_KS[kern][i % 2], rot_family(i), fold) for i, (nh, B, Ntok) in enumerate(PP_QKV) for kern in (0, 2) for fold in (0, 1)]
    return out


def convt_sweep(prec):
    """(kern, Cout, B, pixH, pixW, K, family)"""
    out = [(None, Cout, B, pixH, pixW, rot_k(i, prec), rot_family(i)) for i, (Cout, B, pixH, pixW) in enumerate(LAT_CONVT)]
    if prec == 1:
        out += [(kern, Cout, B, pixH, pixW, PP_KS[kern][i % 2], rot_family(i)) for i, (Cout, B, pixH, pixW) in enumerate(PP_CONVT) for kern in (0, 2)]
    return out


def uv_sweep(prec):
    """(kern, N, B, pixH, pixW, K, family, act)"""
    out = [(None, N, B, pixH, pixW, rot_k(i, prec), rot_family(i), act) for i, (N, B, pixH, pixW, act) in enumerate(LAT_UV)]
    if prec == 1:
        out += [(kern, N, B, pixH, pixW, PP_KS[kern][i % 2], rot_family(i), 0) for i, (N, B, pixH, pixW) in enumerate(PP_UV) for kern in (0, 2)]
    return out
