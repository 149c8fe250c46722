"""GPU: the matrix-core kernels - GEMM (gemm.hip, gemm_pp.hip), 3x3 conv / x2 resampler / ConvTranspose2d (conv_pp.hip and the generic path of gemm.hip),
attention forward (attention_pp.hip, attention.hip) and the LayerNorm statistics gemm_glds_kernel finalises itself - against the float64 references of
tests/core_reference.py (derivation of every bound: that module's docstring; the references, an honest emulation of each kernel and the injected faults the
bounds catch: tests/test_core_reference_cpu.py).  The gate is element-wise, |got - ref| <= bound(element): no element left out, nothing normalised by a
maximum.  Shapes straddle each tile (core_reference.gemm_cases, conv_cases, UP2_CASES, CONVT_CASES, ATTN_SMALL / ATTN_LARGE, FUSED_LN_CASES), not the workload.

Every kernel the product library can dispatch is pinned with moge_amd._lib.tuned(...):
  GEMM       default dispatch (gemm_kernel 128 x 32 / 128 x 64 / 128 x 128 by N and for a K that is no multiple of a slab; gemm_glds_kernel 64 x 128 from N > 64),
             GLDS_SMALL_BLOCKS = 0 (gemm_glds_kernel 128 x 128), GLDS_VARIANT = 3 (256 x 128), PP_MIN_TILES = 0 with PP_KERN 0 / 2 (gemm_pp128m16 / gemm_pp128p)
  conv       default (fp16, Cin % 64 == 0: conv_pp; the rest gemm_kernel's implicit GEMM), CONV_PP = 0 (fp16 on the implicit GEMM)
  attention  fp32 (attention.hip); fp16 under ATTN_KERN 0 / 1 / 2 (attn_pp16_kernel, the form before the row sums moved to the matrix pipe; attn_pp16mq<2> / <4>),
             ATTN_KS 0 / 2 / 4 (no key split / attn_pp16ks<2> / <4>, with ATTN_KS_MID at the first and the last admissible tile from three key tiles on), and
             the default dispatch; two calls must give the same bits
Nothing is asserted about which kernel ran beyond what those keys guarantee; the labels of the table below name the tuning, not a trace.
hip_util.attention converts its arguments to contiguous fp32 and the entry point copies them into its own buffers, so the inference entry cannot be given a view:
the NaN-padded-allocation check of test_hip_attention_grad.test_layouts_give_the_same_bits has no counterpart here.

Worst observed error / bound per class on an MI355X (178 passed, 17 - 38 s for the module depending on the host's CPU; `pytest -s` prints the table of the run at hand; EXPERIMENTS.md R18):
  gemm_kernel 128x32 / 128x64 / 128x128   f16 0.986 / 0.997 / 0.996   f32 0.261 / 0.348 / 0.363
  gemm_glds 64x128 = 128x128 = 256x128    f16 0.983                   f32 0.050          gemm_pp128m16 = gemm_pp128p 0.974
  conv_pp<f16> 0.816   implicit-GEMM conv f16 0.920, f32 0.025   up2 f16 0.277, f32 0.017 (against self-rounded combined weights: 0.885 / 0.030)
  convt2x2 f16 0.970, f32 0.050
  attention.hip<f32> 0.082   attn_pp ATTN_KERN=0 0.640   every other fp16 form (ATTN_KERN 1 / 2, ATTN_KS 0 / 2 / 4 with every split point, default) 0.475
  fused LN finalize: stream 0.986 (fp16 store)   ln_part 0.421   ln_mr 0.284 of ln_finalize's bound on the returned partials, 0.030 of the any-order bound on the stream
The 0.82 - 1.00 figures are fp16 stores: the bound is the fp32 bound plus HALF an fp16 ulp of the result, which round-to-nearest all but reaches; the fp32 paths
show what the accumulation itself uses (0.03 - 0.36 of a bound that admits K sequential additions).  No kernel was over its bound, on the first run on the GPU
or since, and no term was added to a bound after it; the fp16 MFMA allowance is (n + c) u.
"""
import numpy as np
import pytest
import torch

import core_reference as CR
from tail_reference import to_storage

pytestmark = pytest.mark.gpu

WORST = {}
PRECS = [0, 1]
IDS = ["fp32", "fp16"]
PN = {0: "f32", 1: "f16"}


@pytest.fixture(scope="module")
def H():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    import hip_util
    yield hip_util
    print("\nworst error / bound per kernel class:")
    for k in sorted(WORST):
        print(f"  {k:44s} {WORST[k][0]:8.4f}   ({WORST[k][1]} cases)   worst at {WORST[k][2]}")


def tuned(**keys):
    from moge_amd import _lib as L
    return L.tuned(**keys)


def fraction(got, ref, bound):
    got = got.detach().cpu().double().numpy() if torch.is_tensor(got) else np.asarray(got, dtype=np.float64)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    assert np.isfinite(got).all()
    ratio = np.abs(got - ref) / bound
    return float(ratio.max()), np.unravel_index(ratio.argmax(), ratio.shape)


def check(kernel, got, ref, bound, what):
    worst, at = fraction(got, ref, bound)
    w = WORST.setdefault(kernel, [0.0, 0, ""])
    if worst >= w[0]:
        w[0], w[2] = worst, what
    w[1] += 1
    assert worst <= 1.0, f"{kernel} {what}: error / bound = {worst:.3f} at {at}"


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a))


# ------------------------------------------------------------------------------------------------------------------ GEMM
def glds_shape(N, K, prec):
    return N > 64 and K % (8 * CR.chunk(prec)) == 0


def gemm_label(N, K, prec):
    if glds_shape(N, K, prec):
        return f"gemm_glds 64x128<{PN[prec]}>"
    return f"gemm_kernel 128x{32 if N <= 32 else 64 if N <= 64 else 128}<{PN[prec]}>"


@pytest.mark.parametrize("prec", PRECS, ids=IDS)
def test_gemm_default_dispatch(H, prec):
    for (M, N, K, act, fam) in CR.gemm_cases(prec):
        c = CR.gemm_case(M, N, K, act, fam, prec)
        got = H.gemm(prec, T(c["A"]), T(c["W"]), T(c["bias"]), act)
        check(gemm_label(N, K, prec), got, c["ref"], c["bound"], f"M={M} N={N} K={K} act={act} {fam}")


@pytest.mark.parametrize("tile,keys", [("128x128", dict(GLDS_SMALL_BLOCKS=0)), ("256x128", dict(GLDS_VARIANT=3))])
@pytest.mark.parametrize("prec", PRECS, ids=IDS)
def test_gemm_direct_to_lds_tiles(H, prec, tile, keys):
    n = 0
    for (M, N, K, act, fam) in CR.gemm_cases(prec):
        if not glds_shape(N, K, prec):
            continue
        c = CR.gemm_case(M, N, K, act, fam, prec)
        with tuned(**keys):
            got = H.gemm_ex(H.TG_STORE, T(c["A"]), T(c["W"]), T(c["bias"]), prec=prec, act=act)["out"]
        check(f"gemm_glds {tile}<{PN[prec]}>", got, c["ref"], c["bound"], f"M={M} N={N} K={K} act={act} {fam}")
        n += 1
    assert n >= 20


@pytest.mark.parametrize("kern,keys", [("gemm_pp128m16", dict(PP_MIN_TILES=0, PP_KERN=0)), ("gemm_pp128p", dict(PP_MIN_TILES=0, PP_KERN=2, PP_GRID=24))])
def test_gemm_ping_pong(H, kern, keys):
    """N % 256 == 0, K % 64 == 0, M >= 256: M = 257 is a full 256-row tile and a one-row tail; K of one slab, two, sixteen and sixty-four."""
    n = 0
    for (M, N, K, act, fam) in CR.gemm_cases(1):
        if N % 256 or K % 64 or M < 256:
            continue
        c = CR.gemm_case(M, N, K, act, fam, 1)
        with tuned(**keys):
            got = H.gemm_ex(H.TG_STORE, T(c["A"]), T(c["W"]), T(c["bias"]), prec=1, act=act)["out"]
        check(kern, got, c["ref"], c["bound"], f"M={M} N={N} K={K} act={act} {fam}")
        n += 1
    assert n >= 4


# ------------------------------------------------------------------------------------------------------------------ conv
@pytest.mark.parametrize("prec,mode", [(0, "default"), (1, "default"), (1, "implicit_gemm")], ids=["fp32", "fp16", "fp16-CONV_PP=0"])
def test_conv3x3(H, prec, mode):
    """mode implicit_gemm: CONV_PP = 0 sends the fp16 shapes conv_pp would take (Cin % 64 == 0) to gemm_kernel's implicit GEMM - only those are run there
    (fp32 always runs the implicit GEMM)."""
    for (B, Hh, W, Cin, Cout, relu_in, act, fam) in CR.conv_cases():
        pp = prec == 1 and Cin % 64 == 0
        if mode == "implicit_gemm" and not pp:
            continue
        c = CR.conv_case(B, Hh, W, Cin, Cout, relu_in, act, fam, prec)
        with tuned(CONV_PP=0 if mode == "implicit_gemm" else 1):
            got = H.conv_ex(T(c["x"]), T(c["w"]), T(c["bias"]), prec=prec, relu_in=bool(relu_in), act=act)
        label = "conv_pp<f16>" if pp and mode == "default" else f"gemm_kernel conv3<{PN[prec]}>"
        check(label, got, c["ref"], c["bound"], f"B={B} {Hh}x{W} {Cin}->{Cout} relu_in={relu_in} act={act} {fam}")


@pytest.mark.parametrize("prec", PRECS, ids=IDS)
def test_up2_resampler(H, prec):
    """Gate: the definition (bilinear x2, then the 3x3 conv) with the rounding of the combined weights bounded.  Printed beside it: the same output against the
    reference that rounds the combined weights itself (core_reference.conv_up2_phase), which has no such term - a measurement, see that module's docstring."""
    for (B, Hh, W, Cin, Cout, fam) in CR.UP2_CASES:
        c = CR.up2_case(B, Hh, W, Cin, Cout, fam, prec)
        got = H.conv3x3(prec, T(c["x"]), T(c["w"]), T(c["bias"]), up2=True)
        what = f"B={B} {Hh}x{W} {Cin}->{Cout} {fam}"
        fp, _ = fraction(got, c["ref_phase"], c["bound_phase"])
        w = WORST.setdefault(f"up2<{PN[prec]}> vs self-rounded weights (measured)", [0.0, 0, ""])
        w[0], w[1], w[2] = max(w[0], fp), w[1] + 1, what if fp >= w[0] else w[2]
        check(f"up2<{PN[prec]}>", got, c["ref"], c["bound"], what)


@pytest.mark.parametrize("prec", PRECS, ids=IDS)
def test_convtranspose2x2(H, prec):
    for (B, Hh, W, Cin, Cout, fam) in CR.CONVT_CASES:
        c = CR.convt_case(B, Hh, W, Cin, Cout, fam, prec)
        got = H.convt2x2(prec, T(c["x"]), T(c["w"]), T(c["bias"]))
        check(f"convt2x2<{PN[prec]}>", got, c["ref"], c["bound"], f"B={B} {Hh}x{W} {Cin}->{Cout} {fam}")


# ------------------------------------------------------------------------------------------------------------------ attention
def attention_configs(N):
    """(label, precision, tuning keys) of every form the dispatch can be pinned to at this sequence length."""
    nt = (N + 63) // 64
    cfg = [("attention.hip<f32>", 0, {}), ("attn_pp ATTN_KERN=0", 1, dict(ATTN_KERN=0)), ("attn_pp ATTN_KERN=1", 1, dict(ATTN_KERN=1)), ("attn_pp ATTN_KERN=2", 1, dict(ATTN_KERN=2)),
           ("attn_pp ATTN_KS=0", 1, dict(ATTN_KS=0)), ("attn_pp default", 1, {})]
    for ks in (2, 4):
        cfg.append((f"attn_pp ATTN_KS={ks}", 1, dict(ATTN_KS=ks)))
        if nt >= 3:
            cfg += [(f"attn_pp ATTN_KS={ks}", 1, dict(ATTN_KS=ks, ATTN_KS_MID=mid)) for mid in (1, nt - 1)]
    return cfg


def run_attention(H, B, nh, N, family, precs=(0, 1)):
    for label, prec, keys in attention_configs(N):
        if prec not in precs:
            continue
        c = CR.attention_case(B, nh, N, family, prec)
        q, k, v = T(c["q"]), T(c["k"]), T(c["v"])
        with tuned(**keys):
            a = H.attention(prec, q, k, v)
            b = H.attention(prec, q, k, v)
        what = f"B={B} nh={nh} N={N} {family} {keys}"
        assert torch.equal(a, b), f"{label} {what}: two calls differ"
        check(label, a, c["ref"], c["bound"], what)


@pytest.mark.parametrize("family", CR.ATTN_FAMILIES)
@pytest.mark.parametrize("B,nh,N", CR.ATTN_SMALL)
def test_attention_tile_edges(H, B, nh, N, family):
    run_attention(H, B, nh, N, family)


@pytest.mark.parametrize("prec", PRECS, ids=IDS)
@pytest.mark.parametrize("family", CR.ATTN_FAMILIES)
@pytest.mark.parametrize("B,nh,N", CR.ATTN_LARGE)
def test_attention_workload_lengths(H, B, nh, N, family, prec):
    """N = 1370 (38 padding keys in the last tile) and N = 3601 (47; 17 queries in the last block): the float64 bound is O(N^2 64) - 0.5 to 1.5 seconds of CPU at
    N = 3601 - and is built once per family and precision, shared by every form of the dispatch."""
    run_attention(H, B, nh, N, family, (prec,))


# ------------------------------------------------------------------------------------------------------------------ fused LN finalize
def fused_ln_inputs(M, N, K):
    rng = np.random.default_rng([M, N, K])
    A, W = rng.standard_normal((M, K)), rng.standard_normal((N, K)) / np.sqrt(K)
    bias, gamma = rng.standard_normal(N), rng.standard_normal(N)
    x0 = rng.standard_normal((M, N)) * 3.0 + rng.standard_normal((M, 1))          # rows with a mean of their own
    return tuple(a.astype(np.float32) for a in (A, W, bias, gamma, x0))


@pytest.mark.parametrize("half_stream", [True, False], ids=["x16_stream", "f32_stream"])
@pytest.mark.parametrize("M,N,K", CR.FUSED_LN_CASES)
def test_gemm_fused_ln_finalize(H, M, N, K, half_stream):
    """The EPI_RESID producer with GemmArgs::ln_mr_out / ln_cnt (moge_test_gemm_fused_ln: the branch the ViT block takes for proj / fc2 in the latency regime): one
    first launch on zeroed counters and one second launch on the same buffers, nothing repeated.  The stream against its float64 reference, ln_part against the
    float64 partial sums of the RETURNED stream, ln_mr against the finalize formula on the returned partials and against the moments of the returned stream,
    the counters (and the two guard entries behind them) zero after each launch, the second launch bit-identical."""
    A, W, bias, gamma, x0 = fused_ln_inputs(M, N, K)
    o = H.gemm_fused_ln(T(A), T(W), T(bias), T(gamma), T(x0), half_stream=half_stream)
    what = f"M={M} N={N} K={K} {'x16' if half_stream else 'f32'} stream"
    # the residual update: x + gamma (acc + bias); K + 4 roundings (the chain, gamma * bias, the fma, the addition)
    A64, W64, g64, b64 = to_storage(A, 1), to_storage(W, 1), gamma.astype(np.float64), bias.astype(np.float64)
    xs = to_storage(x0, 1) if half_stream else x0.astype(np.float64)
    ref = xs + g64 * (A64 @ W64.T + b64)
    e = (K + 4) * CR.U32 * (np.abs(xs) + np.abs(g64) * (np.abs(A64) @ np.abs(W64).T + np.abs(b64)))
    check("fused_ln stream", o["stream"], ref, CR.store(ref, e, 1 if half_stream else 0), what)
    stream = o["stream"].cpu().double().numpy()
    if not half_stream:
        assert torch.equal(o["x16"], o["stream"].half().float()), "x16 is not the fp16 rounding of the updated stream"
    part, pb = CR.ln_partials(stream)
    check("fused_ln ln_part", o["ln_part"], part, np.maximum(pb, 1e-300), what)
    for label, (mr, emr) in (("fused_ln ln_mr | returned partials", CR.ln_stats(o["ln_part"].cpu().numpy(), N)), ("fused_ln ln_mr | stream moments", CR.ln_stats_of_stream(stream))):
        check(label, o["ln_mr"], mr, emr, what)
    assert int(o["cnt"].abs().sum()) == 0, f"{what}: counters not left zero: {o['cnt'].tolist()}"
    first = {k: o[k].clone() for k in ("stream", "x16", "ln_part", "ln_mr")}
    o["ln_part"].fill_(float("nan"))
    o["ln_mr"].fill_(float("nan"))
    o2 = H.gemm_fused_ln(T(A), T(W), T(bias), T(gamma), T(x0), half_stream=half_stream, bufs=o)
    for k in first:
        assert torch.equal(o2[k], first[k]), f"{what}: second launch on the same buffers differs in {k}"
    assert int(o2["cnt"].abs().sum()) == 0


def test_gemm_fused_ln_refuses_other_dispatch(H):
    """A shape launch_gemm would not send to gemm_glds_kernel is an error, not a quiet run without the fused finalize."""
    A, W, bias, gamma, x0 = fused_ln_inputs(8, 64, 64)           # N <= 64: the generic kernel
    assert H.gemm_fused_ln(T(A), T(W), T(bias), T(gamma), T(x0), raw=True) != 0
