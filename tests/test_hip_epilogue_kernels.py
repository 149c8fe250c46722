"""GPU: the fused GEMM epilogues a ViT block and the neck entrance run - the residual update with the LayerNorm-fold producer outputs (EPI_RESID: EPK_RESID,
EPK_RESID16), the LN-fold consumer (GemmArgs::ln_mr: EPK_GELU_LN and the latency kernels' act none / GELU), the row-major QKV scatter with and without the fold
(EPK_QKV, EPK_QKV_LN), the 1x1 with the uv term (EPK_UV) and ConvTranspose2d as a GEMM (EPK_CONVT) - against the float64 references of
tests/epilogue_reference.py (derivation of every bound: that module's docstring; the references against torch, an honest emulation of each epilogue and the
injected faults the bounds catch: tests/test_epilogue_reference_cpu.py).  The gate is element-wise, |got - ref| <= bound(element), at the smallest shapes at
which each form can go wrong (epilogue_reference's sweep: tile edges, index wraps, image boundaries inside a tile), not at the workload's.  Every configuration
is called twice and the two calls must give the same bits.  The test entry fills every buffer the epilogue is to write in full with 0xFF bytes before the
launch (test_api.hip: poison), and `fraction` asserts finiteness: an element no store reached is a NaN, not the previous call's answer.

Every kernel the product dispatch can reach is pinned with moge_amd._lib.tuned(...), as tests/test_hip_core_kernels.py does:
  latency cases    default dispatch (gemm_kernel 128 x 32 / 128 x 64 / 128 x 128 by N and for a K that is no whole slab; gemm_glds_kernel 64 x 128 from N > 64),
                   GLDS_SMALL_BLOCKS = 0 (gemm_glds_kernel 128 x 128) and GLDS_VARIANT = 3 (256 x 128) where the shape opens gemm_glds_kernel
  ping-pong cases  PP_MIN_TILES = 0 with PP_KERN = 0 (gemm_pp128m16, K 64 / 128) and with PP_KERN = 2, PP_GRID = 24 (gemm_pp128p, K 192 / 256)
Nothing is asserted about which kernel ran beyond what those keys guarantee; the labels of the table name the tuning, not a trace.

The producer outputs are checked against the RETURNED stream: x16 == fp16(xres) bit for bit, ln_part within core_reference.ln_partials(stream).
EPI_RESID with GemmArgs::x16 - the producer AND the fp16 stream, which takes the same branch of epilogue_tile32 / epilogue_pair16 - has no column check, so
launch_gemm refuses it unless N is a whole number of the kernel's column tiles: the fp16 stream therefore runs at N in {32, 64, 128, 256, 384} only and its
refusal at a column tail is asserted by return code (test_host_refuses_what_the_epilogues_cannot_index), never run.

Worst observed error / bound per flavour and class on an MI355X (21 passed, 4.5 s for the module, slowest test 0.23 s - beside the core module's 17 - 38 s; `pytest -s`
prints the table of the run at hand; EXPERIMENTS.md R19).  gemm_kernel: 128x32 / 128x64 / 128x128 where the flavour's N reach them; gemm_glds: the same figure under
all three tile pins (same MFMAs, same K order); pp: gemm_pp128m16 / gemm_pp128p.
  flavour                     gemm_kernel f16          gemm_kernel f32          gemm_glds f16 / f32    pp
  resid, fp32 stream          0.087 / 0.139 / 0.173    0.079 / 0.186 / 0.279    0.023 / 0.044          0.024 / 0.007
    its ln_part               0.295 / 0.352 / 0.406    -                        0.363                  0.401 / 0.408
  resid16 (fp16 stream)       0.963 / 0.992 / 0.997    -                        0.981                  0.984 / 0.956
    its ln_part               0.346 / 0.326 / 0.435    -                        0.368                  0.401 / 0.401
  ln_consumer (none / GELU)   - / 0.951 / 0.992        - / 0.123 / 0.292        0.974 / 0.035          0.961 / 0.934 (GELU_LN)
  qkv                         - / - / 0.994            - / - / 0.336            0.978 / 0.055          0.982 / 0.934
  qkv_ln                      - / - / 0.993            - / - / 0.332            0.980 / 0.045          0.986 / 0.947
  uv (none / ReLU)            0.922 / 0.981 / 0.988    0.085 / 0.163 / 0.269    0.969 / 0.032          0.984 / 0.940
  convt                       0.971 / 0.987 / 0.981    0.252 / 0.351 / 0.292    0.958 / 0.049          0.985 / 0.938
  convt, uv at the output pixel (gemm_kernel 128x32, one case)   f16 0.958   f32 0.039
x16 == fp16(xres) held bit for bit and two calls gave the same bits at every configuration; no NaN came back from a poisoned buffer.  As in the core module the
0.92 - 1.00 figures are fp16 stores (the bound is the fp32 bound plus HALF an fp16 ulp of the result) and the fp32 figures show what the arithmetic itself uses.
No class was over its bound on the first run on the GPU, and no term was added to a bound after it.
"""
import numpy as np
import pytest
import torch

import core_reference as CR
import epilogue_reference as EP

pytestmark = pytest.mark.gpu

WORST = {}
PRECS = [0, 1]
IDS = ["fp32", "fp16"]
PN = {0: "f32", 1: "f16"}
LAT_PINS = [("default", {}), ("gemm_glds 128x128", dict(GLDS_SMALL_BLOCKS=0)), ("gemm_glds 256x128", dict(GLDS_VARIANT=3))]
PP_PINS = {0: ("gemm_pp128m16", dict(PP_MIN_TILES=0, PP_KERN=0)), 2: ("gemm_pp128p", dict(PP_MIN_TILES=0, PP_KERN=2, PP_GRID=24))}


@pytest.fixture(scope="module")
def H():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    import hip_util
    yield hip_util
    print("\nworst error / bound per flavour and kernel class:")
    for k in sorted(WORST):
        print(f"  {k:52s} {WORST[k][0]:8.4f}   ({WORST[k][1]} cases)   worst at {WORST[k][2]}")


def tuned(**keys):
    from moge_amd import _lib as L
    return L.tuned(**keys)


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def fraction(got, ref, bound):
    """As test_hip_core_kernels.fraction: every element finite (the poison of the test entry is NaN), then the worst error / bound and where."""
    got = got.detach().cpu().double().numpy()
    assert got.shape == ref.shape, (got.shape, ref.shape)
    assert np.isfinite(got).all(), f"{int((~np.isfinite(got)).sum())} elements no store reached"
    ratio = np.abs(got - ref) / bound
    return float(ratio.max()), np.unravel_index(ratio.argmax(), ratio.shape)


def check(kernel, got, ref, bound, what):
    worst, at = fraction(got, ref, bound)
    w = WORST.setdefault(kernel, [0.0, 0, ""])
    if worst >= w[0]:
        w[0], w[2] = worst, what
    w[1] += 1
    assert worst <= 1.0, f"{kernel} {what}: error / bound = {worst:.3f} at {at}"


def glds_shape(N, K, prec):
    return N > 64 and K % (8 * CR.chunk(prec)) == 0


def gemm_label(N, K, prec):
    if glds_shape(N, K, prec):
        return f"gemm_glds 64x128<{PN[prec]}>"
    return f"gemm_kernel 128x{32 if N <= 32 else 64 if N <= 64 else 128}<{PN[prec]}>"


def pins(kern, N, K, prec):
    """(kernel label, tuning keys) of every pin a case runs under."""
    if kern is not None:
        return [PP_PINS[kern]]
    out = [(gemm_label(N, K, prec), {})]
    if glds_shape(N, K, prec):
        out += [(f"{label}<{PN[prec]}>", keys) for label, keys in LAT_PINS[1:]]
    return out


def twice(run, keys, what):
    """The configuration called twice under the same pin: the two calls must give the same bits (a NaN differs from itself: an unwritten element fails here too)."""
    with tuned(**keys):
        a, b = run(), run()
    for k in a:
        assert torch.equal(a[k], b[k]), f"{what}: two calls differ in {k}"
    return a


def selected(sweep, pp):
    return [c for c in sweep if (c[0] is not None) == pp]


# ------------------------------------------------------------------------------------------------------------------ host-side refusals
def test_host_refuses_what_the_epilogues_cannot_index(H):
    """Return codes only: launch_gemm returns before any GEMM launch.  N = 192 (128-column kernels) and N = 36 (128 x 64) with the producer outputs or the fp16
    stream would update the next row and read gamma / bias past their end; ln_mr without a bias would load through a null pointer."""
    for N, K in ((192, 64), (192, 40), (36, 64), (36, 8)):
        c = EP.epilogue_inputs(5, N, K, "random")
        args = (H.TG_RESID, T(c["A"]), T(c["W"]), T(c["bias"]))
        assert H.gemm_ex(*args, xres=T(c["x"]), gamma=T(c["gamma"]), want_x16=True, raw=True) != 0, (N, K, "producer outputs")
        assert H.gemm_ex(*args, gamma=T(c["gamma"]), x16_stream=T(c["x"]), raw=True) != 0, (N, K, "fp16 stream with ln_part")
        assert H.gemm_ex(*args, gamma=T(c["gamma"]), x16_stream=T(c["x"]), want_part=False, raw=True) != 0, (N, K, "fp16 stream")
    for (M, N, K) in EP.lat_mk(EP.LAT_RESID_N, 1):            # the column-tail N of the latency sweep: the fp32 stream runs there (epilogue4), the fp16 stream must not
        c = EP.epilogue_inputs(M, N, K, "random")
        assert H.gemm_ex(H.TG_RESID, T(c["A"]), T(c["W"]), T(c["bias"]), gamma=T(c["gamma"]), x16_stream=T(c["x"]), want_part=False, raw=True) != 0, (M, N, K, "fp16 stream")
    c = EP.epilogue_inputs(5, 192, 64, "random")
    assert H.gemm_fused_ln(T(c["A"]), T(c["W"]), T(c["bias"]), T(c["gamma"]), T(c["x"]), raw=True) != 0
    for prec in PRECS:
        c = EP.epilogue_inputs(5, 64, 64, "random")
        assert H.gemm_ex(H.TG_STORE, T(c["A"]), T(c["W"]), None, prec=prec, ln_mr=T(c["mr"]), ln_c=T(c["c"]), raw=True) != 0, "ln_mr without a bias"
        assert H.gemm_ex(H.TG_STORE, T(c["A"]), T(c["W"]), T(c["bias"]), prec=prec, ln_mr=T(c["mr"]), raw=True) != 0, "ln_mr without ln_c"
        assert H.gemm_ex(H.TG_RESID, T(c["A"]), T(c["W"]), T(c["bias"]), prec=prec, xres=T(c["x"]), raw=True) != 0, "EPI_RESID without gamma"


# ------------------------------------------------------------------------------------------------------------------ RESID
def run_resid(H, prec, cases):
    for (kern, M, N, K, fam, hs, prod) in cases:
        c = EP.resid_case(M, N, K, fam, prec, hs)
        args = (H.TG_RESID, T(c["A"]), T(c["W"]), T(c["bias"]))
        # (stream key, keyword arguments): the fp32 stream with / without the producer outputs, the fp16 stream with / without the statistics
        if hs:
            variants = [("x16", dict(x16_stream=T(c["x"]))), ("x16", dict(x16_stream=T(c["x"]), want_part=False))]
        else:
            variants = [("xres", dict(xres=T(c["x"]), want_x16=True))] if prod else []
            if kern is not None or not prod:
                variants.append(("xres", dict(xres=T(c["x"]))))
        for label, keys in pins(kern, N, K, prec):
            for key, kw in variants:
                what = f"M={M} N={N} K={K} {fam} {'fp16' if hs else 'fp32'} stream {sorted(k for k in kw if k.startswith('want'))}"
                o = twice(lambda: H.gemm_ex(*args, prec=prec, gamma=T(c["gamma"]), **kw), keys, what)
                check(f"resid{'16' if hs else ''} | {label}", o[key], c["ref"], c["bound"], what)
                stream = o[key].cpu().double().numpy()
                if "ln_part" in o:
                    part, pb = CR.ln_partials(stream)
                    check(f"resid{'16' if hs else ''} ln_part | {label}", o["ln_part"], part, np.maximum(pb, 1e-300), what)
                if not hs and "x16" in o:
                    assert torch.equal(o["x16"], o["xres"].half().float()), f"{what}: x16 is not the fp16 rounding of the updated stream"
                if hs:
                    assert torch.equal(o["x16"], o["x16"].half().float())


@pytest.mark.parametrize("prec", PRECS, ids=IDS)
def test_resid_latency_kernels(H, prec):
    """Without the producer outputs at N = 4 .. 260 (column tails; fp32 stream, epilogue4); with them, and on the fp16 stream, at whole column tiles - K = chunk
    and K = 40 keep gemm_kernel: the producer branch of epilogue_tile32."""
    run_resid(H, prec, selected(EP.resid_sweep(prec), False))


@pytest.mark.parametrize("kern", [0, 2], ids=["pp128m16", "pp128p"])
def test_resid_ping_pong(H, kern):
    run_resid(H, 1, [c for c in selected(EP.resid_sweep(1), True) if c[0] == kern])


# ------------------------------------------------------------------------------------------------------------------ LN consumer
def run_ln(H, prec, cases):
    for (kern, M, N, K, fam, act) in cases:
        c = EP.ln_case(M, N, K, fam, prec, act)
        for label, keys in pins(kern, N, K, prec):
            what = f"M={M} N={N} K={K} act={act} {fam}"
            o = twice(lambda: H.gemm_ex(H.TG_STORE, T(c["A"]), T(c["W"]), T(c["bias"]), prec=prec, act=act, ln_mr=T(c["mr"]), ln_c=T(c["c"])), keys, what)
            check(f"ln_consumer | {label}", o["out"], c["ref"], c["bound"], what)


@pytest.mark.parametrize("prec", PRECS, ids=IDS)
def test_ln_consumer_latency_kernels(H, prec):
    run_ln(H, prec, selected(EP.ln_sweep(prec), False))


@pytest.mark.parametrize("kern", [0, 2], ids=["pp128m16", "pp128p"])
def test_gelu_ln_ping_pong(H, kern):
    run_ln(H, 1, [c for c in selected(EP.ln_sweep(1), True) if c[0] == kern])


# ------------------------------------------------------------------------------------------------------------------ QKV
def run_qkv(H, prec, cases):
    for (kern, nh, B, Ntok, K, fam, fold) in cases:
        c = EP.qkv_case(nh, B, Ntok, K, fam, prec, fold)
        kw = dict(ln_mr=T(c["mr"]), ln_c=T(c["c"])) if fold else {}
        for label, keys in pins(kern, 3 * nh * 64, K, prec):
            what = f"nh={nh} B={B} Ntok={Ntok} K={K} fold={fold} {fam}"
            o = twice(lambda: H.gemm_ex(H.TG_QKV, T(c["A"]), T(c["W"]), T(c["bias"]), prec=prec, nh=nh, Ntok=Ntok, qscale=EP.LOG2E_8, **kw), keys, what)
            for k in "qkv":
                check(f"qkv{'_ln' if fold else ''} | {label}", o[k], *c["out"][k], f"{what} {k}")


@pytest.mark.parametrize("prec", PRECS, ids=IDS)
def test_qkv_latency_kernels(H, prec):
    run_qkv(H, prec, selected(EP.qkv_sweep(prec), False))


@pytest.mark.parametrize("kern", [0, 2], ids=["pp128m16", "pp128p"])
def test_qkv_ping_pong(H, kern):
    run_qkv(H, 1, [c for c in selected(EP.qkv_sweep(1), True) if c[0] == kern])


# ------------------------------------------------------------------------------------------------------------------ ConvTranspose2d as a GEMM
def run_convt(H, prec, cases):
    for (kern, Cout, B, pixH, pixW, K, fam) in cases:
        c = EP.convt_case(Cout, B, pixH, pixW, K, fam, prec)
        for label, keys in pins(kern, 4 * Cout, K, prec):
            what = f"Cout={Cout} B={B} {pixH}x{pixW} K={K} {fam}"
            o = twice(lambda: H.gemm_ex(H.TG_CONVT, T(c["A"]), T(c["W"]), T(c["bias"]), prec=prec, pix=(pixW, pixH), Cout=Cout), keys, what)
            check(f"convt | {label}", o["out"].reshape(c["ref"].shape), c["ref"], c["bound"], what)


@pytest.mark.parametrize("prec", PRECS, ids=IDS)
def test_convt_latency_kernels(H, prec):
    run_convt(H, prec, selected(EP.convt_sweep(prec), False))
    # the uv term at the output pixel: the branch of epilogue4 no model call site sets (epilogue_reference's docstring)
    Cout, B, pixH, pixW = EP.LAT_CONVT_UV_OUT
    c = EP.convt_case(Cout, B, pixH, pixW, 40, "random", prec, uv_out=True)
    what = f"uv_out Cout={Cout} B={B} {pixH}x{pixW} K=40"
    o = twice(lambda: H.gemm_ex(H.TG_CONVT, T(c["A"]), T(c["W"]), T(c["bias"]), prec=prec, pix=(pixW, pixH), Cout=Cout, uv=(T(c["wu"]), T(c["wv"])) + EP.UV_RANGE), {}, what)
    check(f"convt, uv at the output pixel | {gemm_label(4 * Cout, 40, prec)}", o["out"].reshape(c["ref"].shape), c["ref"], c["bound"], what)


@pytest.mark.parametrize("kern", [0, 2], ids=["pp128m16", "pp128p"])
def test_convt_ping_pong(H, kern):
    run_convt(H, 1, [c for c in selected(EP.convt_sweep(1), True) if c[0] == kern])


# ------------------------------------------------------------------------------------------------------------------ uv term
def run_uv(H, prec, cases):
    for (kern, N, B, pixH, pixW, K, fam, act) in cases:
        c = EP.uv_case(N, B, pixH, pixW, K, fam, prec, act)
        for label, keys in pins(kern, N, K, prec):
            what = f"N={N} B={B} {pixH}x{pixW} K={K} act={act} {fam}"
            o = twice(lambda: H.gemm_ex(H.TG_STORE, T(c["A"]), T(c["W"]), T(c["bias"]), prec=prec, act=act, uv=(T(c["wu"]), T(c["wv"])) + EP.UV_RANGE, pix=(pixW, pixH)), keys, what)
            check(f"uv | {label}", o["out"], c["ref"], c["bound"], what)


@pytest.mark.parametrize("prec", PRECS, ids=IDS)
def test_uv_latency_kernels(H, prec):
    run_uv(H, prec, selected(EP.uv_sweep(prec), False))


@pytest.mark.parametrize("kern", [0, 2], ids=["pp128m16", "pp128p"])
def test_uv_ping_pong(H, kern):
    run_uv(H, 1, [c for c in selected(EP.uv_sweep(1), True) if c[0] == kern])
