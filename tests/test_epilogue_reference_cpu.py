"""CPU: the float64 references of tests/epilogue_reference.py against independent torch float64 formulations, and the POWER of the bounds: an honest fp32
emulation of each epilogue stays inside the bound on every element of every case of the GPU sweep, and each injected fault is outside it at every case where
it changes the result at all.

Emulations.  Storage-type inputs; the accumulator is an fp32 k-ordered chain (one fused multiply-add per k: the product of two storage values is exact in
float64, the sum is rounded to fp32); then the fp32 operation sequence of common.h in np.float32, an fma being the float64 product and sum rounded once:
resid_term + one addition, ln_fold_term, q_scaled, uv_term_add over linspace_at, the bias addition of the ConvTranspose2d store; GELU as the exact erf form
rounded to fp32; the fp16 store.  The producer outputs: x16 = fp16(x), ln_part by ln_quad_sums and the pairwise tree over the eight quads of a group.

Faults, and where each CANNOT change the result (asserted: at those cases the faulty output is bit-equal to the honest one; everywhere else it must be
outside the bound on at least one element):
  QKV          image index bumped one 8-row step late at an image boundary (tokens 0 .. 7 of image b >= 1 land in image b - 1): not with B = 1
               head index off by one (cyclic): not with nh = 1          scale applied to k instead of q: always visible
               v stored transposed (64 x Ntok in the place of Ntok x 64): not with Ntok = 1, where the two layouts are the same 64 numbers
  CONVT        dy / dx swapped: always          px wrap one 8-pixel step late (the first 8 pixels of a row land one output row too high): not with B pixH = 1
               image index not advanced when pixH == 1: only cases with pixH == 1 and B > 1          bias of quadrant 0 used for all four: always
  uv           u taken at x + 1: not with pixW = 1 (a single step is `start` whatever the index)          u and v swapped: always
               y without `% pixH`: not with B = 1 and not with pixH = 1
  RESID        bias not multiplied by gamma, update applied twice: always          ln_part group shifted by one (cyclic): not with N = 32 (one group)
               x16 taken before the update: always (checked as the GPU test does: x16 against fp16 of the stream)
  LN consumer  `mean c` dropped, rstd applied to the bias too: always
Not covered: nothing - every (fault, case) pair of the sweep is either caught or is one of the cases above.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import core_reference as CR
import epilogue_reference as EP
from tail_reference import to_storage

PRECS = [0, 1]
IDS = ["fp32", "fp16"]
F32 = np.float32


def r32(x):
    return np.asarray(x, dtype=np.float64).astype(np.float32).astype(np.float64)


def r16(x):
    return r32(x).astype(np.float16).astype(np.float64)


def fma(a, b, c):
    return r32(np.asarray(a, dtype=np.float64) * b + c)


def st(x, prec):
    return r16(x) if prec == 1 else r32(x)


def chain32(A, W):
    """The fp32 accumulator of A (M,K) W (N,K)^T as a k-ordered chain of fused multiply-adds."""
    acc = np.zeros((A.shape[0], W.shape[0]))
    for k in range(A.shape[1]):
        acc = r32(acc + A[:, k:k + 1] * W[None, :, k])
    return acc


def frac(got, ref, bound):
    return float((np.abs(got - ref) / bound).max())


def T64(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64))


# ------------------------------------------------------------------------------------------------------------------ references against torch
@pytest.mark.parametrize("prec_stream", PRECS, ids=["f32_stream", "f16_stream"])
def test_resid_reference(prec_stream):
    c = EP.epilogue_inputs(5, 64, 24, "random")
    x = to_storage(c["x"], prec_stream)
    ref, bound = EP.resid(x, to_storage(c["A"], 1), to_storage(c["W"], 1), c["bias"], c["gamma"], prec_stream)
    want = T64(x) + T64(c["gamma"]) * F.linear(T64(to_storage(c["A"], 1)), T64(to_storage(c["W"], 1)), T64(c["bias"]))
    assert np.allclose(ref, want.numpy(), rtol=0, atol=1e-12) and (bound > 0).all()


@pytest.mark.parametrize("act", [0, 2])
def test_ln_consumer_reference_is_layer_norm_then_linear(act):
    """The fold: LN(x; g, beta) W^T + b = rstd (x Wf^T - mean c) + bf with Wf = W g, c = Wf 1, bf = W beta + b."""
    rng = np.random.default_rng(3)
    x, W, g, beta, b = rng.standard_normal((7, 48)) + 0.4, rng.standard_normal((12, 48)) / 7, rng.standard_normal(48), rng.standard_normal(48), rng.standard_normal(12)
    want = F.linear(F.layer_norm(T64(x), (48,), T64(g), T64(beta), eps=1e-6), T64(W), T64(b))
    want = F.gelu(want) if act == 2 else want
    mr, _ = CR.ln_stats_of_stream(x)
    Wf = W * g[None]
    ref, bound = EP.ln_consumer(x, Wf, W @ beta + b, Wf.sum(1), mr, act, 0)
    assert np.allclose(ref, want.numpy(), rtol=0, atol=1e-11) and (bound > 0).all()


@pytest.mark.parametrize("fold", [0, 1])
@pytest.mark.parametrize("nh,B,Ntok", [(1, 1, 1), (2, 3, 5), (3, 2, 9)])
def test_qkv_reference_is_the_reshape_and_permute_of_attention_py(nh, B, Ntok, fold):
    c = EP.qkv_case(nh, B, Ntok, 24, "random", 0, fold)
    A, W = T64(to_storage(c["A"], 0)), T64(to_storage(c["W"], 0))
    y = A @ W.T
    if fold:
        mr = T64(c["mr"])
        y = mr[:, 1:2] * (y - mr[:, 0:1] * T64(c["c"]))
    y = (y + T64(c["bias"])).reshape(B, Ntok, 3, nh, 64).permute(2, 0, 3, 1, 4)
    qs = float(F32(EP.LOG2E_8))
    for name, want in (("q", y[0] * qs), ("k", y[1]), ("v", y[2])):
        ref, bound = c["out"][name]
        assert ref.shape == (B, nh, Ntok, 64)
        assert np.allclose(ref, want.numpy(), rtol=0, atol=1e-12) and (bound > 0).all()


@pytest.mark.parametrize("act", [0, 1])
@pytest.mark.parametrize("B,pixH,pixW", [(1, 1, 1), (2, 1, 6), (2, 5, 1), (2, 3, 4), (1, 4, 7)])
def test_uv_reference_is_linspace_and_meshgrid(B, pixH, pixW, act):
    c = EP.uv_case(12, B, pixH, pixW, 16, "random", 0, act)
    u0, u1, v0, v1 = EP.UV_RANGE
    u, v = torch.linspace(u0, u1, pixW, dtype=torch.float32).double(), torch.linspace(v0, v1, pixH, dtype=torch.float32).double()
    vv, uu = torch.meshgrid(v, u, indexing="ij")
    uu, vv = (t[None].expand(B, pixH, pixW).reshape(-1, 1) for t in (uu, vv))
    want = T64(to_storage(c["A"], 0)) @ T64(to_storage(c["W"], 0)).T + T64(c["bias"]) + T64(c["wu"]) * uu + T64(c["wv"]) * vv
    want = F.relu(want) if act else want
    assert np.allclose(c["ref"], want.numpy(), rtol=0, atol=1e-12) and (c["bound"] > 0).all()


@pytest.mark.parametrize("B,pixH,pixW,Cout", [(1, 1, 1, 4), (2, 1, 5, 8), (2, 3, 5, 12), (1, 4, 2, 20)])
def test_convt_reference_is_conv_transpose2d(B, pixH, pixW, Cout):
    c = EP.convt_case(Cout, B, pixH, pixW, 16, "random", 0)
    A, W = to_storage(c["A"], 0), to_storage(c["W"], 0)
    K = A.shape[1]
    xt = T64(A).reshape(B, pixH, pixW, K).permute(0, 3, 1, 2)
    wt = T64(W).reshape(2, 2, Cout, K).permute(3, 2, 0, 1).contiguous()                   # [ci][co][dy][dx]
    want = F.conv_transpose2d(xt, wt, None, stride=2).permute(0, 2, 3, 1).clone()
    b4 = T64(c["bias"]).reshape(2, 2, Cout)
    for dy in range(2):
        for dx in range(2):
            want[:, dy::2, dx::2] += b4[dy, dx]
    assert np.allclose(c["ref"], want.numpy(), rtol=0, atol=1e-12) and (c["bound"] > 0).all()
    # a bias replicated over the quadrants, as the model packs it: torch's own bias argument, and core_reference.convt2x2 (reference AND bound)
    bias = c["bias"][:Cout]
    ref, bound = EP.convt(A, W, np.tile(bias, 4), B, pixH, pixW, Cout, 0)
    want = F.conv_transpose2d(xt, wt, T64(bias), stride=2).permute(0, 2, 3, 1)
    assert np.allclose(ref, want.numpy(), rtol=0, atol=1e-12)
    ref2, bound2, _ = CR.convt2x2(A.reshape(B, pixH, pixW, K), wt.numpy(), bias, 0)
    assert np.allclose(ref, ref2, rtol=0, atol=1e-12) and np.allclose(bound, bound2, rtol=1e-12, atol=0)
    # the uv term at the output pixel
    cu = EP.convt_case(Cout, B, pixH, pixW, 16, "random", 0, uv_out=True)
    u0, u1, v0, v1 = EP.UV_RANGE
    u, v = torch.linspace(u0, u1, 2 * pixW, dtype=torch.float32).double(), torch.linspace(v0, v1, 2 * pixH, dtype=torch.float32).double()
    vv, uu = torch.meshgrid(v, u, indexing="ij")
    want = T64(c["ref"]) + T64(cu["wu"]) * uu[None, :, :, None] + T64(cu["wv"]) * vv[None, :, :, None]
    assert np.allclose(cu["ref"], want.numpy(), rtol=0, atol=1e-12) and (cu["bound"] >= c["bound"]).all()


# ------------------------------------------------------------------------------------------------------------------ emulations and faults
def lin_at(start, end, steps, i):
    """common.h linspace_at in fp32, one fma per element; i may lie outside [0, steps) (faults)."""
    start, end = float(F32(start)), float(F32(end))
    step = float(F32(F32(end - start) / F32(steps - 1))) if steps > 1 else 0.0
    i = np.asarray(i, dtype=np.float64)
    return np.where((i < steps // 2) | (steps == 1), r32(start + step * i), r32(end - step * (steps - 1 - i)))


def gelu32(v):
    return r32(CR.gelu(v))


def emu_resid(c, acc, half_stream, fault=None):
    """-> (stream, x16 or None, ln_part)."""
    g, b = c["gamma"].astype(np.float64), c["bias"].astype(np.float64)
    x = to_storage(c["x"], 1 if half_stream else 0)
    t = fma(g, acc, b if fault == "bias not multiplied by gamma" else r32(g * b))
    xn = r32(x + t)
    if fault == "update applied twice":
        xn = r32(xn + t)
    if half_stream:
        xn = r16(xn)
    x16 = None if half_stream else r16(x if fault == "x16 taken before the update" else xn)
    if xn.shape[1] % 32:
        return xn, x16, None
    q = xn.reshape(xn.shape[0], -1, 8, 4)
    s1 = r32(r32(q[..., 0] + q[..., 1]) + r32(q[..., 2] + q[..., 3]))
    s2 = r32(fma(q[..., 1], q[..., 1], r32(q[..., 0] * q[..., 0])) + fma(q[..., 3], q[..., 3], r32(q[..., 2] * q[..., 2])))

    def tree(s):
        p = r32(s[..., 0::2] + s[..., 1::2])
        p = r32(p[..., 0::2] + p[..., 1::2])
        return r32(p[..., 0] + p[..., 1])

    part = np.stack([tree(s1), tree(s2)], -1)
    if fault == "ln_part group shifted by one":
        part = np.roll(part, 1, axis=1)
    return xn, x16, part


RESID_FAULTS = {"bias not multiplied by gamma": lambda N: True, "update applied twice": lambda N: True,
                "ln_part group shifted by one": lambda N: N > 32, "x16 taken before the update": lambda N: True}


@pytest.mark.parametrize("prec", PRECS, ids=IDS)
def test_resid_emulation_is_inside_and_faults_are_outside(prec):
    worst, caught = 0.0, {}
    for (_, M, N, K, fam, hs, prod) in EP.resid_sweep(prec):
        c = EP.resid_case(M, N, K, fam, prec, hs)
        acc = chain32(to_storage(c["A"], prec), to_storage(c["W"], prec))
        xn, x16, part = emu_resid(c, acc, hs)
        f = frac(xn, c["ref"], c["bound"])
        worst = max(worst, f)
        assert f <= 1.0, (M, N, K, fam, hs, f)
        if not prod:
            faults = ("bias not multiplied by gamma", "update applied twice")
        else:
            pref, pb = CR.ln_partials(xn)
            assert (np.abs(part - pref) <= pb).all() and (hs or np.array_equal(x16, r16(xn)))
            faults = [k for k in RESID_FAULTS if not (hs and k.startswith("x16"))]
        for name in faults:
            bx, b16, bpart = emu_resid(c, acc, hs, fault=name)
            if name.startswith("ln_part"):
                pref, pb = CR.ln_partials(bx)
                changed, f = not np.array_equal(bpart, part), frac(bpart, pref, np.maximum(pb, 1e-300))
            elif name.startswith("x16"):
                changed = not np.array_equal(b16, x16)
                f = np.inf if not np.array_equal(b16, r16(bx)) else 0.0
            else:
                changed, f = not np.array_equal(bx, xn), frac(bx, c["ref"], c["bound"])
            assert changed == RESID_FAULTS[name](N), (name, M, N, K)
            if changed:
                assert f > 1.0, f"RESID {M}x{N}x{K} {fam}: '{name}' stays inside the bound ({f:.3f})"
                caught[name] = min(caught.get(name, np.inf), f)
    print(f"\nRESID prec {prec}: honest emulation worst error / bound {worst:.3f}; weakest catch per fault:", {k: round(v, 2) for k, v in caught.items()})


def emu_ln(c, acc, act, prec, fault=None):
    b, lc = c["bias"].astype(np.float64), c["c"].astype(np.float64)
    mean, rstd = c["mr"][:, :1].astype(np.float64), c["mr"][:, 1:2].astype(np.float64)
    inner = acc if fault == "mean c dropped" else fma(-mean, lc, acc)
    v = r32(rstd * r32(inner + b)) if fault == "rstd applied to the bias too" else fma(rstd, inner, b)
    return st(gelu32(v) if act == 2 else v, prec)


@pytest.mark.parametrize("prec", PRECS, ids=IDS)
def test_ln_consumer_emulation_is_inside_and_faults_are_outside(prec):
    worst, caught = 0.0, {}
    for (_, M, N, K, fam, act) in EP.ln_sweep(prec):
        c = EP.ln_case(M, N, K, fam, prec, act)
        acc = chain32(to_storage(c["A"], prec), to_storage(c["W"], prec))
        good = emu_ln(c, acc, act, prec)
        f = frac(good, c["ref"], c["bound"])
        worst = max(worst, f)
        assert f <= 1.0, (M, N, K, fam, act, f)
        for name in ("mean c dropped", "rstd applied to the bias too"):
            f = frac(emu_ln(c, acc, act, prec, fault=name), c["ref"], c["bound"])
            assert f > 1.0, f"LN consumer {M}x{N}x{K} act {act} {fam}: '{name}' stays inside the bound ({f:.3f})"
            caught[name] = min(caught.get(name, np.inf), f)
    print(f"\nLN consumer prec {prec}: honest emulation worst error / bound {worst:.3f}; weakest catch per fault:", {k: round(v, 2) for k, v in caught.items()})


def emu_qkv(c, acc, B, Ntok, nh, prec, fold, fault=None):
    D = nh * 64
    b = c["bias"].astype(np.float64)
    if fold:
        mean, rstd = c["mr"][:, :1].astype(np.float64), c["mr"][:, 1:2].astype(np.float64)
        pre = fma(rstd, fma(-mean, c["c"].astype(np.float64), acc), b)
    else:
        pre = r32(acc + b)
    qs = float(F32(EP.LOG2E_8))
    m = np.arange(B * Ntok)
    img, tok = m // Ntok, m % Ntok
    late = (tok < 8) & (img >= 1) if fault == "image index one step late" else np.zeros_like(m, dtype=bool)
    out = {}
    for which, name in enumerate("qkv"):
        o = np.zeros((B, nh, Ntok, 64))
        scaled = which == (1 if fault == "scale applied to k" else 0)
        for h in range(nh):
            v = pre[:, which * D + h * 64: which * D + (h + 1) * 64]
            v = st(r32(v * qs) if scaled else v, prec)
            hh = (h + 1) % nh if fault == "head index off by one" else h
            o[img[~late], hh, tok[~late]] = v[~late]
            o[img[late] - 1, hh, tok[late]] = v[late]
        if name == "v" and fault == "v stored transposed":
            o = np.ascontiguousarray(o.transpose(0, 1, 3, 2)).reshape(B, nh, Ntok, 64)
        out[name] = o
    return out


QKV_FAULTS = {"image index one step late": lambda nh, B, Ntok: B > 1, "head index off by one": lambda nh, B, Ntok: nh > 1,
              "scale applied to k": lambda nh, B, Ntok: True, "v stored transposed": lambda nh, B, Ntok: Ntok > 1}


@pytest.mark.parametrize("prec", PRECS, ids=IDS)
def test_qkv_emulation_is_inside_and_faults_are_outside(prec):
    worst, caught = 0.0, {}
    for (_, nh, B, Ntok, K, fam, fold) in EP.qkv_sweep(prec):
        c = EP.qkv_case(nh, B, Ntok, K, fam, prec, fold)
        acc = chain32(to_storage(c["A"], prec), to_storage(c["W"], prec))
        good = emu_qkv(c, acc, B, Ntok, nh, prec, fold)
        f = max(frac(good[k], *c["out"][k]) for k in "qkv")
        worst = max(worst, f)
        assert f <= 1.0, (nh, B, Ntok, K, fam, fold, f)
        for name, applies in QKV_FAULTS.items():
            bad = emu_qkv(c, acc, B, Ntok, nh, prec, fold, fault=name)
            changed = any(not np.array_equal(bad[k], good[k]) for k in "qkv")
            assert changed == applies(nh, B, Ntok), (name, nh, B, Ntok)
            if changed:
                f = max(frac(bad[k], *c["out"][k]) for k in "qkv")
                assert f > 1.0, f"QKV nh={nh} B={B} Ntok={Ntok} K={K} fold={fold}: '{name}' stays inside the bound ({f:.3f})"
                caught[name] = min(caught.get(name, np.inf), f)
    print(f"\nQKV prec {prec}: honest emulation worst error / bound {worst:.3f}; weakest catch per fault:", {k: round(v, 2) for k, v in caught.items()})


def emu_convt(c, acc, B, pixH, pixW, Cout, prec, fault=None):
    b4 = c["bias"].astype(np.float64)
    if fault == "bias of quadrant 0 for all four":
        b4 = np.tile(b4[:Cout], 4)
    val = st(r32(acc + b4), prec)
    m = np.arange(B * pixH * pixW)
    x, y, img = m % pixW, (m // pixW) % pixH, m // (pixW * pixH)
    if fault == "image index not advanced when pixH == 1" and pixH == 1:
        img = np.zeros_like(img)
    late = (x < 8) & ((y > 0) | (img > 0)) if fault == "px wrap one step late" else np.zeros_like(m, dtype=bool)
    out = np.zeros((B * 2 * pixH, 2 * pixW, Cout))
    for qd in range(4):
        dy, dx = qd >> 1, qd & 1
        if fault == "dy / dx swapped":
            dy, dx = dx, dy
        v = val[:, qd * Cout:(qd + 1) * Cout]
        row, col = img * 2 * pixH + 2 * y + dy, 2 * x + dx
        out[row[~late], col[~late]] = v[~late]
        out[row[late] - 1, col[late]] = v[late]
    return out.reshape(B, 2 * pixH, 2 * pixW, Cout)


CONVT_FAULTS = {"dy / dx swapped": lambda B, pixH, pixW: True, "px wrap one step late": lambda B, pixH, pixW: B * pixH > 1,
                "image index not advanced when pixH == 1": lambda B, pixH, pixW: pixH == 1 and B > 1, "bias of quadrant 0 for all four": lambda B, pixH, pixW: True}


@pytest.mark.parametrize("prec", PRECS, ids=IDS)
def test_convt_emulation_is_inside_and_faults_are_outside(prec):
    worst, caught = 0.0, {}
    for (_, Cout, B, pixH, pixW, K, fam) in EP.convt_sweep(prec):
        c = EP.convt_case(Cout, B, pixH, pixW, K, fam, prec)
        acc = chain32(to_storage(c["A"], prec), to_storage(c["W"], prec))
        good = emu_convt(c, acc, B, pixH, pixW, Cout, prec)
        f = frac(good, c["ref"], c["bound"])
        worst = max(worst, f)
        assert f <= 1.0, (Cout, B, pixH, pixW, K, fam, f)
        for name, applies in CONVT_FAULTS.items():
            bad = emu_convt(c, acc, B, pixH, pixW, Cout, prec, fault=name)
            changed = not np.array_equal(bad, good)
            assert changed == applies(B, pixH, pixW), (name, Cout, B, pixH, pixW)
            if changed:
                f = frac(bad, c["ref"], c["bound"])
                assert f > 1.0, f"CONVT Cout={Cout} B={B} {pixH}x{pixW} K={K}: '{name}' stays inside the bound ({f:.3f})"
                caught[name] = min(caught.get(name, np.inf), f)
    # the uv term at the output pixel: `v += wu * u + wv * vv` unfused (the compiler may fuse; either is inside)
    Cout, B, pixH, pixW = EP.LAT_CONVT_UV_OUT
    c = EP.convt_case(Cout, B, pixH, pixW, 40, "random", prec, uv_out=True)
    acc = chain32(to_storage(c["A"], prec), to_storage(c["W"], prec))
    u0, u1, v0, v1 = EP.UV_RANGE
    m = np.arange(B * pixH * pixW)[:, None]
    n = np.arange(4 * Cout)[None, :]
    qd, co = n // Cout, n % Cout
    u = lin_at(u0, u1, 2 * pixW, 2 * (m % pixW) + (qd & 1))
    vv = lin_at(v0, v1, 2 * pixH, 2 * ((m // pixW) % pixH) + (qd >> 1))
    val = r32(r32(acc + c["bias"].astype(np.float64)) + r32(r32(c["wu"].astype(np.float64)[co] * u) + r32(c["wv"].astype(np.float64)[co] * vv)))
    f = frac(EP.pixel_shuffle(st(val, prec), B, pixH, pixW, Cout), c["ref"], c["bound"])
    assert f <= 1.0, f
    print(f"\nCONVT prec {prec}: honest emulation worst error / bound {worst:.3f} (uv at the output pixel {f:.3f}); weakest catch per fault:",
          {k: round(v, 2) for k, v in caught.items()})


def emu_uv(c, acc, B, pixH, pixW, act, prec, fault=None):
    u0, u1, v0, v1 = EP.UV_RANGE
    m = np.arange(B * pixH * pixW)[:, None]
    x = m % pixW + (1 if fault == "u taken at x + 1" else 0)
    y = m // pixW if fault == "y without % pixH" else (m // pixW) % pixH
    u, vv = lin_at(u0, u1, pixW, x), lin_at(v0, v1, pixH, y)
    if fault == "u and v swapped":
        u, vv = vv, u
    v = fma(c["wu"].astype(np.float64), u, fma(c["wv"].astype(np.float64), vv, r32(acc + c["bias"].astype(np.float64))))
    return st(np.maximum(v, 0.0) if act == 1 else v, prec)


UV_FAULTS = {"u taken at x + 1": lambda B, pixH, pixW: pixW > 1, "u and v swapped": lambda B, pixH, pixW: True,
             "y without % pixH": lambda B, pixH, pixW: B > 1 and pixH > 1}


@pytest.mark.parametrize("prec", PRECS, ids=IDS)
def test_uv_emulation_is_inside_and_faults_are_outside(prec):
    worst, caught = 0.0, {}
    for (_, N, B, pixH, pixW, K, fam, act) in EP.uv_sweep(prec):
        c = EP.uv_case(N, B, pixH, pixW, K, fam, prec, act)
        acc = chain32(to_storage(c["A"], prec), to_storage(c["W"], prec))
        good = emu_uv(c, acc, B, pixH, pixW, act, prec)
        f = frac(good, c["ref"], c["bound"])
        worst = max(worst, f)
        assert f <= 1.0, (N, B, pixH, pixW, K, fam, act, f)
        for name, applies in UV_FAULTS.items():
            bad = emu_uv(c, acc, B, pixH, pixW, act, prec, fault=name)
            changed = not np.array_equal(bad, good)
            assert changed == applies(B, pixH, pixW), (name, N, B, pixH, pixW)
            if changed:
                f = frac(bad, c["ref"], c["bound"])
                assert f > 1.0, f"uv N={N} B={B} {pixH}x{pixW} K={K} act={act}: '{name}' stays inside the bound ({f:.3f})"
                caught[name] = min(caught.get(name, np.inf), f)
    print(f"\nuv prec {prec}: honest emulation worst error / bound {worst:.3f}; weakest catch per fault:", {k: round(v, 2) for k, v in caught.items()})
