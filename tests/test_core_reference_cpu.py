"""CPU: the float64 references of tests/core_reference.py against independent torch float64 formulations, and the POWER of the bounds: an honest float64
emulation of each kernel (the stated roundings, nothing else) stays inside the bound on every element of every case of the GPU sweep the CPU can do in
seconds, and each injected fault breaks the bound on at least one element at every shape where it applies, in at least one input family.

Emulations.  GEMM / conv / ConvTranspose2d: storage-type inputs, the exact sum rounded once to fp32, the bias added in fp32, the activation (exact GELU
rounded to fp32), the fp16 store.  Attention, fp16: q' = fp16(fp32(q * fp32(log2(e) / 8))), scores rounded to fp32, a stale max taken from the first 64 keys and
raised only when a weight would pass 2^14, P rounded to fp16, l from the rounded P in the tiles between the first and the last and from the unrounded P in
those two (attention_pp.hip exact_block), fp32 O and l, the fp16 store; fp32: q' in fp32, the true max, nothing rounded to fp16.

Faults and where they apply (every one is caught at every shape of the sweep where it applies, unless listed under "not covered"):
  GEMM          last K element dropped (K >= 2) - last chunk of K dropped (K >= 2 chunks) - last row computed from the row before it (M >= 2) - bias missing on
                the last column - running sum rounded to fp16 every 32 terms (64 <= K <= 1024, at least 16 outputs)
  conv 3x3      the same five on the im2col form (K = 9 Cin) - zero padding instead of replicate at the top-left corner tap - with H = 2, the top halo row
                taken from row 1 (the wrong side) instead of row 0
  attention     last key dropped (N >= 2) - the padding keys of the last tile unmasked with score 0 and v = 0 (N % 64 != 0) - the same with the next head's
                first rows as keys (N % 64 != 0, B nh > 1) - queries i and i + 16 swapped (N >= 17) - heads swapped (nh > 1)
Not covered:
  running sum rounded to fp16 every 32 terms, K < 64: there is one rounded partial, the final sum, and for fp16 storage it is rounded to fp16 again on the
  store: the fault is a double rounding, inside any bound that admits the store.
  the same fault with fewer than 16 outputs (the sweep has one such case, M = 1, N = 4, K = 128, fp16: 0.54 / 0.56 of the bound in the two families): the four
  rounded partials are no larger than the result, so their errors stay within the half fp16 ulp the store is allowed; with 16 or more outputs some element
  always has a partial sum larger than its result.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import core_reference as CR
from tail_reference import to_storage

PRECS = [0, 1]
IDS = ["fp32", "fp16"]


def r32(x):
    return np.asarray(x, dtype=np.float64).astype(np.float32).astype(np.float64)


def r16(x):
    return r32(x).astype(np.float16).astype(np.float64)


def inside(got, c, key=("ref", "bound")):
    return float((np.abs(got - c[key[0]]) / c[key[1]]).max())


# ------------------------------------------------------------------------------------------------------------------ references
@pytest.mark.parametrize("prec", PRECS, ids=IDS)
def test_gemm_reference_is_a_matmul(prec):
    for M, N, K, act, fam in [(5, 12, 24, 0, "random"), (3, 8, 40, 1, "offset"), (7, 4, 16, 2, "random")]:
        c = CR.gemm_case(M, N, K, act, fam, prec)
        A, W, b = (torch.from_numpy(to_storage(c[k], prec) if k != "bias" else c[k].astype(np.float64)) for k in ("A", "W", "bias"))
        pre = A @ W.T + b
        want = (pre, F.relu(pre), F.gelu(pre))[act]
        assert np.allclose(c["ref"], want.numpy(), rtol=0, atol=1e-13)
        assert (c["bound"] > 0).all()


@pytest.mark.parametrize("relu_in", [0, 1])
@pytest.mark.parametrize("H,W", [(1, 1), (1, 5), (2, 2), (5, 1), (4, 7)])
def test_conv_reference_is_conv2d_on_a_replicate_padded_input(H, W, relu_in):
    x, w, bias = CR.conv_inputs(2, H, W, 8, 12, "coded")
    ref, bound, _ = CR.conv3x3(x, w, bias, 0, bool(relu_in), 0)
    xt = torch.from_numpy(x).double().permute(0, 3, 1, 2)
    if relu_in:
        xt = F.relu(xt)
    want = F.conv2d(F.pad(xt, (1, 1, 1, 1), mode="replicate"), torch.from_numpy(w).double(), torch.from_numpy(bias).double()).permute(0, 2, 3, 1)
    assert np.allclose(ref, want.numpy(), rtol=0, atol=1e-12)


@pytest.mark.parametrize("H,W", [(1, 1), (2, 3), (1, 4), (5, 1), (4, 6)])
def test_up2_reference_is_interpolate_then_conv2d(H, W):
    x, w, bias = CR.conv_inputs(2, H, W, 8, 4, "coded")
    xt = torch.from_numpy(x).double().permute(0, 3, 1, 2)
    up = F.interpolate(xt, scale_factor=2, mode="bilinear", align_corners=False)
    assert np.allclose(CR.up2(x.astype(np.float64)), up.permute(0, 2, 3, 1).numpy(), rtol=0, atol=1e-14)
    want = F.conv2d(F.pad(up, (1, 1, 1, 1), mode="replicate"), torch.from_numpy(w).double(), torch.from_numpy(bias).double()).permute(0, 2, 3, 1).numpy()
    ref, bound, _ = CR.conv_up2(x, w, bias, 0)
    assert np.allclose(ref, want, rtol=0, atol=1e-12)
    # the four-phase form with UNROUNDED combined weights is the same operation (replicate padding at the high resolution = index clamping at the low one)
    weff = np.einsum("oiyx,pya,qxb->pqoabi", w.astype(np.float64), CR.UP2_R, CR.UP2_R)
    ref_p, _ = CR.conv_up2_phase(x, w, bias, 0, weff=weff)
    assert np.allclose(ref_p, want, rtol=0, atol=1e-12)
    # ... and the rounding of the combined weights, fp16, is inside the term that bounds it
    ref16, bound16, _ = CR.conv_up2(to_storage(x, 1), w, bias, 1)
    ref16p, _ = CR.conv_up2_phase(to_storage(x, 1), w, bias, 1)
    assert (np.abs(ref16p - ref16) <= bound16).all()


@pytest.mark.parametrize("H,W", [(1, 1), (1, 3), (4, 5)])
def test_convt_reference_is_conv_transpose2d(H, W):
    x, w, bias = CR.conv_inputs(2, H, W, 8, 12, "random", transposed=True)
    ref, bound, _ = CR.convt2x2(x, w, bias, 0)
    want = F.conv_transpose2d(torch.from_numpy(x).double().permute(0, 3, 1, 2), torch.from_numpy(w).double(), torch.from_numpy(bias).double(), stride=2)
    assert np.allclose(ref, want.permute(0, 2, 3, 1).numpy(), rtol=0, atol=1e-12)


@pytest.mark.parametrize("family", CR.ATTN_FAMILIES)
@pytest.mark.parametrize("B,nh,N", [(1, 1, 1), (2, 3, 17), (1, 2, 130)])
def test_attention_reference_is_sdpa(B, nh, N, family):
    c = CR.attention_case(B, nh, N, family, 0)
    q, k, v = (torch.from_numpy(c[t]).double() for t in "qkv")
    want = F.scaled_dot_product_attention(q, k, v).permute(0, 2, 1, 3).reshape(B, N, nh * 64)
    assert np.allclose(c["ref"], want.numpy(), rtol=0, atol=1e-12)
    assert (c["bound"] > 0).all()


def test_ln_references():
    rng = np.random.default_rng(0)
    x = to_storage(rng.standard_normal((5, 128)) * 2 + 0.7, 1)
    part, pb = CR.ln_partials(x)
    assert part.shape == (5, 4, 2) and np.allclose(part[..., 0].sum(-1), x.sum(-1)) and np.allclose(part[..., 1].sum(-1), (x * x).sum(-1))
    for mr, e in (CR.ln_stats(part, 128), CR.ln_stats_of_stream(x)):
        t = torch.from_numpy(x)
        assert np.allclose(mr[:, 0], t.mean(-1).numpy(), rtol=0, atol=1e-13)
        assert np.allclose(mr[:, 1], torch.rsqrt(t.var(-1, unbiased=False) + 1e-6).numpy(), rtol=1e-12, atol=0)
        assert (e > 0).all()
    # the statistics an fp32 epilogue and finalize would produce (everything rounded to fp32 at every step) are inside both bounds
    g = r32(x).reshape(5, 4, 32)
    p32 = np.stack([r32(g.sum(-1)), r32(r32(g * g).sum(-1))], -1)
    assert (np.abs(p32 - part) <= pb).all()
    mean = r32(r32(p32[..., 0].sum(-1)) / 128)
    rstd = r32(1 / np.sqrt(r32(np.maximum(r32(r32(p32[..., 1].sum(-1)) / 128) - mean * mean, 0)) + 1e-6))
    for mr, e in (CR.ln_stats(p32, 128), CR.ln_stats_of_stream(x)):
        assert (np.abs(np.stack([mean, rstd], -1) - mr) <= e).all()
    # ... and statistics that miss one 32-column group are far outside
    mr, e = CR.ln_stats_of_stream(x)
    bad, _ = CR.ln_stats(part[:, :3], 128)
    assert (np.abs(bad - mr) > e).all()


# ------------------------------------------------------------------------------------------------------------------ GEMM: emulation and faults
def emu_dot(a, w, bias, act, prec, fp16_every=0):
    """a (..., K), w (N, K) storage values -> the honest kernel's output; fp16_every > 0 injects the fault of a running sum kept in fp16."""
    if fp16_every:
        acc = np.zeros(a.shape[:-1] + (w.shape[0],))
        for k0 in range(0, a.shape[-1], fp16_every):
            acc = r16(acc + a[..., k0:k0 + fp16_every] @ w[:, k0:k0 + fp16_every].T)
    else:
        acc = r32(a @ w.T)
    v = r32(acc + bias)
    if act == 1:
        v = np.maximum(v, 0.0)
    elif act == 2:
        v = r32(CR.gelu(v))
    return r16(v) if prec == 1 else v


def dot_faults(a, w, bias, act, prec, ch):
    """name -> faulty output, for a (rows, K), w (N, K), the faults of the docstring that apply to the shape."""
    K = a.shape[-1]
    out = {}
    if K >= 2:
        out["last K element dropped"] = emu_dot(a[..., :-1], w[:, :-1], bias, act, prec)
    if K >= 2 * ch:
        out["last chunk of K dropped"] = emu_dot(a[..., :-ch], w[:, :-ch], bias, act, prec)
    if a.shape[0] >= 2:
        a2 = a.copy()
        a2[-1] = a2[-2]
        out["last row from the row before"] = emu_dot(a2, w, bias, act, prec)
    b2 = bias.copy()
    b2[-1] = 0.0
    out["bias missing on the last column"] = emu_dot(a, w, b2, act, prec)
    if 64 <= K <= 1024 and a.shape[0] * w.shape[0] >= 16:
        out["running sum in fp16 every 32 terms"] = emu_dot(a, w, bias, act, prec, fp16_every=32)
    return out


@pytest.mark.parametrize("prec", PRECS, ids=IDS)
def test_gemm_emulation_is_inside_and_faults_are_outside(prec):
    worst, caught = 0.0, {}
    for (M, N, K, act, fam) in CR.gemm_cases(prec):
        shape_caught = {}
        for family in CR.FAMILIES:                       # a fault must be caught in at least one family; the emulation must hold in both
            if act == 2 and family == "offset" and K > 1024:
                continue
            c = CR.gemm_case(M, N, K, act, family, prec)
            A, W, bias = to_storage(c["A"], prec), to_storage(c["W"], prec), c["bias"].astype(np.float64)
            frac = inside(emu_dot(A, W, bias, act, prec), c)
            worst = max(worst, frac)
            assert frac <= 1.0, (M, N, K, act, family, frac)
            for name, bad in dot_faults(A, W, bias, act, prec, CR.chunk(prec)).items():
                shape_caught[name] = max(shape_caught.get(name, 0.0), inside(bad, c))
        for name, f in shape_caught.items():
            assert f > 1.0, f"GEMM {M}x{N}x{K} act {act}: '{name}' stays inside the bound ({f:.3f}) in every family"
            caught[name] = min(caught.get(name, np.inf), f)
    print(f"\nGEMM prec {prec}: honest emulation worst error / bound {worst:.3f}; weakest catch per fault:", {k: round(v, 2) for k, v in caught.items()})


# ------------------------------------------------------------------------------------------------------------------ conv: emulation and faults
def im2col(x, halo="replicate"):
    """x (B,H,W,C) -> (B H W, 9 C) in (dy, dx, c) order.  halo: 'replicate'; 'zero_corner': the top-left halo pixel is 0; 'wrong_side': the top halo row is
    row 1 (H = 2: the row the bottom halo should take)."""
    B, H, W, C = x.shape
    xp = np.pad(x, ((0, 0), (1, 1), (1, 1), (0, 0)), mode="edge")
    if halo == "zero_corner":
        xp[:, 0, 0] = 0.0
    elif halo == "wrong_side":
        xp[:, 0] = xp[:, 2]
    return np.concatenate([xp[:, dy:dy + H, dx:dx + W] for dy in range(3) for dx in range(3)], -1).reshape(B * H * W, 9 * C)


@pytest.mark.parametrize("prec", PRECS, ids=IDS)
def test_conv_emulation_is_inside_and_faults_are_outside(prec):
    worst, caught = 0.0, {}
    for (B, H, W, Cin, Cout, relu_in, act, fam) in CR.conv_cases():
        if Cin > 64 and prec == 0:
            continue                                  # (the fp32 form of the wide cases adds nothing to the power of the bound; the GPU sweep runs them)
        shape_caught = {}
        for family in CR.CONV_FAMILIES:
            c = CR.conv_case(B, H, W, Cin, Cout, relu_in, act, family, prec)
            x, w, bias = to_storage(c["x"], prec), to_storage(c["w"], prec), c["bias"].astype(np.float64)
            if relu_in:
                x = np.maximum(x, 0.0)
            wk = w.transpose(0, 2, 3, 1).reshape(Cout, 9 * Cin)
            cc = dict(ref=c["ref"].reshape(-1, Cout), bound=c["bound"].reshape(-1, Cout))
            a = im2col(x)
            frac = inside(emu_dot(a, wk, bias, act, prec), cc)
            worst = max(worst, frac)
            assert frac <= 1.0, (B, H, W, Cin, Cout, family, prec, frac)
            faults = dot_faults(a, wk, bias, act, prec, CR.chunk(prec))
            faults["zero padding at the corner tap"] = emu_dot(im2col(x, "zero_corner"), wk, bias, act, prec)
            if H == 2:
                faults["top halo from the wrong side (H = 2)"] = emu_dot(im2col(x, "wrong_side"), wk, bias, act, prec)
            for name, bad in faults.items():
                shape_caught[name] = max(shape_caught.get(name, 0.0), inside(bad, cc))
        for name, f in shape_caught.items():
            assert f > 1.0, f"conv {B}x{H}x{W} {Cin}->{Cout} prec {prec}: '{name}' stays inside the bound ({f:.3f}) in every family"
            caught[name] = min(caught.get(name, np.inf), f)
    print(f"\nconv prec {prec}: honest emulation worst error / bound {worst:.3f}; weakest catch per fault:", {k: round(v, 2) for k, v in caught.items()})


@pytest.mark.parametrize("prec", PRECS, ids=IDS)
def test_up2_and_convt_emulations_are_inside(prec):
    """up2: the kernel's own form - four phase convs with combined weights rounded once (here: fp32 combination, as pack_phase_conv_kernel) - against the
    DEFINITION's reference and its bound; ConvTranspose2d: four 1x1 GEMMs."""
    worst = 0.0
    for (B, H, W, Cin, Cout, fam) in CR.UP2_CASES:
        c = CR.up2_case(B, H, W, Cin, Cout, fam, prec)
        x = to_storage(c["x"], prec)
        w32 = c["w"].astype(np.float32)
        R = CR.UP2_R.astype(np.float32)
        weff = np.zeros((2, 2, Cout, 3, 3, Cin), dtype=np.float32)
        for dy in range(3):
            for dx in range(3):                           # the same order of fp32 additions as the pack kernel
                weff += w32[:, :, dy, dx][None, None, :, None, None, :] * (R[:, dy, :][:, None, None, :, None, None] * R[:, dx, :][None, :, None, None, :, None])
        weff = to_storage(weff, prec)
        got = np.zeros_like(c["ref"])
        a = im2col(x)
        for py in range(2):
            for px in range(2):
                wk = weff[py, px].reshape(Cout, 9 * Cin)
                got[:, py::2, px::2] = emu_dot(a, wk, c["bias"].astype(np.float64), 0, prec).reshape(B, H, W, Cout)
        worst = max(worst, inside(got, c), inside(got, c, ("ref_phase", "bound_phase")) if prec == 0 else 0.0)
        assert inside(got, c) <= 1.0, (B, H, W, Cin, Cout, fam)
        bad = got.copy()
        bad[:, 0, 0] = emu_dot(im2col(x, "zero_corner"), weff[0, 0].reshape(Cout, 9 * Cin), c["bias"].astype(np.float64), 0, prec).reshape(B, H, W, Cout)[:, 0, 0]
        assert inside(bad, c) > 1.0, ("up2 zero corner", B, H, W, Cin, Cout, fam)
    for (B, H, W, Cin, Cout, fam) in CR.CONVT_CASES:
        c = CR.convt_case(B, H, W, Cin, Cout, fam, prec)
        x, w, bias = to_storage(c["x"], prec), to_storage(c["w"], prec), c["bias"].astype(np.float64)
        got = np.zeros_like(c["ref"])
        for dy in range(2):
            for dx in range(2):
                got[:, dy::2, dx::2] = emu_dot(x.reshape(-1, Cin), w[:, :, dy, dx].T, bias, 0, prec).reshape(B, H, W, Cout)
        worst = max(worst, inside(got, c))
        assert inside(got, c) <= 1.0, (B, H, W, Cin, Cout, fam)
        bad = got.copy()
        bad[:, 0::2, 0::2], bad[:, 0::2, 1::2] = got[:, 0::2, 1::2], got[:, 0::2, 0::2]           # the dx phases swapped
        assert inside(bad, c) > 1.0
        assert inside(emu_dot(x.reshape(-1, Cin)[:, :-1], w[:-1, :, 0, 0].T, bias, 0, prec).reshape(B, H, W, Cout), dict(ref=c["ref"][:, 0::2, 0::2], bound=c["bound"][:, 0::2, 0::2])) > 1.0
    print(f"\nup2 / convT prec {prec}: honest emulation worst error / bound {worst:.3f}")


# ------------------------------------------------------------------------------------------------------------------ attention: emulation and faults
SC32 = float(np.float32(0.125) * np.float32(1.4426950408889634))


def emu_attention_head(q, k, v, prec):
    """One head: q (Nq,64), k, v (Nk,64) storage values -> (Nq,64).  See the module docstring."""
    Nk = k.shape[0]
    if prec == 0:
        s = r32(r32(q * SC32) @ k.T)
        m = s.max(1, keepdims=True)
        p = r32(np.exp2(s - m))
        return r32(r32(p @ v) / r32(p.sum(1, keepdims=True)))
    s = r32(r16(q * SC32) @ k.T)
    nt = (Nk + 63) // 64
    m = s[:, :64].max(1, keepdims=True)
    O, l = np.zeros_like(q), np.zeros((q.shape[0], 1))
    for t in range(nt):
        st = s[:, 64 * t:64 * t + 64]
        need = st.max(1, keepdims=True) - m > 14.0                        # a weight above 2^14: raise the max (exactly), rescale
        m_new = np.where(need, np.maximum(m, st.max(1, keepdims=True)), m)
        alpha = r32(np.exp2(m - m_new))
        O, l, m = r32(O * alpha), r32(l * alpha), m_new
        p = r32(np.exp2(st - m))
        exact = (t == 0) | (t == nt - 1) | need
        l = r32(l + np.where(exact, p.sum(1, keepdims=True), r16(p).sum(1, keepdims=True)))
        O = r32(O + r16(p) @ v[64 * t:64 * t + 64])
    return r16(r32(O / l))


def emu_attention(q, k, v, prec, fault=None):
    """q, k, v (B,nh,N,64) -> (B,N,nh 64); fault: one of the attention faults of the docstring."""
    B, nh, N, _ = q.shape
    npad = -N % 64
    out = np.zeros((B, N, nh, 64))
    kf, vf = k.reshape(B * nh, N, 64), v.reshape(B * nh, N, 64)
    for b in range(B):
        for h in range(nh):
            kk, vv = k[b, h], v[b, h]
            if fault == "last key dropped":
                kk, vv = kk[:-1], vv[:-1]
            elif fault == "padding keys unmasked (score 0, v 0)":
                kk, vv = np.concatenate([kk, np.zeros((npad, 64))]), np.concatenate([vv, np.zeros((npad, 64))])
            elif fault == "padding keys unmasked (next head's rows)":
                nxt = (b * nh + h + 1) % (B * nh)
                kk, vv = np.concatenate([kk, kf[nxt, :npad]]), np.concatenate([vv, vf[nxt, :npad]])
            out[b, :, h] = emu_attention_head(q[b, h], kk, vv, prec)
    if fault == "queries i and i + 16 swapped":
        i = np.arange(N)
        j = np.where((i % 32 < 16) & (i + 16 < N), i + 16, np.where((i % 32 >= 16), i - 16, i))
        out = out[:, j]
    elif fault == "heads swapped":
        out = out[:, :, ::-1]
    return out.reshape(B, N, nh * 64)


def attention_faults(B, nh, N):
    f = []
    if N >= 2:
        f.append("last key dropped")
    if N % 64:
        f.append("padding keys unmasked (score 0, v 0)")
        if B * nh > 1 and N >= 64 - N % 64:
            f.append("padding keys unmasked (next head's rows)")
    if N >= 17:
        f.append("queries i and i + 16 swapped")
    if nh > 1:
        f.append("heads swapped")
    return f


@pytest.mark.parametrize("prec", PRECS, ids=IDS)
@pytest.mark.parametrize("B,nh,N", CR.ATTN_SMALL + CR.ATTN_LARGE[:1])
def test_attention_emulation_is_inside_and_faults_are_outside(B, nh, N, prec):
    caught = {}
    for family in CR.ATTN_FAMILIES:
        c = CR.attention_case(B, nh, N, family, prec)
        q, k, v = (c[t].astype(np.float64) for t in "qkv")
        frac = inside(emu_attention(q, k, v, prec), c)
        print(f"attention B{B} nh{nh} N{N} {family} prec {prec}: honest emulation error / bound {frac:.3f}")
        assert frac <= 1.0
        for name in attention_faults(B, nh, N):
            caught[name] = max(caught.get(name, 0.0), inside(emu_attention(q, k, v, prec, name), c))
    print("  faults, best family:", {k: round(v, 2) for k, v in caught.items()})
    for name, f in caught.items():
        assert f > 1.0, f"attention B{B} nh{nh} N{N} prec {prec}: '{name}' stays inside the bound ({f:.3f}) in every family"
