"""CPU: the float64 reference of the trainable attention (tests/attention_reference.py) against torch's own float64 autograd of
F.scaled_dot_product_attention, and the POWER of its per-element bounds: an honest float64 emulation of the four kernels of csrc/attention_grad.hip
(the stated roundings, nothing else) stays inside every bound on every element of every small case of the GPU sweep, in every input family and both
precisions, and each injected fault breaks a bound on at least one element at every shape where it applies, in at least one family - the rule of
tests/test_core_reference_cpu.py.  The GPU tests (tests/test_hip_attention_grad.py) measure the HIP kernels against the same cached cases.

Emulation.  Scores: the exact 64-term sum rounded once to fp32, times the fp32 constant fl(log2 e) / 8, rounded.  Forward: key tiles of 64, a true running
max, alpha = exp2 of the rounded difference, p = exp2 of the rounded difference, l and O rescaled and summed in fp32 (l from the unrounded p, O from p
rounded to fp16 in fp16), 1 / l and the product rounded, the store; lse = fl(fl(m + fl(log2 l)) fl(ln 2)) in fp32.  D: the exact sum of dO o O_stored
rounded to fp32.  Backward: p = fl(exp2(fl(chain fl(log2 e) / 8 - fl(lse fl(log2 e))))), dS = fl(p fl(fl(dP) - D)), both rounded to fp16 in fp16, the
three products summed exactly and rounded once to fp32, the 1/8, the store.

Faults (each is outside at every shape of the sweep where it applies, in both precisions unless marked).  With a single key dS = P (dP - D) is identically 0
and dq = dk = 0: a fault that only rescales, moves or adds copies of dS-terms leaves the result as it is, so those apply from N = 2:
  last key dropped from dq (N >= 2) - last query dropped from dk / dv (N >= 2) - the padded keys of the last key tile unmasked in dq, as clamped copies
  of key N - 1 (N % 64 != 0, N >= 2: at N = 1 the copies' dS is 0 like the key's own) - the padded queries of the last query tile unmasked in dk / dv, as
  clamped copies of query N - 1 (N % TQ != 0, TQ = 64 in fp16 and 32 in fp32; from N = 1, through dv) - the same two with the next head's first rows read
  instead (B nh > 1) - lse rounded to fp16 before the backward - lse + 1e-3 - D omitted (dS = P dP) - D of row N - 2 used for row N - 1 (N >= 2) - the 1/8
  missing on dk alone (N >= 2) - running sums rounded to fp16 once per tile (64 keys in dq, TQ queries in dk / dv; fp32 N >= 129, fp16 N = 1370) - within
  each 32-row sub-tile, rows with bits 2 and 3 of the index swapped in the second product only (ag_perm32 applied to one operand; fp16, N >= 9) - heads
  swapped in dk (nh > 1, N >= 2) - dq and dk exchanged (N >= 2).
  D taken from the unstored fp32 O (fp16) is NOT a fault: it must stay inside, and is asserted to.
Not covered (1 of 29 fault-and-precision pairs):
  running sums rounded to fp16 once per tile, fp16 storage, 129 <= N <= 257 (0.76 .. 0.99 of the bound at (1, 1, N); caught at some of the (2, 3, N)): a
  rounded partial sum costs at most h |partial| <= h sum |terms so far|, and with T = 3 .. 5 tiles the T - 1 extra roundings add up to at most (T - 1) / 2
  times h sum |terms| when nothing cancels, half of that on average.  A bound that admits the kernel's own rounding of P and dS to fp16 (h sum |terms|,
  worst case, which random roundings do not reach) and the store (h |result|) therefore cannot separate the fault before T is about 10.  At N = 1370
  (22 key tiles) it is outside, in dv: test_fp16_running_sums_are_outside_at_1370.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import attention_reference as AR
from tests.attention_reference import reference

PRECS = [0, 1]
IDS = ["fp32", "fp16"]


@pytest.mark.parametrize("B,nh,N", [(1, 1, 1), (2, 3, 65), (1, 2, 257)])
def test_reference_is_torch_float64_autograd(B, nh, N):
    g = torch.Generator().manual_seed(100 + N)
    q, k, v, do = (torch.randn(B, nh, N, 64, generator=g, dtype=torch.float64) for _ in range(4))
    q = q * 1.5
    v[:, :, N // 2] += 5.0
    ref = reference(q, k, v, do)
    bounded = AR.attention_grad(q, k, v, do, 0)
    ql, kl, vl = (t.clone().requires_grad_(True) for t in (q, k, v))
    o = F.scaled_dot_product_attention(ql, kl, vl)
    o.backward(do)
    lse = torch.logsumexp(q @ k.transpose(-1, -2) / 8.0, dim=-1)
    want = {"o": o.detach(), "lse": lse, "D": (do * o.detach()).sum(-1), "dq": ql.grad, "dk": kl.grad, "dv": vl.grad}
    # with a single key dS = P (dO V^T - D) is identically 0: dq and dk have no scale of their own (0, or 1e-16 of summation noise), so theirs is the
    # scale of the two terms that cancel, max|dO V^T| max|K| / 8 and max|dO V^T| max|Q| / 8
    scale = {n: float(w.abs().max()) for n, w in want.items()}
    if N == 1:
        cancel = float((do * v).sum(-1).abs().max())
        scale["dq"], scale["dk"] = cancel * float(k.abs().max()) / 8.0, cancel * float(q.abs().max()) / 8.0
    for name, w in want.items():
        for which, got in (("reference", ref.get(name)), ("attention_grad", torch.from_numpy(bounded[name][0]))):
            if got is None:                                        # reference() has no D
                continue
            assert scale[name] > 0.0
            err = float((got - w).abs().max()) / scale[name]
            assert err < 1e-12, (which, name, err)
            assert got.dtype == torch.float64 and got.shape == w.shape
        assert bounded[name][1].shape == w.shape and bounded[name][1].dtype == np.float64 and bool((bounded[name][1] > 0).all())


def test_families_and_cases_are_seeded_and_shared():
    a, b = AR.case(2, 3, 65, "offset", 1), AR.case(2, 3, 65, "offset", 1)
    assert a is b
    q, k, v, do = a["inputs"]
    assert all(t.dtype == np.float32 and t.shape == (2, 3, 65, 64) and np.array_equal(t, t.astype(np.float16).astype(np.float32)) for t in (q, k, v, do))
    q0, _, v0, do0 = AR.inputs(2, 3, 65, "random")
    assert all(torch.equal(torch.from_numpy(got), want.half().float()) for got, want in ((q, q0), (v, v0 + 3.0), (do, do0 + 0.25)))
    assert AR.SWEEP_N == (1, 2, 31, 32, 33, 63, 64, 65, 95, 96, 97, 127, 128, 129, 200, 255, 256, 257) and len(AR.SMALL) == 36


# ------------------------------------------------------------------------------------------------------------------ emulation and faults
LOG2E32 = float(np.float32(1.4426950408889634))
LN2_32 = float(np.float32(0.6931471805599453))
SCALE2 = LOG2E32 * 0.125


def r32(x):
    return np.asarray(x, dtype=np.float64).astype(np.float32).astype(np.float64)


def r16(x):
    return r32(x).astype(np.float16).astype(np.float64)


def rs(x, prec):
    return r16(x) if prec == 1 else x


def emu_forward(Q, K, V, prec):
    """One head -> (O as stored, O before the store, lse)."""
    N = K.shape[0]
    t = r32(r32(Q @ K.T) * SCALE2)
    m, l, O = np.full((N, 1), -1e30), np.zeros((N, 1)), np.zeros((N, 64))
    for t0 in range(0, N, 64):
        tt = t[:, t0:t0 + 64]
        m_new = np.maximum(m, tt.max(1, keepdims=True))
        alpha = r32(np.exp2(r32(m - m_new)))
        p = r32(np.exp2(r32(tt - m_new)))
        l = r32(r32(l * alpha) + r32(p.sum(1, keepdims=True)))
        O = r32(r32(O * alpha) + rs(p, prec) @ V[t0:t0 + 64])
        m = m_new
    o32 = r32(O * r32(1.0 / l))
    return rs(o32, prec), o32, r32(r32(m + r32(np.log2(l))) * LN2_32)[:, 0]


def emu_p_ds(Q, K, V, dO, lse, D, prec):
    """The recomputed P and dS (queries x keys), as the second products read them."""
    p = r32(np.exp2(r32(r32(Q @ K.T) * SCALE2 - r32(lse * LOG2E32)[:, None])))
    ds = r32(p * r32(r32(dO @ V.T) - D[:, None]))
    return rs(p, prec), rs(ds, prec)


def product(At, X, tile=0):
    """fl32(At^T X), contracted over rows; tile > 0 injects the fault of a running sum rounded to fp16 once per `tile` rows."""
    if not tile:
        return r32(At.T @ X)
    acc = np.zeros((At.shape[1], X.shape[1]))
    for r0 in range(0, At.shape[0], tile):
        acc = r16(acc + At[r0:r0 + tile].T @ X[r0:r0 + tile])
    return acc


def perm32_rows(M, clamp):
    """M padded to a multiple of 32 rows (clamped copies of the last row, or zeros) and the row order with bits 2 and 3 of the index swapped."""
    n = M.shape[0]
    pad = -n % 32
    M = np.concatenate([M, np.repeat(M[-1:], pad, 0) if clamp else np.zeros((pad,) + M.shape[1:])])
    i = np.arange(n + pad)
    return M, (i & ~0xC) | ((i & 4) << 1) | ((i & 8) >> 1)


INSIDE = "D from the unstored fp32 O"
FP16_SUMS = "running sums in fp16 per tile"


def faults(B, nh, N, prec):
    tq = 64 if prec == 1 else 32
    f = ["lse rounded to fp16", "lse + 1e-3", "D omitted"]
    if N >= 2:                                                     # with one key dq = dk = 0 whatever their scale or their places
        f += ["last key dropped from dq", "last query dropped from dk/dv", "D of the row before for the last row", "1/8 missing on dk", "dq and dk exchanged"]
    if N % 64 and N >= 2:
        f.append("padded keys unmasked in dq (clamped)")
    if N % tq:
        f.append("padded queries unmasked in dk/dv (clamped)")
    if B * nh > 1:
        if N % 64:
            f.append("padded keys unmasked in dq (next head)")
        if N % tq:
            f.append("padded queries unmasked in dk/dv (next head)")
    if N >= 129 and prec == 0:                                     # fp16: "Not covered" in the docstring, and the test at N = 1370 below
        f.append(FP16_SUMS)
    if prec == 1 and N >= 9:
        f.append("perm32 on one operand of the second product")
    if nh > 1 and N >= 2:
        f.append("heads swapped in dk")
    return f




def emu_forward_all(q, k, v, prec):
    return [emu_forward(q[g], k[g], v[g], prec) for g in range(q.shape[0])]


def emulate(q, k, v, do, prec, fwd, fault=None):
    """q, k, v, do (B nh, N, 64) float64 storage values, fwd = emu_forward_all(...) (the honest run, fault None, must come first) -> dict of (B nh, N, ...) arrays; fault: one of faults() or INSIDE."""
    G, N, _ = q.shape
    tq = 64 if prec == 1 else 32
    lse = np.stack([f[2] for f in fwd])
    o = np.stack([f[1] if fault == INSIDE else f[0] for f in fwd])
    D = r32((o * do).sum(-1))
    lse_b = r16(lse) if fault == "lse rounded to fp16" else r32(lse + 1e-3) if fault == "lse + 1e-3" else lse
    D_b = D.copy()
    if fault == "D omitted":
        D_b[:] = 0.0
    elif fault == "D of the row before for the last row":
        D_b[:, -1] = D_b[:, -2]
    tile_q, tile_kv = (64, tq) if fault == FP16_SUMS else (0, 0)
    res = {"o": np.stack([f[0] for f in fwd]), "lse": lse, "D": D_b if fault != "D omitted" else D}
    dq, dk, dv = np.empty_like(q), np.empty_like(q), np.empty_like(q)
    for g in range(G):
        Q, K, V, dO, ls, Dg = q[g], k[g], v[g], do[g], lse_b[g], D_b[g]
        nxt = (g + 1) % G
        Kq, Vq = K, V
        Qk, dOk, lk, Dk = Q, dO, ls, Dg
        npk, npq = -N % 64, -N % tq
        if fault == "last key dropped from dq":
            Kq, Vq = K[:-1], V[:-1]
        elif fault == "padded keys unmasked in dq (clamped)":
            Kq, Vq = np.concatenate([K, np.repeat(K[-1:], npk, 0)]), np.concatenate([V, np.repeat(V[-1:], npk, 0)])
        elif fault == "padded keys unmasked in dq (next head)":
            Kq, Vq = np.concatenate([K, k[nxt, :npk]]), np.concatenate([V, v[nxt, :npk]])
        elif fault == "last query dropped from dk/dv":
            Qk, dOk, lk, Dk = Q[:-1], dO[:-1], ls[:-1], Dg[:-1]
        elif fault == "padded queries unmasked in dk/dv (clamped)":
            Qk, dOk, lk, Dk = (np.concatenate([t, np.repeat(t[-1:], npq, 0)]) for t in (Q, dO, ls, Dg))
        elif fault == "padded queries unmasked in dk/dv (next head)":
            Qk, dOk, lk, Dk = (np.concatenate([t, s[nxt, :npq]]) for t, s in ((Q, q), (dO, do), (ls, lse_b), (Dg, D_b)))
        # the honest P and dS of a head are computed once (with the honest run, which comes first) and kept beside its forward
        changed = fault in (INSIDE, "lse rounded to fp16", "lse + 1e-3", "D omitted", "D of the row before for the last row")
        if fault is None:
            fwd[g] = fwd[g][:3] + (emu_p_ds(Q, K, V, dO, ls, Dg, prec),)
        honest = emu_p_ds(Q, K, V, dO, ls, Dg, prec) if changed else fwd[g][3]
        Pq, dSq = honest if Kq is K else emu_p_ds(Q, Kq, Vq, dO, ls, Dg, prec)
        Pk, dSk = honest if Qk is Q else emu_p_ds(Qk, K, V, dOk, lk, Dk, prec)
        if fault == "perm32 on one operand of the second product":
            Kp, perm = perm32_rows(Kq, True)
            dSq = perm32_rows(dSq.T, False)[0][perm].T
            Kq = Kp
            Qk, dOk = perm32_rows(Qk, True)[0], perm32_rows(dOk, True)[0]
            Pk, dSk = perm32_rows(Pk, False)[0][perm], perm32_rows(dSk, False)[0][perm]
        dq[g] = rs(r32(product(dSq.T, Kq, tile_q) * 0.125), prec)
        dk[g] = rs(r32(product(dSk, Qk, tile_kv) * (1.0 if fault == "1/8 missing on dk" else 0.125)), prec)
        dv[g] = rs(product(Pk, dOk, tile_kv), prec)
    res.update(dq=dq, dk=dk, dv=dv)
    return res


def fractions(got, c, B, nh, fault=None):
    """Worst |got - ref| / bound per tensor."""
    out = {}
    for name in AR.NAMES:
        ref, bound = c["ref"][name]
        g = got[name].reshape(ref.shape)
        if fault == "heads swapped in dk" and name == "dk":
            g = g[:, ::-1]
        out[name] = float((np.abs(g - ref) / bound).max())
    if fault == "dq and dk exchanged":
        out["dq"], out["dk"] = (float((np.abs(got[a].reshape(B, nh, -1, 64) - c["ref"][b][0]) / c["ref"][b][1]).max())
                                for a, b in (("dk", "dq"), ("dq", "dk")))
    return out


def worst_of(fr):
    """The worst fraction of a faulty run; inf or NaN in a result is outside."""
    return max(x if np.isfinite(x) else np.inf for x in fr.values())


@pytest.mark.parametrize("prec", PRECS, ids=IDS)
@pytest.mark.parametrize("B,nh,N", AR.SMALL)
def test_emulation_is_inside_and_faults_are_outside(B, nh, N, prec):
    todo = faults(B, nh, N, prec)
    caught = {}
    for family in AR.FAMILIES:
        c = AR.case(B, nh, N, family, prec)
        q, k, v, do = (t.astype(np.float64).reshape(B * nh, N, 64) for t in c["inputs"])
        fwd = emu_forward_all(q, k, v, prec)
        for what in (None, INSIDE)[:1 + prec]:                     # in fp32 the stored O is the fp32 O
            fr = fractions(emulate(q, k, v, do, prec, fwd, what), c, B, nh)
            print(f"B{B} nh{nh} N{N} {family} prec {prec}: {what or 'honest emulation'}, error / bound", " ".join(f"{n}={x:.3f}" for n, x in fr.items()))
            assert all(np.isfinite(x) and x <= 1.0 for x in fr.values()), (family, what, fr)
        for name in todo:
            if caught.get(name, 0.0) <= 1.0:                       # one family is enough: a fault already caught is not run again
                with np.errstate(over="ignore", invalid="ignore"):                     # an unmasked row can overflow to inf: outside, as it should be
                    caught[name] = max(caught.get(name, 0.0), worst_of(fractions(emulate(q, k, v, do, prec, fwd, name), c, B, nh, name)))
    print("  faults, best family:", {n: round(x, 2) for n, x in caught.items()})
    for name, x in caught.items():
        assert x > 1.0, f"B{B} nh{nh} N{N} prec {prec}: '{name}' stays inside every bound ({x:.3f}) in every family"


def test_fp16_running_sums_are_outside_at_1370():
    B, nh, N = AR.LARGE[0]
    worst = {}
    for family in ("random", "offset"):
        c = AR.case(B, nh, N, family, 1)
        q, k, v, do = (t.astype(np.float64).reshape(B * nh, N, 64) for t in c["inputs"])
        fwd = emu_forward_all(q, k, v, 1)
        fr = fractions(emulate(q, k, v, do, 1, fwd), c, B, nh)
        print(f"B{B} nh{nh} N{N} {family} fp16: honest emulation, error / bound", " ".join(f"{n}={x:.3f}" for n, x in fr.items()))
        assert all(x <= 1.0 for x in fr.values()), (family, fr)
        worst[family] = worst_of(fractions(emulate(q, k, v, do, 1, fwd, FP16_SUMS), c, B, nh))
    print("  running sums in fp16 per tile:", worst)
    assert all(x > 1.0 for x in worst.values()), worst
