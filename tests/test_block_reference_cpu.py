"""CPU: the float64 references of tests/block_reference.py are the right ones (torch's float64 autograd of F.layer_norm, F.gelu and x + r * gamma),
their bounds hold an honest fp32 emulation that sums in another order than the kernels (another split of the row, another slab size, partials
added in reverse), and each of a list of injected faults - what csrc/block_grad.hip could get wrong - lands OUTSIDE a bound on the inputs chosen
here.  No GPU."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import block_reference as BR
from block_reference import to_storage

F32 = np.float32
SHAPES = [(1, 8), (5, 72), (33, 520), (65, 1024)]


def rounded(v, prec):
    """fp32 -> storage type -> float64: the kernel's single rounding of a result."""
    return to_storage(np.asarray(v, dtype=F32), prec)


def inside(got, ref_bound):
    ref, bound = ref_bound
    return bool((np.abs(got - ref) <= bound).all())


frac = BR.fraction


def close(ref, t):
    return ref.shape == tuple(t.shape) and np.abs(ref - t.numpy()).max() <= 1e-12 * max(1.0, np.abs(ref).max())


@pytest.mark.parametrize("M,C", SHAPES)
@pytest.mark.parametrize("family", BR.FAMILIES)
def test_references_agree_with_torch_float64_autograd(M, C, family):
    t = {k: torch.tensor(v, dtype=torch.float64, requires_grad=True) for k, v in BR.inputs(M, C, family).items()}
    # layer_norm
    n = F.layer_norm(t["x"], (C,), t["w"], t["b"], BR.EPS)
    gx, gw, gb = torch.autograd.grad(n, (t["x"], t["w"], t["b"]), t["dn"].detach())
    ref = BR.layer_norm(*(t[k].detach().numpy() for k in ("x", "w", "b", "dn")), 0, 0)
    for name, got in (("n", n.detach()), ("dx", gx), ("dw", gw), ("db", gb), ("mean", t["x"].detach().mean(1)),
                      ("rstd", 1.0 / torch.sqrt(t["x"].detach().var(1, unbiased=False) + BR.EPS))):
        assert close(ref[name][0], got) and (ref[name][1] > 0).all(), name
    # gelu
    y = F.gelu(t["h"])
    (gh,) = torch.autograd.grad(y, t["h"], t["dn"].detach())
    ref = BR.gelu_pair(t["h"].detach().numpy(), t["dn"].detach().numpy(), 0)
    assert close(ref["y"][0], y.detach()) and close(ref["dx"][0], gh) and (ref["y"][1] > 0).all() and (ref["dx"][1] > 0).all()
    # scale_residual
    y = t["x"] + t["r"] * t["gamma"]
    gx, gr, gg = torch.autograd.grad(y, (t["x"], t["r"], t["gamma"]), t["dx1"].detach())
    ref = BR.scale_residual(*(t[k].detach().numpy() for k in ("x", "r", "gamma", "dx1")), 0, 0)
    assert torch.equal(gx, t["dx1"].detach())                          # the gradient of x is dy itself
    assert close(ref["y"][0], y.detach()) and close(ref["dr"][0], gr) and close(ref["dgamma"][0], gg)
    # the fused pair, with both gradients and with each alone; prec 0 and the x1 torch computed, so that nothing is rounded in between
    x1 = t["x"] + t["r"] * t["gamma"]
    n = F.layer_norm(x1, (C,), t["w"], t["b"], BR.EPS)
    names = ("x", "r", "gamma", "w", "b")
    for use1, usen in ((True, True), (True, False), (False, True)):
        outs = [o for o, use in ((x1, use1), (n, usen)) if use]
        gs = [t[k].detach() for k, use in (("dx1", use1), ("dn", usen)) if use]
        grads = torch.autograd.grad(outs, [t[k] for k in names], gs, retain_graph=True, allow_unused=True)
        ref = BR.fused(*(t[k].detach().numpy() for k in names), t["dx1"].detach().numpy() if use1 else None, t["dn"].detach().numpy() if usen else None, 0, 0, 0,
                       x1=x1.detach().numpy())
        assert close(ref["x1"][0], x1.detach()) and close(ref["n"][0], n.detach())
        for name, g in zip(("dx", "dr", "dgamma", "dw", "db"), grads):
            assert close(ref[name][0], torch.zeros(ref[name][0].shape, dtype=torch.float64) if g is None else g), (name, use1, usen)


# ---- an honest fp32 emulation in another order -------------------------------------------------------------------------------------------------------
def rowsum(a, pieces=3):
    """fp32 row sums over C as `pieces` partial sums added afterwards (the kernels: per lane, then a butterfly)."""
    edges = np.linspace(0, a.shape[1], pieces + 1).astype(int)
    s = np.zeros((a.shape[0], 1), dtype=F32)
    for c0, c1 in zip(edges[:-1], edges[1:]):
        s = s + a[:, c0:c1].sum(1, dtype=F32, keepdims=True)
    return s


def colsum(a, slab=7):
    """fp32 column sums over M: slabs of 7 rows (the kernels: 32), the partials added in REVERSE slab order."""
    parts = [a[m0:m0 + slab].sum(0, dtype=F32) for m0 in range(0, a.shape[0], slab)]
    s = np.zeros(a.shape[1], dtype=F32)
    for p in reversed(parts):
        s = s + p
    return s


def emu_ln_forward(x, w, b, eps=BR.EPS, fault=None):
    C = x.shape[1]
    inv = F32(1.0) / F32(C)
    xs = x[:, :-BR.chunk(0)] if fault == "last chunk dropped from the statistics" else x
    mean = rowsum(xs) * inv
    if fault == "one-pass variance":
        var = rowsum(xs * xs) * inv - mean * mean
    else:
        d = xs - mean
        var = rowsum(d * d) * inv
    if fault == "last chunk dropped from the statistics":
        mean, var = mean * F32(xs.shape[1] / C), var * F32(xs.shape[1] / C)          # divided by C, summed over less
    rstd = F32(1.0) / (np.sqrt(var) + F32(eps)) if fault == "eps after the square root" else F32(1.0) / np.sqrt(var + F32(eps))
    return mean.astype(F32), rstd.astype(F32), ((x - mean) * rstd * w + b).astype(F32)


def emu_ln_backward(x, w, dn, mean, rstd, fault=None):
    inv = F32(1.0) / F32(x.shape[1])
    xh = (x - mean) * rstd
    g = dn * w
    m1, m2 = rowsum(g) * inv, rowsum(g * xh) * inv
    if fault == "mean(g xh) term missing":
        m2 = m2 * F32(0)
    dx = rstd * (g - m1 - xh * m2)
    return dx.astype(F32), colsum(dn * xh), colsum(dn)


def emu_norm(c, px, pn, fault=None):
    x, w, b, dn = (c[k].astype(F32) for k in ("x", "w", "b", "dn"))
    mean, rstd, n = emu_ln_forward(x, w, b, fault=fault)
    dx, dw, db = emu_ln_backward(x, w, dn, mean, rstd, fault=fault)
    if fault == "a row past M counted in dw":
        dw = dw + dn[-1] * ((x[-1] - mean[-1]) * rstd[-1])
    return {"n": rounded(n, pn), "mean": mean[:, 0].astype(np.float64), "rstd": rstd[:, 0].astype(np.float64), "dx": rounded(dx, px), "dw": rounded(dw, px),
            "db": rounded(db, px)}


def erf32(x):
    return torch.erf(torch.from_numpy(np.ascontiguousarray(x, dtype=F32))).numpy()


def emu_gelu(c, prec, fault=None):
    x, dy = c["x"].astype(F32), c["dy"].astype(F32)
    if fault == "gelu_fast in place of erf":                           # common.h gelu_fast: x sigmoid(x P(x^2))
        x2 = x * x
        p = F32(2.09755530e-06)
        for k in (-5.83663339e-05, -2.66659641e-04, 7.29729188e-02, 1.59563637):
            p = p * x2 + F32(k)
        y = x / (F32(1) + np.exp(-(p * x)))
    else:
        y = F32(0.5) * x * (F32(1) + erf32(x * F32(math.sqrt(0.5))))
    if fault == "tanh derivative":                                     # the derivative of the tanh approximation
        k, a = F32(math.sqrt(2.0 / math.pi)), F32(0.044715)
        th = np.tanh(k * (x + a * x * x * x))
        G = F32(0.5) * (F32(1) + th) + F32(0.5) * x * (F32(1) - th * th) * k * (F32(1) + F32(3) * a * x * x)
    else:
        G = F32(0.5) * (F32(1) + erf32(x * F32(math.sqrt(0.5)))) + x * (F32(1.0 / math.sqrt(2.0 * math.pi)) * np.exp(F32(-0.5) * x * x))
    return {"y": rounded(y, prec), "dx": rounded(dy * G, prec)}


def emu_sr(c, px, pr, fault=None):
    x, r, gamma, dy = (c[k].astype(F32) for k in ("x", "r", "gamma", "dx1"))
    return {"y": rounded(x + r * gamma, px), "dr": rounded(dy if fault == "gamma missing in dr" else dy * gamma, pr), "dgamma": rounded(colsum(dy * r), px)}


def emu_fused(c, px, pr, pn, fault=None, use1=True, usen=True):
    x, r, gamma, w, b, dn, dx1 = (c[k].astype(F32) for k in ("x", "r", "gamma", "w", "b", "dn", "dx1"))
    x1 = rounded(x + r * gamma, px).astype(F32)
    mean, rstd, n = emu_ln_forward(x1, w, b)
    zero = np.zeros_like(x)
    dxl, dw, db = emu_ln_backward(x1, w, dn, mean, rstd) if usen else (zero, np.zeros_like(w), np.zeros_like(w))
    dx = dxl + (dx1 if use1 and fault != "the fused backward drops dx1" else zero)
    return {"x1": x1.astype(np.float64), "n": rounded(n, pn), "dx": rounded(dx, px), "dr": rounded(dx * gamma, pr), "dgamma": rounded(colsum(dx * r), px),
            "dw": rounded(dw, px), "db": rounded(db, px)}, x1


def fused_ref(c, px, pr, pn, x1, use1=True, usen=True):
    return BR.fused(c["x"], c["r"], c["gamma"], c["w"], c["b"], c["dx1"] if use1 else None, c["dn"] if usen else None, px, pr, pn, x1=x1)


def report(what, got, ref, names=None):
    fr = {n: frac(got[n], ref[n]) for n in (names or got)}
    print(what, " ".join(f"{n}={f:.3f}" for n, f in fr.items()), "(worst error / bound)")
    return fr


@pytest.mark.parametrize("family", BR.FAMILIES)
@pytest.mark.parametrize("M,C", SHAPES + [(300, 136)])
def test_an_honest_fp32_emulation_stays_inside_every_bound(M, C, family):
    for px, pn in BR.PAIRS_LN:
        c = BR.case_norm(M, C, family, px, pn)
        for n, f in report(f"emulation layer_norm M{M} C{C} {family} px{px} pn{pn}", emu_norm(c, px, pn), c["ref"]).items():
            assert f <= 1.0, n
    for prec in (0, 1):
        c = BR.case_gelu(M, C, family, prec)
        for n, f in report(f"emulation gelu M{M} C{C} {family} prec{prec}", emu_gelu(c, prec), c["ref"]).items():
            assert f <= 1.0, n
    for px, pr in BR.TRIPLES_SR:
        c = BR.case_sr(M, C, family, px, pr)
        for n, f in report(f"emulation scale_residual M{M} C{C} {family} px{px} pr{pr}", emu_sr(c, px, pr), c["ref"]).items():
            assert f <= 1.0, n
    for px, pr, pn in BR.FUSED:
        c = BR.case_fused(M, C, family, px, pr, pn)
        for use1, usen in ((True, True), (True, False), (False, True)):
            got, x1 = emu_fused(c, px, pr, pn, use1=use1, usen=usen)
            for n, f in report(f"emulation fused M{M} C{C} {family} {px}{pr}{pn} dx1={use1} dn={usen}", got, fused_ref(c, px, pr, pn, x1, use1, usen)).items():
                assert f <= 1.0, n


def cancelling_columns(M=512, C=64):
    """dn = +1 on the first half of the rows, -1 on the second (plus noise): the slab partials of db are ~ +-7 and nearly cancel in the sum."""
    rng = np.random.default_rng(11)
    c = {k: v.copy() for k, v in BR.inputs(M, C, "random").items()}
    c["dn"] = (np.where(np.arange(M)[:, None] < M // 2, 1.0, -1.0) + 0.05 * rng.standard_normal((M, C))).astype(F32)
    return c


@pytest.mark.parametrize("family", BR.FAMILIES)
def test_injected_faults_land_outside_the_bounds(family):
    M, C = 33, 72
    # LayerNorm, in each dtype pair: the honest emulation is inside, the fault is outside in the named output
    for px, pn in BR.PAIRS_LN:
        c = BR.case_norm(M, C, family, px, pn)
        assert all(f <= 1.0 for f in report("honest", emu_norm(c, px, pn), c["ref"]).values())
        for fault, name in (("last chunk dropped from the statistics", "n"), ("mean(g xh) term missing", "dx"), ("a row past M counted in dw", "dw")):
            f = frac(emu_norm(c, px, pn, fault)[name], c["ref"][name])
            print(f"{fault}, {family} px{px} pn{pn}: {name} worst error / bound = {f:.2f}")
            assert f > 1.0, (fault, px, pn)
        # eps after the square root shows where eps counts: rows of spread 0.01 (var = 1e-4 beside eps = 1e-5)
        s = {k: to_storage(v, p) for k, v, p in (("x", 0.01 * BR.inputs(M, C, "random")["x"], px), ("w", c["w"], px), ("b", c["b"], px), ("dn", c["dn"], pn))}
        small = dict(s, ref=BR.layer_norm(s["x"], s["w"], s["b"], s["dn"], px, pn))
        assert all(f <= 1.0 for f in report("honest, spread 0.01", emu_norm(small, px, pn), small["ref"]).values())
        f = frac(emu_norm(small, px, pn, "eps after the square root")["n"], small["ref"]["n"])
        print(f"eps after the square root, spread 0.01 px{px} pn{pn}: n worst error / bound = {f:.2f}")
        assert f > 1.0, (px, pn)
    # a one-pass variance on the offset family (row mean 8, spread 1): the saved statistic is outside its bound at every width.  (n is held by the worst-case
    # bound of the MEAN, (C + 2) u mean |x| - eight times the spread here - which a one-pass variance's error stays below from a few chunks on: it is rstd, an
    # output of the forward that the GPU test checks, that catches it)
    if family == "offset":
        for Cw in (8, 72, 136):          # at C = 1024 the worst-case (C + 6) u allowance of the variance exceeds what a one-pass form loses at mean 8
            c = BR.case_norm(M, Cw, "offset", 0, 0)
            got = emu_norm(c, 0, 0, "one-pass variance")
            f = {n: frac(got[n], c["ref"][n]) for n in ("rstd", "n")}
            print(f"one-pass variance, offset C{Cw}: rstd {f['rstd']:.2f} n {f['n']:.2f} (worst error / bound)")
            assert f["rstd"] > 1.0, Cw
    # column partials rounded to fp16 before they are summed, where they nearly cancel (either storage type: the partials are fp32 in both)
    cc = cancelling_columns()
    for px in (0, 1):
        s = {k: to_storage(cc[k], px) for k in ("x", "w", "b", "dn")}
        ref = BR.layer_norm(s["x"], s["w"], s["b"], s["dn"], px, px)["db"]
        dn = s["dn"].astype(F32)
        parts = [dn[m0:m0 + 32].sum(0, dtype=F32) for m0 in range(0, dn.shape[0], 32)]
        honest = rounded(np.sum(parts, axis=0, dtype=F32), px)
        faulty = rounded(np.sum([to_storage(p, 1) for p in parts], axis=0), px)
        print(f"partials rounded to fp16, px{px}: honest {frac(honest, ref):.3f}, faulty {frac(faulty, ref):.2f} (worst error / bound)")
        assert inside(honest, ref) and frac(faulty, ref) > 1.0
    # GELU
    c = BR.case_gelu(M, C, family, 0)
    assert all(f <= 1.0 for f in report("honest gelu", emu_gelu(c, 0), c["ref"]).values())
    assert frac(emu_gelu(c, 0, "gelu_fast in place of erf")["y"], c["ref"]["y"]) > 1.0
    for prec in (0, 1):
        c = BR.case_gelu(M, C, family, prec)
        assert frac(emu_gelu(c, prec, "tanh derivative")["dx"], c["ref"]["dx"]) > 1.0, prec
    # scale_residual and the fused backward
    for px, pr in BR.TRIPLES_SR:
        c = BR.case_sr(M, C, family, px, pr)
        assert frac(emu_sr(c, px, pr, "gamma missing in dr")["dr"], c["ref"]["dr"]) > 1.0
    for px, pr, pn in BR.FUSED:
        c = BR.case_fused(M, C, family, px, pr, pn)
        got, x1 = emu_fused(c, px, pr, pn, "the fused backward drops dx1")
        ref = fused_ref(c, px, pr, pn, x1)
        assert frac(got["dx"], ref["dx"]) > 1.0 and frac(got["dr"], ref["dr"]) > 1.0 and frac(got["dgamma"], ref["dgamma"]) > 1.0, (px, pr, pn)



def test_the_sweep_is_the_one_the_kernels_ask_for():
    """The shapes tests/test_hip_block.py sweeps straddle the kernels' edges: four rows per workgroup, slabs of 32 rows, the slab-count cap with a tail, one
    chunk per lane of a wave and its neighbours, the widest built row."""
    assert BR.sweep_c(8) == (8, 504, 512, 520, 384, 1024)
    assert {1, 3, 4, 5, 31, 32, 33, 65} == set(BR.SWEEP_M) and BR.CAP_M == 16421 and BR.slab_rows(BR.CAP_M) == 64
    assert BR.slab_rows(32 * 512) == 32 and BR.slab_rows(32 * 512 + 1) == 64 and BR.CAP_M % 64 == 37
    assert (5, BR.MAX_C) in BR.sweep_shapes(8) and (BR.CAP_M, 8) in BR.sweep_shapes(8)
