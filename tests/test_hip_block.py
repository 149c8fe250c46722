"""GPU: LayerNorm, GELU, the LayerScale residual and the fused pair (moge_amd.block, csrc/block_grad.hip) against the float64 references of
tests/block_reference.py.

Gate: |got - ref| <= bound element by element, for every output of every operation in every built dtype combination; every output is filled with
NaN before the call and must come back finite.  Shapes are the kernels' own edges (four rows per workgroup, slabs of 32 rows, the slab-count cap, one
chunk per lane of a wave and its neighbours, the widest built row), not the workload: a cross of M and C, plus three slabs at C = 1032 and the cap at C = 1024.  Inputs are rounded to their storage types before the reference
runs, so the figures are the kernels' own error.  Every test prints its figures before it asserts.

Measured worst error / bound on an MI355X (DESIGN.md section 20 has the table per output and dtype combination): where fp32 sums decide - n, mean, rstd, dx
and the column sums of the fp32 instances - at most 0.34; every fp16 output 0.90-0.999 and the fp32 x1 / dr 0.995 / 0.9996, each a single rounding whose
bound is that rounding (the fp16 store's h |ref|, the one fma of x + r gamma, the one product of dr); GELU fp32 y 0.213, dx 0.307.  The whole block through
autograd: at most 6.3e-7 plain and 6.1e-4 under fp16 autocast, the same through torch.utils.checkpoint; stochastic depth 7.4e-7 and 7.3e-4."""
import copy

import numpy as np
import pytest
import torch
from torch import nn
from torch.nn import functional as F
from torch.utils.checkpoint import checkpoint

import block_reference as BR
from tests.test_hip_linear import StandInBlock
from tests.test_linear_module_cpu import model_of

pytestmark = pytest.mark.gpu

DT = {0: torch.float32, 1: torch.float16}
BAND = {False: 2e-5, True: 1e-2}           # the project's bands for the path through autograd: plain, fp16 autocast
EPS = BR.EPS


@pytest.fixture(scope="module")
def Blk():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from moge_amd import block
    return block


def dev(a, prec):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda", DT[prec])


def nan(*shape, prec):
    return torch.full(shape, float("nan"), dtype=DT[prec], device="cuda")


def host(t):
    return t.double().cpu().numpy()


def check(got, ref, what):
    frac = {}
    for n in got:
        g = host(got[n])
        assert np.isfinite(g).all(), (what, n)
        frac[n] = BR.fraction(g, ref[n])
    print(what, " ".join(f"{n}={f:.3f}" for n, f in frac.items()), "(worst error / bound)")
    for n, f in frac.items():
        assert f <= 1.0, (what, n, f)


def same_bits(a, b, names=None):
    return all(torch.equal(a[n], b[n]) for n in (names or a))


# ---- the operations through the low-level calls, into NaN-filled outputs (`o`: views to write instead) ------------------------------------------------
def run_norm(Blk, t, px, pn, o=None):
    M, C = t["x"].shape
    o = o or {"n": nan(M, C, prec=pn), "dx": nan(M, C, prec=px)}
    mr, dw, db = nan(M, 2, prec=0), nan(C, prec=px), nan(C, prec=px)
    assert Blk.norm_forward(t["x"], t["w"], t["b"], EPS, out=o["n"], mean_rstd=mr) is o["n"]
    Blk.norm_backward(t["x"], mr, t["w"], t["dn"], o["dx"], dw, db)
    return {"n": o["n"], "mean": mr[:, 0], "rstd": mr[:, 1], "dx": o["dx"], "dw": dw, "db": db}


def run_gelu(Blk, t, prec, o=None):
    M, C = t["x"].shape
    o = o or {"y": nan(M, C, prec=prec), "dx": nan(M, C, prec=prec)}
    assert Blk.gelu_forward(t["x"], out=o["y"]) is o["y"]
    assert Blk.gelu_backward(t["x"], t["dy"], dx=o["dx"]) is o["dx"]
    return {"y": o["y"], "dx": o["dx"]}


def run_sr(Blk, t, px, pr, o=None):
    M, C = t["x"].shape
    o = o or {"y": nan(M, C, prec=px), "dr": nan(M, C, prec=pr)}
    dg = nan(C, prec=px)
    assert Blk.scale_residual_forward(t["x"], t["r"], t["gamma"], out=o["y"]) is o["y"]
    Blk.scale_residual_backward(t["dx1"], t["r"], t["gamma"], o["dr"], dg)
    return {"y": o["y"], "dr": o["dr"], "dgamma": dg}


def run_fused(Blk, t, px, pr, pn, o=None, use1=True, usen=True):
    M, C = t["x"].shape
    o = o or {"x1": nan(M, C, prec=px), "n": nan(M, C, prec=pn), "dx": nan(M, C, prec=px), "dr": nan(M, C, prec=pr)}
    mr, dw, db, dg = nan(M, 2, prec=0), nan(C, prec=px), nan(C, prec=px), nan(C, prec=px)
    x1, n = Blk.norm_forward(t["x"], t["w"], t["b"], EPS, out=o["n"], mean_rstd=mr, r=t["r"], gamma=t["gamma"], x1=o["x1"])
    assert x1 is o["x1"] and n is o["n"]
    Blk.norm_backward(x1, mr, t["w"], t["dn"] if usen else None, o["dx"], dw, db, dx1=t["dx1"] if use1 else None, r=t["r"], gamma=t["gamma"], dr=o["dr"], dgamma=dg)
    return {"x1": x1, "n": n, "mean": mr[:, 0], "rstd": mr[:, 1], "dx": o["dx"], "dr": o["dr"], "dgamma": dg, "dw": dw, "db": db}


def fused_ref(c, got, px, pr, pn, use1=True, usen=True):
    """The LayerNorm part reads x1 as the kernel stored it (block_reference: "fused")."""
    return BR.fused(c["x"], c["r"], c["gamma"], c["w"], c["b"], c["dx1"] if use1 else None, c["dn"] if usen else None, px, pr, pn, x1=host(got["x1"]))


def tensors(c, precs):
    return {k: dev(c[k], p) for k, p in precs.items()}


def norm_t(c, px, pn):
    return tensors(c, {"x": px, "w": px, "b": px, "dn": pn})


def sr_t(c, px, pr):
    return tensors(c, {"x": px, "r": pr, "gamma": px, "dx1": px})


def fused_t(c, px, pr, pn):
    return tensors(c, {"x": px, "r": pr, "gamma": px, "w": px, "b": px, "dn": pn, "dx1": px})


def gelu_t(c, prec):
    return tensors(c, {"x": prec, "dy": prec})


def shape_id(s):
    return f"M{s[0]}-C{s[1]}"


# ---- the edge sweep --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", BR.sweep_shapes(8), ids=shape_id)
@pytest.mark.parametrize("px,pn", BR.PAIRS_LN)
def test_layer_norm_edges_against_float64(Blk, px, pn, shape):
    M, C = shape
    for family in BR.FAMILIES:
        c = BR.case_norm(M, C, family, px, pn)
        check(run_norm(Blk, norm_t(c, px, pn), px, pn), c["ref"], f"layer_norm M{M} C{C} {family} x{px} n{pn}")


@pytest.mark.parametrize("shape", BR.sweep_shapes(8), ids=shape_id)
@pytest.mark.parametrize("prec", [0, 1])
def test_gelu_edges_against_float64(Blk, prec, shape):
    M, C = shape
    for family in BR.FAMILIES:
        c = BR.case_gelu(M, C, family, prec)
        check(run_gelu(Blk, gelu_t(c, prec), prec), c["ref"], f"gelu M{M} C{C} {family} prec{prec}")


@pytest.mark.parametrize("shape", BR.sweep_shapes(8), ids=shape_id)
@pytest.mark.parametrize("px,pr", BR.TRIPLES_SR)
def test_scale_residual_edges_against_float64(Blk, px, pr, shape):
    M, C = shape
    for family in BR.FAMILIES:
        c = BR.case_sr(M, C, family, px, pr)
        check(run_sr(Blk, sr_t(c, px, pr), px, pr), c["ref"], f"scale_residual M{M} C{C} {family} x{px} r{pr}")


@pytest.mark.parametrize("shape", BR.sweep_shapes(8), ids=shape_id)
@pytest.mark.parametrize("px,pr,pn", BR.FUSED)
def test_fused_pair_edges_against_float64(Blk, px, pr, pn, shape):
    M, C = shape
    for family in BR.FAMILIES:
        c = BR.case_fused(M, C, family, px, pr, pn)
        got = run_fused(Blk, fused_t(c, px, pr, pn), px, pr, pn)
        check(got, fused_ref(c, got, px, pr, pn), f"fused M{M} C{C} {family} x{px} r{pr} n{pn}")


@pytest.mark.parametrize("px,pr,pn", BR.FUSED)
def test_wide_rows_over_several_slabs_against_float64(Blk, px, pr, pn):
    """More than one slab with the 32-elements-per-lane instances (C above 1024), which the sweep's cross of M and C does not reach: every operation, in
    the dtypes the triple has."""
    M, C = 2 * BR.SLAB + 1, 1032
    for family in BR.FAMILIES:
        c = BR.case_fused(M, C, family, px, pr, pn)
        got = run_fused(Blk, fused_t(c, px, pr, pn), px, pr, pn)
        check(got, fused_ref(c, got, px, pr, pn), f"fused M{M} C{C} {family} x{px} r{pr} n{pn}")
        c = BR.case_norm(M, C, family, px, pn)
        check(run_norm(Blk, norm_t(c, px, pn), px, pn), c["ref"], f"layer_norm M{M} C{C} {family} x{px} n{pn}")
        c = BR.case_sr(M, C, family, px, pr)
        check(run_sr(Blk, sr_t(c, px, pr), px, pr), c["ref"], f"scale_residual M{M} C{C} {family} x{px} r{pr}")


def test_the_slab_count_cap_at_the_vit_l_width_against_float64(Blk):
    """The slab-count cap (slabs of 64 rows, 257 of them, a tail of 37 rows) at C = 1024, the 16-elements-per-lane instances: once, the fused pair in the
    dtypes a block has under fp16 autocast - its backward is the one kernel that writes all three column sums.  The inputs are drawn here in float32 (the
    families of block_reference draw eight float64 arrays of this size); the reference is the same."""
    M, C, (px, pr, pn) = BR.CAP_M, 1024, (0, 1, 1)
    rng = np.random.default_rng(20)
    draw = lambda *shape: rng.standard_normal(shape, dtype=np.float32)          # noqa: E731
    raw = dict(x=draw(M, C), r=draw(M, C), gamma=0.25 + rng.random(C, dtype=np.float32), w=1 + 0.25 * draw(C), b=0.25 * draw(C), dn=draw(M, C) + np.float32(0.25),
               dx1=draw(M, C) + np.float32(0.25))
    c = {k: BR.to_storage(v, p).astype(np.float32) for (k, v), p in zip(raw.items(), (px, pr, px, px, px, pn, px))}
    got = run_fused(Blk, fused_t(c, px, pr, pn), px, pr, pn)
    check(got, fused_ref(c, got, px, pr, pn), f"fused M{M} C{C} x{px} r{pr} n{pn}")


@pytest.mark.parametrize("C", [4, 12, 508, 516, 2044])
def test_fp32_half_groups_against_float64(Blk, C):
    """A lane's group is 8 elements in every storage type; an all-fp32 call takes any multiple of 4, so its last group can be half: one 16-byte access of the
    two.  Half a group alone, behind one group, and as the 64th and 65th group of a row (the last lane, the first lane's second group), and of the widest row."""
    for M in (5, 33):
        for family in BR.FAMILIES:
            c = BR.case_norm(M, C, family, 0, 0)
            check(run_norm(Blk, norm_t(c, 0, 0), 0, 0), c["ref"], f"layer_norm M{M} C{C} {family} fp32")
            c = BR.case_fused(M, C, family, 0, 0, 0)
            got = run_fused(Blk, fused_t(c, 0, 0, 0), 0, 0, 0)
            check(got, fused_ref(c, got, 0, 0, 0), f"fused M{M} C{C} {family} fp32")
            c = BR.case_sr(M, C, family, 0, 0)
            check(run_sr(Blk, sr_t(c, 0, 0), 0, 0), c["ref"], f"scale_residual M{M} C{C} {family} fp32")
            c = BR.case_gelu(M, C, family, 0)
            check(run_gelu(Blk, gelu_t(c, 0), 0), c["ref"], f"gelu M{M} C{C} {family} fp32")


@pytest.mark.parametrize("px,pr,pn", BR.FUSED)
def test_a_missing_gradient_of_the_fused_pair_is_a_zero(Blk, px, pr, pn):
    """dx1 or dn absent: held to the same reference with a zero in its place; without dn the LayerNorm's parameters receive zeros."""
    M, C = 65, 136
    c = BR.case_fused(M, C, "offset", px, pr, pn)
    t = fused_t(c, px, pr, pn)
    for use1, usen in ((True, False), (False, True)):
        got = run_fused(Blk, t, px, pr, pn, use1=use1, usen=usen)
        check(got, fused_ref(c, got, px, pr, pn, use1, usen), f"fused M{M} C{C} x{px} r{pr} n{pn} dx1={use1} dn={usen}")
    assert not got["dw"].isnan().any()
    got = run_fused(Blk, t, px, pr, pn, use1=True, usen=False)
    assert torch.equal(got["dx"], t["dx1"]) and not got["dw"].any() and not got["db"].any()
    # the public function agrees: n unused, so its gradient is absent - x receives dx1 itself, the LayerNorm's parameters receive zeros, the rest keeps its bits
    leaves = {k: t[k].clone().requires_grad_(True) for k in ("x", "r", "gamma", "w", "b")}
    x1, _ = Blk.scale_residual_norm(*leaves.values(), EPS, out_dtype=None if pn == px else DT[pn])
    x1.backward(t["dx1"])
    assert torch.equal(leaves["x"].grad, t["dx1"]) and torch.equal(leaves["r"].grad, got["dr"]) and torch.equal(leaves["gamma"].grad, got["dgamma"])
    for k in ("w", "b"):
        assert leaves[k].grad is not None and leaves[k].grad.dtype == DT[px] and leaves[k].grad.shape == (C,) and not leaves[k].grad.any(), k


# ---- NaN padding ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("px,pr,pn", BR.FUSED)
def test_slices_of_nan_padded_allocations_give_the_same_bits(Blk, px, pr, pn):
    for M, C in [(33, 520), (5, 8)] + ([(5, 12)] if (px, pr, pn) == (0, 0, 0) else []):          # half a group exists in the all-fp32 instance only
        nan_padded(Blk, M, C, px, pr, pn)


def nan_padded(Blk, M, C, px, pr, pn):
    """x, r, the incoming gradients and every output as [:rows, :cols] slices of allocations with NaN rows and NaN chunks behind: nothing outside is
    read, nothing outside is written.  The fused pair in every dtype combination, and each operation alone in the dtypes the combination has."""
    bigs = []

    def padded(t):
        big = torch.full((t.shape[0] + 3, t.shape[1] + 16), float("nan"), dtype=t.dtype, device="cuda")
        view = big[:t.shape[0], :t.shape[1]]
        view.copy_(t)
        assert not view.is_contiguous()
        return view

    def outs(**precs):
        o = {}
        for n, p in precs.items():
            big = nan(M + 3, C + 16, prec=p)
            bigs.append((n, big))
            o[n] = big[:M, :C]
        return o

    def pad_in(t):
        return {k: padded(v) if v.dim() == 2 else v for k, v in t.items()}

    t = fused_t(BR.case_fused(M, C, "random", px, pr, pn), px, pr, pn)
    assert same_bits(run_fused(Blk, pad_in(t), px, pr, pn, outs(x1=px, n=pn, dx=px, dr=pr)), run_fused(Blk, t, px, pr, pn))
    t = norm_t(BR.case_norm(M, C, "random", px, pn), px, pn)
    assert same_bits(run_norm(Blk, pad_in(t), px, pn, outs(n=pn, dx=px)), run_norm(Blk, t, px, pn))
    t = sr_t(BR.case_sr(M, C, "random", px, pr), px, pr)
    assert same_bits(run_sr(Blk, pad_in(t), px, pr, outs(y=px, dr=pr)), run_sr(Blk, t, px, pr))
    t = gelu_t(BR.case_gelu(M, C, "random", pn), pn)
    assert same_bits(run_gelu(Blk, pad_in(t), pn, outs(y=pn, dx=pn)), run_gelu(Blk, t, pn))
    for n, big in bigs:                                      # the padding of the outputs is untouched
        assert torch.isnan(big[M:]).all() and torch.isnan(big[:, C:]).all() and not torch.isnan(big[:M, :C]).any(), n


# ---- bits -------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("px,pr,pn", BR.FUSED)
def test_deterministic_a_row_is_the_row_it_is_alone_and_the_fused_pair_is_the_two_calls(Blk, px, pr, pn):
    M, C = 2 * BR.SLAB + 1, 520
    t = fused_t(BR.case_fused(M, C, "offset", px, pr, pn), px, pr, pn)
    first = run_fused(Blk, t, px, pr, pn)
    assert same_bits(first, run_fused(Blk, t, px, pr, pn))
    row0 = {k: v[:1] if v.dim() == 2 else v for k, v in t.items()}
    alone = run_fused(Blk, row0, px, pr, pn)
    for n in ("x1", "n", "dx", "dr"):
        assert torch.equal(alone[n], first[n][:1]), n
    # the fused forward = scale_residual, then layer_norm of what it stored
    y = run_sr(Blk, t, px, pr)
    assert torch.equal(first["x1"], y["y"])
    ln = run_norm(Blk, dict(t, x=y["y"]), px, pn)
    assert same_bits(first, ln, ("n", "mean", "rstd"))
    # each operation alone: two calls, and row 0
    assert same_bits(ln, run_norm(Blk, dict(t, x=y["y"]), px, pn)) and same_bits(y, run_sr(Blk, t, px, pr))
    alone = run_norm(Blk, dict(row0, x=y["y"][:1]), px, pn)
    assert torch.equal(alone["n"], ln["n"][:1]) and torch.equal(alone["dx"], ln["dx"][:1])
    alone = run_sr(Blk, row0, px, pr)
    assert torch.equal(alone["y"], y["y"][:1]) and torch.equal(alone["dr"], y["dr"][:1])
    g = gelu_t(BR.case_gelu(M, C, "random", pn), pn)
    both = run_gelu(Blk, g, pn)
    assert same_bits(both, run_gelu(Blk, g, pn))
    alone = run_gelu(Blk, {k: v[:1] for k, v in g.items()}, pn)
    assert torch.equal(alone["y"], both["y"][:1]) and torch.equal(alone["dx"], both["dx"][:1])


def grads_of(fn, inputs, need, douts):
    """fn over clones of `inputs` (requires_grad as `need`), back-propagated from `douts` -> (outputs, grads)."""
    leaves = [t.clone().requires_grad_(n) for t, n in zip(inputs, need)]
    outs = fn(*leaves)
    outs = outs if isinstance(outs, tuple) else (outs,)
    torch.autograd.backward(outs, douts)
    return [o.detach() for o in outs], [leaf.grad for leaf in leaves]


@pytest.mark.parametrize("px,pr,pn", BR.FUSED)
def test_the_public_functions_equal_the_low_level_calls_and_skip_what_is_not_needed(Blk, px, pr, pn):
    M, C = 66, 136
    t = fused_t(BR.case_fused(M, C, "random", px, pr, pn), px, pr, pn)
    v = lambda a: a.view(2, 33, C)                           # noqa: E731
    od = None if pn == px else DT[pn]

    def sweep(fn, inputs, douts, base_outs, base_grads):
        outs, grads = grads_of(fn, inputs, [True] * len(inputs), douts)
        assert all(torch.equal(a.reshape(b.shape), b) for a, b in zip(outs, base_outs))
        assert all(torch.equal(a.reshape(b.shape), b) for a, b in zip(grads, base_grads))
        for skip in range(len(inputs) if len(inputs) > 1 else 0):       # each gradient skipped alone: it is None, the others keep their bits
            _, grads = grads_of(fn, inputs, [i != skip for i in range(len(inputs))], douts)
            assert grads[skip] is None
            assert all(torch.equal(a.reshape(b.shape), b) for i, (a, b) in enumerate(zip(grads, base_grads)) if i != skip), skip

    low = run_fused(Blk, t, px, pr, pn)
    sweep(lambda x, r, g, w, b: Blk.scale_residual_norm(v(x), v(r), g, w, b, EPS, out_dtype=od), [t[k] for k in ("x", "r", "gamma", "w", "b")], [v(t["dx1"]), v(t["dn"])],
          [low["x1"], low["n"]], [low[k] for k in ("dx", "dr", "dgamma", "dw", "db")])
    low = run_norm(Blk, t, px, pn)
    sweep(lambda x, w, b: Blk.layer_norm(v(x), (C,), w, b, EPS, out_dtype=od), [t[k] for k in ("x", "w", "b")], [v(t["dn"])], [low["n"]], [low[k] for k in ("dx", "dw", "db")])
    low = run_sr(Blk, t, px, pr)
    sweep(lambda x, r, g: Blk.scale_residual(v(x), v(r), g), [t[k] for k in ("x", "r", "gamma")], [v(t["dx1"])], [low["y"]], [t["dx1"], low["dr"], low["dgamma"]])
    g = gelu_t(BR.case_gelu(M, C, "random", pn), pn)
    low = run_gelu(Blk, g, pn)
    sweep(lambda x: Blk.gelu(v(x)), [g["x"]], [v(g["dy"])], [low["y"]], [low["dx"]])
    # nothing needs a gradient: nothing is saved, and the low-level calls that ask for no column sum need no workspace
    n = Blk.layer_norm(t["x"], (C,), t["w"], t["b"], EPS, out_dtype=od)
    assert not n.requires_grad and torch.equal(n, run_norm(Blk, t, px, pn)["n"])
    mr, dx = nan(M, 2, prec=0), nan(M, C, prec=px)
    Blk.norm_forward(t["x"], t["w"], t["b"], EPS, out_dtype=DT[pn], mean_rstd=mr)
    Blk.norm_backward(t["x"], mr, t["w"], t["dn"], dx)
    assert torch.equal(dx, run_norm(Blk, t, px, pn)["dx"])
    dr = nan(M, C, prec=pr)
    Blk.scale_residual_backward(t["dx1"], None, t["gamma"], dr=dr)
    assert torch.equal(dr, run_sr(Blk, t, px, pr)["dr"])


# ---- autocast ----------------------------------------------------------------------------------------------------------------------------------------
def test_autocast(Blk):
    torch.manual_seed(1)
    x = torch.randn(3, 11, 136, device="cuda", requires_grad=True)
    ln = Blk.wrap_layer_norm(nn.LayerNorm(136).cuda())
    ln16 = Blk.wrap_layer_norm(copy.deepcopy(ln), emit_autocast_dtype=True)
    with torch.autocast("cuda", dtype=torch.bfloat16):
        with pytest.raises(NotImplementedError, match="bfloat16"):
            ln(x)
        with pytest.raises(NotImplementedError, match="bfloat16"):
            Blk.scale_residual_norm(x, x, ln.weight, ln.weight, ln.bias)
    with torch.autocast("cuda", dtype=torch.float16):
        n32, n16 = ln(x), ln16(x)
        h = ln(x.half())                                       # an fp16 input goes to fp32 too, as with torch
    assert n32.dtype == torch.float32 and n16.dtype == torch.float16 and h.dtype == torch.float32
    assert torch.equal(n16, n32.half())                        # the fp32 result rounded once
    assert ln16(x).dtype == torch.float32                      # outside autocast the flag does nothing
    n16.backward(torch.ones_like(n16))
    assert x.grad.dtype == ln16.weight.grad.dtype == ln16.bias.grad.dtype == torch.float32       # fp32 tensors receive fp32 gradients
    want = F.layer_norm(x.detach(), (136,), ln.weight.detach(), ln.bias.detach(), ln.eps)
    assert float((n32.detach() - want).abs().max()) <= 1e-5 * float(want.abs().max())
    xg = x.detach().requires_grad_(True)                       # double backward is not built: once_differentiable refuses it
    for fn in (lambda a: ln(a), lambda a: Blk.gelu(a), lambda a: Blk.scale_residual(a, a, ln.weight.detach()),
               lambda a: Blk.scale_residual_norm(a, a, ln.weight.detach(), ln.weight.detach(), ln.bias.detach())[1]):
        y = fn(xg)
        (g,) = torch.autograd.grad(y, xg, grad_outputs=torch.ones_like(y).requires_grad_(True), create_graph=True)
        with pytest.raises(RuntimeError, match="once_differentiable"):
            g.sum().backward()


# ---- the whole block ----------------------------------------------------------------------------------------------------------------------------------
class DropPath(nn.Module):
    """dinov2/layers/drop_path.py: a per-sample mask, rescaled."""

    def __init__(self, p):
        super().__init__()
        self.p = p

    def forward(self, x):
        if self.p == 0.0 or not self.training:
            return x
        mask = x.new_empty(x.shape[0], *([1] * (x.dim() - 1))).bernoulli_(1 - self.p)
        return x * mask.div_(1 - self.p)


class DropBlock(StandInBlock):
    """The stand-in block with the stochastic-depth branch of dinov2/layers/block.py:107-109."""

    def __init__(self, ratio=0.0):
        super().__init__()
        self.sample_drop_ratio, self.drop_path1 = ratio, DropPath(ratio)

    def forward(self, x):
        if self.training and self.sample_drop_ratio > 0.0:
            x = x + self.drop_path1(self.ls1(self.attn(self.norm1(x))))
            return x + self.drop_path1(self.ls2(self.mlp(self.norm2(x))))
        return super().forward(x)


def make_block(ratio=0.0):
    torch.manual_seed(5)
    block = DropBlock(ratio)
    with torch.no_grad():
        for p in list(block.norm1.parameters()) + list(block.norm2.parameters()):
            p.add_(0.1 * torch.randn_like(p))
    return block, torch.randn(2, 65, 128), torch.randn(2, 65, 128)


def results(block, x, y):
    return {"y": y.detach(), "x": x.grad, **{n: p.grad for n, p in block.named_parameters()}}


def compare(got, want, band, what):
    assert set(got) == set(want) and len(want) == 2 + 14
    err = {n: float((got[n].double().cpu() - want[n].double().cpu()).abs().max() / want[n].double().abs().max()) for n in want}
    print(what, " ".join(f"{n}={e:.3e}" for n, e in err.items()))
    for n in want:
        assert got[n].dtype == torch.float32 and err[n] < band, (n, err[n])


@pytest.mark.parametrize("through_checkpoint", [False, True], ids=["plain", "checkpoint"])
@pytest.mark.parametrize("autocast", [False, True], ids=["fp32", "autocast-fp16"])
def test_a_whole_block_trains_a_step_through_this_library(Blk, autocast, through_checkpoint, monkeypatch):
    block, x, gy = make_block()
    ref_block = copy.deepcopy(block).double()
    xr = x.double().requires_grad_(True)
    yr = ref_block(xr)
    yr.backward(gy.double())
    want = results(ref_block, xr, yr)

    model = Blk.use_hip_encoder(model_of(block.cuda()))
    block = model.encoder.backbone.blocks[0]

    def refuse(*a, **k):
        raise AssertionError("torch's own linear / attention / layer_norm / gelu was called inside the block")

    for name in ("linear", "scaled_dot_product_attention", "layer_norm", "gelu"):
        monkeypatch.setattr(F, name, refuse)
    hooks = [m.register_forward_hook(refuse) for m in (block.ls1, block.ls2)]           # LayerScale is never called: its gamma is read by the fused kernels
    xg = x.cuda().requires_grad_(True)
    with torch.autocast("cuda", dtype=torch.float16, enabled=autocast):
        y = checkpoint(block, xg, use_reentrant=False) if through_checkpoint else block(xg)
    y.backward(gy.cuda().to(y.dtype))
    monkeypatch.undo()
    for h in hooks:
        h.remove()
    compare(results(block, xg, y), want, BAND[autocast], f"block autocast={autocast} checkpoint={through_checkpoint}")


@pytest.mark.parametrize("autocast", [False, True], ids=["fp32", "autocast-fp16"])
def test_stochastic_depth_takes_the_parent_forward_over_the_wrapped_pieces(Blk, autocast, monkeypatch):
    block, x, gy = make_block(0.05)
    block = block.cuda().train()
    ref_block = copy.deepcopy(block)

    def step(b, seed=11):
        torch.manual_seed(seed)
        xg = x.cuda().requires_grad_(True)
        with torch.autocast("cuda", dtype=torch.float16, enabled=autocast):
            y = b(xg)
        y.backward(gy.cuda().to(y.dtype))
        return results(b, xg, y)

    want = step(ref_block)
    Blk.use_hip_encoder(model_of(block))

    def refuse(*a, **k):
        raise AssertionError("torch's own linear / attention / layer_norm / gelu was called inside the block")

    for name in ("linear", "scaled_dot_product_attention", "layer_norm", "gelu"):
        monkeypatch.setattr(F, name, refuse)
    called = []
    hook = block.ls1.register_forward_hook(lambda *a: called.append(1))
    got = step(block)
    monkeypatch.undo()
    hook.remove()
    assert called                                              # the parent path: LayerScale itself ran
    compare(got, want, BAND[autocast], f"stochastic depth autocast={autocast}")
