"""CPU: the float64 references of tests/resblock_reference.py are the right ones (torch's float64 autograd of the block and of the single fused conv
with a residual), their bounds hold an honest fp32 emulation that sums in another order than the kernels, and each of a list of injected faults - what
the fused flavours of csrc/conv_grad.hip could get wrong - lands OUTSIDE a bound.  No GPU, no library."""
import numpy as np
import pytest
import torch
from torch.nn import functional as F

import conv_reference as VR
import resblock_reference as RR
from conv_reference import to_storage

PRECS = [0, 1]


def rounded(v, prec):
    return to_storage(np.asarray(v, dtype=np.float32), prec)


def inside(got, ref_bound):
    ref, bound = ref_bound
    return bool((np.abs(got - ref) <= bound).all())


def t64(a, grad=False):
    return torch.tensor(np.asarray(a, dtype=np.float64), dtype=torch.float64, requires_grad=grad)


def nchw(t):
    return t.permute(0, 3, 1, 2)


def conv(x, w, b):
    return F.conv2d(F.pad(x, (1, 1, 1, 1), mode="replicate"), w, b)


def close(ref, t, what):
    assert ref.shape == tuple(t.shape) and np.abs(ref - t.detach().numpy()).max() <= 1e-12 * max(1.0, np.abs(ref).max()), what


@pytest.mark.parametrize("H,W", VR.HW)
def test_references_agree_with_torch_float64_autograd(H, W):
    for Cin, Cout in VR.sweep_channels(0):
        c = RR.case(VR.SWEEP_B, H, W, Cin, Cout, "coded", 0)
        # the single fused conv with a residual; the addend of dx is the gradient of a second use of x, here (x * add).sum()
        x = nchw(t64(c["x"])).requires_grad_(True)
        w, b, res = t64(c["w"], True), t64(c["b"], True), nchw(t64(c["res"])).requires_grad_(True)
        y = conv(torch.relu(x), w, b) + res
        (y * nchw(t64(c["dy"]))).sum().add((x * nchw(t64(c["add"]))).sum()).backward()
        for name, t in (("y", y.permute(0, 2, 3, 1)), ("dx", x.grad.permute(0, 2, 3, 1)), ("dw", w.grad), ("db", b.grad)):
            close(c["ref"][name][0], t, (name, Cin, Cout))
            assert (c["ref"][name][1] > 0).all(), name
        close(c["dy"], res.grad.permute(0, 2, 3, 1), "the residual's gradient is dy itself")
        # the whole block: hidden width Cout, back to Cin
        rng = np.random.default_rng([H, W, Cin, Cout])
        w2v, b2v, gy = rng.standard_normal((Cin, Cout, 3, 3)) / np.sqrt(9 * Cout), rng.standard_normal(Cin), rng.standard_normal(c["x"].shape)
        x = nchw(t64(c["x"])).requires_grad_(True)
        w1, b1, w2, b2 = t64(c["w"], True), t64(c["b"], True), t64(w2v, True), t64(b2v, True)
        h = conv(torch.relu(x), w1, b1)
        y = x + conv(torch.relu(h), w2, b2)
        y.backward(nchw(t64(gy)))
        ref = RR.block(c["x"], c["w"], c["b"], w2v, b2v, gy)
        for name, t in (("h", h.permute(0, 2, 3, 1)), ("y", y.permute(0, 2, 3, 1)), ("dx", x.grad.permute(0, 2, 3, 1)), ("dw1", w1.grad), ("db1", b1.grad), ("dw2", w2.grad),
                        ("db2", b2.grad)):
            close(ref[name], t, ("block", name, Cin, Cout))
        # ... and the block is two fused convs chained: stage 2 on h with the residual x, stage 1 on x with the addend dy
        s2 = RR.relu_conv(ref["h"], w2v, b2v, gy, c["x"], None, 0)
        s1 = RR.relu_conv(c["x"], c["w"], c["b"], s2["dx"][0], None, gy, 0)
        for a, bb in ((s2["y"][0], ref["y"]), (s2["dx"][0], ref["dh"]), (s2["dw"][0], ref["dw2"]), (s1["dx"][0], ref["dx"]), (s1["dw"][0], ref["dw1"]), (s1["db"][0], ref["db1"])):
            assert np.abs(a - bb).max() <= 1e-12 * max(1.0, np.abs(bb).max())
    assert "db" not in RR.relu_conv(c["x"], c["w"], None, c["dy"], None, None, 0)


def test_relu_and_mask_are_defined_on_the_stored_value():
    for prec in PRECS:
        s = RR.SUBNORMAL[prec]
        v = np.array([0.0, -0.0, s, -s, 1.0, -1.0, np.nan, np.inf, -np.inf])
        assert to_storage(s, prec) == s and to_storage(s / 2, prec) == 0                 # the smallest subnormal of the storage type
        np.testing.assert_array_equal(RR.relu(v), [0, 0, s, 0, 1, 0, 0, np.inf, 0])    # a NaN gives 0: not torch.relu's NaN
        np.testing.assert_array_equal(RR.mask(v), [0, 0, 1, 0, 1, 0, 0, 1, 0])
        x = RR.case(VR.SWEEP_B, 16, 17, 72, 136, "random", prec)["x"]
        n = x.size
        zero, neg = (x == 0), np.signbit(x)
        assert abs((zero & ~neg).sum() / n - 0.125) < 0.01 and abs((zero & neg).sum() / n - 0.125) < 0.01 and abs((np.abs(x) == s).sum() / n - 0.0625) < 0.01
        assert (x == s).any() and (x == -s).any()


def emulate(c, prec, res, add, kt=24, splits=3):
    """fp32 arithmetic in another order than the kernels': taps outermost in reverse, channel tiles of `kt`, the input gradient as an fp32 scatter,
    the weight and bias gradients as `splits` fp32 partials, res / add added in fp32 behind the bias / the mask, one rounding at the end."""
    x, w, b, dy = (c[n].astype(np.float32) for n in ("x", "w", "b", "dy"))
    B, H, W, Cin = x.shape
    Cout = w.shape[0]
    rx = np.where(x > 0, x, np.float32(0))
    taps = [(s, t) for s in (1, 0, -1) for t in (1, 0, -1)]

    def tiled(a, bt):
        acc = np.zeros(a.shape[:-1] + (bt.shape[0],), dtype=np.float32)
        for k0 in range(0, a.shape[-1], kt):
            acc = acc + a[..., k0:k0 + kt] @ bt[:, k0:k0 + kt].T
        return acc

    y, dx = np.zeros((B, H, W, Cout), dtype=np.float32), np.zeros((B, H, W, Cin), dtype=np.float32)
    for s, t in taps:
        yy, xx = VR.clamped(H, s), VR.clamped(W, t)
        y = y + tiled(rx[:, yy][:, :, xx], w[:, :, s + 1, t + 1])
        np.add.at(dx, (slice(None), yy[:, None], xx[None, :]), tiled(dy, np.ascontiguousarray(w[:, :, s + 1, t + 1].T)))
    y = y + b
    dx = np.where(x > 0, dx, np.float32(0))
    if res is not None:
        y = y + res.astype(np.float32)
    if add is not None:
        dx = dx + add.astype(np.float32)
    rows = dy.reshape(B * H, W, Cout)
    edges = np.linspace(0, B * H, splits + 1).astype(int)
    dw, db = np.zeros((Cout, Cin, 3, 3), dtype=np.float32), np.zeros(Cout, dtype=np.float32)
    for s, t in taps:
        xg = rx[:, VR.clamped(H, s)][:, :, VR.clamped(W, t)].reshape(B * H, W, Cin)
        for r0, r1 in zip(edges[:-1], edges[1:]):
            dw[:, :, s + 1, t + 1] = dw[:, :, s + 1, t + 1] + np.einsum("rqo,rqi->oi", rows[r0:r1], xg[r0:r1]).astype(np.float32)
    for r0, r1 in zip(edges[:-1], edges[1:]):
        db = db + rows[r0:r1].sum((0, 1), dtype=np.float32)
    return {"y": rounded(y, prec), "dx": rounded(dx, prec), "dw": rounded(dw, prec), "db": rounded(db, prec)}


@pytest.mark.parametrize("prec", PRECS, ids=["fp32", "fp16"])
@pytest.mark.parametrize("H,W", VR.HW)
def test_an_honest_fp32_emulation_stays_inside_every_bound(H, W, prec):
    for Cin, Cout in VR.sweep_channels(prec):
        for family in VR.FAMILIES:
            c = RR.case(VR.SWEEP_B, H, W, Cin, Cout, family, prec)
            for ref, res, add in ((c["ref"], c["res"], c["add"]), (c["ref_plain"], None, None)):
                got = emulate(c, prec, res, add)
                for name in RR.NAMES:
                    frac = RR.worst(got[name], ref[name])
                    print(f"emulation {H}x{W} {Cin}->{Cout} {family} prec{prec} res/add={res is not None} {name}: worst error / bound = {frac:.3f}")
                    assert frac <= 1.0, (name, Cin, Cout, family)


@pytest.mark.parametrize("prec", PRECS, ids=["fp32", "fp16"])
@pytest.mark.parametrize("H,W", [(16, 17), (2, 2), (1, 17)])
def test_injected_faults_land_outside_the_bounds(H, W, prec):
    Cin = Cout = 72                                     # Cin = Cout: a mask taken from the output keeps its shape
    for family in ("random", "coded"):                  # not "offset": with every x positive or zero a missing ReLU changes nothing
        c = RR.case(VR.SWEEP_B, H, W, Cin, Cout, family, prec)
        x, w, dy, res, add = (c[n] for n in ("x", "w", "dy", "res", "add"))
        ref = c["ref"]
        good = {n: ref[n][0] for n in RR.NAMES}
        for name in RR.NAMES:                           # the exact value, rounded once, is inside: the faults below are what moves it out
            assert inside(rounded(good[name], prec), ref[name]), name
        g = ref["unmasked"]
        faults = {
            "the mask taken from relu(x) >= 0": ("dx", (RR.relu(x) >= 0) * g + add),
            "the mask taken from the output instead of the input": ("dx", (good["y"] > 0) * g + add),
            "the residual added twice": ("y", good["y"] + res),
            "the addend dropped": ("dx", good["dx"] - add),
            "ReLU missing in the wgrad": ("dw", RR.wgrad_core(dy, x)),
            "ReLU missing in the forward": ("y", good["y"] - RR.conv3x3_core(RR.relu(x), w) + RR.conv3x3_core(x, w)),
        }
        for what, (name, value) in faults.items():
            assert value.shape == good[name].shape, what
            assert not inside(rounded(value, prec), ref[name]), (what, family, H, W)


def test_a_multiplied_mask_turns_an_infinite_gradient_into_nan_where_the_select_gives_zero():
    x, g = np.array([-1.0, 0.0, 2.0]), np.array([np.inf, np.inf, 3.0])
    with np.errstate(invalid="ignore"):
        assert np.isnan(RR.mask(x) * g).sum() == 2
    np.testing.assert_array_equal(np.where(x > 0, g, 0.0), [0, 0, 3])
