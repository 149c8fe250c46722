"""GPU: the fused residual-block convs (moge_amd.resblock, the FUSE / RELU flavours of csrc/conv_grad.hip) against the float64 references of
tests/resblock_reference.py, and against the plain kernels of moge_amd.conv on the same device.

Gate: |got - ref| <= bound element by element, for y, dx, dw and db in both storage types, with and without res / add; every output is filled with NaN
before the call and must come back finite.  Shapes are conv_reference's borders and tile edges.  x carries +0, -0 and the smallest subnormals of the
storage type (resblock_reference.inputs).  Beside the bounds, every sweep case holds the fused flavours to the BITS of the plain kernels (torch.equal
compares as numbers, so -0 = +0): y without res is conv.forward(relu(x)), dw and db are conv.backward(relu(x))'s, dx without add is
where(x > 0, conv's dx, 0) - so a multiplied mask, a mask from another tensor or another accumulation order fails here.  Every test prints its figures
before it asserts.

The decoder level under fp16 autocast: the float64 copy with autocast points defines the computation (test_hip_conv.py), and for a fused block the
point behind the second conv lies BEHIND the skip add - y = fp16(x + conv2(..)) is rounded once, where torch's level rounds conv2's output and adds in
a second step.  Measured against torch's points, the fused points alone move this level's gradients by 1.2e-2 ... 5.2e-2 of their largest element
(float64 emulation on the CPU, seeds 5 - 8, whatever computes the convs): the two forms disagree on the sign of a handful of the 78336 block outputs
that are within an fp16 ulp of zero, and the next block's ReLU mask flips there.  So the autocast case is held, within the same band, to the same torch
level with the point moved behind the add; the plain fp32 case is held to the unmodified level.

Measured worst error / bound on an MI355X: see DESIGN.md section 24."""
import copy

import numpy as np
import pytest
import torch
from torch import nn
from torch.nn import functional as F

import conv_reference as VR
import resblock_reference as RR
from tests.test_conv_module_cpu import Checkpointed, conv
from tests.test_hip_conv import BAND, Fp16Point, with_autocast_points
from tests.test_linear_module_cpu import Block, model_of
from tests.test_resblock_module_cpu import ResBlockStandIn

pytestmark = pytest.mark.gpu

DTYPES = [torch.float32, torch.float16]
PREC = {torch.float32: 0, torch.float16: 1}
NP = {torch.float32: np.float32, torch.float16: np.float16}
NAMES = RR.NAMES


@pytest.fixture(scope="module")
def R():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from moge_amd import resblock
    return resblock


@pytest.fixture(scope="module")
def Cv():
    from moge_amd import conv
    return conv


def dev(a, dtype):
    """float64 values of the storage type -> a GPU tensor of it; converted on the host, so -0 and the subnormals arrive as they are."""
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a).astype(NP[dtype]))).cuda()


def gpu(c, dtype):
    return tuple(dev(c[n], dtype) for n in ("x", "w", "b", "dy", "res", "add"))


def nan(*shape, dtype):
    return torch.full(shape, float("nan"), dtype=dtype, device="cuda")


def run(R, x, w, b, dy, res=None, add=None, outs=None):
    """Forward and backward through the low-level calls into NaN-filled outputs (`outs`: views to write instead) -> {name: tensor}."""
    (B, H, W, Cin), Cout = x.shape, w.shape[0]
    o = outs or {"y": nan(B, H, W, Cout, dtype=x.dtype), "dx": nan(B, H, W, Cin, dtype=x.dtype), "dw": nan(Cout, Cin, 3, 3, dtype=x.dtype), "db": nan(Cout, dtype=x.dtype)}
    assert R.forward(x, w, b, res, out=o["y"]) is o["y"]
    R.backward(x, w, dy, add, o["dx"], o["dw"], o["db"])
    return o


def run_plain(Cv, x, w, b, dy):
    """The same through moge_amd.conv on torch.relu(x): the kernels the fused flavours are flavours of."""
    (B, H, W, Cin), Cout = x.shape, w.shape[0]
    rx = torch.relu(x)
    o = {"y": Cv.forward(rx, w, b), "dx": nan(B, H, W, Cin, dtype=x.dtype), "dw": nan(Cout, Cin, 3, 3, dtype=x.dtype), "db": nan(Cout, dtype=x.dtype)}
    Cv.backward(rx, w, dy, o["dx"], o["dw"], o["db"])
    return o


def check(got, ref, what, names=NAMES):
    frac = {}
    for n in names:
        g = got[n].double().cpu().numpy()
        assert g.shape == ref[n][0].shape and np.isfinite(g).all(), (what, n)
        frac[n] = RR.worst(g, ref[n])
    print(what, " ".join(f"{n}={f:.3f}" for n, f in frac.items()), "(worst error / bound)")
    for n in names:
        assert frac[n] <= 1.0, (what, n, frac[n])


def same_bits(a, b, names=NAMES):
    return all(torch.equal(a[n], b[n]) for n in names)


def held_to_the_plain_kernels(Cv, c, dtype, fused, plain_fused, what):
    """fused: with res / add; plain_fused: without.  The mask rule, and the bits of moge_conv3x3_* on relu(x)."""
    x, w, b, dy, res, add = gpu(c, dtype)
    plain = run_plain(Cv, x, w, b, dy)
    live = x > 0
    assert torch.equal(plain_fused["y"], plain["y"]), (what, "y without res is conv.forward(relu(x))")
    for got in (fused, plain_fused):
        assert torch.equal(got["dw"], plain["dw"]) and torch.equal(got["db"], plain["db"]), (what, "dw, db are conv.backward(relu(x))'s")
    assert torch.equal(plain_fused["dx"], torch.where(live, plain["dx"], torch.zeros_like(plain["dx"]))), (what, "dx without add is where(x > 0, conv's dx, 0)")
    assert not plain_fused["dx"][~live].any(), (what, "dx is exactly 0 where x <= 0")
    assert torch.equal(fused["dx"][~live], add[~live]), (what, "dx is the addend where x <= 0")
    sub = x == RR.SUBNORMAL[PREC[dtype]]                 # the positive subnormals: mask 1, the unmasked gradient passes
    assert torch.equal(plain_fused["dx"][sub], plain["dx"][sub]), (what, "the mask of a positive subnormal is 1")
    return int(sub.sum()), int((~live).sum())


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "fp16"])
@pytest.mark.parametrize("ch", range(4))
@pytest.mark.parametrize("H,W", VR.HW)
def test_borders_and_tile_edges_against_float64_and_the_plain_kernels(R, Cv, H, W, ch, dtype):
    Cin, Cout = VR.sweep_channels(PREC[dtype])[ch]
    subs = 0
    for family in VR.FAMILIES:
        c = RR.case(VR.SWEEP_B, H, W, Cin, Cout, family, PREC[dtype])
        x, w, b, dy, res, add = gpu(c, dtype)
        what = f"edges {H}x{W} {Cin}->{Cout} {family} {dtype}"
        fused, plain_fused = run(R, x, w, b, dy, res, add), run(R, x, w, b, dy)
        check(fused, c["ref"], what + " res/add")
        check(plain_fused, c["ref_plain"], what)
        subs += held_to_the_plain_kernels(Cv, c, dtype, fused, plain_fused, what)[0]
    assert subs > 0 or VR.SWEEP_B * H * W * Cin <= 64          # the family put positive subnormals under the mask (all but the smallest cases)


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "fp16"])
def test_an_infinite_gradient_under_masked_elements_gives_zero(R, dtype):
    """dy = inf at one (pixel, channel); every x of the 3 x 3 pixels it reaches is <= 0.  The sums there are inf or NaN (inf times a weight of either
    sign); the select turns them into 0 - a multiplied mask would store NaN.  dx only: dw = wgrad(relu(x), dy) is inf . 0 by definition."""
    B, H, W, Cin, Cout = VR.SWEEP_B, 16, 17, 72, 136
    c = RR.case(B, H, W, Cin, Cout, "random", PREC[dtype])
    x, w, b, dy, res, add = gpu(c, dtype)
    x, dy = x.clone(), dy.clone()
    x[1, 6:9, 3:6] = -x[1, 6:9, 3:6].abs()
    dy[1, 7, 4, 5] = float("inf")
    hit = torch.zeros(B, H, W, dtype=torch.bool, device="cuda")
    hit[1, 6:9, 3:6] = True
    clean = dy.clone()
    clean[1, 7, 4, 5] = 0
    for addend in (None, add):
        dx, want = nan(B, H, W, Cin, dtype=dtype), nan(B, H, W, Cin, dtype=dtype)
        R.backward(x, w, dy, addend, dx=dx)
        R.backward(x, w, clean, addend, dx=want)
        assert not torch.isnan(dx).any() and torch.isfinite(dx).all()
        assert torch.equal(dx[hit], torch.zeros_like(dx[hit]) if addend is None else addend[hit])
        assert torch.equal(dx[~hit], want[~hit])             # the other pixels never saw it


def block_inputs(B, H, W, C, Ch, prec, seed=11):
    rng = np.random.default_rng([seed, B, H, W, C, Ch])
    x = RR.special_x(RR.to_storage(rng.standard_normal((B, H, W, C)), prec), prec, [seed + 1, B, H, W, C, Ch])
    w1, w2 = rng.standard_normal((Ch, C, 3, 3)) / np.sqrt(9 * C), rng.standard_normal((C, Ch, 3, 3)) / np.sqrt(9 * Ch)
    b1, b2, dy = rng.standard_normal(Ch), rng.standard_normal(C), rng.standard_normal((B, H, W, C))
    return (x,) + tuple(RR.to_storage(t, prec) for t in (w1, b1, w2, b2, dy))


def chained(R, x, w1, b1, w2, b2, dy):
    """The block as two chained pairs of low-level calls -> {h, y, dh, dx, dw1, db1, dw2, db2}."""
    (B, H, W, C), Ch = x.shape, w1.shape[0]
    o = {"h": R.forward(x, w1, b1), "dh": nan(B, H, W, Ch, dtype=x.dtype), "dw2": nan(C, Ch, 3, 3, dtype=x.dtype), "db2": nan(C, dtype=x.dtype),
         "dx": nan(B, H, W, C, dtype=x.dtype), "dw1": nan(Ch, C, 3, 3, dtype=x.dtype), "db1": nan(Ch, dtype=x.dtype)}
    o["y"] = R.forward(o["h"], w2, b2, x)
    R.backward(o["h"], w2, dy, None, o["dh"], o["dw2"], o["db2"])
    R.backward(x, w1, o["dh"], dy, o["dx"], o["dw1"], o["db1"])
    return o


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "fp16"])
@pytest.mark.parametrize("C,Ch", [(64, 64), (72, 136)], ids=["64-64-64", "72-136-72"])
def test_the_block_is_the_two_chained_calls_and_each_stage_is_inside_its_bounds(R, C, Ch, dtype):
    B, H, W, prec = VR.SWEEP_B, 16, 17, PREC[dtype]
    host = block_inputs(B, H, W, C, Ch, prec)
    x, w1, b1, w2, b2, dy = (dev(t, dtype) for t in host)
    low = chained(R, x, w1, b1, w2, b2, dy)
    xg = x.permute(0, 3, 1, 2).clone(memory_format=torch.preserve_format).requires_grad_(True)
    params = [t.clone().requires_grad_(True) for t in (w1, b1, w2, b2)]
    y = R.residual_conv_block(xg, *params)
    assert y.shape == (B, C, H, W) and y.dtype == dtype and y.is_contiguous(memory_format=torch.channels_last)
    y.backward(dy.permute(0, 3, 1, 2))
    got = {"y": y.detach().permute(0, 2, 3, 1), "dx": xg.grad.permute(0, 2, 3, 1), "dw1": params[0].grad, "db1": params[1].grad, "dw2": params[2].grad, "db2": params[3].grad}
    assert same_bits(got, low, list(got))
    # against float64, each stage on the device's own stored h and dh, so the per-stage bounds apply unchanged
    hx, hw1, hb1, hw2, hb2, hdy = host
    h64, dh64 = low["h"].double().cpu().numpy(), low["dh"].double().cpu().numpy()
    s2 = RR.relu_conv(h64, hw2, hb2, hdy, hx, None, prec)
    s1 = RR.relu_conv(hx, hw1, hb1, dh64, None, hdy, prec)
    check({"y": low["y"], "dx": low["dh"], "dw": low["dw2"], "db": low["db2"]}, s2, f"block {C}-{Ch}-{C} {dtype} stage 2 (y, dh, dw2, db2)")
    check({"y": low["h"], "dx": low["dx"], "dw": low["dw1"], "db": low["db1"]}, s1, f"block {C}-{Ch}-{C} {dtype} stage 1 (h, dx, dw1, db1)")
    # only the gradients that are needed: the input frozen, then the first conv frozen as well
    params = [t.clone().requires_grad_(n) for t, n in zip((w1, b1, w2, b2), (True, True, True, True))]
    y = R.residual_conv_block(x.permute(0, 3, 1, 2), *params)
    y.backward(dy.permute(0, 3, 1, 2))
    assert same_bits({"dw1": params[0].grad, "db1": params[1].grad, "dw2": params[2].grad, "db2": params[3].grad}, low, ["dw1", "db1", "dw2", "db2"])
    params = [t.clone().requires_grad_(n) for t, n in zip((w1, b1, w2, b2), (False, False, True, False))]
    y = R.residual_conv_block(x.permute(0, 3, 1, 2), *params)
    y.backward(dy.permute(0, 3, 1, 2))
    assert torch.equal(params[2].grad, low["dw2"]) and all(p.grad is None for i, p in enumerate(params) if i != 2)
    assert not R.residual_conv_block(x.permute(0, 3, 1, 2), w1, b1, w2, b2).requires_grad
    assert torch.equal(R.residual_conv_block(x.permute(0, 3, 1, 2), w1, None, w2, None).permute(0, 2, 3, 1), R.forward(R.forward(x, w1), w2, None, x))      # no biases


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "fp16"])
@pytest.mark.parametrize("H,W,Cin,Cout", [(16, 17, 72, 136), (2, 2, 136, 72), (33, 18, 32, 64)])
def test_slices_of_nan_padded_allocations_give_the_same_bits(R, H, W, Cin, Cout, dtype):
    """x, res, dy, add and the outputs y, dx as slices of allocations with a NaN image before and after and NaN columns behind every pixel: nothing
    outside is read, nothing outside is written."""
    B = VR.SWEEP_B
    c = RR.case(B, H, W, Cin, Cout, "random", PREC[dtype])
    x, w, b, dy, res, add = gpu(c, dtype)
    base = run(R, x, w, b, dy, res, add)
    pad = 2 * VR.CR.chunk(PREC[dtype])

    def padded(t=None, shape=None):
        shape = shape or t.shape
        big = nan(shape[0] + 2, shape[1], shape[2], shape[3] + pad, dtype=dtype)
        view = big[1:-1, :, :, :shape[3]]
        if t is not None:
            view.copy_(t)
        return big, view

    bigs = {"y": padded(shape=(B, H, W, Cout)), "dx": padded(shape=(B, H, W, Cin))}
    outs = {"y": bigs["y"][1], "dx": bigs["dx"][1], "dw": nan(Cout, Cin, 3, 3, dtype=dtype), "db": nan(Cout, dtype=dtype)}
    xs, dys, ress, adds = (padded(t)[1] for t in (x, dy, res, add))
    assert not ress.is_contiguous() and R._in_place(ress) is ress and R._ld(ress) == Cout + pad and R._ld(adds) == Cin + pad
    got = run(R, xs, w, b, dys, ress, adds, outs)
    assert same_bits(got, base)
    for n in ("y", "dx"):                               # the padding of the outputs is untouched
        big = bigs[n][0]
        assert torch.isnan(big[0]).all() and torch.isnan(big[-1]).all() and torch.isnan(big[..., outs[n].shape[3]:]).all(), n


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "fp16"])
def test_the_split_weight_gradient_sees_relu_on_load_in_a_ragged_last_part(R, Cv, dtype):
    B, H, W, Cin, Cout = VR.SPLIT
    assert R.workspace_bytes(B, H, W, Cin, Cout, dtype) == Cv.workspace_bytes(B, H, W, Cin, Cout, dtype) == VR.expected_workspace(B, H, W, Cin, Cout, PREC[dtype])
    assert VR.expected_split(B * H * W, Cin, Cout, PREC[dtype]) > 1
    c = RR.case(B, H, W, Cin, Cout, "random", PREC[dtype])
    x, w, b, dy, res, add = gpu(c, dtype)
    fused, plain_fused = run(R, x, w, b, dy, res, add), run(R, x, w, b, dy)
    check(fused, c["ref"], f"split {B}x{H}x{W} {Cin}->{Cout} {dtype} res/add")
    held_to_the_plain_kernels(Cv, c, dtype, fused, plain_fused, "split")
    assert same_bits(fused, run(R, x, w, b, dy, res, add))          # ... and deterministic with the split


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "fp16"])
def test_deterministic_and_an_image_is_the_image_it_is_alone(R, dtype):
    B, H, W, C, Ch = VR.SWEEP_B, 16, 17, 72, 136
    x, w1, b1, w2, b2, dy = (dev(t, dtype) for t in block_inputs(B, H, W, C, Ch, PREC[dtype]))
    first, second = chained(R, x, w1, b1, w2, b2, dy), chained(R, x, w1, b1, w2, b2, dy)
    assert same_bits(first, second, list(first))
    for i in range(B):
        alone = chained(R, x[i:i + 1], w1, b1, w2, b2, dy[i:i + 1])
        assert all(torch.equal(alone[n], first[n][i:i + 1]) for n in ("h", "y", "dh", "dx")), i


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "fp16"])
@pytest.mark.parametrize("layout", ["nchw", "channels_last"])
def test_the_public_function_equals_the_low_level_calls_and_skips_what_is_not_needed(R, layout, dtype, monkeypatch):
    B, H, W, Cin, Cout = VR.SWEEP_B, 16, 17, 72, 136
    c = RR.case(B, H, W, Cin, Cout, "random", PREC[dtype])
    x, w, b, dy, res, add = gpu(c, dtype)
    base = run(R, x, w, b, dy, res)

    def arrange(t):                                     # (B, H, W, C) values as a (B, C, H, W) tensor of the layout
        t = t.permute(0, 3, 1, 2)
        return t.contiguous() if layout == "nchw" else t.contiguous(memory_format=torch.channels_last)

    calls = []
    low_backward = R.backward
    monkeypatch.setattr(R, "backward", lambda x, w, dy, add=None, dx=None, dw=None, db=None: (calls.append((x is not None, dx is not None, dw is not None, db is not None)),
                                                                                                 low_backward(x, w, dy, add, dx, dw, db))[1])

    def through_autograd(need):
        xl, wl, bl, rl = (t.clone(memory_format=torch.preserve_format).requires_grad_(n) for t, n in zip((arrange(x), w, b, arrange(res)), need))
        y = R.relu_conv3x3(xl, wl, bl, rl)
        assert y.shape == (B, Cout, H, W) and y.dtype == dtype and y.is_contiguous(memory_format=torch.channels_last)
        assert y.requires_grad == any(need)
        saved = y.grad_fn.saved_tensors if any(need) else (None, None)
        assert (saved[0] is not None) == (need[0] or need[1]) and (saved[1] is not None) == need[0]          # x for dx or dw, the weight for dx
        if any(need):
            y.backward(arrange(dy))
        return {"y": y.detach().permute(0, 2, 3, 1), "dx": xl.grad if xl.grad is None else xl.grad.permute(0, 2, 3, 1), "dw": wl.grad, "db": bl.grad,
                "dres": rl.grad if rl.grad is None else rl.grad.permute(0, 2, 3, 1)}

    got = through_autograd((True, True, True, True))
    assert same_bits(got, base) and torch.equal(got["dres"], dy)          # the residual's gradient is dy itself
    assert calls == [(True, True, True, True)]
    for skip in range(3):                               # each gradient skipped alone: it is None, the others keep their bits, its launch is not asked for
        need = tuple(i != skip for i in range(3)) + (False,)
        del calls[:]
        got = through_autograd(need)
        assert got[NAMES[1 + skip]] is None and got["dres"] is None
        assert same_bits(got, base, [n for i, n in enumerate(NAMES) if i != 1 + skip])
        assert calls == [(True,) + need[:3]], calls     # frozen weights: no dw is asked for, so no wgrad launch
    del calls[:]
    got = through_autograd((False, False, True, False))  # the bias alone: x is not saved
    assert torch.equal(got["db"], base["db"]) and calls == [(False, False, False, True)]
    del calls[:]
    got = through_autograd((False, False, False, True))  # the residual alone: no launch at all
    assert torch.equal(got["dres"], dy) and calls == []
    monkeypatch.undo()
    y = R.relu_conv3x3(arrange(x), w)                   # no bias, no residual, no gradient
    assert not y.requires_grad and torch.equal(y.permute(0, 2, 3, 1), R.forward(x, w))
    if layout == "channels_last":                       # a channel slice of a channels_last tensor is read through its pixel stride, the residual too
        wide = torch.cat([arrange(x), arrange(x)], 1).contiguous(memory_format=torch.channels_last)
        rwide = torch.cat([arrange(res), arrange(res)], 1).contiguous(memory_format=torch.channels_last)
        assert torch.equal(R.relu_conv3x3(wide[:, Cin:], w, b, rwide[:, Cout:]).permute(0, 2, 3, 1), base["y"])
    we, be = w.clone().requires_grad_(True), b.clone().requires_grad_(True)          # B = 0: nothing is launched, the parameter gradients are zero
    e = R.relu_conv3x3(arrange(x)[:0], we, be, arrange(res)[:0])
    assert e.shape == (0, Cout, H, W)
    e.sum().backward()
    assert we.grad.shape == w.shape and be.grad.shape == b.shape and not we.grad.any() and not be.grad.any()
    with pytest.raises(ValueError, match="residual must be"):
        R.relu_conv3x3(arrange(x), w, b, arrange(add))


def test_autocast(R):
    x = torch.randn(2, 32, 9, 10, device="cuda", requires_grad=True)
    m = R.wrap_res_block(ResBlockStandIn(32, hidden=40).cuda())
    with torch.autocast("cuda", dtype=torch.bfloat16):
        with pytest.raises(NotImplementedError, match="moge_amd.resblock.*bfloat16"):
            m(x)
    with torch.autocast("cuda", dtype=torch.float16):
        y = m(x)
    assert y.dtype == torch.float16 and y.shape == (2, 32, 9, 10)
    y.backward(torch.ones_like(y))
    assert x.grad.dtype == torch.float32 and all(p.grad.dtype == torch.float32 for p in m.parameters())      # fp32 tensors receive fp32 gradients through the cast
    c1, c2 = m.layers[2], m.layers[5]
    pad = lambda t: F.pad(t, (1, 1, 1, 1), mode="replicate")          # noqa: E731
    h = F.conv2d(pad(torch.relu(x.detach().half())), c1.weight.detach().half(), c1.bias.detach().half())
    want = x.detach().half().float() + F.conv2d(pad(torch.relu(h)), c2.weight.detach().half(), c2.bias.detach().half()).float()
    assert float((y.detach().float() - want).abs().max()) <= 2.0 ** -8 * float(want.abs().max())
    xg = x.detach().requires_grad_(True)                 # double backward is not built: once_differentiable refuses it
    yg = m(xg)
    (g,) = torch.autograd.grad(yg, xg, grad_outputs=torch.ones_like(yg).requires_grad_(True), create_graph=True)
    with pytest.raises(RuntimeError, match="once_differentiable"):
        g.sum().backward()


# ---- through autograd: a decoder level -----------------------------------------------------------------------------------------------------
def decoder_level():
    """A decoder level without norms: ConvTranspose2d(2, 2), a pair of residual blocks, a 1x1."""
    torch.manual_seed(5)
    return nn.Sequential(nn.ConvTranspose2d(64, 32, 2, 2), ResBlockStandIn(32), ResBlockStandIn(32), conv(32, 32, 1))


def hip_model(level):
    model = model_of(Block())
    model.neck = level
    return model


def with_fused_points(module):
    """with_autocast_points, with the point behind a block's second conv moved behind the skip add (the module's text)."""
    P = Fp16Point.apply
    with_autocast_points(module)
    for m in module.modules():
        if isinstance(m, nn.ConvTranspose2d):
            m.forward = lambda t, m=m: P(F.conv_transpose2d(P(t), P(m.weight), P(m.bias), m.stride))
        elif isinstance(m, ResBlockStandIn):
            c1, c2 = m.layers[2], m.layers[5]
            m.forward = lambda t, c1=c1, c2=c2: P(P(t) + c2._conv_forward(P(torch.relu(c1(torch.relu(P(t))))), P(c2.weight), P(c2.bias)))
    return module


def torch_points(module):
    """torch's own rounding points: every conv and transposed conv, the skip add outside."""
    P = Fp16Point.apply
    with_autocast_points(module)
    for m in module.modules():
        if isinstance(m, nn.ConvTranspose2d):
            m.forward = lambda t, m=m: P(F.conv_transpose2d(P(t), P(m.weight), P(m.bias), m.stride))
    return module


def refusing(name):
    def refuse(*a, **k):
        raise AssertionError(f"torch's own {name} was called inside the level")
    return refuse


def step(level, x, gy, points=None):
    ref_level = copy.deepcopy(level).double()
    if points:
        points(ref_level)
    xr = x.double().requires_grad_(True)
    yr = ref_level(xr)
    yr.backward(gy.double())
    return {"y": yr.detach(), "x": xr.grad, **{n: p.grad for n, p in ref_level.named_parameters()}}


@pytest.mark.parametrize("autocast", [False, True], ids=["fp32", "autocast-fp16"])
def test_a_decoder_level_trains_a_step_through_this_library(R, autocast, monkeypatch):
    from moge_amd.convt import use_hip_decoder
    level = decoder_level()
    x, gy = torch.randn(2, 64, 17, 18), torch.randn(2, 32, 34, 36)
    want = step(level, x, gy, with_fused_points if autocast else None)
    torchs = step(level, x, gy, torch_points) if autocast else want

    model = R.use_hip_res_blocks(use_hip_decoder(hip_model(level.cuda())))
    assert sum(getattr(type(m), R.FLAG, False) for m in model.neck.modules()) == 2
    for name in ("conv2d", "conv_transpose2d", "relu"):  # nothing of the level is torch's: no conv, and no ReLU either
        monkeypatch.setattr(F, name, refusing(name))
    xg = x.cuda().requires_grad_(True)
    with torch.autocast("cuda", dtype=torch.float16, enabled=autocast):
        y = model.neck(xg)
    y.backward(gy.cuda().to(y.dtype))
    monkeypatch.undo()
    got = {"y": y.detach(), "x": xg.grad, **{n: p.grad for n, p in model.neck.named_parameters()}}
    assert set(got) == set(want) and len(want) == 2 + 12
    err = {n: float((got[n].double().cpu() - want[n]).abs().max() / want[n].abs().max()) for n in want}
    print(f"decoder level autocast={autocast}", " ".join(f"{n}={e:.3e}" for n, e in err.items()))
    if autocast:
        print("  ... against torch's rounding points (not asserted: the module's text):",
              " ".join(f"{n}={float((got[n].double().cpu() - torchs[n]).abs().max() / torchs[n].abs().max()):.3e}" for n in torchs))
    for n in want:
        assert got[n].dtype == (torch.float16 if autocast and n == "y" else torch.float32) and got[n].shape == want[n].shape and err[n] < BAND[autocast], (n, err[n])


def test_the_level_under_checkpointing_gives_the_same_bits(R):
    from moge_amd.convt import use_hip_decoder
    plain = R.use_hip_res_blocks(use_hip_decoder(hip_model(decoder_level().cuda())))
    wrapped = use_hip_decoder(R.use_hip_res_blocks(hip_model(Checkpointed(decoder_level().cuda()))))          # the other order, through the wrapper
    assert sum(getattr(type(m), R.FLAG, False) for m in wrapped.neck.modules()) == 2
    x, gy = torch.randn(2, 64, 17, 18, device="cuda"), torch.randn(2, 32, 34, 36, device="cuda")
    got = []
    for model in (plain, wrapped):
        xg = x.clone().requires_grad_(True)
        y = model.neck(xg)
        y.backward(gy)
        got.append([y.detach(), xg.grad] + [p.grad for p in model.neck.parameters()])
    assert len(got[0]) == len(got[1]) == 2 + 12 and all(torch.equal(a, b) for a, b in zip(*got))
