"""GPU: the trainable 3x3 convolution (moge_amd.conv, csrc/conv_grad.hip) against the float64 references of tests/conv_reference.py.

Gate: |got - ref| <= bound element by element, for y, dx, dw and db in both storage types; every output is filled with NaN before the call and must
come back finite.  Shapes are the borders and the tile edges (one pixel, one row, one column, 2 x 2; 128 flat pixels and 128 channels per workgroup, K
tiles of 64 fp16 / 32 fp32 elements), not the workload; (1, 96, 128, 64, 64) and a shape at which the weight gradient splits the pixels run once
each.  Inputs are rounded to the storage type before the reference runs, so the figures are the kernels' own error.  Every test prints its figures
before it asserts.

Measured worst error / bound on an MI355X: fp32 y 0.087, dx 0.094, dw 0.432, db 0.264 at the edges (dw and db at the sums of
2 terms of the one-pixel image) and at most 0.009 at the larger shapes; fp16 y 0.972, dx 0.965, dw 0.995, db 0.995 at the edges and y 0.774, dx 0.755, dw 0.157,
db 0.065 at the larger shapes - the fp16 bound is dominated by the store's h |ref| with h the unit roundoff, which one correct rounding of a value
just above a power of two uses up, so a fraction close to 1 is the store, not the sum.  The decoder level through autograd: at most 6.5e-7 plain and
5.3e-4 under fp16 autocast."""
import copy

import numpy as np
import pytest
import torch
from torch import nn
from torch.nn import functional as F

import conv_reference as VR
from tests.test_conv_module_cpu import Checkpointed, ResidualStandIn
from tests.test_linear_module_cpu import Block, model_of

pytestmark = pytest.mark.gpu

DTYPES = [torch.float32, torch.float16]
PREC = {torch.float32: 0, torch.float16: 1}
NAMES = ("y", "dx", "dw", "db")
BAND = {False: 2e-5, True: 1e-2}           # the project's bands for the path through autograd: plain, fp16 autocast


@pytest.fixture(scope="module")
def Cv():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from moge_amd import conv
    return conv


def gpu(c, dtype):
    return tuple(torch.from_numpy(c[n]).to("cuda", dtype) for n in ("x", "w", "b", "dy"))


def nan(*shape, dtype):
    return torch.full(shape, float("nan"), dtype=dtype, device="cuda")


def run(Cv, x, w, b, dy, outs=None):
    """Forward and backward through the low-level calls into NaN-filled outputs (`outs`: views to write instead) -> {name: tensor}."""
    (B, H, W, Cin), Cout = x.shape, w.shape[0]
    o = outs or {"y": nan(B, H, W, Cout, dtype=x.dtype), "dx": nan(B, H, W, Cin, dtype=x.dtype), "dw": nan(Cout, Cin, 3, 3, dtype=x.dtype), "db": nan(Cout, dtype=x.dtype)}
    assert Cv.forward(x, w, b, out=o["y"]) is o["y"]
    Cv.backward(x, w, dy, o["dx"], o["dw"], o["db"])
    return o


def check(got, ref, what):
    frac = {}
    for n in NAMES:
        r, bound = ref[n]
        g = got[n].double().cpu().numpy()
        assert g.shape == r.shape and np.isfinite(g).all(), (what, n)
        frac[n] = float((np.abs(g - r) / bound).max())
    print(what, " ".join(f"{n}={f:.3f}" for n, f in frac.items()), "(worst error / bound)")
    for n in NAMES:
        assert frac[n] <= 1.0, (what, n, frac[n])


def same_bits(a, b, names=NAMES):
    return all(torch.equal(a[n], b[n]) for n in names)


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "fp16"])
@pytest.mark.parametrize("ch", range(4))
@pytest.mark.parametrize("H,W", VR.HW)
def test_borders_and_tile_edges_against_float64(Cv, H, W, ch, dtype):
    Cin, Cout = VR.sweep_channels(PREC[dtype])[ch]
    for family in VR.FAMILIES:
        c = VR.case(VR.SWEEP_B, H, W, Cin, Cout, family, PREC[dtype])
        check(run(Cv, *gpu(c, dtype)), c["ref"], f"edges {H}x{W} {Cin}->{Cout} {family} {dtype}")


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "fp16"])
@pytest.mark.parametrize("shape", [VR.LARGE, VR.SPLIT], ids=["large", "split"])
def test_larger_shapes_against_float64(Cv, shape, dtype):
    B, H, W, Cin, Cout = shape
    fwd, bwd = Cv.workspace_bytes(B, H, W, Cin, Cout, dtype)
    assert (fwd, bwd) == VR.expected_workspace(B, H, W, Cin, Cout, PREC[dtype])
    split = VR.expected_split(B * H * W, Cin, Cout, PREC[dtype])
    assert split > 1                                    # both shapes split the pixels in the weight gradient
    c = VR.case(B, H, W, Cin, Cout, "random", PREC[dtype])
    check(run(Cv, *gpu(c, dtype)), c["ref"], f"large {B}x{H}x{W} {Cin}->{Cout} split {split} {dtype}")


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "fp16"])
@pytest.mark.parametrize("H,W,Cin,Cout", [(16, 17, 72, 136), (2, 2, 136, 72), (33, 18, 32, 64)])
def test_slices_of_nan_padded_allocations_give_the_same_bits(Cv, H, W, Cin, Cout, dtype):
    """x, dy and every output as slices of allocations with a NaN image before and after and NaN columns behind every pixel; w, bias, dw and db inside
    NaN buffers: nothing outside is read, nothing outside is written."""
    B = VR.SWEEP_B
    c = VR.case(B, H, W, Cin, Cout, "random", PREC[dtype])
    x, w, b, dy = gpu(c, dtype)
    base = run(Cv, x, w, b, dy)
    pad = 2 * VR.CR.chunk(PREC[dtype])

    def padded(t=None, shape=None):
        shape = shape or t.shape
        big = nan(shape[0] + 2, shape[1], shape[2], shape[3] + pad, dtype=dtype)
        view = big[1:-1, :, :, :shape[3]]
        if t is not None:
            view.copy_(t)
        return big, view

    def inside(shape):
        n = int(np.prod(shape))
        buf = nan(n + 32, dtype=dtype)
        return buf, buf[16:16 + n].view(shape)

    bigs = {"y": padded(shape=(B, H, W, Cout)), "dx": padded(shape=(B, H, W, Cin)), "dw": inside((Cout, Cin, 3, 3)), "db": inside((Cout,))}
    outs = {n: v for n, (_, v) in bigs.items()}
    xs, dys = padded(x)[1], padded(dy)[1]
    assert not xs.is_contiguous() and Cv._in_place(xs) is xs and Cv._ld(xs) == Cin + pad
    ws, bs = inside(w.shape)[1].copy_(w), inside(b.shape)[1].copy_(b)
    got = run(Cv, xs, ws, bs, dys, outs)
    assert same_bits(got, base)
    for n in ("y", "dx"):                               # the padding of the outputs is untouched
        big = bigs[n][0]
        assert torch.isnan(big[0]).all() and torch.isnan(big[-1]).all() and torch.isnan(big[..., outs[n].shape[3]:]).all(), n
    for n in ("dw", "db"):
        buf = bigs[n][0]
        assert torch.isnan(buf[:16]).all() and torch.isnan(buf[-16:]).all(), n


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "fp16"])
def test_deterministic_and_an_image_is_the_image_it_is_alone(Cv, dtype):
    c = VR.case(VR.SWEEP_B, 16, 17, 72, 136, "random", PREC[dtype])
    x, w, b, dy = gpu(c, dtype)
    first, second = run(Cv, x, w, b, dy), run(Cv, x, w, b, dy)
    assert same_bits(first, second)
    for i in range(VR.SWEEP_B):
        alone = run(Cv, x[i:i + 1], w, b, dy[i:i + 1])
        assert torch.equal(alone["y"], first["y"][i:i + 1]) and torch.equal(alone["dx"], first["dx"][i:i + 1]), i
    B, H, W, Cin, Cout = VR.SPLIT                       # ... and with the split of the pixels
    c = VR.case(B, H, W, Cin, Cout, "random", PREC[dtype])
    x, w, b, dy = gpu(c, dtype)
    assert same_bits(run(Cv, x, w, b, dy), run(Cv, x, w, b, dy))


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "fp16"])
@pytest.mark.parametrize("layout", ["nchw", "channels_last"])
def test_the_public_function_equals_the_low_level_calls_and_skips_what_is_not_needed(Cv, layout, dtype):
    B, H, W, Cin, Cout = VR.SWEEP_B, 16, 17, 72, 136
    c = VR.case(B, H, W, Cin, Cout, "random", PREC[dtype])
    x, w, b, dy = gpu(c, dtype)
    base = run(Cv, x, w, b, dy)

    def arrange(t):                                     # (B, H, W, C) values as a (B, C, H, W) tensor of the layout
        t = t.permute(0, 3, 1, 2)
        return t.contiguous() if layout == "nchw" else t.contiguous(memory_format=torch.channels_last)

    def through_autograd(need):
        xl, wl, bl = (t.clone(memory_format=torch.preserve_format).requires_grad_(n) for t, n in zip((arrange(x), w, b), need))
        y = Cv.conv3x3(xl, wl, bl)
        assert y.shape == (B, Cout, H, W) and y.dtype == dtype and y.is_contiguous(memory_format=torch.channels_last)
        assert y.requires_grad == any(need)
        if any(need):
            y.backward(arrange(dy))
        return {"y": y.detach().permute(0, 2, 3, 1), "dx": xl.grad if xl.grad is None else xl.grad.permute(0, 2, 3, 1), "dw": wl.grad, "db": bl.grad}

    assert same_bits(through_autograd((True, True, True)), base)
    for skip in range(3):                               # each gradient skipped alone: it is None, the others keep their bits
        need = tuple(i != skip for i in range(3))
        got = through_autograd(need)
        assert got[NAMES[1 + skip]] is None
        assert same_bits(got, base, [n for i, n in enumerate(NAMES) if i != 1 + skip])
    y = Cv.conv3x3(arrange(x), w)                       # no bias, no gradient
    assert not y.requires_grad and torch.equal(y.permute(0, 2, 3, 1), Cv.forward(x, w))
    dx = nan(B, H, W, Cin, dtype=dtype)                 # the low-level call with one output: the others cost nothing and need nothing
    Cv.backward(None, w, dy, dx=dx)
    assert torch.equal(dx, base["dx"])
    dw = nan(Cout, Cin, 3, 3, dtype=dtype)
    Cv.backward(x, None, dy, dw=dw)
    assert torch.equal(dw, base["dw"])
    db = nan(Cout, dtype=dtype)
    Cv.backward(None, None, dy, db=db)
    assert torch.equal(db, base["db"])
    if layout == "channels_last":                       # a channel slice of a channels_last tensor is read through its pixel stride
        wide = torch.cat([arrange(x), arrange(x)], 1).contiguous(memory_format=torch.channels_last)
        part = wide[:, Cin:]
        assert Cv._nhwc(part).data_ptr() == part.data_ptr()
        assert torch.equal(Cv.conv3x3(part, w, b).permute(0, 2, 3, 1), base["y"])
    we, be = w.clone().requires_grad_(True), b.clone().requires_grad_(True)          # B = 0: nothing is launched, the parameter gradients are zero
    e = Cv.conv3x3(arrange(x)[:0], we, be)
    assert e.shape == (0, Cout, H, W)
    e.sum().backward()
    assert we.grad.shape == w.shape and be.grad.shape == b.shape and not we.grad.any() and not be.grad.any()


def test_autocast(Cv):
    x = torch.randn(2, 32, 9, 10, device="cuda", requires_grad=True)
    m = Cv.wrap_conv3x3(nn.Conv2d(32, 40, 3, padding=1, padding_mode="replicate").cuda())
    with torch.autocast("cuda", dtype=torch.bfloat16):
        with pytest.raises(NotImplementedError, match="moge_amd.conv.*bfloat16"):
            m(x)
    with torch.autocast("cuda", dtype=torch.float16):
        y = m(x)
    assert y.dtype == torch.float16 and y.shape == (2, 40, 9, 10)
    y.backward(torch.ones_like(y))
    assert x.grad.dtype == m.weight.grad.dtype == m.bias.grad.dtype == torch.float32          # fp32 tensors receive fp32 gradients through the cast
    want = F.conv2d(F.pad(x.detach().half(), (1, 1, 1, 1), mode="replicate"), m.weight.detach().half(), m.bias.detach().half())
    assert float((y.detach().float() - want.float()).abs().max()) <= 2.0 ** -9 * float(want.float().abs().max())
    xg = x.detach().requires_grad_(True)                 # double backward is not built: once_differentiable refuses it
    yg = m(xg)
    (g,) = torch.autograd.grad(yg, xg, grad_outputs=torch.ones_like(yg).requires_grad_(True), create_graph=True)
    with pytest.raises(RuntimeError, match="once_differentiable"):
        g.sum().backward()


def decoder_level():
    """A decoder level without norms: two residual blocks (ReLU, conv, ReLU, conv, skip add) at 64 channels."""
    torch.manual_seed(5)
    return nn.Sequential(ResidualStandIn(64), ResidualStandIn(64))


def hip_model(level):
    model = model_of(Block())
    model.neck = level
    return model


class Fp16Point(torch.autograd.Function):
    """A tensor that autocast keeps in fp16, inside a float64 graph: the value and its gradient are rounded to fp16, everything between stays float64."""

    @staticmethod
    def forward(ctx, t):
        return t.half().double()

    @staticmethod
    def backward(ctx, g):
        return g.half().double()


def with_autocast_points(module):
    """The float64 copy evaluated as fp16 autocast defines the computation: input, weight, bias and output of every conv - and so their gradients -
    are fp16 values, every sum is exact.  Without this the comparison does not measure the convs: the level is piecewise linear, its gradient
    jumps wherever an input of a ReLU or of the skip add's ReLU changes sign, and the fp16 roundings of a forward move a few of the 2 x 64 x 17 x 18
    values across zero.  torch's own fp16 autocast of this level on the CPU is then 1e-2 ... 1e-1 away from the plain float64 copy in the input
    gradient and 6e-2 ... 1.2e-1 in a weight gradient (seeds 5 - 8), whatever computes the convs; against this form it is within 7.5e-4."""
    for m in module.modules():
        if isinstance(m, nn.Conv2d):
            m.forward = lambda t, m=m: Fp16Point.apply(m._conv_forward(Fp16Point.apply(t), Fp16Point.apply(m.weight), Fp16Point.apply(m.bias)))
    return module


@pytest.mark.parametrize("autocast", [False, True], ids=["fp32", "autocast-fp16"])
def test_a_decoder_level_trains_a_step_through_this_library(Cv, autocast, monkeypatch):
    level = decoder_level()
    x, gy = torch.randn(2, 64, 17, 18), torch.randn(2, 64, 17, 18)
    ref_level = copy.deepcopy(level).double()
    if autocast:
        with_autocast_points(ref_level)
    xr = x.double().requires_grad_(True)
    yr = ref_level(xr)
    yr.backward(gy.double())
    want = {"y": yr.detach(), "x": xr.grad, **{n: p.grad for n, p in ref_level.named_parameters()}}

    model = Cv.use_hip_conv(hip_model(level.cuda()))
    conv2d = F.conv2d

    def refuse(input, weight, *a, **k):
        if tuple(weight.shape[2:]) == (3, 3):
            raise AssertionError("torch's own conv2d was called with a 3x3 weight inside the level")
        return conv2d(input, weight, *a, **k)

    monkeypatch.setattr(F, "conv2d", refuse)
    xg = x.cuda().requires_grad_(True)
    with torch.autocast("cuda", dtype=torch.float16, enabled=autocast):
        y = model.neck(xg)
    y.backward(gy.cuda().to(y.dtype))
    monkeypatch.undo()
    got = {"y": y.detach(), "x": xg.grad, **{n: p.grad for n, p in model.neck.named_parameters()}}
    assert set(got) == set(want) and len(want) == 2 + 8
    err = {n: float((got[n].double().cpu() - want[n]).abs().max() / want[n].abs().max()) for n in want}
    print(f"decoder level autocast={autocast}", " ".join(f"{n}={e:.3e}" for n, e in err.items()))
    for n in want:
        assert got[n].dtype == torch.float32 and err[n] < BAND[autocast], (n, err[n])


def test_the_level_under_checkpointing_gives_the_same_bits(Cv):
    plain = Cv.use_hip_conv(hip_model(decoder_level().cuda()))
    wrapped = Cv.use_hip_conv(hip_model(Checkpointed(decoder_level().cuda())))
    x, gy = torch.randn(2, 64, 17, 18, device="cuda"), torch.randn(2, 64, 17, 18, device="cuda")
    got = []
    for model in (plain, wrapped):
        xg = x.clone().requires_grad_(True)
        y = model.neck(xg)
        y.backward(gy)
        got.append([y.detach(), xg.grad] + [p.grad for p in model.neck.parameters()])
    assert len(got[0]) == len(got[1]) == 2 + 8 and all(torch.equal(a, b) for a, b in zip(*got))
