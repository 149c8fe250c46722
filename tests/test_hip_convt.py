"""GPU: the trainable ConvTranspose2d(2, 2) and the 1x1 conv (moge_amd.convt, csrc/convt_grad.hip) against the float64 references of
tests/convt_reference.py and tests/linear_reference.py.

Gate: |got - ref| <= bound element by element, for y, dx, dw and db in both storage types; every output is filled with NaN before the call and must
come back finite.  Shapes are the tile edges (one pixel, one row, one column, 2 x 2; 128 flat pixels and 128 columns per workgroup, the four taps
inside one column tile or straddling two, K tiles of 64 fp16 / 32 fp32 elements), not the workload; a shape at which the weight gradient splits the
pixels with a ragged last part (S = 8 fp16, 15 fp32) and one whose image rows span three pixel tiles run once each.  Inputs are rounded to the
storage type before the reference runs, so the figures are the kernels' own error.  Every test prints its figures before it asserts.

Measured worst error / bound on an MI355X: fp32 y 0.404, dx 0.164, dw 0.465, db 0.285 at the edges (y and dx at 4 -> 4
channels, dw and db at the sums of 2 terms of the one-pixel image) and at most 0.069 at the larger shapes; fp16 y 0.996, dx 0.984, dw 0.997, db 0.989
at the edges and y 0.975, dx 0.958, dw 0.501, db 0.044 at the larger shapes - the fp16 bound is dominated by the store's h |ref|, which one correct
rounding of a value just above a power of two uses up, so a fraction close to 1 is the store, not the sum.  conv1x1: fp32 at most 0.089, fp16 y 0.982,
dx 0.962, dw 0.654, db 0.440.  The resampler level through autograd: at most 5.6e-7 plain and 4.3e-3 under fp16 autocast."""
import copy

import numpy as np
import pytest
import torch
from torch import nn
from torch.nn import functional as F

import convt_reference as TR
import linear_reference as LR
from tests.test_conv_module_cpu import Checkpointed, ResidualStandIn, conv
from tests.test_linear_module_cpu import Block, model_of

pytestmark = pytest.mark.gpu

DTYPES = [torch.float32, torch.float16]
PREC = {torch.float32: 0, torch.float16: 1}
NAMES = ("y", "dx", "dw", "db")
BAND = {False: 2e-5, True: 1e-2}           # the project's bands for the path through autograd: plain, fp16 autocast


@pytest.fixture(scope="module")
def Ct():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from moge_amd import convt
    return convt


def gpu(c, dtype):
    return tuple(torch.from_numpy(c[n]).to("cuda", dtype) for n in ("x", "w", "b", "dy"))


def nan(*shape, dtype):
    return torch.full(shape, float("nan"), dtype=dtype, device="cuda")


def run(Ct, x, w, b, dy, outs=None):
    """Forward and backward through the low-level calls into NaN-filled outputs (`outs`: views to write instead) -> {name: tensor}."""
    (B, H, W, Cin), Cout = x.shape, w.shape[1]
    o = outs or {"y": nan(B, 2 * H, 2 * W, Cout, dtype=x.dtype), "dx": nan(B, H, W, Cin, dtype=x.dtype), "dw": nan(Cin, Cout, 2, 2, dtype=x.dtype), "db": nan(Cout, dtype=x.dtype)}
    assert Ct.forward(x, w, b, out=o["y"]) is o["y"]
    Ct.backward(x, w, dy, o["dx"], o["dw"], o["db"])
    return o


def check(got, ref, what, names=NAMES):
    frac = {}
    for n in names:
        r, bound = ref[n]
        g = got[n].double().cpu().numpy().reshape(r.shape)
        assert np.isfinite(g).all(), (what, n)
        frac[n] = float((np.abs(g - r) / bound).max())
    print(what, " ".join(f"{n}={f:.3f}" for n, f in frac.items()), "(worst error / bound)")
    for n in names:
        assert frac[n] <= 1.0, (what, n, frac[n])


def same_bits(a, b, names=NAMES):
    return all(torch.equal(a[n], b[n]) for n in names)


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "fp16"])
@pytest.mark.parametrize("ch", range(4))
@pytest.mark.parametrize("H,W", TR.HW)
def test_tile_edges_against_float64(Ct, H, W, ch, dtype):
    Cin, Cout = TR.sweep_channels(PREC[dtype])[ch]
    for family in TR.FAMILIES:
        c = TR.case(TR.SWEEP_B, H, W, Cin, Cout, family, PREC[dtype])
        got = run(Ct, *gpu(c, dtype))
        assert all(got[n].shape == c["ref"][n][0].shape for n in NAMES)
        check(got, c["ref"], f"edges {H}x{W} {Cin}->{Cout} {family} {dtype}")


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "fp16"])
@pytest.mark.parametrize("shape", [TR.SPLIT, TR.ROWS], ids=["split", "rows"])
def test_larger_shapes_against_float64(Ct, shape, dtype):
    B, H, W, Cin, Cout = shape
    fwd, bwd = Ct.workspace_bytes(B, H, W, Cin, Cout, dtype)
    assert (fwd, bwd) == TR.expected_workspace(B, H, W, Cin, Cout, PREC[dtype])
    split = TR.expected_split(B * H * W, Cin, Cout, PREC[dtype])
    if shape == TR.SPLIT:
        assert split == TR.SPLIT_S[PREC[dtype]]          # S = 15 (fp32) / 8 (fp16), the last part ragged
    c = TR.case(B, H, W, Cin, Cout, "random", PREC[dtype])
    check(run(Ct, *gpu(c, dtype)), c["ref"], f"larger {B}x{H}x{W} {Cin}->{Cout} S={split} {dtype}")


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "fp16"])
@pytest.mark.parametrize("H,W,Cin,Cout", [(16, 17, 72, 136), (2, 2, 136, 72), (33, 18, 32, 64)])
def test_slices_of_nan_padded_allocations_give_the_same_bits(Ct, H, W, Cin, Cout, dtype):
    """x, dy and every output as slices of allocations with a NaN image before and after and NaN channel chunks behind every pixel; w, bias, dw and db
    inside NaN buffers: nothing outside is read, nothing outside is written."""
    B = TR.SWEEP_B
    c = TR.case(B, H, W, Cin, Cout, "random", PREC[dtype])
    x, w, b, dy = gpu(c, dtype)
    base = run(Ct, x, w, b, dy)
    pad = 2 * TR.CR.chunk(PREC[dtype])

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

    bigs = {"y": padded(shape=(B, 2 * H, 2 * W, Cout)), "dx": padded(shape=(B, H, W, Cin)), "dw": inside((Cin, Cout, 2, 2)), "db": inside((Cout,))}
    outs = {n: v for n, (_, v) in bigs.items()}
    xs, dys = padded(x)[1], padded(dy)[1]
    assert not xs.is_contiguous() and Ct._in_place(xs) is xs and Ct._ld(xs) == Cin + pad and Ct._in_place(dys) is dys and Ct._ld(dys) == Cout + pad
    ws, bs = inside(w.shape)[1].copy_(w), inside(b.shape)[1].copy_(b)
    got = run(Ct, xs, ws, bs, dys, outs)
    assert same_bits(got, base)
    for n in ("y", "dx"):                               # the padding of the outputs is untouched
        big = bigs[n][0]
        assert torch.isnan(big[0]).all() and torch.isnan(big[-1]).all() and torch.isnan(big[..., outs[n].shape[3]:]).all(), n
    for n in ("dw", "db"):
        buf = bigs[n][0]
        assert torch.isnan(buf[:16]).all() and torch.isnan(buf[-16:]).all(), n


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "fp16"])
def test_deterministic_and_an_image_is_the_image_it_is_alone(Ct, dtype):
    c = TR.case(TR.SWEEP_B, 16, 17, 72, 136, "random", PREC[dtype])
    x, w, b, dy = gpu(c, dtype)
    first, second = run(Ct, x, w, b, dy), run(Ct, x, w, b, dy)
    assert same_bits(first, second)
    for i in range(TR.SWEEP_B):
        alone = run(Ct, x[i:i + 1], w, b, dy[i:i + 1])
        assert torch.equal(alone["y"], first["y"][i:i + 1]) and torch.equal(alone["dx"], first["dx"][i:i + 1]), i
    B, H, W, Cin, Cout = TR.SPLIT                       # ... and with the split of the pixels
    c = TR.case(B, H, W, Cin, Cout, "random", PREC[dtype])
    x, w, b, dy = gpu(c, dtype)
    assert same_bits(run(Ct, x, w, b, dy), run(Ct, x, w, b, dy))


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "fp16"])
@pytest.mark.parametrize("layout", ["nchw", "channels_last"])
def test_the_public_function_equals_the_low_level_calls_and_skips_what_is_not_needed(Ct, layout, dtype):
    B, H, W, Cin, Cout = TR.SWEEP_B, 16, 17, 72, 136
    c = TR.case(B, H, W, Cin, Cout, "random", PREC[dtype])
    x, w, b, dy = gpu(c, dtype)
    base = run(Ct, x, w, b, dy)

    def arrange(t):                                     # (B, H, W, C) values as a (B, C, H, W) tensor of the layout
        t = t.permute(0, 3, 1, 2)
        return t.contiguous() if layout == "nchw" else t.contiguous(memory_format=torch.channels_last)

    def through_autograd(need):
        xl, wl, bl = (t.clone(memory_format=torch.preserve_format).requires_grad_(n) for t, n in zip((arrange(x), w, b), need))
        y = Ct.conv_transpose2x2(xl, wl, bl)
        assert y.shape == (B, Cout, 2 * H, 2 * W) and y.dtype == dtype and y.is_contiguous(memory_format=torch.channels_last)
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
    y = Ct.conv_transpose2x2(arrange(x), w)             # no bias, no gradient
    assert not y.requires_grad and torch.equal(y.permute(0, 2, 3, 1), Ct.forward(x, w))
    dx = nan(B, H, W, Cin, dtype=dtype)                 # the low-level call with one output: the others cost nothing and need nothing
    Ct.backward(None, w, dy, dx=dx)
    assert torch.equal(dx, base["dx"])
    dw = nan(Cin, Cout, 2, 2, dtype=dtype)
    Ct.backward(x, None, dy, dw=dw)
    assert torch.equal(dw, base["dw"])
    db = nan(Cout, dtype=dtype)
    Ct.backward(None, None, dy, db=db)
    assert torch.equal(db, base["db"])
    with pytest.raises(ValueError, match="dw must be"):  # dw is the weight's (Cin, Cout, 2, 2)
        Ct.backward(x, None, dy, dw=nan(Cout, Cin, 2, 2, dtype=dtype))
    if layout == "channels_last":                       # a channel slice of a channels_last tensor is read through its pixel stride
        wide = torch.cat([arrange(x), arrange(x)], 1).contiguous(memory_format=torch.channels_last)
        part = wide[:, Cin:]
        assert Ct._nhwc(part).data_ptr() == part.data_ptr()
        assert torch.equal(Ct.conv_transpose2x2(part, w, b).permute(0, 2, 3, 1), base["y"])
    we, be = w.clone().requires_grad_(True), b.clone().requires_grad_(True)          # B = 0: nothing is launched, the parameter gradients are zero
    e = Ct.conv_transpose2x2(arrange(x)[:0], we, be)
    assert e.shape == (0, Cout, 2 * H, 2 * W)
    e.sum().backward()
    assert we.grad.shape == w.shape and be.grad.shape == b.shape and not we.grad.any() and not be.grad.any()


def test_autocast(Ct):
    x = torch.randn(2, 32, 9, 10, device="cuda", requires_grad=True)
    m = Ct.wrap_conv_transpose2x2(nn.ConvTranspose2d(32, 40, 2, 2).cuda())
    with torch.autocast("cuda", dtype=torch.bfloat16):
        with pytest.raises(NotImplementedError, match="moge_amd.convt.*bfloat16"):
            m(x)
    with torch.autocast("cuda", dtype=torch.float16):
        y = m(x)
    assert y.dtype == torch.float16 and y.shape == (2, 40, 18, 20)
    y.backward(torch.ones_like(y))
    assert x.grad.dtype == m.weight.grad.dtype == m.bias.grad.dtype == torch.float32          # fp32 tensors receive fp32 gradients through the cast
    want = F.conv_transpose2d(x.detach().half(), m.weight.detach().half(), m.bias.detach().half(), stride=2)
    assert float((y.detach().float() - want.float()).abs().max()) <= 2.0 ** -9 * float(want.float().abs().max())
    xg = x.detach().requires_grad_(True)                 # double backward is not built: once_differentiable refuses it
    yg = m(xg)
    (g,) = torch.autograd.grad(yg, xg, grad_outputs=torch.ones_like(yg).requires_grad_(True), create_graph=True)
    with pytest.raises(RuntimeError, match="once_differentiable"):
        g.sum().backward()


# ---- the 1x1 conv: moge_amd.linear on the pixels ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "fp16"])
@pytest.mark.parametrize("Cin,Cout", [(32, 64), (72, 136)])
def test_conv1x1_is_the_linear_on_the_pixels(Ct, Cin, Cout, dtype, monkeypatch):
    from moge_amd import linear as Lin
    B, H, W = 2, 17, 18
    c = LR.case(B * H * W, Cin, Cout, "random", PREC[dtype])
    x, w, b, dy = gpu(c, dtype)                          # x (M, Cin), w (Cout, Cin), dy (M, Cout)
    y = Lin.forward(x, w, b)
    dx, dw, db = nan(B * H * W, Cin, dtype=dtype), nan(Cout, Cin, dtype=dtype), nan(Cout, dtype=dtype)
    Lin.backward(x, w, dy, dx, dw, db)
    seen = []
    fwd, bwd = Lin.forward, Lin.backward
    monkeypatch.setattr(Lin, "forward", lambda x, *a, **k: (seen.append(("x", x.data_ptr(), x.stride())), fwd(x, *a, **k))[1])
    monkeypatch.setattr(Lin, "backward", lambda x, w, dy, *a, **k: (seen.append(("dy", dy.data_ptr(), dy.stride())), bwd(x, w, dy, *a, **k))[1])
    for layout in ("channels_last", "nchw", "slice"):
        def arrange(t, C):                               # (M, C) rows as a (B, C, H, W) tensor of the layout
            t = t.view(B, H, W, C).permute(0, 3, 1, 2)
            if layout == "slice":                        # the second half of the channels of a channels_last tensor
                return torch.cat([torch.full_like(t, float("nan")), t], 1).contiguous(memory_format=torch.channels_last)[:, C:]
            return t.contiguous() if layout == "nchw" else t.contiguous(memory_format=torch.channels_last)
        xl, gl = arrange(x, Cin).requires_grad_(True), arrange(dy, Cout)
        wl, bl = w.view(Cout, Cin, 1, 1).clone().requires_grad_(True), b.clone().requires_grad_(True)
        del seen[:]
        out = Ct.conv1x1(xl, wl, bl)
        assert out.shape == (B, Cout, H, W) and out.dtype == dtype and out.is_contiguous(memory_format=torch.channels_last)
        out.backward(gl)
        got = {"y": out.detach().permute(0, 2, 3, 1), "dx": xl.grad.permute(0, 2, 3, 1), "dw": wl.grad, "db": bl.grad}
        assert wl.grad.shape == (Cout, Cin, 1, 1) and wl.grad.is_contiguous()
        for n, t in (("y", y), ("dx", dx), ("dw", dw), ("db", db)):                  # the bits of linear.forward / backward on the same rows
            assert torch.equal(got[n].reshape(t.shape), t), (layout, n)
        check(got, c["ref"], f"conv1x1 {B}x{H}x{W} {Cin}->{Cout} {layout} {dtype}")
        assert [s[0] for s in seen] == ["x", "dy"]
        if layout != "nchw":                             # a channels_last input and gradient are read where they lie, through their pixel stride
            ld = {"channels_last": 1, "slice": 2}[layout]
            assert seen[0][1:] == (xl.data_ptr(), (ld * Cin, 1)) and seen[1][1:] == (gl.data_ptr(), (ld * Cout, 1)), layout
    y0 = Ct.conv1x1(arrange(x, Cin)[:0], wl, bl)         # B = 0
    assert y0.shape == (0, Cout, H, W)


# ---- through autograd: a resampler level -----------------------------------------------------------------------------------------------------
def resampler_level():
    """A conv_transpose resampler level without norms: 1x1 in, ConvTranspose2d(2, 2), a 3x3, ReLU, a residual block.  torch initialises the four
    taps of the transposed conv independently, so they differ."""
    torch.manual_seed(5)
    return nn.Sequential(nn.Conv2d(64, 64, 1), nn.ConvTranspose2d(64, 32, 2, 2), conv(32, 32), nn.ReLU(), ResidualStandIn(32))


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
    """The float64 copy evaluated as fp16 autocast defines the computation: input, weight, bias and output of every conv - and so
    their gradients - are fp16 values, every sum is exact."""
    P = Fp16Point.apply
    for m in module.modules():
        if isinstance(m, nn.ConvTranspose2d):
            m.forward = lambda t, m=m: P(F.conv_transpose2d(P(t), P(m.weight), P(m.bias), m.stride))
        elif isinstance(m, nn.Conv2d):
            m.forward = lambda t, m=m: P(m._conv_forward(P(t), P(m.weight), P(m.bias)))
    return module


def refusing(name):
    def refuse(*a, **k):
        raise AssertionError(f"torch's own {name} was called inside the level")
    return refuse


@pytest.mark.parametrize("autocast", [False, True], ids=["fp32", "autocast-fp16"])
def test_a_resampler_level_trains_a_step_through_this_library(Ct, autocast, monkeypatch):
    level = resampler_level()
    x, gy = torch.randn(2, 64, 17, 18), torch.randn(2, 32, 34, 36)
    ref_level = copy.deepcopy(level).double()
    if autocast:
        with_autocast_points(ref_level)
    xr = x.double().requires_grad_(True)
    yr = ref_level(xr)
    yr.backward(gy.double())
    want = {"y": yr.detach(), "x": xr.grad, **{n: p.grad for n, p in ref_level.named_parameters()}}

    model = Ct.use_hip_decoder(hip_model(level.cuda()))
    assert sum(Ct._wrapped(m) for m in model.neck.modules()) == 5          # the 1x1, the transposed conv and three 3x3
    monkeypatch.setattr(F, "conv2d", refusing("conv2d"))
    monkeypatch.setattr(F, "conv_transpose2d", refusing("conv_transpose2d"))
    xg = x.cuda().requires_grad_(True)
    with torch.autocast("cuda", dtype=torch.float16, enabled=autocast):
        y = model.neck(xg)
    y.backward(gy.cuda().to(y.dtype))
    monkeypatch.undo()
    got = {"y": y.detach(), "x": xg.grad, **{n: p.grad for n, p in model.neck.named_parameters()}}
    assert set(got) == set(want) and len(want) == 2 + 10
    err = {n: float((got[n].double().cpu() - want[n]).abs().max() / want[n].abs().max()) for n in want}
    print(f"resampler level autocast={autocast}", " ".join(f"{n}={e:.3e}" for n, e in err.items()))
    for n in want:                                      # under autocast the level's skip input is the fp16 output of the 3x3, so y is fp16; every gradient is fp32
        assert got[n].dtype == (torch.float16 if autocast and n == "y" else torch.float32) and got[n].shape == want[n].shape and err[n] < BAND[autocast], (n, err[n])


def test_the_level_under_checkpointing_gives_the_same_bits(Ct):
    plain = Ct.use_hip_decoder(hip_model(resampler_level().cuda()))
    wrapped = Ct.use_hip_decoder(hip_model(Checkpointed(resampler_level().cuda())))
    x, gy = torch.randn(2, 64, 17, 18, device="cuda"), torch.randn(2, 32, 34, 36, device="cuda")
    got = []
    for model in (plain, wrapped):
        xg = x.clone().requires_grad_(True)
        y = model.neck(xg)
        y.backward(gy)
        got.append([y.detach(), xg.grad] + [p.grad for p in model.neck.parameters()])
    assert len(got[0]) == len(got[1]) == 2 + 10 and all(torch.equal(a, b) for a, b in zip(*got))
