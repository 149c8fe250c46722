"""GPU: the trainable bilinear resize and the narrow 1x1 conv (moge_amd.resample, csrc/resample_grad.hip) against the float64 references of
tests/resample_reference.py.

Gate: |got - ref| <= bound element by element, for y and dx of the resize and y, dx, dw, db of the conv, in both storage types; every output is filled
with NaN before the call and must come back finite.  Shapes are the edges (one pixel, one row, one column, x2, non-integer up, down with input rows
that receive nothing, identity, mixed; 1 and 3 channels on the element path, one and several 16-byte chunks on the vector path; pixel counts around the
64 pixels of a forward workgroup and a ragged last slab of the weight gradient), not the workload.  Inputs are rounded to the storage type before the
reference runs, so the figures are the kernels' own error.  Every test prints its figures before it asserts.  The bounds were stated in
tests/resample_reference.py before the first GPU run; the measured figures are in DESIGN.md section 23."""
import copy

import numpy as np
import pytest
import torch
from torch import nn
from torch.nn import functional as F

import resample_reference as RR
from tests.test_conv_module_cpu import Checkpointed, conv
from tests.test_hip_convt import BAND, Fp16Point, nan, same_bits
from tests.test_linear_module_cpu import Block, model_of

pytestmark = pytest.mark.gpu

DTYPES = [torch.float32, torch.float16]
PREC = {torch.float32: 0, torch.float16: 1}
SHAPE_ID = lambda s: f"{s[0][0]}x{s[0][1]}-{s[1][0]}x{s[1][1]}"      # noqa: E731


@pytest.fixture(scope="module")
def Rs():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from moge_amd import resample
    return resample


def dev(a, dtype):
    return torch.from_numpy(a).to("cuda", dtype)


def check(got, ref, what, names=("y", "dx", "dw", "db")):
    """test_hip_convt's check, with a bound of exactly zero (an input sample of the resize that no output reads, in fp32) met by an error of exactly zero."""
    frac = {}
    for n in names:
        r, bound = ref[n]
        g = got[n].double().cpu().numpy().reshape(r.shape)
        assert np.isfinite(g).all(), (what, n)
        err = np.abs(g - r)
        frac[n] = float(np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.where(err == 0, 0.0, np.inf)).max())
    print(what, " ".join(f"{n}={f:.3f}" for n, f in frac.items()), "(worst error / bound)")
    for n in names:
        assert frac[n] <= 1.0, (what, n, frac[n])


def run_resize(Rs, x, dy, size, scales=None, outs=None):
    """Forward and backward through the low-level calls into NaN-filled outputs (`outs`: views to write instead) -> {"y", "dx"}."""
    B, Hin, Win, C = x.shape
    o = outs or {"y": nan(B, size[0], size[1], C, dtype=x.dtype), "dx": nan(B, Hin, Win, C, dtype=x.dtype)}
    assert Rs.resize_forward(x, size, scales, out=o["y"]) is o["y"]
    assert Rs.resize_backward(dy, (Hin, Win), scales, dx=o["dx"]) is o["dx"]
    return o


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "fp16"])
@pytest.mark.parametrize("shape", RR.RESIZE, ids=SHAPE_ID)
def test_resize_edges_against_float64(Rs, shape, dtype):
    (Hin, Win), (Hout, Wout) = shape
    for C in RR.resize_channels(PREC[dtype]):
        c = RR.resize_case(RR.SWEEP_B, Hin, Win, Hout, Wout, C, PREC[dtype])
        x, dy = dev(c["x"], dtype), dev(c["dy"], dtype)
        got = run_resize(Rs, x, dy, (Hout, Wout))
        check(got, c["ref"], f"resize {SHAPE_ID(shape)} C={C} {dtype}", ("y", "dx"))
        if shape == RR.IDENTITY:
            assert torch.equal(got["y"], x)
        if shape in RR.EMPTY_ROWS:                           # the rows nothing reads were written, with zero
            bound32 = RR.resize(c["x"], (Hout, Wout), c["dy"], 0)["dx"][1]          # without the fp16 store's terms: zero where nothing can arrive
            zero = [r for r in range(Hin) if not bound32[:, r].any()]
            assert len(zero) >= RR.EMPTY_ROWS[shape] - 2 and not got["dx"][:, zero].any()
        if shape in RR.X2:                                   # the x2 by size, by scale and as the module has it: the same bits
            assert same_bits(run_resize(Rs, x, dy, (Hout, Wout), (0.5, 0.5)), got, ("y", "dx"))
            xs = x.permute(0, 3, 1, 2).clone(memory_format=torch.preserve_format).requires_grad_(True)
            ys = Rs.wrap_upsample(nn.Upsample(scale_factor=2, mode="bilinear", align_corners=False))(xs)
            ys.backward(dy.permute(0, 3, 1, 2))
            assert torch.equal(ys.detach().permute(0, 2, 3, 1), got["y"]) and torch.equal(xs.grad.permute(0, 2, 3, 1), got["dx"])
            xz = x.permute(0, 3, 1, 2).clone(memory_format=torch.preserve_format).requires_grad_(True)
            yz = Rs.interpolate(xz, size=(Hout, Wout))
            yz.backward(dy.permute(0, 3, 1, 2))
            assert yz.is_contiguous(memory_format=torch.channels_last) and torch.equal(yz.detach(), ys.detach()) and torch.equal(xz.grad, xs.grad)


def run_conv(Rs, x, w, b, dy, outs=None):
    (B, H, W, Cin), Cout = x.shape, w.shape[0]
    o = outs or {"y": nan(B, H, W, Cout, dtype=x.dtype), "dx": nan(B, H, W, Cin, dtype=x.dtype), "dw": nan(Cout, Cin, 1, 1, dtype=x.dtype), "db": nan(Cout, dtype=x.dtype)}
    assert Rs.conv_forward(x, w, b, out=o["y"]) is o["y"]
    Rs.conv_backward(x, w, dy, o["dx"], o["dw"], o["db"])
    return o


def conv_tensors(c, dtype, B, H, W):
    x, w, b, dy = (dev(c[n], dtype) for n in ("x", "w", "b", "dy"))
    return x.view(B, H, W, -1), w.view(*w.shape, 1, 1), b, dy.view(B, H, W, -1)


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "fp16"])
@pytest.mark.parametrize("M", RR.CONV_M)
def test_conv_edges_against_float64(Rs, M, dtype):
    for Cin, Cout in RR.conv_channels(PREC[dtype]):
        if M == RR.RAGGED_M:
            assert Rs.conv_workspace_bytes(1, 1, M, Cin, Cout, dtype) == (0, -(-4 * 3 * Cout * (Cin + 1) // 16) * 16)          # three slabs
        for family in ("random", "offset"):
            c = RR.conv_case(M, Cin, Cout, family, PREC[dtype])
            check(run_conv(Rs, *conv_tensors(c, dtype, 1, 1, M)), c["ref"], f"conv M={M} {Cin}->{Cout} {family} {dtype}")


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "fp16"])
def test_slices_of_nan_padded_allocations_give_the_same_bits(Rs, dtype):
    """Every activation as a channel slice of a wider allocation with a NaN image before and after and NaN channels beside it: nothing outside
    [0, pixels) x [0, C) is read or written, and the tensor's own memory is what the library gets."""
    ch = RR.CR.chunk(PREC[dtype])

    def padded(shape, t=None, before=0, after=None):
        after = ch if after is None else after
        big = nan(shape[0] + 2, shape[1], shape[2], before + shape[3] + after, dtype=dtype)
        view = big[1:-1, :, :, before:before + shape[3]]
        if t is not None:
            view.copy_(t)
        return big, view

    def untouched(big, view, before):
        C = view.shape[3]
        return bool(torch.isnan(big[0]).all() and torch.isnan(big[-1]).all() and torch.isnan(big[..., :before]).all() and torch.isnan(big[..., before + C:]).all())

    (Hin, Win), (Hout, Wout) = (7, 5), (16, 9)
    for C, before in ((3, 0), (3, 1), (1, 2), (ch, ch), (40, 0)):              # element path at three alignments, vector path with a chunk on either side
        c = RR.resize_case(RR.SWEEP_B, Hin, Win, Hout, Wout, C, PREC[dtype])
        x, dy = dev(c["x"], dtype), dev(c["dy"], dtype)
        base = run_resize(Rs, x, dy, (Hout, Wout))
        xs, dys = padded(x.shape, x, before)[1], padded(dy.shape, dy, before)[1]
        bigs = {"y": padded(dy.shape, None, before), "dx": padded(x.shape, None, before)}
        assert Rs._pixels(xs) is xs and Rs._pixels(dys) is dys and Rs._ld(xs) == before + C + ch and not xs.is_contiguous()
        got = run_resize(Rs, xs, dys, (Hout, Wout), outs={n: v for n, (_, v) in bigs.items()})
        assert same_bits(got, base, ("y", "dx")) and all(untouched(*bigs[n], before) for n in bigs), (C, before)
        cl = torch.cat([torch.full_like(x, float("nan")), x], 3).permute(0, 3, 1, 2)          # a channels_last tensor's second half, through autograd
        part = cl[:, C:].requires_grad_(True)
        assert Rs._nhwc(part).data_ptr() == part.data_ptr()
        y = Rs.interpolate(part, size=(Hout, Wout))
        gl = torch.cat([torch.full_like(dy, float("nan")), dy], 3).permute(0, 3, 1, 2)[:, C:]
        assert Rs._nhwc(gl).data_ptr() == gl.data_ptr()
        (gx,) = torch.autograd.grad(y, part, gl)
        assert torch.equal(y.detach().permute(0, 2, 3, 1), base["y"]) and torch.equal(gx.permute(0, 2, 3, 1), base["dx"]), (C, before)

    B, H, W = 2, 9, 11
    for Cin, Cout, before in ((32, 3, 0), (32, 3, 1), (32, 1, 3), (72, 7, 0)):
        c = RR.conv_case(B * H * W, Cin, Cout, "random", PREC[dtype])
        x, w, b, dy = conv_tensors(c, dtype, B, H, W)
        base = run_conv(Rs, x, w, b, dy)
        xs, dys = padded(x.shape, x, ch)[1], padded(dy.shape, dy, before, 2)[1]
        bigs = {"y": padded(dy.shape, None, before, 2), "dx": padded(x.shape, None, ch)}
        flat = {"dw": nan(Cout * Cin + 32, dtype=dtype), "db": nan(Cout + 32, dtype=dtype)}
        outs = {"y": bigs["y"][1], "dx": bigs["dx"][1], "dw": flat["dw"][16:16 + Cout * Cin].view(Cout, Cin, 1, 1), "db": flat["db"][16:16 + Cout]}
        assert Rs._pixels(dys) is dys and Rs._ld(dys) == before + Cout + 2
        got = run_conv(Rs, xs, w, b, dys, outs)
        assert same_bits(got, base, ("y", "dx", "dw", "db")), (Cin, Cout, before)
        assert untouched(*bigs["y"], before) and untouched(*bigs["dx"], ch) and all(torch.isnan(f[:16]).all() and torch.isnan(f[-16:]).all() for f in flat.values())


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "fp16"])
def test_deterministic_and_an_image_is_the_image_it_is_alone(Rs, dtype):
    for (Hin, Win), (Hout, Wout), C in (((33, 18), (66, 36), 40), ((16, 9), (7, 5), 3), ((5, 7), (4, 23), 1)):
        c = RR.resize_case(RR.SWEEP_B, Hin, Win, Hout, Wout, C, PREC[dtype])
        x, dy = dev(c["x"], dtype), dev(c["dy"], dtype)
        first = run_resize(Rs, x, dy, (Hout, Wout))
        assert same_bits(run_resize(Rs, x, dy, (Hout, Wout)), first, ("y", "dx"))
        for i in range(RR.SWEEP_B):
            alone = run_resize(Rs, x[i:i + 1], dy[i:i + 1], (Hout, Wout))
            assert torch.equal(alone["y"], first["y"][i:i + 1]) and torch.equal(alone["dx"], first["dx"][i:i + 1]), i
    B, H, W = 2, 25, 26                                      # 1300 pixels: three slabs, the second one spans both images
    c = RR.conv_case(B * H * W, 72, 7, "random", PREC[dtype])
    x, w, b, dy = conv_tensors(c, dtype, B, H, W)
    first = run_conv(Rs, x, w, b, dy)
    assert same_bits(run_conv(Rs, x, w, b, dy), first, ("y", "dx", "dw", "db"))
    for i in range(B):
        alone = run_conv(Rs, x[i:i + 1], w, b, dy[i:i + 1])
        assert torch.equal(alone["y"], first["y"][i:i + 1]) and torch.equal(alone["dx"], first["dx"][i:i + 1]), i


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "fp16"])
@pytest.mark.parametrize("layout", ["nchw", "channels_last"])
def test_the_public_conv_equals_the_low_level_calls_and_skips_what_is_not_needed(Rs, layout, dtype):
    B, H, W, Cin, Cout = 2, 9, 11, 32, 3
    c = RR.conv_case(B * H * W, Cin, Cout, "random", PREC[dtype])
    x, w, b, dy = conv_tensors(c, dtype, B, H, W)
    base = run_conv(Rs, x, w, b, dy)
    names = ("y", "dx", "dw", "db")

    def arrange(t):
        t = t.permute(0, 3, 1, 2)
        return t.contiguous() if layout == "nchw" else t.contiguous(memory_format=torch.channels_last)

    def through_autograd(need):
        xl, wl, bl = (t.clone(memory_format=torch.preserve_format).requires_grad_(n) for t, n in zip((arrange(x), w, b), need))
        y = Rs.conv1x1_narrow(xl, wl, bl)
        assert y.shape == (B, Cout, H, W) and y.dtype == dtype and y.is_contiguous(memory_format=torch.channels_last) and y.requires_grad == any(need)
        if any(need):
            y.backward(arrange(dy))
        return {"y": y.detach().permute(0, 2, 3, 1), "dx": xl.grad if xl.grad is None else xl.grad.permute(0, 2, 3, 1), "dw": wl.grad, "db": bl.grad}

    assert same_bits(through_autograd((True, True, True)), base, names)
    for skip in range(3):                                    # each gradient skipped alone: it is None, the others keep their bits
        got = through_autograd(tuple(i != skip for i in range(3)))
        assert got[names[1 + skip]] is None and same_bits(got, base, [n for i, n in enumerate(names) if i != 1 + skip])
    y = Rs.conv1x1_narrow(arrange(x), w)                     # no bias, no gradient
    assert not y.requires_grad and torch.equal(y.permute(0, 2, 3, 1), Rs.conv_forward(x, w))
    db = nan(Cout, dtype=dtype)                              # db alone needs neither x nor w; without a Cin its row lanes are those of one chunk, so
    Rs.conv_backward(None, None, dy, db=db)                  # it is held to the bound, not to the bits of the call above
    check({"db": db}, c["ref"], f"db alone {dtype}", ("db",))
    again = nan(Cout, dtype=dtype)
    Rs.conv_backward(None, None, dy, db=again)
    assert torch.equal(db, again)
    we, be = w.clone().requires_grad_(True), b.clone().requires_grad_(True)          # B = 0: nothing is launched, the parameter gradients are zero
    e = Rs.conv1x1_narrow(arrange(x)[:0], we, be)
    e.sum().backward()
    assert e.shape == (0, Cout, H, W) and not we.grad.any() and not be.grad.any()
    z = Rs.interpolate(arrange(dy)[:0], size=(4, 5))
    assert z.shape == (0, Cout, 4, 5)


def test_autocast(Rs):
    x = torch.randn(2, 32, 9, 10, device="cuda", requires_grad=True)
    m = Rs.wrap_conv1x1_narrow(nn.Conv2d(32, 3, 1).cuda())
    with torch.autocast("cuda", dtype=torch.bfloat16):
        with pytest.raises(NotImplementedError, match="moge_amd.resample.*bfloat16"):
            m(x)
        assert Rs.interpolate(x, scale_factor=2).dtype == torch.float32          # interpolate is not cast, as torch's is not
    with torch.autocast("cuda", dtype=torch.float16):
        y = m(x)
        up = Rs.interpolate(y, size=(13, 17))
        assert Rs.interpolate(x, scale_factor=2).dtype == torch.float32
    assert y.dtype == up.dtype == torch.float16 and up.shape == (2, 3, 13, 17)
    up.backward(torch.ones_like(up))
    assert x.grad.dtype == m.weight.grad.dtype == m.bias.grad.dtype == torch.float32
    want = F.conv2d(x.detach().half(), m.weight.detach().half(), m.bias.detach().half())
    assert float((y.detach().float() - want.float()).abs().max()) <= 2.0 ** -9 * float(want.float().abs().max())
    xg = x.detach().requires_grad_(True)                     # double backward is not built: once_differentiable refuses it
    yg = Rs.interpolate(xg, scale_factor=2)
    (g,) = torch.autograd.grad(yg, xg, grad_outputs=torch.ones_like(yg).requires_grad_(True), create_graph=True)
    with pytest.raises(RuntimeError, match="once_differentiable"):
        g.sum().backward()


# ---- through autograd: level 4 of a head -------------------------------------------------------------------------------------------------------
class Level4(nn.Module):
    """The exit of a head: the bilinear x2 resampler, its 3x3 conv 64 -> 32, the 1x1 output conv 32 -> 3 and the resize to the image (an odd size)."""

    def __init__(self):
        super().__init__()
        self.up, self.conv3, self.exit = nn.Upsample(scale_factor=2, mode="bilinear", align_corners=False), conv(64, 32), nn.Conv2d(32, 3, 1)
        self.interpolate, self.size = F.interpolate, (41, 37)

    def forward(self, x):
        return self.interpolate(self.exit(torch.relu(self.conv3(self.up(x)))), self.size, mode="bilinear", align_corners=False)


def level4():
    torch.manual_seed(7)
    return Level4()


def hip_model(Rs, level):
    from moge_amd import conv as Cv
    model = model_of(Block())
    model.neck = level
    Rs.use_hip_resample(Cv.use_hip_conv(model))
    (level.module if isinstance(level, Checkpointed) else level).interpolate = Rs.interpolate          # the function call no walker reaches
    return model


def step(model, x, gy, autocast):
    xg = x.clone().requires_grad_(True)
    with torch.autocast("cuda", dtype=torch.float16, enabled=autocast):
        y = model(xg)
    y.backward(gy.to(y.dtype))
    return {"y": y.detach(), "x": xg.grad, **{n: p.grad for n, p in model.named_parameters()}}


@pytest.mark.parametrize("autocast", [False, True], ids=["fp32", "autocast-fp16"])
def test_level_4_of_a_head_trains_a_step_through_this_library(Rs, autocast, monkeypatch):
    level = level4()
    x, gy = torch.randn(2, 64, 17, 18), torch.randn(2, 3, 41, 37)
    ref_level = copy.deepcopy(level).double()
    if autocast:                                             # the float64 copy evaluated as fp16 autocast defines it: the convs' tensors
        P = Fp16Point.apply                                  # are fp16 values, and so is the resize of the fp16 output; the x2 stays in the input's fp32
        ref_level.conv3.forward = lambda t, m=ref_level.conv3: P(m._conv_forward(P(t), P(m.weight), P(m.bias)))
        ref_level.exit.forward = lambda t, m=ref_level.exit: P(m._conv_forward(P(t), P(m.weight), P(m.bias)))
        ref_level.interpolate = lambda *a, **k: P(F.interpolate(*a, **k))
    want = step(ref_level, x.double(), gy.double(), False)
    torch_own = step(copy.deepcopy(level).cuda(), x.cuda(), gy.cuda(), autocast)          # torch's own kernels on the same stand-in: the measure if a band fails

    model = hip_model(Rs, level.cuda())
    assert [type(m).__name__ for m in (level.up, level.conv3, level.exit)] == ["HipUpsample", "HipConv3x3", "HipConv1x1Narrow"]
    for name in ("conv2d", "interpolate", "upsample"):
        monkeypatch.setattr(F, name, lambda *a, name=name, **k: (_ for _ in ()).throw(AssertionError(f"torch's own {name} was called inside the level")))
    got = step(model.neck, x.cuda(), gy.cuda(), autocast)
    monkeypatch.undo()
    assert set(got) == set(want) and len(want) == 2 + 4
    err = {n: float((got[n].double().cpu() - want[n]).abs().max() / want[n].abs().max()) for n in want}
    own = {n: float((torch_own[n].double().cpu() - want[n]).abs().max() / want[n].abs().max()) for n in want}
    print(f"level 4 autocast={autocast} this library:", " ".join(f"{n}={e:.3e}" for n, e in err.items()))
    print(f"level 4 autocast={autocast} torch's own: ", " ".join(f"{n}={e:.3e}" for n, e in own.items()))
    for n in want:
        assert got[n].dtype == (torch.float16 if autocast and n == "y" else torch.float32) and got[n].shape == want[n].shape and err[n] < BAND[autocast], (n, err[n], own[n])


def test_the_level_under_checkpointing_gives_the_same_bits(Rs):
    plain, wrapped = hip_model(Rs, level4().cuda()), hip_model(Rs, Checkpointed(level4().cuda()))
    x, gy = torch.randn(2, 64, 17, 18, device="cuda"), torch.randn(2, 3, 41, 37, device="cuda")
    for autocast in (False, True):
        a, b = step(plain.neck, x, gy, autocast), step(wrapped.neck, x, gy, autocast)
        assert len(a) == len(b) == 2 + 4 and all(torch.equal(a[n], b["module." + n if n not in ("y", "x") else n]) for n in a)
        for m in (plain, wrapped):
            m.zero_grad(set_to_none=True)
