"""CPU: the float64 references of tests/resample_reference.py agree with torch's float64 autograd (F.interpolate(size=...), nn.Upsample(scale_factor=2),
F.conv2d) at every sweep shape; an fp32 / fp16 emulation of the kernels' order of operations lies inside every bound; a list of injected faults lies
outside.  The emulation is written from csrc/resample_grad.hip: the one coordinate function (fp32, one fma), the gather over the first[] tables with
rows outer and columns inner, the quad sum of the narrow conv's forward, the row lanes and the slabs of its weight gradient.  No GPU, no library call."""
import numpy as np
import pytest
import torch
from torch import nn
from torch.nn import functional as F

import resample_reference as RR

PRECS = (0, 1)
f32 = np.float32


def fma(a, b, c):
    """fp32 fused multiply-add: the product is exact in float64, the sum is rounded there first (53 bits) and then to fp32."""
    return (np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(f32)


def inside(got, ref_bound, what):
    ref, bound = ref_bound
    frac = float((np.abs(np.asarray(got, np.float64).reshape(ref.shape) - ref) / np.maximum(bound, 1e-300)).max())
    assert np.isfinite(got).all() and frac <= 1.0, (what, frac)
    return frac


def outside(got, ref_bound, what):
    ref, bound = ref_bound
    err = np.abs(np.asarray(got, np.float64).reshape(ref.shape) - ref)
    assert not (np.nan_to_num(err, nan=np.inf) <= bound).all(), what


# ---- the references against torch ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", RR.RESIZE, ids=lambda s: f"{s[0][0]}x{s[0][1]}-{s[1][0]}x{s[1][1]}")
def test_resize_reference_is_torchs_float64_autograd(shape):
    (Hin, Win), (Hout, Wout) = shape
    for C in (1, 3):
        x, dy = RR.resize_inputs(RR.SWEEP_B, Hin, Win, Hout, Wout, C)
        ref = RR.resize(x, (Hout, Wout), dy, 0)
        xt = torch.from_numpy(x).double().permute(0, 3, 1, 2).requires_grad_(True)
        forms = [lambda t: F.interpolate(t, size=(Hout, Wout), mode="bilinear", align_corners=False, antialias=False)]
        if shape in RR.X2:
            forms.append(nn.Upsample(scale_factor=2, mode="bilinear", align_corners=False))
            by_scale = RR.resize(x, (Hout, Wout), dy, 0, scales=(0.5, 0.5))
            assert all(np.array_equal(by_scale[n][0], ref[n][0]) and np.array_equal(by_scale[n][1], ref[n][1]) for n in ref)
        for form in forms:
            xt.grad = None
            yt = form(xt)
            yt.backward(torch.from_numpy(dy).double().permute(0, 3, 1, 2))
            assert np.abs(yt.detach().permute(0, 2, 3, 1).numpy() - ref["y"][0]).max() <= 1e-12
            assert np.abs(xt.grad.permute(0, 2, 3, 1).numpy() - ref["dx"][0]).max() <= 1e-12
    if shape == RR.IDENTITY:
        assert np.array_equal(ref["y"][0], x.astype(np.float64))
    rows = RR.EMPTY_ROWS.get(shape)
    if rows is not None:                                   # input rows no output reads: exactly zero, and a zero bound - but for rows 7 and 9 beside
        empty = [r for r in range(Hin) if not np.abs(ref["dx"][0][:, r]).any()]          # s(1) = 8 of 17 -> 3: a computed s just off 8 reaches one of them with a weight of delta
        assert len(empty) == rows and sum(not ref["dx"][1][:, r].any() for r in empty) == rows - 2 * (shape == ((17, 17), (3, 3)))
        t = RR.first_table(Hin, Hout)
        assert sum(t[r + 1] == t[max(r - 1, 0)] for r in range(Hin)) == rows - (shape == ((17, 17), (3, 3)))       # row 9 is in the range of s(1) = 8, with l1 = 0


def test_the_first_table_is_the_gather_form_of_the_transpose():
    for (Hin, _), (Hout, _) in RR.RESIZE:
        s, i0, i1, l0, l1 = RR.taps(Hin, Hout)
        t = RR.first_table(Hin, Hout)
        assert t[0] == 0 and t[Hin] == Hout and (np.diff(t) >= 0).all()
        A = np.zeros((Hout, Hin))
        for r in range(Hin):
            for o in range(t[max(r - 1, 0)], t[r + 1]):
                A[o, r] = (l0[o] + (l1[o] if r == Hin - 1 else 0.0)) if o >= t[r] else l1[o]
        assert np.array_equal(A, RR.axis_matrix(Hin, Hout))


@pytest.mark.parametrize("prec", PRECS, ids=["fp32", "fp16"])
def test_conv_reference_is_torchs_float64_autograd(prec):
    for M in RR.CONV_M:
        for Cin, Cout in RR.conv_channels(prec):
            c = RR.conv_case(M, Cin, Cout, "random", prec)
            x = torch.from_numpy(c["x"]).double().t().reshape(1, Cin, 1, M).requires_grad_(True)
            w = torch.from_numpy(c["w"]).double().reshape(Cout, Cin, 1, 1).requires_grad_(True)
            b = torch.from_numpy(c["b"]).double().requires_grad_(True)
            y = F.conv2d(x, w, b)
            y.backward(torch.from_numpy(c["dy"]).double().t().reshape(1, Cout, 1, M))
            got = {"y": y.detach()[0, :, 0].t(), "dx": x.grad[0, :, 0].t(), "dw": w.grad[:, :, 0, 0], "db": b.grad}
            for n, g in got.items():
                ref = c["ref"][n][0]
                assert np.abs(g.numpy() - ref).max() <= 1e-12 * max(1.0, np.abs(ref).max()), (M, Cin, Cout, n)


# ---- the kernels' order, emulated; `fault` switches one thing wrong ------------------------------------------------------------------------------
def coord(o, sigma, fault=None, exact=False):
    """rs_coord: fmaxf(__fmaf_rn(sigma, (float)o + 0.5f, -0.5f), 0.f); exact: the same in float64."""
    o = np.asarray(o)
    half_in, half_out = (0.0 if fault == "no+0.5" else 0.5), (0.0 if fault == "no-0.5" else 0.5)
    s = sigma * (o + half_in) - half_out if exact else fma(f32(sigma), (o.astype(f32) + f32(half_in)), f32(-half_out))
    return s if fault == "no_clamp0" else np.maximum(s, 0)


def tap(o, sigma, n_in, fault=None, exact=False):
    s = coord(o, sigma, fault, exact)
    i0 = np.minimum(np.floor(s).astype(np.int64), n_in - 1)
    i1 = i0 + 1 if fault == "i1_unclamped" else np.minimum(i0 + 1, n_in - 1)
    l1 = s - i0 if exact else (s - i0.astype(f32)).astype(f32)
    l0 = 1.0 - l1 if exact else (f32(1) - l1).astype(f32)
    return i0, i1, l0, l1


def emulate_forward(x, size, scales, fault=None, exact=False):
    """x (B, Hin, Win, C) -> y; memory is flat, so an index past a row or an image reads what lies there (the next row, the next image; the end wraps)."""
    B, Hin, Win, C = x.shape
    (Hout, Wout), (sh, sw) = size, scales
    if fault == "inverted":
        sh, sw = 1.0 / sh, 1.0 / sw
    if fault == "hw_swapped":
        sh, sw = sw, sh
    h0, h1, lh0, lh1 = tap(np.arange(Hout), sh, Hin, fault, exact)
    w0, w1, lw0, lw1 = tap(np.arange(Wout), sw, Win, fault, exact)
    flat = x.reshape(-1, C)

    def at(ih, iw):
        idx = (np.arange(B)[:, None, None] * Hin + ih[None, :, None]) * Win + iw[None, None, :]
        return flat[idx % flat.shape[0]]
    lw0, lw1, lh0, lh1 = lw0[None, None, :, None], lw1[None, None, :, None], lh0[None, :, None, None], lh1[None, :, None, None]
    if exact:
        return lh0 * (lw0 * at(h0, w0) + lw1 * at(h0, w1)) + lh1 * (lw0 * at(h1, w0) + lw1 * at(h1, w1))
    top = fma(lw1, at(h0, w1), (lw0 * at(h0, w0)).astype(f32))
    bot = fma(lw1, at(h1, w1), (lw0 * at(h1, w0)).astype(f32))
    return fma(lh1, bot, (lh0 * top).astype(f32))


def table(n_in, n_out, sigma, exact):
    i0 = tap(np.arange(n_out), sigma, n_in, None, exact)[0]
    return np.array([int(np.searchsorted(i0, r, side="left")) for r in range(n_in + 1)])


def emulate_backward(dy, size, scales, fault=None, exact=False):
    """dy (B, Hout, Wout, C) -> dx (B, Hin, Win, C): resize_bilinear_grad_kernel's gather, rows outer, columns inner, both ascending."""
    B, Hout, Wout, C = dy.shape
    (Hin, Win), (sh, sw) = size, scales
    th, tw = table(Hin, Hout, sh, exact), table(Win, Wout, sw, exact)
    dt = np.float64 if exact else f32
    mad = (lambda a, b, c: a * b + c) if exact else fma
    dx = np.ones((B, Hin, Win, C), dt) if fault == "empty_unwritten" else np.zeros((B, Hin, Win, C), dt)
    lo, hi = (1 if fault == "range_lo+1" else 0), (1 if fault == "range_hi-1" else 0)

    def weight(o, sigma, n_in, own, last):
        _, _, l0, l1 = tap(np.array([o]), sigma, n_in, None, exact)
        return ((l0[0] + l1[0]) if last and fault != "no_double" else l0[0]) if own else l1[0]
    for r in range(Hin):
        oa, om, ob = th[max(r - 1, 0)] + lo, th[r], th[r + 1] - hi
        for q in range(Win):
            pa, pm, pb = tw[max(q - 1, 0)] + lo, tw[q], tw[q + 1] - hi
            if fault == "empty_unwritten" and (oa >= ob or pa >= pb):
                continue
            acc = np.zeros((B, C), dt)
            for o in range(oa, ob):
                inner = np.zeros((B, C), dt)
                for p in range(pa, pb):
                    inner = mad(dt(weight(p, sw, Win, p >= pm, q == Win - 1)), dy[:, o, p].astype(dt), inner)
                acc = mad(dt(weight(o, sh, Hin, o >= om, r == Hin - 1)), inner, acc)
            dx[:, r, q] = acc
    return dx


def stored(v, prec):
    return np.asarray(v, f32).astype(np.float16).astype(np.float64) if prec == 1 else np.asarray(v, np.float64)


@pytest.mark.parametrize("prec", PRECS, ids=["fp32", "fp16"])
@pytest.mark.parametrize("shape", RR.RESIZE, ids=lambda s: f"{s[0][0]}x{s[0][1]}-{s[1][0]}x{s[1][1]}")
def test_an_emulation_of_the_resize_kernels_lies_inside_the_bounds(shape, prec):
    (Hin, Win), (Hout, Wout) = shape
    c = RR.resize_case(RR.SWEEP_B, Hin, Win, Hout, Wout, 3, prec)
    scales = (Hin / Hout, Win / Wout)
    y = emulate_forward(c["x"], (Hout, Wout), scales)
    inside(stored(y, prec), c["ref"]["y"], ("y", shape))
    inside(stored(emulate_backward(c["dy"], (Hin, Win), scales), prec), c["ref"]["dx"], ("dx", shape))
    if shape == RR.IDENTITY:
        assert np.array_equal(y, c["x"])
    # ... and the float64 form of the same code is the reference, so the faults below differ from it by their fault alone
    assert np.abs(emulate_forward(c["x"].astype(np.float64), (Hout, Wout), scales, exact=True) - c["ref"]["y"][0]).max() <= 1e-12
    assert np.abs(emulate_backward(c["dy"].astype(np.float64), (Hin, Win), scales, exact=True) - c["ref"]["dx"][0]).max() <= 1e-12


UP_NONSQUARE = (((3, 4), (6, 8)), ((7, 5), (16, 9)), ((5, 7), (4, 23)))
FORWARD_FAULTS = {"inverted": UP_NONSQUARE, "no+0.5": UP_NONSQUARE, "no-0.5": UP_NONSQUARE, "no_clamp0": UP_NONSQUARE, "i1_unclamped": UP_NONSQUARE,
                  "hw_swapped": UP_NONSQUARE[1:]}               # the two scales differ there
BACKWARD_FAULTS = {"range_lo+1": UP_NONSQUARE, "range_hi-1": UP_NONSQUARE, "no_double": UP_NONSQUARE, "empty_unwritten": tuple(RR.EMPTY_ROWS)}


@pytest.mark.parametrize("prec", PRECS, ids=["fp32", "fp16"])
@pytest.mark.parametrize("fault", list(FORWARD_FAULTS) + list(BACKWARD_FAULTS))
def test_injected_resize_faults_lie_outside_the_bounds(fault, prec):
    for shape in {**FORWARD_FAULTS, **BACKWARD_FAULTS}[fault]:
        (Hin, Win), (Hout, Wout) = shape
        c = RR.resize_case(RR.SWEEP_B, Hin, Win, Hout, Wout, 3, prec)
        scales = (Hin / Hout, Win / Wout)
        if fault in FORWARD_FAULTS:
            outside(stored(emulate_forward(c["x"], (Hout, Wout), scales, fault), prec), c["ref"]["y"], (fault, shape))
        else:
            outside(stored(emulate_backward(c["dy"], (Hin, Win), scales, fault), prec), c["ref"]["dx"], (fault, shape))


# ---- the narrow conv ---------------------------------------------------------------------------------------------------------------------------
def emulate_conv(x, w, b, dy, prec, fault=None):
    """x (M, Cin), w (Cout, Cin), b (Cout,), dy (M, Cout) fp32 arrays of storage values -> y, dx, dw, db in the kernels' order."""
    M, Cin = x.shape
    Cout, ch = w.shape[0], RR.CR.chunk(prec)
    nch = Cin // ch
    lanes = []
    for lane in range(4):                                  # conv1x1n_kernel: lane l of the quad takes the chunks l, l + 4, ...
        acc = np.zeros((M, Cout), f32)
        for j in range(lane, nch, 4):
            for e in range(j * ch, (j + 1) * ch):
                acc = fma(x[:, e:e + 1], w[None, :, e], acc)
        lanes.append(acc)
    y = ((lanes[0] + lanes[1]).astype(f32) + (lanes[2] + lanes[3]).astype(f32)).astype(f32)
    if fault != "no_bias":
        y = (y + b[None, :]).astype(f32)
    dx = np.zeros((M, Cin), f32)
    for o in range(Cout):                                  # conv1x1n_dgrad_kernel: a chain over o
        dx = fma(dy[:, o:o + 1], w[o][None, :], dx)
    R = 256 // nch                                         # conv1x1n_wgrad_kernel: row lanes, then the slabs in order
    slabs, per = RR.slabs_of(M)
    rows = M - 1 if fault == "db_short" else M
    dw, db = None, None
    for z in range(slabs):
        beg, end = z * per, min(M, (z + 1) * per)
        pw, pb = None, None
        for r in range(min(R, end - beg)):
            aw, ab = np.zeros((Cout, Cin), f32), np.zeros(Cout, f32)
            for m in range(beg + r, end, R):
                aw = fma(dy[m][:, None], x[m][None, :], aw)
                if m < rows:
                    ab = (ab + dy[m]).astype(f32)
            pw, pb = (aw, ab) if pw is None else ((pw + aw).astype(f32), (pb + ab).astype(f32))
        if fault == "fp16_partials":
            pw, pb = pw.astype(np.float16).astype(f32), pb.astype(np.float16).astype(f32)
        dw, db = (pw, pb) if dw is None else ((dw + pw).astype(f32), (db + pb).astype(f32))
    if fault == "dw_transposed":
        dw = dw.T.copy()
    return {"y": y, "dx": dx, "dw": dw, "db": db}


@pytest.mark.parametrize("prec", PRECS, ids=["fp32", "fp16"])
def test_an_emulation_of_the_conv_kernels_lies_inside_the_bounds(prec):
    assert RR.slabs_of(RR.RAGGED_M) == (3, 434) and RR.slabs_of(1) == (1, 1) and RR.slabs_of(512) == (1, 512) and RR.slabs_of(513) == (2, 257)
    for M in RR.CONV_M:
        for Cin, Cout in RR.conv_channels(prec):
            if M == RR.RAGGED_M and Cin > 72:
                continue                                   # a Python loop over the pixels: the split is the same at every channel count
            for family in ("random", "offset"):
                c = RR.conv_case(M, Cin, Cout, family, prec)
                got = emulate_conv(c["x"], c["w"], c["b"], c["dy"], prec)
                for n in ("y", "dx", "dw", "db"):
                    inside(stored(got[n], prec), c["ref"][n], (M, Cin, Cout, family, n))


def cancelling_case(prec):
    """Two slabs of 512 pixels whose sums of dy[:, 0] are 600.25 and -600: fp32 partials give 0.25, partials rounded to fp16 give 0 (600.25 is a tie
    between 600 and 600.5).  x = 1, so dw[0, :] and db[0] are both that sum; every value is an fp16 value."""
    Cin = RR.CR.chunk(prec)
    x, w, b = np.ones((1024, Cin), f32), np.ones((1, Cin), f32), np.zeros(1, f32)
    dy = np.concatenate([np.full(511, 1.171875), [1.421875], np.full(512, -1.171875)]).astype(f32)[:, None]
    assert dy[:512].astype(np.float64).sum() == 600.25 and dy[512:].astype(np.float64).sum() == -600.0 and np.array_equal(dy, dy.astype(np.float16).astype(f32))
    return x, w, b, dy


@pytest.mark.parametrize("prec", PRECS, ids=["fp32", "fp16"])
def test_injected_conv_faults_lie_outside_the_bounds(prec):
    ch = RR.CR.chunk(prec)
    c = RR.conv_case(129, 32, 3, "offset", prec)
    args = (c["x"], c["w"], c["b"], c["dy"], prec)
    outside(stored(emulate_conv(*args, fault="no_bias")["y"], prec), c["ref"]["y"], "no_bias")
    outside(stored(emulate_conv(*args, fault="db_short")["db"], prec), c["ref"]["db"], "db_short")
    sq = RR.conv_case(129, ch, ch, "offset", prec)         # Cout = Cin (8 or 4, within the limit): a transposed dw has the right shape
    outside(stored(emulate_conv(sq["x"], sq["w"], sq["b"], sq["dy"], prec, fault="dw_transposed")["dw"], prec), sq["ref"]["dw"], "dw_transposed")
    x, w, b, dy = cancelling_case(prec)
    ref = RR.conv1x1n(x, w, b, dy, prec)
    assert RR.slabs_of(1024) == (2, 512) and ref["db"][0][0] == 0.25
    good, bad = emulate_conv(x, w, b, dy, prec), emulate_conv(x, w, b, dy, prec, fault="fp16_partials")
    for n in ("dw", "db"):
        inside(stored(good[n], prec), ref[n], ("cancelling", n))
        outside(stored(bad[n], prec), ref[n], ("fp16_partials", n))
