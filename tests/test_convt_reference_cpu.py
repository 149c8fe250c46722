"""CPU: the float64 references of tests/convt_reference.py are the right ones (torch's float64 autograd of F.conv_transpose2d(x, w, b, stride=2)),
their bounds hold an honest fp32 emulation that tiles and splits in another order than the kernels, and each of a list of injected faults - what
csrc/convt_grad.hip could get wrong in its row map, its taps or its tails - lands OUTSIDE a bound on the inputs chosen here.  No GPU, no library."""
import numpy as np
import pytest
import torch
from torch.nn import functional as F

import convt_reference as TR
from convt_reference import to_storage

PRECS = [0, 1]
NAMES = ("y", "dx", "dw", "db")


def rounded(v, prec):
    """fp32 -> storage type -> float64: the kernel's single rounding of a result."""
    return to_storage(np.asarray(v, dtype=np.float32), prec)


def inside(got, ref_bound):
    ref, bound = ref_bound
    return bool((np.abs(got - ref) <= bound).all())


@pytest.mark.parametrize("H,W", TR.HW)
def test_references_agree_with_torch_float64_autograd(H, W):
    for Cin, Cout in TR.sweep_channels(0):
        c = TR.case(TR.SWEEP_B, H, W, Cin, Cout, "coded", 0)
        x = torch.tensor(c["x"], dtype=torch.float64).permute(0, 3, 1, 2).requires_grad_(True)
        w, b = (torch.tensor(c[n], dtype=torch.float64, requires_grad=True) for n in ("w", "b"))
        y = F.conv_transpose2d(x, w, b, stride=2)
        y.backward(torch.tensor(c["dy"], dtype=torch.float64).permute(0, 3, 1, 2))
        for name, t in (("y", y.detach().permute(0, 2, 3, 1)), ("dx", x.grad.permute(0, 2, 3, 1)), ("dw", w.grad), ("db", b.grad)):
            ref, bound = c["ref"][name]
            assert ref.shape == tuple(t.shape) and np.abs(ref - t.numpy()).max() <= 1e-12 * max(1.0, np.abs(ref).max()), (name, Cin, Cout)
            assert (bound > 0).all(), name
    assert "db" not in TR.convt(c["x"], c["w"], None, c["dy"], 0)


def test_the_taps_of_the_weights_differ():
    """A tap swap is invisible on weights whose four taps are equal, which is how the reference model initialises them."""
    for family in TR.FAMILIES:
        w = TR.case(TR.SWEEP_B, 2, 2, 72, 72, family, 1)["w"].astype(np.float64)
        taps = [w[:, :, i, j] for i in (0, 1) for j in (0, 1)]
        assert all(np.abs(a - b).max() > 0.1 for k, a in enumerate(taps) for b in taps[k + 1:]), family


def emulate(c, prec, kt=24, splits=3):
    """fp32 arithmetic in another order than the kernels': taps outermost in reverse, channel tiles of `kt`, the input gradient as a sum of four
    per-tap fp32 products, the weight and bias gradients as `splits` fp32 partials over the pixels added afterwards, one rounding to the storage
    type at the end."""
    x, w, b, dy = (c[n].astype(np.float32) for n in ("x", "w", "b", "dy"))
    B, H, W, Cin = x.shape
    Cout = w.shape[1]
    taps = [(1, 1), (1, 0), (0, 1), (0, 0)]

    def tiled(a, bt):                                  # a (..., C) . bt (J, C)^T with fp32 partial sums per tile of C
        acc = np.zeros(a.shape[:-1] + (bt.shape[0],), dtype=np.float32)
        for k0 in range(0, a.shape[-1], kt):
            acc = acc + a[..., k0:k0 + kt] @ bt[:, k0:k0 + kt].T
        return acc

    y, dx = np.zeros((B, 2 * H, 2 * W, Cout), dtype=np.float32), np.zeros((B, H, W, Cin), dtype=np.float32)
    dw, db = np.zeros((Cin, Cout, 2, 2), dtype=np.float32), np.zeros(Cout, dtype=np.float32)
    edges = np.linspace(0, B * H * W, splits + 1).astype(int)
    xs = x.reshape(-1, Cin)
    for i, j in taps:
        y[:, i::2, j::2] = tiled(x, np.ascontiguousarray(w[:, :, i, j].T)) + b
        dx = dx + tiled(dy[:, i::2, j::2], w[:, :, i, j])
        dys = dy[:, i::2, j::2].reshape(-1, Cout)
        for r0, r1 in zip(edges[:-1], edges[1:]):
            dw[:, :, i, j] = dw[:, :, i, j] + (xs[r0:r1].T @ dys[r0:r1]).astype(np.float32)
    rows = dy.reshape(-1, Cout)
    for r0, r1 in zip(4 * edges[:-1], 4 * edges[1:]):
        db = db + rows[r0:r1].sum(0, dtype=np.float32)
    return {"y": rounded(y, prec), "dx": rounded(dx, prec), "dw": rounded(dw, prec), "db": rounded(db, prec)}


@pytest.mark.parametrize("prec", PRECS, ids=["fp32", "fp16"])
@pytest.mark.parametrize("H,W", TR.HW)
def test_an_honest_fp32_emulation_stays_inside_every_bound(H, W, prec):
    for Cin, Cout in TR.sweep_channels(prec):
        for family in TR.FAMILIES:
            c = TR.case(TR.SWEEP_B, H, W, Cin, Cout, family, prec)
            got = emulate(c, prec)
            for name in NAMES:
                ref, bound = c["ref"][name]
                frac = float((np.abs(got[name] - ref) / bound).max())
                print(f"emulation {H}x{W} {Cin}->{Cout} {family} prec{prec} {name}: worst error / bound = {frac:.3f}")
                assert frac <= 1.0, (name, Cin, Cout, family)


def hi_index(B, H, W, image_stride, row_stride):
    """[b,p,q,i,j] -> the flat high-resolution pixel b image_stride + (2p + i) row_stride + 2q + j; right: image_stride = 2H 2W, row_stride = 2W."""
    b, p, q, i, j = np.ogrid[:B, :H, :W, :2, :2]
    return b * image_stride + (2 * p + i) * row_stride + 2 * q + j


def scattered(y, idx):
    """The forward's store through another row map: y (B,2H,2W,Cout) written to the flat pixels idx[b,p,q,i,j] (a later write wins, a pixel that is
    never written stays zero, a write past the tensor is dropped)."""
    vals = TR.taps_of(y).reshape(-1, y.shape[-1])
    out = np.zeros((y.shape[0] * y.shape[1] * y.shape[2], y.shape[-1]))
    flat = idx.reshape(-1)
    ok = flat < out.shape[0]
    out[flat[ok]] = vals[ok]
    return out.reshape(y.shape)


def gathered(dy, idx):
    """The gradient as a wrong row map would gather it: [b,2p+i,2q+j] = dy at the flat pixel idx[b,p,q,i,j] (the last pixel where that is past the end)."""
    B, H2, W2, Cout = dy.shape
    g = dy.reshape(-1, Cout)[np.minimum(idx, B * H2 * W2 - 1)]                   # (B,H,W,2,2,Cout)
    return g.transpose(0, 1, 3, 2, 4, 5).reshape(dy.shape)


@pytest.mark.parametrize("prec", PRECS, ids=["fp32", "fp16"])
@pytest.mark.parametrize("H,W", [(16, 17), (2, 2), (1, 17)])
def test_injected_faults_land_outside_the_bounds(H, W, prec):
    Cin = Cout = 72                                     # Cin = Cout: the swapped-channel fault keeps its shapes
    B = TR.SWEEP_B
    for family in ("coded", "offset"):
        c = TR.case(B, H, W, Cin, Cout, family, prec)
        x, w, b, dy = (c[n].astype(np.float64) for n in ("x", "w", "b", "dy"))
        ref = c["ref"]
        good = {n: ref[n][0] for n in NAMES}
        for name in NAMES:                              # the exact value, rounded once, is inside: the faults below are what moves it out
            assert inside(rounded(good[name], prec), ref[name]), name
        right = hi_index(B, H, W, 4 * H * W, 2 * W)
        assert np.array_equal(scattered(good["y"], right), good["y"]) and np.array_equal(gathered(dy, right), dy)
        wt = np.ascontiguousarray(w.transpose(0, 1, 3, 2))                  # i and j swapped
        wc = np.ascontiguousarray(w.transpose(1, 0, 2, 3))                  # the channel roles swapped
        w3 = w.copy()
        w3[:, :, 1, 1] = 0.0
        last = (np.arange(B)[:, None, None, None] == B - 1) & (np.arange(H)[None, :, None, None] == H - 1)      # the last image's last row
        half_rows, no_image = hi_index(B, H, W, 4 * H * W, W), hi_index(B, H, W, 2 * H * W, 2 * W)
        faults = {
            "i and j swapped in the forward": ("y", TR.convt2x2(x, wt, b, prec)[0]),
            "i and j swapped in the dgrad": ("dx", TR.dgrad_core(dy, wt)),
            "i and j swapped in the wgrad": ("dw", good["dw"].transpose(0, 1, 3, 2)),
            "the weight's channel roles swapped in the forward": ("y", TR.convt2x2(x, wc, b, prec)[0]),
            "the weight's channel roles swapped in the dgrad": ("dx", TR.dgrad_core(dy, wc)),
            "the weight's channel roles swapped in the wgrad": ("dw", good["dw"].transpose(1, 0, 2, 3)),
            "the output row computed with stride W instead of 2W": ("y", scattered(good["y"], half_rows)),
            "the gradient row computed with stride W instead of 2W": ("dx", TR.dgrad_core(gathered(dy, half_rows), w)),
            "a tap dropped from the dgrad": ("dx", TR.dgrad_core(dy, w3)),
            "the last pixels dropped from the wgrad": ("dw", TR.wgrad_core(dy, np.where(last, 0.0, x))),
            "db over B H W instead of 4 B H W pixels": ("db", dy[:, ::2, ::2].sum((0, 1, 2))),
            "the bias missing": ("y", good["y"] - b),
            "a row map that ignores the image index in the forward": ("y", scattered(good["y"], no_image)),
            "a row map that ignores the image index in the dgrad": ("dx", TR.dgrad_core(gathered(dy, no_image), w)),
            "a row map that ignores the image index in the wgrad": ("dw", TR.wgrad_core(gathered(dy, no_image), x)),
        }
        for what, (name, value) in faults.items():
            assert value.shape == good[name].shape, what
            assert not inside(rounded(value, prec), ref[name]), (what, family, H, W)


def cancelling_case(prec, B=2, H=16, W=16, Cin=32, Cout=32):
    """The weight gradient as two partials over the images that nearly cancel: dy = +1 on the first image, -1 (both plus noise) on the second, x
    positive.  Each partial is ~ B H W / 2 times the sum it leaves, so a rounding of the PARTIALS to fp16 is far more than the rounding of the sum."""
    rng = np.random.default_rng(7)
    x = to_storage(1.0 + 0.25 * rng.standard_normal((B, H, W, Cin)), prec)
    dy = to_storage(np.where(np.arange(B)[:, None, None, None] < B // 2, 1.0, -1.0) + 0.05 * rng.standard_normal((B, 2 * H, 2 * W, Cout)), prec)
    w = to_storage(rng.standard_normal((Cin, Cout, 2, 2)) / 8.0, prec)
    b = to_storage(rng.standard_normal(Cout), prec)
    return dict(x=x, w=w, b=b, dy=dy, ref=TR.convt(x, w, b, dy, prec))


@pytest.mark.parametrize("prec", PRECS, ids=["fp32", "fp16"])
def test_partials_rounded_to_fp16_land_outside_the_bound(prec):
    c = cancelling_case(prec)
    x, dy = c["x"], c["dy"]
    parts = [TR.wgrad_core(dy[:1], x[:1]), TR.wgrad_core(dy[1:], x[1:])]
    f32 = lambda v: v.astype(np.float32).astype(np.float64)          # noqa: E731
    assert inside(rounded(f32(parts[0]) + f32(parts[1]), prec), c["ref"]["dw"])
    ref, bound = c["ref"]["dw"]
    frac = float((np.abs(rounded(to_storage(parts[0], 1) + to_storage(parts[1], 1), prec) - ref) / bound).max())
    print(f"wgrad partials rounded to fp16, prec{prec}: worst error / bound = {frac:.2f}")
    assert frac > 1.0


def test_the_larger_shapes_are_what_their_names_say():
    for prec in PRECS:
        B, H, W, Cin, Cout = TR.SPLIT
        (s, per), kt = TR.split_of(B * H * W, Cin, Cout, prec), TR.k_tile(prec)
        tiles = -(-B * H * W // kt)
        assert s == TR.SPLIT_S[prec] > 1 and (s - 1) * per < tiles and B * H * W % kt and tiles % per      # every part has work, the last one less, and a partial K tile
        B, H, W, Cin, Cout = TR.ROWS
        assert W > 2 * TR.PIXEL_TILE and W % TR.PIXEL_TILE and B * H * W % TR.PIXEL_TILE                   # several pixel tiles per image row, none ends with a row
        assert TR.expected_split(TR.SWEEP_B * 33 * 18, 136, 72, prec) >= 1
