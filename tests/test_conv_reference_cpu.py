"""CPU: the float64 references of tests/conv_reference.py are the right ones (torch's float64 autograd of the replicate pad followed by F.conv2d),
their bounds hold an honest fp32 emulation that tiles and splits in another order than the kernels, and each of a list of injected faults - what
csrc/conv_grad.hip could get wrong at a border or a tile edge - lands OUTSIDE a bound on the inputs chosen here.  No GPU, no library."""
import numpy as np
import pytest
import torch
from torch.nn import functional as F

import conv_reference as VR
from conv_reference import to_storage

PRECS = [0, 1]
NAMES = ("y", "dx", "dw", "db")


def rounded(v, prec):
    """fp32 -> storage type -> float64: the kernel's single rounding of a result."""
    return to_storage(np.asarray(v, dtype=np.float32), prec)


def inside(got, ref_bound):
    ref, bound = ref_bound
    return bool((np.abs(got - ref) <= bound).all())


def test_every_index_of_an_axis_has_three_pairs():
    for n in (1, 2, 3, 17):
        pairs = VR.axis_pairs(n)
        assert all(len(v) == 3 for v in pairs.values()), n
    assert sorted(VR.axis_pairs(1)[0]) == [(0, -1), (0, 0), (0, 1)]
    assert sorted(VR.axis_pairs(5)[0]) == [(0, -1), (0, 0), (1, -1)] and sorted(VR.axis_pairs(5)[4]) == [(3, 1), (4, 0), (4, 1)]
    assert sorted(VR.axis_pairs(5)[2]) == [(1, 1), (2, 0), (3, -1)]


@pytest.mark.parametrize("H,W", VR.HW)
def test_references_agree_with_torch_float64_autograd(H, W):
    for Cin, Cout in VR.sweep_channels(0):
        c = VR.case(VR.SWEEP_B, H, W, Cin, Cout, "coded", 0)
        x = torch.tensor(c["x"], dtype=torch.float64).permute(0, 3, 1, 2).requires_grad_(True)
        w, b = (torch.tensor(c[n], dtype=torch.float64, requires_grad=True) for n in ("w", "b"))
        y = F.conv2d(F.pad(x, (1, 1, 1, 1), mode="replicate"), w, b)
        y.backward(torch.tensor(c["dy"], dtype=torch.float64).permute(0, 3, 1, 2))
        for name, t in (("y", y.detach().permute(0, 2, 3, 1)), ("dx", x.grad.permute(0, 2, 3, 1)), ("dw", w.grad), ("db", b.grad)):
            ref, bound = c["ref"][name]
            assert ref.shape == tuple(t.shape) and np.abs(ref - t.numpy()).max() <= 1e-12 * max(1.0, np.abs(ref).max()), (name, Cin, Cout)
            assert (bound > 0).all(), name
    assert "db" not in VR.conv(c["x"], c["w"], None, c["dy"], 0)


def emulate(c, prec, kt=24, splits=3):
    """fp32 arithmetic in another order than the kernels': taps outermost in reverse, channel tiles of `kt`, the input gradient as an fp32 scatter,
    the weight and bias gradients as `splits` fp32 partials over the images' rows added afterwards, one rounding to the storage type at the end."""
    x, w, b, dy = (c[n].astype(np.float32) for n in ("x", "w", "b", "dy"))
    B, H, W, Cin = x.shape
    Cout = w.shape[0]
    taps = [(s, t) for s in (1, 0, -1) for t in (1, 0, -1)]

    def tiled(a, bt):                                  # a (..., C) . bt (J, C)^T with fp32 partial sums per tile of C
        acc = np.zeros(a.shape[:-1] + (bt.shape[0],), dtype=np.float32)
        for k0 in range(0, a.shape[-1], kt):
            acc = acc + a[..., k0:k0 + kt] @ bt[:, k0:k0 + kt].T
        return acc

    y, dx = np.zeros((B, H, W, Cout), dtype=np.float32), np.zeros((B, H, W, Cin), dtype=np.float32)
    for s, t in taps:
        yy, xx = VR.clamped(H, s), VR.clamped(W, t)
        y = y + tiled(x[:, yy][:, :, xx], w[:, :, s + 1, t + 1])
        np.add.at(dx, (slice(None), yy[:, None], xx[None, :]), tiled(dy, np.ascontiguousarray(w[:, :, s + 1, t + 1].T)))
    rows = dy.reshape(B * H, W, Cout)
    edges = np.linspace(0, B * H, splits + 1).astype(int)
    dw, db = np.zeros((Cout, Cin, 3, 3), dtype=np.float32), np.zeros(Cout, dtype=np.float32)
    for s, t in taps:
        xg = x[:, VR.clamped(H, s)][:, :, VR.clamped(W, t)].reshape(B * H, W, Cin)
        for r0, r1 in zip(edges[:-1], edges[1:]):
            dw[:, :, s + 1, t + 1] = dw[:, :, s + 1, t + 1] + np.einsum("rqo,rqi->oi", rows[r0:r1], xg[r0:r1]).astype(np.float32)
    for r0, r1 in zip(edges[:-1], edges[1:]):
        db = db + rows[r0:r1].sum((0, 1), dtype=np.float32)
    return {"y": rounded(y + b, prec), "dx": rounded(dx, prec), "dw": rounded(dw, prec), "db": rounded(db, prec)}


@pytest.mark.parametrize("prec", PRECS, ids=["fp32", "fp16"])
@pytest.mark.parametrize("H,W", VR.HW)
def test_an_honest_fp32_emulation_stays_inside_every_bound(H, W, prec):
    for i, (Cin, Cout) in enumerate(VR.sweep_channels(prec)):
        for family in VR.FAMILIES:
            c = VR.case(VR.SWEEP_B, H, W, Cin, Cout, family, prec)
            got = emulate(c, prec)
            for name in NAMES:
                ref, bound = c["ref"][name]
                frac = float((np.abs(got[name] - ref) / bound).max())
                print(f"emulation {H}x{W} {Cin}->{Cout} {family} prec{prec} {name}: worst error / bound = {frac:.3f}")
                assert frac <= 1.0, (name, Cin, Cout, family)


def zero_padded(x, s, t):
    """x (B,H,W,C) shifted by the tap (s, t) with ZEROS where the source pixel is outside the image."""
    B, H, W, Cc = x.shape
    big = np.zeros((B, H + 2, W + 2, Cc))
    big[:, 1:-1, 1:-1] = x
    return big[:, 1 + s:1 + s + H, 1 + t:1 + t + W]


def dgrad_parts(dy, w):
    """The input gradient as (interior, border): the zero-padded transposed conv, and the terms replicate padding sends back to the border pixels."""
    interior = np.zeros(dy.shape[:3] + (w.shape[1],))
    for s in (-1, 0, 1):
        for t in (-1, 0, 1):
            interior += zero_padded(dy, -s, -t) @ w[:, :, s + 1, t + 1]
    return interior, VR.dgrad_core(dy, w) - interior


@pytest.mark.parametrize("prec", PRECS, ids=["fp32", "fp16"])
@pytest.mark.parametrize("H,W", [(16, 17), (2, 2), (1, 17)])
def test_injected_faults_land_outside_the_bounds(H, W, prec):
    Cin = Cout = 72                                     # Cin = Cout: the swapped-tap faults keep their shapes
    B = VR.SWEEP_B
    for family in ("coded", "offset"):
        c = VR.case(B, H, W, Cin, Cout, family, prec)
        x, w, b, dy = (c[n].astype(np.float64) for n in ("x", "w", "b", "dy"))
        ref = c["ref"]
        good = {n: ref[n][0] for n in NAMES}
        for name in NAMES:                              # the exact value, rounded once, is inside: the faults below are what moves it out
            assert inside(rounded(good[name], prec), ref[name]), name
        interior, border = dgrad_parts(dy, w)
        assert np.abs(interior + border - good["dx"]).max() <= 1e-12 * np.abs(good["dx"]).max() and np.abs(border).max() > 0
        wt = np.ascontiguousarray(w.transpose(0, 1, 3, 2))                  # s and t swapped
        pix = dy.reshape(-1, Cout)
        faults = {
            "zero padding instead of replicate in the forward": ("y", sum(zero_padded(x, s, t) @ w[:, :, s + 1, t + 1].T for s in (-1, 0, 1) for t in (-1, 0, 1)) + b),
            "the dgrad as a plain zero-padded transposed conv": ("dx", interior),
            "the border terms counted twice": ("dx", interior + 2 * border),
            "s and t swapped in the forward": ("y", VR.conv3x3_core(x, wt) + b),
            "s and t swapped in the dgrad": ("dx", VR.dgrad_core(dy, wt)),
            "s and t swapped in the wgrad": ("dw", good["dw"].transpose(0, 1, 3, 2)),
            "a wgrad with zero neighbours instead of clamped ones": ("dw", np.stack([np.stack([np.einsum("bpqo,bpqi->oi", dy, zero_padded(x, s, t)) for t in (-1, 0, 1)], -1)
                                                                                         for s in (-1, 0, 1)], -2)),
            "the last pixel chunk dropped in the wgrad": ("dw", good["dw"] - VR.wgrad_core(np.where(np.arange(H)[None, :, None, None] == H - 1, dy, 0.0)
                                                                                         * (np.arange(B)[:, None, None, None] == B - 1), x)),
            "the bias missing": ("y", good["y"] - b),
            "db short by the last pixel": ("db", good["db"] - pix[-1]),
            "a tap that crosses into the next image": ("y", good["y"] + np.where((np.arange(B)[:, None, None, None] == 0) & (np.arange(H)[None, :, None, None] == H - 1),
                                                                               (np.roll(x, -1, 0)[:, :1] - x[:, -1:]) @ w[:, :, 2, 1].T, 0.0)),
        }
        for what, (name, value) in faults.items():
            assert value.shape == good[name].shape, what
            assert not inside(rounded(value, prec), ref[name]), (what, family, H, W)


def cancelling_case(prec, B=2, H=16, W=16, Cin=32, Cout=32):
    """The weight gradient as two partials over the images that nearly cancel: dy = +1 on the first image, -1 (both plus noise) on the second, x
    positive.  Each partial is ~ B H W / 2 times the sum it leaves, so a rounding of the PARTIALS to fp16 is far more than the rounding of the sum."""
    rng = np.random.default_rng(7)
    x = to_storage(1.0 + 0.25 * rng.standard_normal((B, H, W, Cin)), prec)
    dy = to_storage(np.where(np.arange(B)[:, None, None, None] < B // 2, 1.0, -1.0) + 0.05 * rng.standard_normal((B, H, W, Cout)), prec)
    w = to_storage(rng.standard_normal((Cout, Cin, 3, 3)) / 16.0, prec)
    b = to_storage(rng.standard_normal(Cout), prec)
    return dict(x=x, w=w, b=b, dy=dy, ref=VR.conv(x, w, b, dy, prec))


@pytest.mark.parametrize("prec", PRECS, ids=["fp32", "fp16"])
def test_partials_rounded_to_fp16_land_outside_the_bound(prec):
    c = cancelling_case(prec)
    x, dy = c["x"], c["dy"]
    parts = [VR.wgrad_core(dy[:1], x[:1]), VR.wgrad_core(dy[1:], x[1:])]
    f32 = lambda v: v.astype(np.float32).astype(np.float64)          # noqa: E731
    assert inside(rounded(f32(parts[0]) + f32(parts[1]), prec), c["ref"]["dw"])
    ref, bound = c["ref"]["dw"]
    frac = float((np.abs(rounded(to_storage(parts[0], 1) + to_storage(parts[1], 1), prec) - ref) / bound).max())
    print(f"wgrad partials rounded to fp16, prec{prec}: worst error / bound = {frac:.2f}")
    assert frac > 1.0


def test_the_dgrad_border_added_onto_a_rounded_interior_lands_outside_the_bound():
    """Two roundings: the zero-padded transposed conv rounded to fp16, the border terms added in a second pass and the sum rounded again.  The fault
    is visible where the accumulation term (9 Cout + 2) u sum |dy w| is small beside the store's h |ref|, that is at few channels: at the
    (chunk, chunk) pair the first rounding alone is more than e_dx allows.  At (72, 136) the same fault stays inside (0.87 at the worst element of the
    whole sweep): the figures are printed per channel pair."""
    H, W = 33, 18
    worst = {}
    for Cin, Cout in VR.sweep_channels(1):
        c = VR.case(VR.SWEEP_B, H, W, Cin, Cout, "offset", 1)
        interior, border = dgrad_parts(c["dy"].astype(np.float64), c["w"].astype(np.float64))
        ref, bound = c["ref"]["dx"]
        assert inside(rounded(interior + border, 1), (ref, bound)), (Cin, Cout)                # one rounding is inside
        worst[(Cin, Cout)] = float((np.abs(rounded(to_storage(interior, 1) + border, 1) - ref) / bound).max())
    print("dgrad border onto an fp16-rounded interior, 33x18 offset, worst error / bound:", " ".join(f"{k}={v:.2f}" for k, v in worst.items()))
    assert worst[(8, 8)] > 1.0


def test_the_split_shape_splits_with_a_ragged_last_part():
    for prec in PRECS:
        B, H, W, Cin, Cout = VR.SPLIT
        (s, per), kt = VR.split_of(B * H * W, Cin, Cout, prec), VR.k_tile(prec)
        tiles = -(-B * H * W // kt)
        assert s > 1 and (s - 1) * per < tiles and B * H * W % kt and tiles % per           # every part has work, the last one less, and a partial K tile
        assert VR.expected_split(VR.SWEEP_B * 33 * 18, 136, 72, prec) >= 1
