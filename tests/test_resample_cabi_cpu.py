"""CPU: the resize and narrow-conv entry points of the C ABI (include/moge_hip.h, csrc/resample_grad.hip) are declared, exported and bound, the
workspaces are the documented arithmetic, and bad arguments come back as MOGE_ERR_INVALID with a message naming the entry and the argument before
anything touches a GPU.  No GPU call is made here."""
import ctypes as C
import os
import re

import pytest

import resample_reference as RR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["moge_narrow_conv1x1_backward", "moge_narrow_conv1x1_forward", "moge_narrow_conv1x1_workspace", "moge_resize_bilinear_backward", "moge_resize_bilinear_forward",
         "moge_resize_bilinear_workspace"]
INVALID = -1
FP32, FP16 = 0, 1


def last_error(L):
    return (L.lib.moge_last_error() or b"").decode()


def up16(n):
    return -(-n // 16) * 16


def test_symbols_are_declared_exported_and_bound():
    from moge_amd import _lib as L
    import moge_amd.build as B
    hdr = open(os.path.join(ROOT, "include", "moge_hip.h")).read()
    for name in NAMES:
        assert re.search(r"\bint\s+" + name + r"\s*\(", hdr), name
        assert name in L.EXPORTS and getattr(L.lib, name).argtypes is not None, name
    assert sorted(n for n in L.EXPORTS if n.startswith(("moge_resize_bilinear_", "moge_narrow_conv1x1_"))) == NAMES
    assert L.lib.moge_abi_version() == 5                                   # purely additive
    assert "resample_grad.hip" in B.SOURCES
    for which in ("workspace", "forward", "backward"):                     # the narrow conv: the argument lists of moge_conv3x3_*, word for word
        assert L.SIGNATURES["moge_narrow_conv1x1_" + which] == L.SIGNATURES["moge_conv3x3_" + which]


def rs_workspace(L, B, Hin, Win, Hout, Wout, Cc, dtype):
    f, b = C.c_int64(-1), C.c_int64(-1)
    return L.lib.moge_resize_bilinear_workspace(B, Hin, Win, Hout, Wout, Cc, dtype, C.byref(f), C.byref(b)), f.value, b.value


def n1_workspace(L, B, H, W, Cin, Cout, dtype):
    f, b = C.c_int64(-1), C.c_int64(-1)
    return L.lib.moge_narrow_conv1x1_workspace(B, H, W, Cin, Cout, dtype, C.byref(f), C.byref(b)), f.value, b.value


def test_workspaces_are_the_documented_arithmetic():
    from moge_amd import _lib as L
    for dtype in (FP16, FP32):
        for B, Hin, Win, Hout, Wout, Cc in ((0, 1, 1, 1, 1, 1), (2, 1, 1, 2, 2, 3), (2, 17, 17, 3, 3, 40), (8, 480, 480, 960, 960, 64), (8, 960, 960, 518, 518, 3),
                                            (1, 2 ** 15, 2 ** 15, 1, 1, 1), (1, 1, 2 ** 30, 2 ** 30, 1, 2)):
            assert rs_workspace(L, B, Hin, Win, Hout, Wout, Cc, dtype) == (0, 0, up16(4 * (Hin + 1)) + up16(4 * (Win + 1))), (B, Hin, Win, Hout, Wout, Cc, last_error(L))
        for B, H, W, Cin, Cout in ((0, 1, 1, 8, 1), (1, 1, 1, 8, 1), (1, 10, 130, 32, 3), (2, 17, 19, 72, 7), (8, 960, 960, 32, 3), (1, 2 ** 15, 2 ** 15, 256, 8)):
            slabs = RR.slabs_of(B * H * W)[0] if B else 1
            assert n1_workspace(L, B, H, W, Cin, Cout, dtype) == (0, 0, up16(4 * slabs * Cout * (Cin + 1))), (B, H, W, Cin, Cout, last_error(L))
    assert RR.slabs_of(8 * 960 * 960)[0] == 1024 and RR.slabs_of(RR.RAGGED_M) == (3, 434)
    f, b = C.c_int64(-1), C.c_int64(-1)
    for entry, args in (("moge_resize_bilinear_workspace", (1, 1, 1, 1, 1, 1, FP16)), ("moge_narrow_conv1x1_workspace", (1, 1, 1, 8, 1, FP16))):
        assert getattr(L.lib, entry)(*args, None, C.byref(b)) == INVALID and entry in last_error(L) and "forward_bytes" in last_error(L)
        assert getattr(L.lib, entry)(*args, C.byref(f), None) == INVALID and entry in last_error(L) and "backward_bytes" in last_error(L)
    for args, word in (((-1, 1, 1, 1, 1, 1, FP16), "B < 0"), ((1, 0, 1, 1, 1, 1, FP16), "Hin = 0"), ((1, 1, -2, 1, 1, 1, FP16), "Win = -2"), ((1, 1, 1, 0, 1, 1, FP16), "Hout = 0"),
                       ((1, 1, 1, 1, 0, 1, FP32), "Wout = 0"), ((1, 1, 1, 1, 1, 0, FP32), "C = 0"), ((1, 1, 1, 1, 1, 1, 2), "dtype"),
                       ((2, 2 ** 15, 2 ** 15, 1, 1, 1, FP16), "input grid"), ((1, 1, 1, 2 ** 15, 2 ** 15 + 1, 1, FP16), "output grid"),
                       ((2 ** 20, 2 ** 20, 2 ** 20, 1, 1, 1, FP16), "input grid"), ((1, 1, 1, 2 ** 30, 2 ** 30, 1, FP16), "output grid"),
                       ((1, 2 ** 15, 2 ** 15, 1, 1, 2 ** 30, FP16), "workgroups")):
        code, f_, b_ = rs_workspace(L, *args)
        assert code == INVALID and (f_, b_) == (0, 0) and "moge_resize_bilinear_workspace" in last_error(L) and word in last_error(L), (args, last_error(L))
    for args, word in (((-1, 1, 1, 8, 1, FP16), "B < 0"), ((1, 0, 1, 8, 1, FP16), "H = 0"), ((1, 1, -3, 8, 1, FP16), "W = -3"), ((1, 1, 1, 0, 1, FP16), "Cin = 0"),
                       ((1, 1, 1, 12, 1, FP16), "Cin = 12"), ((1, 1, 1, 6, 1, FP32), "Cin = 6"), ((1, 1, 1, 264, 1, FP16), "Cin = 264 exceeds 256"),
                       ((1, 1, 1, 8, 0, FP16), "Cout = 0"), ((1, 1, 1, 8, 9, FP32), "Cout = 9"), ((1, 1, 1, 8, 16, FP16), "Cout = 16"), ((1, 1, 1, 8, 1, 7), "dtype"),
                       ((2, 2 ** 15, 2 ** 15, 8, 1, FP16), "2^30 pixels"), ((2 ** 20, 2 ** 20, 2 ** 20, 8, 1, FP16), "2^30 pixels")):
        code, f_, b_ = n1_workspace(L, *args)
        assert code == INVALID and (f_, b_) == (0, 0) and "moge_narrow_conv1x1_workspace" in last_error(L) and word in last_error(L), (args, last_error(L))
    assert n1_workspace(L, 1, 1, 1, 12, 5, FP32)[0] == 0                  # multiples of 4 are fine in fp32, Cout whatever its remainder


def _scratch():
    buf = (C.c_int64 * 64)()
    p = C.addressof(buf)                   # host scratch stands in for device memory: nothing is launched, so nothing dereferences it
    _scratch.keep = buf
    return p + (-p) % 16


def rs_call(L, which, dtype=FP16, B=2, Hin=3, Win=5, Hout=6, Wout=7, Cc=16, sh=0.5, sw=0.7, **over):
    p = _scratch()
    v = lambda n, default: over[n] if n in over else default      # noqa: E731
    if which == "forward":
        return L.lib.moge_resize_bilinear_forward(dtype, v("x", p), v("ldx", Cc), v("y", p), v("ldy", Cc), B, Hin, Win, Hout, Wout, Cc, sh, sw, None, None), p
    return L.lib.moge_resize_bilinear_backward(dtype, v("dy", p), v("lddy", Cc), v("dx", p), v("lddx", Cc), v("workspace", p), B, Hin, Win, Hout, Wout, Cc, sh, sw, None), p


@pytest.mark.parametrize("which", ["forward", "backward"])
def test_resize_bad_arguments_are_rejected_with_a_message(which):
    from moge_amd import _lib as L
    entry = "moge_resize_bilinear_" + which
    tensors = {"forward": (("x", "ldx"), ("y", "ldy")), "backward": (("dy", "lddy"), ("dx", "lddx"))}[which]
    _, p = rs_call(L, which, B=0)
    for name, ld in tensors:
        assert rs_call(L, which, **{name: None})[0] == INVALID and entry in last_error(L) and name in last_error(L) and "null" in last_error(L), name
        assert rs_call(L, which, **{name: p + 1})[0] == INVALID and entry in last_error(L) and name in last_error(L) and "aligned" in last_error(L), name
        assert rs_call(L, which, dtype=FP32, **{name: p + 2})[0] == INVALID and "aligned" in last_error(L), name
        for bad in (15, 0, -16):
            assert rs_call(L, which, **{ld: bad})[0] == INVALID and entry in last_error(L) and ld in last_error(L) and "channel count" in last_error(L), (ld, bad)
    if which == "backward":
        assert rs_call(L, which, workspace=None)[0] == INVALID and entry in last_error(L) and "workspace" in last_error(L) and "null" in last_error(L)
        assert rs_call(L, which, workspace=p + 8)[0] == INVALID and "workspace" in last_error(L) and "aligned" in last_error(L)
    for dtype in (-1, 2, 7):
        assert rs_call(L, which, dtype=dtype)[0] == INVALID and entry in last_error(L) and "dtype" in last_error(L), dtype
    for kw, word in ((dict(B=-1), "B < 0"), (dict(Hin=0), "Hin = 0"), (dict(Win=-1), "Win = -1"), (dict(Hout=0), "Hout = 0"), (dict(Wout=0), "Wout = 0"), (dict(Cc=0), "C = 0"),
                     (dict(sh=0.0), "scale_h"), (dict(sh=-0.5), "scale_h"), (dict(sw=0.0), "scale_w"), (dict(sw=float("inf")), "scale_w"), (dict(sh=float("nan")), "scale_h"),
                     (dict(B=2 ** 9, Hin=2 ** 11, Win=2 ** 11), "input grid"), (dict(B=2 ** 9, Hout=2 ** 11, Wout=2 ** 11), "output grid")):
        assert rs_call(L, which, **kw)[0] == INVALID and entry in last_error(L) and word in last_error(L), (kw, last_error(L))
    nothing = {n: None for pair in tensors for n in pair[:1]}
    assert rs_call(L, which, B=0, workspace=None, **nothing)[0] == 0        # B = 0 is no work and no error, whatever the pointers ...
    assert rs_call(L, which, B=0, Cc=0, **nothing)[0] == INVALID and "C = 0" in last_error(L)          # ... but the sizes are still checked


FWD = ["x", "ldx", "w", "bias", "y", "ldy"]
BWD = ["x", "ldx", "w", "dy", "lddy", "dx", "lddx", "dw", "db", "workspace"]
LD_OF = {"x": "ldx", "y": "ldy", "dy": "lddy", "dx": "lddx"}
CHANNELS = {"x": "Cin", "y": "Cout", "dy": "Cout", "dx": "Cin"}


def n1_call(L, which, dtype=FP16, B=2, H=3, W=5, Cin=24, Cout=3, **over):
    p = _scratch()
    sizes, tensor_of = {"Cin": Cin, "Cout": Cout}, {ld: t for t, ld in LD_OF.items()}
    val = lambda n: over[n] if n in over else sizes[CHANNELS[tensor_of[n]]] if n in tensor_of else p      # noqa: E731  (a pixel stride: the channel count)
    if which == "forward":
        return L.lib.moge_narrow_conv1x1_forward(dtype, *[val(n) for n in FWD], B, H, W, Cin, Cout, None, None), p
    return L.lib.moge_narrow_conv1x1_backward(dtype, *[val(n) for n in BWD], B, H, W, Cin, Cout, None), p


@pytest.mark.parametrize("which", ["forward", "backward"])
def test_narrow_conv_bad_arguments_are_rejected_with_a_message(which):
    from moge_amd import _lib as L
    entry = "moge_narrow_conv1x1_" + which
    _, p = n1_call(L, which, B=0)
    for name in (["x", "w", "y"] if which == "forward" else ["x", "w", "dy", "workspace"]):
        assert n1_call(L, which, **{name: None})[0] == INVALID and entry in last_error(L) and name in last_error(L) and "null" in last_error(L), (name, last_error(L))
    for name in (["x", "w", "bias", "y"] if which == "forward" else ["x", "w", "dy", "dx", "dw", "db"]):      # x and dx: 16 bytes; the rest: their element
        assert n1_call(L, which, **{name: p + 1})[0] == INVALID and entry in last_error(L) and name in last_error(L) and "aligned" in last_error(L), (name, last_error(L))
    for name in (["x"] if which == "forward" else ["x", "dx", "workspace"]):
        assert n1_call(L, which, **{name: p + 8})[0] == INVALID and name in last_error(L) and "aligned" in last_error(L), name
    for dtype in (-1, 2, 7):
        assert n1_call(L, which, dtype=dtype)[0] == INVALID and entry in last_error(L) and "dtype" in last_error(L), dtype
    for kw, word in ((dict(B=-1), "B < 0"), (dict(H=0), "H = 0"), (dict(W=0), "W = 0"), (dict(Cout=0), "Cout = 0"), (dict(Cout=9), "Cout = 9"), (dict(Cin=12), "Cin = 12"),
                     (dict(Cin=-8), "Cin = -8"), (dict(Cin=264), "Cin = 264"), (dict(dtype=FP32, Cin=18), "Cin = 18"), (dict(B=2 ** 9, H=2 ** 11, W=2 ** 11), "2^30 pixels")):
        assert n1_call(L, which, **kw)[0] == INVALID and entry in last_error(L) and word in last_error(L), (kw, last_error(L))
    for name in (n for n in (FWD if which == "forward" else BWD) if n in LD_OF):
        ld, wide = LD_OF[name], CHANNELS[name] == "Cin"
        for dtype, bad in (((FP16, 16), (FP16, 28), (FP32, 26), (FP16, 0), (FP16, -24)) if wide else ((FP16, 2), (FP32, 0), (FP16, -3))):
            assert n1_call(L, which, dtype=dtype, **{ld: bad})[0] == INVALID, (ld, bad)
            assert entry in last_error(L) and ld in last_error(L) and ("multiple" if wide else "channel count") in last_error(L), (ld, bad, last_error(L))
    if which == "backward":
        assert n1_call(L, which, dx=None, dw=None, db=None, x=None, w=None, dy=None, workspace=None)[0] == 0          # nothing asked for: no work, no error
        assert n1_call(L, which, dx=None, dw=None, db=None, Cout=12)[0] == INVALID and "Cout = 12" in last_error(L)    # ... but the sizes are still checked
        assert n1_call(L, which, dw=None, db=None, w=None)[0] == INVALID and " w " in last_error(L)                    # w is needed for dx ...
        assert n1_call(L, which, dx=None, db=None, x=None)[0] == INVALID and " x " in last_error(L)                    # ... and x for dw only
    nothing = {name: None for name in (FWD if which == "forward" else BWD) if not name.startswith("ld")}
    assert n1_call(L, which, B=0, **nothing)[0] == 0
    assert n1_call(L, which, B=0, Cin=12, **nothing)[0] == INVALID and "Cin = 12" in last_error(L)
