"""CPU: the trainable-conv entry points of the C ABI (include/moge_hip.h, csrc/conv_grad.hip) are declared, exported and bound, the workspace is the
documented arithmetic, and bad arguments come back as MOGE_ERR_INVALID with a message naming the entry and the argument before anything touches a
GPU.  No GPU call is made here."""
import ctypes as C
import os
import re

import pytest

import conv_reference as VR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["moge_conv3x3_backward", "moge_conv3x3_forward", "moge_conv3x3_workspace"]
INVALID = -1
FP32, FP16 = 0, 1


def last_error(L):
    return (L.lib.moge_last_error() or b"").decode()


def test_symbols_are_declared_exported_and_bound():
    from moge_amd import _lib as L
    import moge_amd.build as B
    hdr = open(os.path.join(ROOT, "include", "moge_hip.h")).read()
    for name in NAMES:
        assert re.search(r"\bint\s+" + name + r"\s*\(", hdr), name
        assert name in L.EXPORTS and getattr(L.lib, name).argtypes is not None, name
    assert sorted(n for n in L.EXPORTS if n.startswith("moge_conv3x3_")) == NAMES
    assert L.lib.moge_abi_version() == 5                                   # purely additive
    assert "conv_grad.hip" in B.SOURCES and "lds_image.h" in B.HEADERS and "grad_host.h" in B.HEADERS


def workspace(L, B, H, W, Cin, Cout, dtype):
    f, b = C.c_int64(-1), C.c_int64(-1)
    code = L.lib.moge_conv3x3_workspace(B, H, W, Cin, Cout, dtype, C.byref(f), C.byref(b))
    return code, f.value, b.value


def test_workspace_is_the_documented_arithmetic_and_monotone_in_the_pixels():
    from moge_amd import _lib as L
    seen = set()
    for dtype in (FP16, FP32):
        for B, H, W, Cin, Cout in ((0, 1, 1, 8, 8), (1, 1, 1, 8, 8), VR.SPLIT, VR.LARGE, (2, 33, 18, 136, 72), (1, 120, 120, 256, 256), (8, 480, 480, 64, 64), (8, 960, 960, 64, 32),
                                   (1, 2 ** 15, 2 ** 15, 8, 8), (2 ** 10, 2 ** 10, 2 ** 10, 8, 8)):
            code, f, b = workspace(L, B, H, W, Cin, Cout, dtype)
            assert code == 0, (B, H, W, Cin, Cout, last_error(L))
            assert (f, b) == VR.expected_workspace(B, H, W, Cin, Cout, dtype), (B, H, W, Cin, Cout, dtype)
            seen.add(VR.expected_split(B * H * W, Cin, Cout, dtype) > 1)
        last = 0
        for H in (1, 2, 7, 16, 45, 64, 100, 480, 960):                      # more pixels never want less
            code, f, b = workspace(L, 2, H, H + 2, 72, 136, dtype)
            assert code == 0 and f == workspace(L, 1, 1, 1, 72, 136, dtype)[1] and b >= last, H
            last = b
    assert seen == {False, True}
    f, b = C.c_int64(-1), C.c_int64(-1)
    assert L.lib.moge_conv3x3_workspace(1, 1, 1, 8, 8, FP16, None, C.byref(b)) == INVALID and "moge_conv3x3_workspace" in last_error(L) and "forward_bytes" in last_error(L)
    assert L.lib.moge_conv3x3_workspace(1, 1, 1, 8, 8, FP16, C.byref(f), None) == INVALID and "moge_conv3x3_workspace" in last_error(L) and "backward_bytes" in last_error(L)
    for (B, H, W, Cin, Cout, dtype), word in (((-1, 1, 1, 8, 8, FP16), "B < 0"), ((1, 0, 1, 8, 8, FP16), "H = 0"), ((1, 1, -3, 8, 8, FP16), "W = -3"), ((1, 1, 1, 0, 8, FP16), "Cin = 0"),
                                              ((1, 1, 1, 12, 8, FP16), "Cin = 12"), ((1, 1, 1, 8, 4, FP16), "Cout = 4"), ((1, 1, 1, 8, -8, FP32), "Cout = -8"),
                                              ((1, 1, 1, 6, 8, FP32), "Cin = 6"), ((1, 1, 1, 8, 8, 2), "dtype"), ((2, 2 ** 15, 2 ** 15, 8, 8, FP16), "2^30 pixels"),
                                              ((1, 1, 1, 2 ** 14, 2 ** 14, FP16), "Cin Cout")):
        code, f, b = workspace(L, B, H, W, Cin, Cout, dtype)
        assert code == INVALID and (f, b) == (0, 0), (B, H, W, Cin, Cout)
        assert "moge_conv3x3_workspace" in last_error(L) and word in last_error(L), (word, last_error(L))
    assert workspace(L, 1, 1, 1, 12, 4, FP32)[0] == 0                     # multiples of 4 are fine in fp32


FWD = ["x", "ldx", "w", "bias", "y", "ldy"]
BWD = ["x", "ldx", "w", "dy", "lddy", "dx", "lddx", "dw", "db", "workspace"]
LD_OF = {"x": "ldx", "y": "ldy", "dy": "lddy", "dx": "lddx"}
CHANNELS = {"x": "Cin", "y": "Cout", "dy": "Cout", "dx": "Cin"}


def _call(L, which, dtype=FP16, B=2, H=3, W=5, Cin=24, Cout=16, **over):
    buf = (C.c_int64 * 64)()
    p = C.addressof(buf)                   # host scratch stands in for device memory: nothing is launched, so nothing dereferences it
    p += (-p) % 16
    sizes, tensor_of = {"Cin": Cin, "Cout": Cout}, {ld: t for t, ld in LD_OF.items()}
    val = lambda n: over[n] if n in over else sizes[CHANNELS[tensor_of[n]]] if n in tensor_of else p      # noqa: E731  (a pixel stride: the channel count)
    _call.keep = buf
    if which == "forward":
        return L.lib.moge_conv3x3_forward(dtype, *[val(n) for n in FWD], B, H, W, Cin, Cout, val("workspace"), None), p
    return L.lib.moge_conv3x3_backward(dtype, *[val(n) for n in BWD], B, H, W, Cin, Cout, None), p


@pytest.mark.parametrize("which", ["forward", "backward"])
def test_bad_arguments_are_rejected_with_a_message(which):
    from moge_amd import _lib as L
    entry = "moge_conv3x3_" + which
    _, p = _call(L, which, B=0)
    for name in (["x", "w", "y", "workspace"] if which == "forward" else ["x", "w", "dy", "workspace"]):
        assert _call(L, which, **{name: None})[0] == INVALID, name
        assert entry in last_error(L) and name in last_error(L) and "null" in last_error(L), (name, last_error(L))
        assert _call(L, which, **{name: p + 8})[0] == INVALID and entry in last_error(L) and name in last_error(L) and "aligned" in last_error(L), name
    for name in (["bias"] if which == "forward" else ["dx", "dw", "db"]):
        assert _call(L, which, **{name: p + 8})[0] == INVALID and entry in last_error(L) and name in last_error(L) and "aligned" in last_error(L), name
    for dtype in (-1, 2, 7):
        assert _call(L, which, dtype=dtype)[0] == INVALID and entry in last_error(L) and "dtype" in last_error(L), dtype
    for kw, word in ((dict(B=-1), "B < 0"), (dict(H=0), "H = 0"), (dict(W=0), "W = 0"), (dict(Cout=0), "Cout = 0"), (dict(Cout=20), "Cout = 20"), (dict(Cin=12), "Cin = 12"),
                     (dict(Cin=-8), "Cin = -8"), (dict(dtype=FP32, Cout=18), "Cout = 18"), (dict(B=2 ** 11, H=2 ** 10, W=2 ** 10), "2^30 pixels")):
        assert _call(L, which, **kw)[0] == INVALID and entry in last_error(L) and word in last_error(L), (kw, last_error(L))
    # pixel strides: multiples of the 16-byte vector (8 halves, 4 floats), at least the channel count
    for name in (n for n in (FWD if which == "forward" else BWD) if n in LD_OF):
        ld = LD_OF[name]
        cols = {"Cin": 24, "Cout": 16}[CHANNELS[name]]
        for dtype, bad in ((FP16, cols - 8), (FP16, cols + 4), (FP32, cols + 2), (FP16, 0), (FP16, -cols)):
            assert _call(L, which, dtype=dtype, **{ld: bad})[0] == INVALID, (ld, bad)
            assert entry in last_error(L) and ld in last_error(L) and "multiple" in last_error(L), (ld, bad, last_error(L))
    if which == "backward":
        assert _call(L, which, dx=None, dw=None, db=None, x=None, w=None, dy=None, workspace=None)[0] == 0          # nothing asked for: no work, no error
        assert _call(L, which, dx=None, dw=None, db=None, Cout=12)[0] == INVALID and "Cout = 12" in last_error(L)    # ... but the sizes are still checked
        assert _call(L, which, dw=None, x=None, B=0)[0] == 0
        assert _call(L, which, dw=None, db=None, w=None)[0] == INVALID and " w " in last_error(L)                    # w is needed for dx ...
        assert _call(L, which, dx=None, db=None, x=None)[0] == INVALID and " x " in last_error(L)                    # ... and x for dw only
    # B = 0 is no work and no error, whatever the pointers
    nothing = {name: None for name in (FWD if which == "forward" else BWD) + ["workspace"] if not name.startswith("ld")}
    assert _call(L, which, B=0, **nothing)[0] == 0
    assert _call(L, which, B=0, Cin=12, **nothing)[0] == INVALID and "Cin = 12" in last_error(L)
