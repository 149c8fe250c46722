"""CPU: the two entry points of the fused residual-block convs (include/moge_hip.h, csrc/conv_grad.hip) are declared, exported and bound with the
declared signatures, and bad arguments come back as MOGE_ERR_INVALID with a message naming the entry and the argument before anything touches a GPU.
No GPU call is made here."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID = -1
FP32, FP16 = 0, 1
I32, I64, VP = C.c_int, C.c_int64, C.c_void_p
SIGNATURES = {
    # int dtype, x, ldx, w, bias, res, ldres, y, ldy, B, H, W, Cin, Cout, workspace, stream
    "moge_relu_conv3x3_forward": [I32, VP, I64, VP, VP, VP, I64, VP, I64, I32, I32, I32, I32, I32, VP, VP],
    # int dtype, x, ldx, w, dy, lddy, add, ldadd, dx, lddx, dw, db, workspace, B, H, W, Cin, Cout, stream
    "moge_relu_conv3x3_backward": [I32, VP, I64, VP, VP, I64, VP, I64, VP, I64, VP, VP, VP, I32, I32, I32, I32, I32, VP],
}
HEADER_ARGS = {
    "moge_relu_conv3x3_forward": "int dtype, const void* x, int64_t ldx, const void* w, const void* bias, const void* res, int64_t ldres, void* y, int64_t ldy, "
                                 "int B, int H, int W, int Cin, int Cout, void* workspace, void* stream",
    "moge_relu_conv3x3_backward": "int dtype, const void* x, int64_t ldx, const void* w, const void* dy, int64_t lddy, const void* add, int64_t ldadd, void* dx, "
                                  "int64_t lddx, void* dw, void* db, void* workspace, int B, int H, int W, int Cin, int Cout, void* stream",
}


def last_error(L):
    return (L.lib.moge_last_error() or b"").decode()


def test_symbols_are_declared_exported_and_bound_with_the_declared_signatures():
    from moge_amd import _lib as L
    hdr = open(os.path.join(ROOT, "include", "moge_hip.h")).read()
    for name, argtypes in SIGNATURES.items():
        m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)", hdr)
        assert m and " ".join(m.group(1).split()) == HEADER_ARGS[name], name
        assert name in L.EXPORTS and getattr(L.lib, name).restype is C.c_int and list(getattr(L.lib, name).argtypes) == argtypes, name
    assert sorted(n for n in L.EXPORTS if n.startswith("moge_relu_conv3x3_")) == sorted(SIGNATURES)      # no workspace query of its own
    assert "moge_conv3x3_workspace" in hdr.split("moge_relu_conv3x3_forward")[0].split("the decoder's residual block without norms")[1]      # ... and the header says whose it is
    assert L.lib.moge_abi_version() == 5                                   # purely additive


FWD = ["x", "ldx", "w", "bias", "res", "ldres", "y", "ldy"]
BWD = ["x", "ldx", "w", "dy", "lddy", "add", "ldadd", "dx", "lddx", "dw", "db", "workspace"]
LD_OF = {"x": "ldx", "y": "ldy", "dy": "lddy", "dx": "lddx", "res": "ldres", "add": "ldadd"}
CHANNELS = {"x": "Cin", "y": "Cout", "dy": "Cout", "dx": "Cin", "res": "Cout", "add": "Cin"}


def _call(L, which, dtype=FP16, B=2, H=3, W=5, Cin=24, Cout=16, **over):
    buf = (C.c_int64 * 64)()
    p = C.addressof(buf)                   # host scratch stands in for device memory: nothing is launched, so nothing dereferences it
    p += (-p) % 16
    sizes, tensor_of = {"Cin": Cin, "Cout": Cout}, {ld: t for t, ld in LD_OF.items()}
    val = lambda n: over[n] if n in over else sizes[CHANNELS[tensor_of[n]]] if n in tensor_of else p      # noqa: E731  (a pixel stride: the channel count)
    _call.keep = buf
    if which == "forward":
        return L.lib.moge_relu_conv3x3_forward(dtype, *[val(n) for n in FWD], B, H, W, Cin, Cout, val("workspace"), None), p
    return L.lib.moge_relu_conv3x3_backward(dtype, *[val(n) for n in BWD], B, H, W, Cin, Cout, None), p


@pytest.mark.parametrize("which", ["forward", "backward"])
def test_bad_arguments_are_rejected_with_a_message(which):
    """Every call here fails a check (or has B = 0, or asks for nothing), so nothing is launched."""
    from moge_amd import _lib as L
    entry = "moge_relu_conv3x3_" + which
    _, p = _call(L, which, B=0)
    for name in (["x", "w", "y", "workspace"] if which == "forward" else ["x", "w", "dy", "dx", "workspace"]):
        if name == "dx":
            continue                                                     # a null dx is "not asked for"
        assert _call(L, which, **{name: None})[0] == INVALID, name
        assert entry in last_error(L) and name in last_error(L) and "null" in last_error(L), (name, last_error(L))
    for name in (["x", "w", "bias", "res", "y", "workspace"] if which == "forward" else ["x", "w", "dy", "add", "dx", "dw", "db", "workspace"]):
        assert _call(L, which, **{name: p + 8})[0] == INVALID and entry in last_error(L) and name in last_error(L) and "aligned" in last_error(L), (name, last_error(L))
    for dtype in (-1, 2, 7):
        assert _call(L, which, dtype=dtype)[0] == INVALID and entry in last_error(L) and "dtype" in last_error(L), dtype
    for kw, word in ((dict(B=-1), "B < 0"), (dict(H=0), "H = 0"), (dict(W=0), "W = 0"), (dict(Cout=0), "Cout = 0"), (dict(Cout=20), "Cout = 20"), (dict(Cin=12), "Cin = 12"),
                     (dict(Cin=-8), "Cin = -8"), (dict(dtype=FP32, Cout=18), "Cout = 18"), (dict(B=2 ** 11, H=2 ** 10, W=2 ** 10), "2^30 pixels")):
        assert _call(L, which, **kw)[0] == INVALID and entry in last_error(L) and word in last_error(L), (kw, last_error(L))
    # pixel strides, ldres and ldadd among them: multiples of the 16-byte vector (8 halves, 4 floats), at least the channel count
    for name in (n for n in (FWD if which == "forward" else BWD) if n in LD_OF):
        ld = LD_OF[name]
        cols = {"Cin": 24, "Cout": 16}[CHANNELS[name]]
        for dtype, bad in ((FP16, cols - 8), (FP16, cols + 4), (FP32, cols + 2), (FP16, 0), (FP16, -cols)):
            assert _call(L, which, dtype=dtype, **{ld: bad})[0] == INVALID, (ld, bad)
            assert entry in last_error(L) and ld in last_error(L) and "multiple" in last_error(L), (ld, bad, last_error(L))
    if which == "backward":
        assert _call(L, which, dx=None, dw=None, db=None, x=None, w=None, dy=None, add=None, workspace=None)[0] == 0      # nothing asked for: no work, no error
        assert _call(L, which, dx=None, dw=None, db=None, Cout=12)[0] == INVALID and "Cout = 12" in last_error(L)          # ... but the sizes are still checked
        assert _call(L, which, dw=None, db=None, w=None)[0] == INVALID and " w " in last_error(L)                          # w is needed for dx ...
        assert _call(L, which, dx=None, db=None, x=None)[0] == INVALID and " x " in last_error(L)                          # ... x for dw ...
        assert _call(L, which, dw=None, db=None, x=None)[0] == INVALID and " x " in last_error(L)                          # ... AND for dx: it is the mask
        assert _call(L, which, dx=None, dw=None, x=None, w=None, add=None, workspace=None)[0] == INVALID and "workspace" in last_error(L)      # db alone needs no x
    # B = 0 is no work and no error, whatever the pointers
    nothing = {name: None for name in (FWD if which == "forward" else BWD) + ["workspace"] if not name.startswith("ld")}
    assert _call(L, which, B=0, **nothing)[0] == 0
    assert _call(L, which, B=0, Cin=12, **nothing)[0] == INVALID and "Cin = 12" in last_error(L)
