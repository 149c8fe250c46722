"""CPU: the trainable-attention entry points of the C ABI (include/moge_hip.h, csrc/attention_grad.hip) are declared, exported and bound, the
workspace is the documented arithmetic, and bad arguments come back as MOGE_ERR_INVALID with a message naming the entry and the argument
before anything touches a GPU.  No GPU call is made here."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["moge_attn_backward", "moge_attn_forward", "moge_attn_workspace"]
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
    assert sorted(n for n in L.EXPORTS if n.startswith("moge_attn_")) == NAMES
    assert L.lib.moge_abi_version() == 5                                   # purely additive
    assert "attention_grad.hip" in B.SOURCES
    assert (L.FP32, L.FP16) == (FP32, FP16)


def test_workspace_is_the_documented_arithmetic():
    from moge_amd import _lib as L
    n = C.c_int64(-1)
    for B, nh, N in ((0, 16, 3601), (8, 0, 1370), (1, 1, 1), (2, 3, 65), (8, 16, 3601), (1, 16, 2 ** 24 - 1), (2 ** 15, 2 ** 15, 2 ** 24 - 1), (2 ** 31 - 1, 1, 7)):
        assert L.lib.moge_attn_workspace(B, nh, N, C.byref(n)) == 0, (B, nh, N)
        assert n.value == 8 * B * nh * N, (B, nh, N)
    assert L.lib.moge_attn_workspace(1, 1, 1, None) == INVALID and "moge_attn_workspace" in last_error(L) and "bytes" in last_error(L)
    for (B, nh, N), word in (((-1, 1, 5), "B < 0"), ((1, -1, 5), "nh < 0"), ((1, 1, 0), "N outside"), ((1, 1, -3), "N outside"), ((1, 1, 2 ** 24), "N outside"),
                             ((2 ** 16, 2 ** 16, 5), "B * nh")):
        assert L.lib.moge_attn_workspace(B, nh, N, C.byref(n)) == INVALID and n.value == 0, (B, nh, N)
        assert "moge_attn_workspace" in last_error(L) and word in last_error(L), (B, nh, N, last_error(L))


def _calls(L):
    buf = (C.c_int64 * 64)()
    p = C.addressof(buf)                   # host scratch stands in for device memory: nothing is launched, so nothing dereferences it
    p += (-p) % 16
    s = (C.c_int64 * 3)(64 * 5, 64 * 5 * 2, 64)
    sp = C.addressof(s)
    fwd_names = ["q", "q_strides", "k", "k_strides", "v", "v_strides", "out", "workspace"]
    bwd_names = ["q", "q_strides", "k", "k_strides", "v", "v_strides", "out", "out_strides", "dout", "dout_strides", "workspace", "dq", "dq_strides", "dk",
                 "dk_strides", "dv", "dv_strides"]

    def call(fn, names, dtype=FP16, B=1, nh=2, N=5, **over):
        args = [over.get(name, sp if name.endswith("_strides") else p) for name in names]
        return fn(dtype, *args, B, nh, N, None)

    call.keep = (buf, s)                   # the scratch lives as long as the caller
    return p, s, (L.lib.moge_attn_forward, fwd_names), (L.lib.moge_attn_backward, bwd_names), call


@pytest.mark.parametrize("which", ["forward", "backward"])
def test_bad_arguments_are_rejected_with_a_message(which):
    from moge_amd import _lib as L
    p, s, fwd, bwd, call = _calls(L)
    fn, names = fwd if which == "forward" else bwd
    entry = "moge_attn_" + which
    for name in names:                                                      # every required pointer
        assert call(fn, names, **{name: None}) == INVALID, name
        assert entry in last_error(L) and name in last_error(L) and "null" in last_error(L), (name, last_error(L))
    for dtype in (-1, 2, 7):
        assert call(fn, names, dtype=dtype) == INVALID and entry in last_error(L) and "dtype" in last_error(L), dtype
    for kw, word in ((dict(N=0), "N outside"), (dict(N=-1), "N outside"), (dict(N=2 ** 24), "N outside"), (dict(B=-1), "B < 0"), (dict(nh=-2), "nh < 0"),
                     (dict(B=2 ** 20, nh=2 ** 12, N=129), "workgroups"), (dict(B=2 ** 16, nh=2 ** 16, N=5), "workgroups")):
        assert call(fn, names, **kw) == INVALID and entry in last_error(L) and word in last_error(L), (kw, last_error(L))
    # strides: multiples of the 16-byte vector (8 halves, 4 floats), not negative; pointers: 16-byte aligned
    tensors = [n for n in names if n + "_strides" in names]
    for name in tensors:
        for dtype, bad in ((FP16, (64, 64, 60)), (FP16, (4, 64, 64)), (FP32, (64, 66, 64)), (FP16, (64, -64, 64))):
            bs = (C.c_int64 * 3)(*bad)
            assert call(fn, names, dtype=dtype, **{name + "_strides": C.addressof(bs)}) == INVALID, (name, bad)
            assert entry in last_error(L) and name + "_strides" in last_error(L) and "multiple" in last_error(L), (name, bad, last_error(L))
        ok4 = (C.c_int64 * 3)(64, 68, 4)                                    # fine for fp32, not for fp16
        assert call(fn, names, dtype=FP16, **{name + "_strides": C.addressof(ok4)}) == INVALID and name + "_strides" in last_error(L)
        assert call(fn, names, **{name: p + 8}) == INVALID and entry in last_error(L) and name in last_error(L) and "aligned" in last_error(L), name
    assert call(fn, names, out=p + 8) == INVALID and "out" in last_error(L) and "aligned" in last_error(L)
    assert call(fn, names, workspace=p + 2) == INVALID and "workspace" in last_error(L) and "aligned" in last_error(L)
    # no work is no error, whatever the pointers
    nothing = {name: None for name in names}
    assert call(fn, names, B=0, **nothing) == 0 and call(fn, names, nh=0, **nothing) == 0 and call(fn, names, B=0, nh=0, N=2 ** 24 - 1, **nothing) == 0
    assert call(fn, names, B=0, N=0, **nothing) == INVALID and "N outside" in last_error(L)          # ... but N is still checked
