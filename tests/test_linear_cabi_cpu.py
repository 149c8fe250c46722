"""CPU: the trainable-Linear entry points of the C ABI (include/moge_hip.h, csrc/linear_grad.hip) are declared, exported and bound, the workspace is
the documented arithmetic, and bad arguments come back as MOGE_ERR_INVALID with a message naming the entry and the argument before anything
touches a GPU.  No GPU call is made here."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["moge_linear_backward", "moge_linear_forward", "moge_linear_workspace"]
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
    assert sorted(n for n in L.EXPORTS if n.startswith("moge_linear_")) == NAMES
    assert L.lib.moge_abi_version() == 5                                   # purely additive
    assert "linear_grad.hip" in B.SOURCES and "lds_image.h" in B.HEADERS and "grad_host.h" in B.HEADERS
    assert (L.FP32, L.FP16) == (FP32, FP16)


def expected_split(M, N, K, dtype):
    """The documented rule: as many splits of M as bring the 128 x 128 tiles of dW to 256 workgroups, each keeping at least 8 K tiles (64 fp16 / 32
    fp32 rows), 32 at the most."""
    tiles = -(-N // 128) * -(-K // 128)
    ktiles = -(-M // (64 if dtype == FP16 else 32))
    return max(1, min(256 // tiles, ktiles // 8, 32))


def test_workspace_is_the_documented_arithmetic():
    from moge_amd import _lib as L
    n = C.c_int64(-1)
    seen = set()
    for dtype in (FP16, FP32):
        for M, N, K in ((0, 8, 8), (1, 8, 8), (129, 136, 264), (1370, 1536, 384), (2049, 136, 72), (3601, 1024, 1024), (3601, 3072, 1024), (3601, 4096, 1024),
                        (28808, 1024, 4096), (2 ** 31 - 1, 8, 8), (1, 2 ** 20 * 8, 8)):
            assert L.lib.moge_linear_workspace(M, N, K, dtype, C.byref(n)) == 0, (M, N, K, last_error(L))
            s = expected_split(M, N, K, dtype)
            assert n.value == (4 * s * N * K if s > 1 else 0), (M, N, K, dtype, n.value, s)
            seen.add(s > 1)
    assert seen == {False, True}
    assert L.lib.moge_linear_workspace(1, 8, 8, FP16, None) == INVALID and "moge_linear_workspace" in last_error(L) and "bytes" in last_error(L)
    for (M, N, K, dtype), word in (((-1, 8, 8, FP16), "M < 0"), ((1, 0, 8, FP16), "N = 0"), ((1, 12, 8, FP16), "N = 12"), ((1, 8, 4, FP16), "K = 4"), ((1, 8, -8, FP32), "K = -8"),
                                   ((1, 6, 8, FP32), "N = 6"), ((1, 8, 8, 2), "dtype"), ((2 ** 31 - 1, 2 ** 31 - 8, 8, FP16), "workgroups")):
        assert L.lib.moge_linear_workspace(M, N, K, dtype, C.byref(n)) == INVALID and n.value == 0, (M, N, K)
        assert "moge_linear_workspace" in last_error(L) and word in last_error(L), (M, N, K, last_error(L))
    assert L.lib.moge_linear_workspace(1, 12, 4, FP32, C.byref(n)) == 0                  # multiples of 4 are fine in fp32


FWD = ["x", "ldx", "w", "ldw", "bias", "y", "ldy"]
BWD = ["x", "ldx", "w", "ldw", "dy", "lddy", "dx", "lddx", "dw", "lddw", "db", "workspace"]
LD_OF = {"x": "ldx", "w": "ldw", "y": "ldy", "dy": "lddy", "dx": "lddx", "dw": "lddw"}
COLS = {"x": "K", "w": "K", "y": "N", "dy": "N", "dx": "K", "dw": "K"}


def _call(L, which, dtype=FP16, M=5, N=16, K=24, **over):
    buf = (C.c_int64 * 64)()
    p = C.addressof(buf)                   # host scratch stands in for device memory: nothing is launched, so nothing dereferences it
    p += (-p) % 16
    fn, names = (L.lib.moge_linear_forward, FWD) if which == "forward" else (L.lib.moge_linear_backward, BWD)
    sizes, tensor_of = {"N": N, "K": K}, {ld: t for t, ld in LD_OF.items()}
    args = [over[n] if n in over else sizes[COLS[tensor_of[n]]] if n in tensor_of else p for n in names]      # a leading dimension: the row length
    _call.keep = buf
    return fn(dtype, *args, M, N, K, None), p


@pytest.mark.parametrize("which", ["forward", "backward"])
def test_bad_arguments_are_rejected_with_a_message(which):
    from moge_amd import _lib as L
    entry = "moge_linear_" + which
    _, p = _call(L, which, M=0)
    required = ["x", "w", "y"] if which == "forward" else ["x", "w", "dy", "dx", "dw"]
    for name in required:
        if which == "backward" and name in ("dx", "dw"):
            continue                                                         # a null output is a product that is not asked for
        assert _call(L, which, **{name: None})[0] == INVALID, name
        assert entry in last_error(L) and name in last_error(L) and "null" in last_error(L), (name, last_error(L))
        assert _call(L, which, **{name: p + 8})[0] == INVALID and entry in last_error(L) and name in last_error(L) and "aligned" in last_error(L), name
    for name in (["bias"] if which == "forward" else ["dx", "dw", "db"]):
        assert _call(L, which, **{name: p + 8})[0] == INVALID and entry in last_error(L) and name in last_error(L) and "aligned" in last_error(L), name
    for dtype in (-1, 2, 7):
        assert _call(L, which, dtype=dtype)[0] == INVALID and entry in last_error(L) and "dtype" in last_error(L), dtype
    for kw, word in ((dict(M=-1), "M < 0"), (dict(N=0), "N = 0"), (dict(N=20), "N = 20"), (dict(K=12), "K = 12"), (dict(K=-8), "K = -8"),
                     (dict(dtype=FP32, N=18), "N = 18"), (dict(M=2 ** 31 - 1, N=2 ** 31 - 8), "workgroups")):
        assert _call(L, which, **kw)[0] == INVALID and entry in last_error(L) and word in last_error(L), (kw, last_error(L))
    # leading dimensions: multiples of the 16-byte vector (8 halves, 4 floats), at least the row length
    for name in (n for n in (FWD if which == "forward" else BWD) if n in LD_OF):
        ld = LD_OF[name]
        cols = {"N": 16, "K": 24}[COLS[name]]
        for dtype, bad in ((FP16, cols - 8), (FP16, cols + 4), (FP32, cols + 2), (FP16, 0), (FP16, -cols)):
            assert _call(L, which, dtype=dtype, **{ld: bad})[0] == INVALID, (ld, bad)
            assert entry in last_error(L) and ld in last_error(L) and "multiple" in last_error(L), (ld, bad, last_error(L))
    # the backward's split of M wants its workspace; without dw nothing does
    if which == "backward":
        assert _call(L, which, M=4096, workspace=None)[0] == INVALID and "workspace" in last_error(L) and "null" in last_error(L)
        assert _call(L, which, M=4096, workspace=p + 8)[0] == INVALID and "workspace" in last_error(L) and "aligned" in last_error(L)
        assert _call(L, which, dx=None, dw=None, db=None, x=None, w=None, dy=None, workspace=None)[0] == 0          # nothing asked for: no work, no error
        assert _call(L, which, dx=None, dw=None, db=None, N=12)[0] == INVALID and "N = 12" in last_error(L)          # ... but the sizes are still checked
    # M = 0 is no work and no error, whatever the pointers
    nothing = {name: None for name in (FWD if which == "forward" else BWD) if not name.startswith("ld")}
    assert _call(L, which, M=0, **nothing)[0] == 0
    assert _call(L, which, M=0, K=12, **nothing)[0] == INVALID and "K = 12" in last_error(L)
