"""CPU: the moge_block_* entry points of the C ABI (include/moge_hip.h, csrc/block_grad.hip) are declared, exported and bound, the workspace is the
documented slab arithmetic, and bad arguments come back as MOGE_ERR_INVALID with a message naming the entry and the argument before anything
touches a GPU.  No GPU call is made here."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["moge_block_gelu_backward", "moge_block_gelu_forward", "moge_block_norm_backward", "moge_block_norm_forward", "moge_block_scale_residual_backward",
         "moge_block_scale_residual_forward", "moge_block_workspace"]
INVALID = -1
FP32, FP16 = 0, 1
MAX_C = 2048


def last_error(L):
    return (L.lib.moge_last_error() or b"").decode()


def test_symbols_are_declared_exported_and_bound():
    from moge_amd import _lib as L
    import moge_amd.build as B
    hdr = open(os.path.join(ROOT, "include", "moge_hip.h")).read()
    for name in NAMES:
        assert re.search(r"\bint\s+" + name + r"\s*\(", hdr), name
        assert name in L.EXPORTS and getattr(L.lib, name).argtypes is not None, name
    assert sorted(n for n in L.EXPORTS if n.startswith("moge_block_")) == NAMES
    assert L.lib.moge_abi_version() == 5                                   # purely additive
    assert "block_grad.hip" in B.SOURCES and os.path.exists(os.path.join(ROOT, "moge_amd", "csrc", "block_grad.hip"))
    assert re.search(r"#define\s+MOGE_BLOCK_MAX_C\s+2048\b", hdr) and L.BLOCK_MAX_C == MAX_C


def expected_slab(M):
    """The documented rule: slabs of 32 rows while that gives at most 512 of them, else of the next multiple of 32 rows that does."""
    return 32 * max(1, -(-M // (32 * 512)))


def test_workspace_is_the_documented_arithmetic():
    from moge_amd import _lib as L
    from moge_amd import block as Blk
    n = C.c_int64(-1)
    slabs = set()
    for M in (0, 1, 31, 32, 33, 65, 3601, 32 * 512 - 1, 32 * 512, 32 * 512 + 1, 16421, 8 * 3601, 64 * 512, 64 * 512 + 1, 2 ** 31 - 1):
        for Cw in (4, 8, 384, 1024, 1536, MAX_C):
            assert L.lib.moge_block_workspace(M, Cw, C.byref(n)) == 0, (M, Cw, last_error(L))
            s = expected_slab(M)
            assert Blk.slab_rows(M) == s
            assert n.value == 4 * 3 * -(-M // s) * Cw == Blk.workspace_bytes(M, Cw), (M, Cw, n.value, s)
            assert -(-M // s) <= 512
            slabs.add(s)
    assert {32, 64, 96} <= slabs
    assert L.lib.moge_block_workspace(1, 8, None) == INVALID and "moge_block_workspace" in last_error(L) and "bytes" in last_error(L)
    for (M, Cw), word in (((-1, 8), "M < 0"), ((1, 0), "C = 0"), ((1, 6), "C = 6"), ((1, -8), "C = -8"), ((1, MAX_C + 4), "MOGE_BLOCK_MAX_C")):
        assert L.lib.moge_block_workspace(M, Cw, C.byref(n)) == INVALID and n.value == 0, (M, Cw)
        assert "moge_block_workspace" in last_error(L) and word in last_error(L), (M, Cw, last_error(L))


# entry -> (leading dtype arguments, the arguments between them and (M, C, stream) in order); a name that starts with "ld" is a leading dimension, "eps" a float
ENTRIES = {
    "gelu_forward": (1, ["x", "ldx", "y", "ldy"]),
    "gelu_backward": (1, ["x", "ldx", "dy", "lddy", "dx", "lddx"]),
    "scale_residual_forward": (2, ["x", "ldx", "r", "ldr", "gamma", "y", "ldy"]),
    "scale_residual_backward": (2, ["dy", "lddy", "r", "ldr", "gamma", "dr", "lddr", "dgamma", "workspace"]),
    "norm_forward": (3, ["x", "ldx", "r", "ldr", "gamma", "x1", "ldx1", "weight", "bias", "eps", "n", "ldn", "mean_rstd"]),
    "norm_backward": (3, ["x", "ldx", "mean_rstd", "weight", "dn", "lddn", "dx1", "lddx1", "r", "ldr", "gamma", "dx", "lddx", "dr", "lddr", "dweight", "dbias", "dgamma",
                          "workspace"]),
}
# the pointers an entry cannot do without (given that every output is asked for), and its outputs
REQUIRED = {"gelu_forward": ["x"], "gelu_backward": ["x", "dy"], "scale_residual_forward": ["x", "r", "gamma"], "scale_residual_backward": ["dy", "r", "gamma"],
            "norm_forward": ["x", "weight", "bias", "n"], "norm_backward": ["x", "mean_rstd", "weight", "gamma", "r"]}        # dn: the plain form only, below
OUTPUTS = {"gelu_forward": ["y"], "gelu_backward": ["dx"], "scale_residual_forward": ["y"], "scale_residual_backward": ["dr", "dgamma"], "norm_forward": ["n"],
           "norm_backward": ["dx", "dr", "dweight", "dbias", "dgamma"]}


def _call(L, which, dtypes=None, M=5, Cw=16, **over):
    buf = (C.c_int64 * 64)()
    p = C.addressof(buf)                   # host scratch stands in for device memory: nothing is launched, so nothing dereferences it
    p += (-p) % 16
    nd, names = ENTRIES[which]
    args = []
    for name in names:
        if name in over:
            args.append(over[name])
        elif name == "eps":
            args.append(1e-5)
        else:
            args.append(Cw if name.startswith("ld") else p)
    _call.keep = buf
    dt = list(dtypes) if dtypes is not None else [FP16] * nd
    return getattr(L.lib, "moge_block_" + which)(*dt, *args, M, Cw, None), p


@pytest.mark.parametrize("which", list(ENTRIES))
def test_bad_arguments_are_rejected_with_a_message(which):
    from moge_amd import _lib as L
    entry = "moge_block_" + which
    nd, names = ENTRIES[which]
    _, p = _call(L, which, M=0)

    def bad(word, *words, **kw):
        code = _call(L, which, **kw)[0]
        msg = last_error(L)
        assert code == INVALID and entry in msg and word in msg and all(w in msg for w in words), (kw, code, msg)

    for name in REQUIRED[which]:
        bad(name, "null", **{name: None})
    for name in names:
        if not name.startswith("ld") and name != "eps":
            bad(name, "aligned", **{name: p + 8})
    # dtypes: unknown values in each position, and the pairs that are not built (fp32 rows beside an fp16 stream)
    for pos in range(nd):
        for v in (-1, 2, 7):
            dt = [FP16] * nd
            dt[pos] = v
            bad("dtype", dtypes=dt)
    if nd >= 2:
        bad("r_dtype", "not built", dtypes=[FP16, FP32] + [FP16] * (nd - 2))
    if nd == 3:
        bad("n_dtype", "not built", dtypes=[FP16, FP16, FP32])
    # sizes; the width unit is 16 bytes in EVERY storage type of the call
    for kw, word in ((dict(M=-1), "M < 0"), (dict(Cw=0), "C = 0"), (dict(Cw=20), "C = 20"), (dict(Cw=-8), "C = -8"), (dict(dtypes=[FP32] * nd, Cw=18), "C = 18")):
        bad(word, **kw)
    if nd >= 2:
        bad("C = 12", dtypes=[FP32, FP16] + [FP32] * (nd - 2), Cw=12)             # 12 floats are 16-byte rows, 12 halves are not
        bad("MOGE_BLOCK_MAX_C", Cw=MAX_C + 8)
        assert _call(L, which, M=0, Cw=MAX_C)[0] == 0
    else:
        assert _call(L, which, M=0, Cw=MAX_C + 8)[0] == 0                          # the element-wise kernels have no width limit
    # leading dimensions: multiples of the 16-byte vector, at least the row length
    for name in names:
        if name.startswith("ld"):
            for dt, ldv in (([FP16] * nd, 8), ([FP16] * nd, 20), ([FP32] * nd, 18), ([FP16] * nd, 0), ([FP16] * nd, -16)):
                bad(name, "multiple", dtypes=dt, **{name: ldv})
    # a column sum wants its workspace.  (That a call without one needs none, and the optional arguments of the fused form, are success paths: they launch,
    # so tests/test_hip_block.py has them.)
    if "workspace" in names:
        bad("workspace", "null", workspace=None)
        bad("workspace", "aligned", workspace=p + 8)
    if which == "norm_backward":
        bad("dweight and dbias", dbias=None)
        bad("dn", "null", dn=None, dx1=None, r=None, gamma=None, dr=None, dgamma=None)        # the plain form cannot do without dn
    if which == "norm_forward":
        bad("x1", "null", x1=None)
    # nothing asked for: no work, no error, whatever the other pointers - but the sizes are still checked
    nothing = {name: None for name in names if not name.startswith("ld") and name != "eps"}
    if which != "norm_forward":
        assert _call(L, which, **{o: None for o in OUTPUTS[which]})[0] == 0
        bad("C = 20", Cw=20, **{o: None for o in OUTPUTS[which]})
    assert _call(L, which, M=0, **nothing)[0] == 0
    bad("C = 12", M=0, Cw=12, **nothing)
