"""CPU: the optimizer entry points of the C ABI (include/moge_hip.h, csrc/optim.hip) are declared, exported and bound, the header's macros are
the module's constants, the plan and the workspace are the documented arithmetic, and bad arguments come back as MOGE_ERR_INVALID with a
message before anything touches a GPU.  No GPU call is made here."""
import ctypes as C
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["moge_optim_plan", "moge_optim_workspace", "moge_optim_state_init", "moge_optim_grad_stats", "moge_optim_adamw"]
INVALID = -1


def last_error(L):
    return (L.lib.moge_last_error() or b"").decode()


def test_symbols_are_declared_exported_and_bound():
    from moge_amd import _lib as L
    import moge_amd.build as B
    import moge_amd.optim as M
    hdr = open(os.path.join(ROOT, "include", "moge_hip.h")).read()
    for name in NAMES:
        assert re.search(r"\bint\s+" + name + r"\s*\(", hdr), name
        assert name in L.EXPORTS and getattr(L.lib, name).argtypes is not None, name
    assert sorted(n for n in L.EXPORTS if n.startswith("moge_optim_")) == sorted(NAMES)
    assert L.lib.moge_abi_version() == 5                                   # purely additive
    assert "optim.hip" in B.SOURCES
    for macro, value in (("MOGE_OPTIM_SLOT_WORDS", M.SLOT_WORDS), ("MOGE_OPTIM_STATE_WORDS", M.STATE_WORDS), ("MOGE_OPTIM_CHUNK", M.CHUNK),
                         ("MOGE_OPTIM_MAX_GROUPS", M.MAX_GROUPS), ("MOGE_OPTIM_HYPER_WORDS", M.HYPER_WORDS)):
        assert int(re.search(r"#define\s+" + macro + r"\s+(\d+)", hdr).group(1)) == value, macro
    assert (M.SLOT_WORDS, M.STATE_WORDS, M.MAX_GROUPS) == (8, 8, 16) and M.CHUNK & (M.CHUNK - 1) == 0
    for fn in ("AdamW", "build_optimizer", "build_lr_scheduler"):
        assert callable(getattr(M, fn)), fn


def test_plan_is_the_documented_arithmetic():
    from moge_amd import _lib as L
    import moge_amd.optim as M
    Ck = M.CHUNK
    numel = [1, 0, Ck - 1, Ck, Ck + 1, 0, 2 * Ck + 3, 7, 0]
    want = np.concatenate([[0], np.cumsum([-(-n // Ck) for n in numel])])
    assert np.array_equal(M.plan(numel), want) and want[-1] == 1 + 1 + 1 + 2 + 3 + 1
    assert np.array_equal(M.plan([]), [0])
    first = (C.c_int64 * 4)()
    one = (C.c_int64 * 1)(5)
    assert L.lib.moge_optim_plan(one, 1, None) == INVALID and "moge_optim_plan" in last_error(L) and "null" in last_error(L)
    assert L.lib.moge_optim_plan(None, 1, first) == INVALID and "null" in last_error(L)
    assert L.lib.moge_optim_plan(one, -1, first) == INVALID and "n < 0" in last_error(L)
    assert L.lib.moge_optim_plan((C.c_int64 * 1)(-3), 1, first) == INVALID and "negative" in last_error(L)
    assert L.lib.moge_optim_plan((C.c_int64 * 2)(2 ** 42, 2 ** 42), 2, first) == INVALID and "2^31" in last_error(L)


def test_workspace_is_the_documented_arithmetic():
    from moge_amd import _lib as L
    n = C.c_int64(-1)
    for chunks in (0, 1, 2, 3, 10, 73421, 2 ** 31 - 1):
        assert L.lib.moge_optim_workspace(chunks, C.byref(n)) == 0
        assert n.value == 8 * (chunks + (chunks + 1) // 2) and n.value >= 12 * chunks and n.value % 8 == 0, chunks
    assert L.lib.moge_optim_workspace(4, None) == INVALID and "null" in last_error(L)
    for chunks in (-1, 2 ** 31):
        assert L.lib.moge_optim_workspace(chunks, C.byref(n)) == INVALID and n.value == 0 and "moge_optim_workspace" in last_error(L)


def test_bad_arguments_are_rejected_with_a_message():
    from moge_amd import _lib as L
    buf = (C.c_int64 * 64)()
    p = C.addressof(buf)                    # host scratch stands in for device memory: nothing is launched, so nothing dereferences it
    lib = L.lib
    good = (C.c_double * 10)(1e-4, 0.9, 0.999, 1e-8, 0.01, 1e-5, 0.8, 0.99, 1e-6, 0.0)
    hp = C.addressof(good)
    assert lib.moge_optim_state_init(None, 1.0, None) == INVALID and "moge_optim_state_init" in last_error(L) and "null" in last_error(L)
    assert lib.moge_optim_state_init(p, 0.0, None) == INVALID and "init_scale" in last_error(L)
    # pass 1
    stats = lambda table=p, n=1, chunks=1, max_norm=1.0, use=0, growth=2.0, backoff=0.5, interval=2000, ws=p, state=p: \
        lib.moge_optim_grad_stats(table, n, chunks, max_norm, use, growth, backoff, interval, ws, state, None)
    assert stats(table=None) == INVALID and "moge_optim_grad_stats" in last_error(L) and "null" in last_error(L)
    assert stats(ws=None) == INVALID and "null" in last_error(L)
    assert stats(state=None) == INVALID and "null" in last_error(L)
    assert stats(n=-1) == INVALID and "n < 0" in last_error(L)
    for n, chunks in ((1, -1), (1, 2 ** 31), (0, 3)):
        assert stats(n=n, chunks=chunks) == INVALID and "chunks" in last_error(L) and "plan" in last_error(L), (n, chunks)
    assert stats(use=1, interval=0) == INVALID and "growth_interval" in last_error(L)
    assert stats(use=1, growth=0.0) == INVALID and "growth" in last_error(L)
    assert stats(max_norm=float("nan")) == INVALID and "max_norm" in last_error(L)
    # pass 2
    adamw = lambda table=p, n=1, chunks=1, hyper=hp, groups=2, ema=0.999, state=p: lib.moge_optim_adamw(table, n, chunks, hyper, groups, ema, 1, 0, state, None)
    assert adamw(table=None) == INVALID and "moge_optim_adamw" in last_error(L) and "null" in last_error(L)
    assert adamw(hyper=None) == INVALID and "null" in last_error(L)
    assert adamw(state=None) == INVALID and "null" in last_error(L)
    assert adamw(n=-1) == INVALID and "n < 0" in last_error(L)
    for groups in (0, -1, 17):
        assert adamw(groups=groups) == INVALID and "groups" in last_error(L), groups
    for n, chunks in ((1, -1), (1, 2 ** 31), (0, 3)):
        assert adamw(n=n, chunks=chunks) == INVALID and "chunks" in last_error(L), (n, chunks)
    assert adamw(ema=1.0) == INVALID and "ema_decay" in last_error(L)
    for slot, value, word in ((1, 1.0, "beta"), (1, -0.1, "beta"), (2, 1.5, "beta"), (7, float("nan"), "beta"), (0, -1e-4, "lr"), (3, -1e-8, "eps"), (4, -0.01, "weight_decay"),
                              (5, float("nan"), "lr")):
        bad = (C.c_double * 10)(*good)
        bad[slot] = value
        assert adamw(hyper=C.addressof(bad)) == INVALID and word in last_error(L) and f"group {slot // 5}" in last_error(L), (slot, value)
    # no work is no error, whatever the pointers
    assert stats(table=None, n=0, chunks=0, ws=None, state=None) == 0 and stats(table=None, n=3, chunks=0, ws=None) == 0
    assert adamw(table=None, n=0, chunks=0, state=None) == 0 and adamw(table=None, n=3, chunks=0) == 0
