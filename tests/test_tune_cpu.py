"""CPU: the runtime tuning switches (moge_amd/csrc/tune.h: THE table of keys and defaults; moge_tune_set / _reset / _value, moge_amd._lib.tune /
tune_reset / tune_value / tuned) and the documents that list them.  The environment is read once per process, so whatever depends on it runs
in a fresh child interpreter."""
import ctypes
import glob
import json
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID = -1        # MOGE_ERR_INVALID


def table():
    """(product keys, experiments-only keys) of tune.h, each {key: default}"""
    src = open(os.path.join(ROOT, "moge_amd", "csrc", "tune.h")).read()
    head, exp = src.split("#ifdef MOGE_EXPERIMENTS", 1)
    rows = [{k: int(d) for k, d in re.findall(r"^\s*X\(([A-Z0-9_]+),\s*(-?\d+)\)", part, re.M)} for part in (head, exp.split("#else", 1)[0])]
    assert len(rows[0]) >= 20 and len(rows[1]) >= 10 and not set(rows[0]) & set(rows[1])
    return rows


CHILD = r"""
import json, sys
from moge_amd import _lib as L
keys = sys.argv[1].split(",")
out = {"start": {k: L.tune_value(k) for k in keys}, "set": {}, "reset": {}}
for k in keys:
    L.tune(k, 41)
    out["set"][k] = L.tune_value(k)
    L.tune_reset(k)
    out["reset"][k] = L.tune_value(k)
L.tune("ATTN_KS", 2); L.tune_reset("ATTN_KS")
out["ks_after_reset"] = L.tune_value("ATTN_KS")
with L.tuned(ATTN_KS=2, ATTN_KERN=1):
    out["ks_inside"] = [L.tune_value("ATTN_KS"), L.tune_value("ATTN_KERN")]
    L.tune("ATTN_KS", 4)              # a tune() inside the block is undone with the block
out["ks_after_block"] = [L.tune_value("ATTN_KS"), L.tune_value("ATTN_KERN")]
try:
    with L.tuned(ATTN_KS=2):
        raise KeyError("body")
except KeyError:
    pass
out["ks_after_raise"] = L.tune_value("ATTN_KS")
for k in keys:
    L.tune(k, 40)
L.tune_reset()
out["reset_all"] = {k: L.tune_value(k) for k in keys}
print("RESULT " + json.dumps(out))
"""


def child(extra_env):
    prod, _ = table()
    env = {k: v for k, v in os.environ.items() if not k.startswith("MOGE_")}
    env.update(extra_env)
    r = subprocess.run([sys.executable, "-c", CHILD, ",".join(prod)], capture_output=True, text=True, env=env, cwd=ROOT, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    res = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])
    return res, [ln for ln in r.stderr.splitlines() if "[libmoge_hip]" in ln]


def test_clean_environment_gives_the_table_defaults_and_reset_returns_to_them():
    prod, _ = table()
    res, announced = child({})
    assert res["start"] == prod
    assert res["set"] == {k: 41 for k in prod}
    assert res["reset"] == prod and res["reset_all"] == prod
    assert res["ks_after_reset"] == prod["ATTN_KS"]
    assert res["ks_inside"] == [2, 1] and res["ks_after_block"] == [prod["ATTN_KS"], prod["ATTN_KERN"]] and res["ks_after_raise"] == prod["ATTN_KS"]
    assert announced == []


def test_environment_override_is_announced_once_and_survives_reset_and_tuned():
    prod, _ = table()
    assert prod["ATTN_KS"] != 0
    res, announced = child({"MOGE_ATTN_KS": "0"})
    want = {**prod, "ATTN_KS": 0}
    assert res["start"] == want
    assert len(announced) == 1 and "MOGE_ATTN_KS=0" in announced[0] and f"({prod['ATTN_KS']})" in announced[0], announced
    assert res["ks_after_reset"] == 0                       # not the table's default: the process was started with 0
    assert res["ks_inside"][0] == 2 and res["ks_after_block"][0] == 0 and res["ks_after_raise"] == 0
    assert res["reset"] == want and res["reset_all"] == want


def test_environment_value_equal_to_the_default_is_not_announced():
    prod, _ = table()
    res, announced = child({"MOGE_ATTN_KS": str(prod["ATTN_KS"]), "MOGE_PP_MIN_TILES": str(prod["PP_MIN_TILES"])})
    assert res["start"] == prod and announced == []


def test_unknown_key_is_an_error():
    from moge_amd import _lib as L
    _, exp = table()
    v = ctypes.c_int(7)
    for key in (b"ATTN_KSS", b"", b"attn_ks", b"ATTN_SK"):            # a typo, nothing, wrong case, a key of --experiments builds only
        assert key.decode() not in table()[0] and (key != b"ATTN_SK" or "ATTN_SK" in exp)
        for rc in (L.lib.moge_tune_set(key, 0), L.lib.moge_tune_reset(key), L.lib.moge_tune_value(key, ctypes.byref(v))):
            assert rc == INVALID
            assert b'"' + key + b'"' in L.lib.moge_last_error()
    assert v.value == 7
    assert L.lib.moge_tune_value(b"ATTN_KS", None) == INVALID
    for call in (lambda: L.tune("ATTN_KSS", 0), lambda: L.tune_reset("ATTN_KSS"), lambda: L.tune_value("ATTN_KSS")):
        with pytest.raises(L.MogeError, match="ATTN_KSS"):
            call()
    before = L.tune_value("ATTN_KERN")
    with pytest.raises(L.MogeError, match="ATTN_KSS"):
        with L.tuned(ATTN_KERN=before + 1, ATTN_KSS=0):
            pytest.fail("the block must not run")
    assert L.tune_value("ATTN_KERN") == before              # ... and the keys set before the bad one are reset


def test_experiments_only_keys_exist_in_the_experiments_library():
    from moge_amd import _lib as L
    if not os.path.exists(L.EXPERIMENTS_LIB_PATH):
        pytest.skip("the --experiments copy of the library is not built")
    prod, exp = table()
    X = L.experiments_lib()
    v = ctypes.c_int()
    for key, dflt in {**prod, **exp}.items():
        assert X.moge_tune_value(key.encode(), ctypes.byref(v)) == 0, key
        if "MOGE_" + key not in os.environ:
            assert v.value == dflt, key
    assert X.moge_tune_value(b"ATTN_KSS", ctypes.byref(v)) == INVALID


def md_table(text, after):
    """rows (lists of cells) of the first markdown table behind the line that contains `after`"""
    lines = text[text.index(after):].splitlines()
    start = next(i for i, ln in enumerate(lines) if ln.startswith("|"))
    rows = []
    for ln in lines[start:]:
        if not ln.startswith("|"):
            break
        rows.append([c.strip() for c in ln.strip().strip("|").split("|")])
    return rows[0], rows[2:]


def test_design_md_lists_exactly_the_product_keys_and_no_defaults():
    prod, _ = table()
    header, rows = md_table(open(os.path.join(ROOT, "DESIGN.md")).read(), "**Runtime switches of the product library.**")
    assert header == ["key", "set by"]
    assert sorted(r[0].strip("`") for r in rows) == sorted(prod)


def test_integration_md_section_6_agrees_with_the_table():
    prod, exp = table()
    both = {**prod, **exp}
    text = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "moge_tune_reset" in text[text.index("## 6."):] and "tune.h" in text[text.index("## 6."):]
    header, rows = md_table(text, "## 6.")
    assert header == ["key", "default", "meaning"]
    seen = []
    for keys_cell, dflt_cell, _ in rows:
        keys = re.findall(r"`([A-Z0-9_]+)`", keys_cell)
        assert keys and keys_cell == ", ".join(f"`{k}`" for k in keys), keys_cell
        dflts = [int(re.match(r"\s*(-?\d+)\b", piece).group(1)) for piece in dflt_cell.split(",")]          # every piece starts with the integer
        assert len(dflts) in (1, len(keys)), keys_cell
        for i, k in enumerate(keys):
            assert k in both, k
            assert both[k] == dflts[i if len(dflts) > 1 else 0], k
        seen += keys
    assert len(seen) == len(set(seen)) and set(prod) <= set(seen)


def test_every_product_key_is_set_by_a_test_or_a_tool():
    """The standing rule of DESIGN.md: a key stays in the product library only while something sets it."""
    prod, _ = table()
    files = [f for f in glob.glob(os.path.join(ROOT, "tests", "*.py")) if os.path.basename(f) != "test_tune_cpu.py"]
    files += glob.glob(os.path.join(ROOT, "tools", "*.py")) + [os.path.join(ROOT, "tools", "kbench.hip"), os.path.join(ROOT, "tools", "gpu_call.sh")]
    text = "\n".join(open(f).read() for f in files)
    unused = [k for k in prod if not re.search(r"(?:MOGE_|(?<![A-Z0-9_]))" + k + r"(?![A-Z0-9_])", text)]
    assert not unused, unused
