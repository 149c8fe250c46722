"""CPU: the training-data entry points are declared, listed and bound; the build compiles their file; the ABI version did not move."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TRAIN_EXPORTS = ["moge_train_depth_edge", "moge_train_finish", "moge_train_normal_map", "moge_train_warp"]


def test_train_entry_points_are_declared_listed_and_bound():
    from moge_amd import _lib as L
    hdr = open(os.path.join(ROOT, "include", "moge_hip.h")).read()
    stateless = hdr[hdr.index("Stateless entry points: everything below"):]
    declared = sorted(set(re.findall(r"\b(moge_train_[a-z0-9_]+)\s*\(", stateless)))
    assert declared == TRAIN_EXPORTS
    assert sorted(n for n in L.EXPORTS if n.startswith("moge_train_")) == TRAIN_EXPORTS
    for name in TRAIN_EXPORTS:
        fn = getattr(L.lib, name)
        assert fn.argtypes == L.SIGNATURES[name][1] and fn.argtypes[-1] is L.SIGNATURES["moge_eval_remap"][1][-1]      # the stream comes last
        args = re.search(name + r"\s*\(([^;]*)\);", hdr).group(1)
        assert len(args.split(",")) == len(fn.argtypes), name
    assert L.lib.moge_abi_version() == L.ABI_VERSION == 5
    assert int(re.search(r"#define MOGE_TRAIN_WARP_MATS (\d+)", hdr).group(1)) == L.TRAIN_WARP_MATS == 3 * 9 + 9 + 3


def test_build_compiles_the_file_and_shares_the_quantile():
    from moge_amd import build as B
    assert "traindata.hip" in B.SOURCES and "quantile.h" in B.HEADERS
    csrc = os.path.join(ROOT, "moge_amd", "csrc")
    header = open(os.path.join(csrc, "quantile.h")).read()
    assert "q_hist_body" in header and "q_select_body" in header and "f2key" in header
    for name in ("evaldata.hip", "traindata.hip"):                    # one radix select, included by both, copied by neither
        src = open(os.path.join(csrc, name)).read()
        assert '#include "quantile.h"' in src and "q_hist_body(" in src and "q_select_body(" in src
        assert "uint32_t f2key" not in src
    src = open(os.path.join(csrc, "traindata.hip")).read()
    assert "#pragma clang fp contract(off)" in src and "mfma" not in src.replace("no MFMA", "").lower()
