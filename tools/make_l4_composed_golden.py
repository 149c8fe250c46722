"""Fixtures of tests/test_hip_l4_composed.py: the REAL reference (imported unmodified through oracle/make_golden.py's stubs) on a tiny model whose level 4 is
64 -> 32 channels wide - the layout of the released decoders, which no named tiny config has - so that the fp16 path takes the composed level-4 resampler
(csrc/l4c.hip).  Same contents as the fixtures of oracle/make_golden.py minus the forward.* arrays: infer.* (fp32), infer16.* (autocast), infer16half.* (.half()),
meta.drift16 / meta.drift16half at full resolution.  Run by hand where the reference is installed:   python tools/make_l4_composed_golden.py [--check-only]"""
import argparse
import hashlib
import json
import os
import sys
import tempfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import make_golden as MG          # noqa: E402
from oracle import moge_oracle as O           # noqa: E402

DIMS = (128, 64, 64, 64, 32)
CASES = [
    dict(name="l4c_tiny_b2_up", seed=0, sane=True, input_seed=41, shape=[2, 3, 98, 126], kwargs=dict(num_tokens=120, use_fp16=False), stride=2),
    dict(name="l4c_tiny_wide", seed=0, sane=True, input_seed=42, shape=[1, 3, 70, 140], kwargs=dict(num_tokens=90, use_fp16=False), stride=2),
]


def config():
    return O.make_config("dinov2_vits14", (2, 5, 8, 11), DIMS, True, scale_hidden=128)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--check-only", action="store_true")
    args = ap.parse_args()
    MG.install_stubs()
    from moge.model import import_model_class_by_version
    MoGeModel = import_model_class_by_version("v2")
    torch.set_num_threads(os.cpu_count())
    for case in CASES:
        cfg = config()
        sd = O.synth_state_dict(cfg, case["seed"], case["sane"])
        with tempfile.TemporaryDirectory() as td:
            path = os.path.join(td, "model.pt")
            O.save_checkpoint(path, cfg, sd)
            model = MoGeModel.from_pretrained(path).eval()
        assert not (set(model.state_dict().keys()) ^ set(sd.keys()))
        x = MG.make_input(case)
        ref = model.infer(x, **case["kwargs"])
        kw16 = dict(case["kwargs"], use_fp16=True)
        ref16 = model.infer(x, **kw16)
        MG.install_half_stub()
        model.half()
        ref16h = {k: (v.float() if v.is_floating_point() else v) for k, v in model.infer(x, **kw16).items()}
        model.float()
        ora = O.infer(cfg, sd, x, **{k: v for k, v in case["kwargs"].items() if k != "use_fp16"})
        d16, d16h = MG.drift_stats(ref16, ref), MG.drift_stats(ref16h, ref)
        print(case["name"], "oracle vs reference:", " ".join(
            f"{k}:{int((ref[k] != ora[k]).sum())}flips" if ref[k].dtype == torch.bool else f"{k}:{MG.maxdiff(ref[k], ora[k]):.1e}" for k in ref))
        print("  autocast drift:", " ".join(f"{k}:{v.get('p999', v.get('flips')):.2e}" for k, v in d16.items()))
        print("  half drift:    ", " ".join(f"{k}:{v.get('p999', v.get('flips')):.2e}" for k, v in d16h.items()), flush=True)
        if args.check_only:
            continue
        st, blob = case["stride"], {}
        for pre, o in (("infer.", ref), ("infer16.", ref16), ("infer16half.", ref16h)):
            for k, v in o.items():
                blob[pre + k] = MG._strided(k, v.numpy(), st)
        meta = dict(case=dict(case, dims=list(DIMS)), weights_sha256=MG.weights_digest(sd), torch=torch.__version__, threads=torch.get_num_threads(),
                    input_sha256=hashlib.sha256(x.numpy().tobytes()).hexdigest(), drift16=d16, drift16half=d16h)
        blob["meta"] = np.frombuffer(json.dumps(meta).encode(), dtype=np.uint8)
        np.savez_compressed(os.path.join(MG.GOLDEN_DIR, case["name"] + ".npz"), **blob)


if __name__ == "__main__":
    main()
