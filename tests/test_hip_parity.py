"""GPU: the parity tests proper.  The HIP path (through the Python mirror -> C ABI) against the committed golden fixtures of the REAL
reference (tests/golden/*.npz, written by oracle/make_golden.py from /root/reference), against the CPU oracle on the same seeded inputs,
and - at the BASELINE sizes - through size-independent properties.

Gates (north_star; tests/golden_util.py, metric = oracle/metrics.py: per pixel, relative to that pixel's own norm):
  FP32 mode  points / depth / normal / intrinsics: EVERY pixel within 1e-3; validity mask bit-exact; same +inf pattern.
  FP16 mode  judged against the reference's fp32 output with the band the reference's OWN fp16 path (infer(use_fp16=True), run on the
             same case when the fixture was made) shows against its fp32 path: p99.9 of the per-pixel error <= 1.6 x the reference's
             (per-image numbers and mask flips: 2 x; tests/golden_util.py FP16_FACTOR).  Every fixture carries those numbers (meta.drift16)."""
import os

import numpy as np
import pytest
import torch

from tests.golden_util import gate_line, CASE_BY_NAME, FP32_TOL, SLOW_CASES, check_fp16, check_fp32, fp16_band, load_case, rel_err, subsample

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def MoGeModel():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from moge_amd.model import import_model_class_by_version
    return import_model_class_by_version("v2")


_models = {}


def get_model(MoGeModel, cfg_name, seed, sane, tmp_path_factory, massive=False, case=None):
    """The model of a fixture (`case` given: its config overrides - remap_output, dropped heads, z_bias - apply) or of a named config."""
    import json
    from oracle import moge_oracle as O
    from oracle.make_golden import case_config, case_state_dict
    if case is None:
        case = dict(config=cfg_name, seed=seed, sane=sane, massive=massive)
    key = json.dumps({k: case.get(k) for k in ("config", "seed", "sane", "massive", "cfg_override", "z_bias")}, sort_keys=True)
    if key not in _models:
        if len(_models) >= 3:                      # vitl / vitb models hold ~2 GB of device memory each: keep a few, not all
            _models.pop(next(iter(_models)))
        cfg = case_config(case)
        sd = case_state_dict(case, cfg)
        path = os.path.join(str(tmp_path_factory.mktemp("ckpt")), "model.pt")
        O.save_checkpoint(path, cfg, sd)
        _models[key] = (MoGeModel.from_pretrained(path).to("cuda").eval(), cfg, sd)      # through the reference's loader contract
    return _models[key]


def golden_infer(gold, prefix="infer."):
    return {k[len(prefix):]: v for k, v in gold.items() if k.startswith(prefix)}


def sub(out, st):
    return {k: subsample(k, v.cpu().numpy(), st) for k, v in out.items()}


V2_CASES = [n for n, c in CASE_BY_NAME.items() if c.get("version", "v2") == "v2"]          # the MoGe-1 fixtures are tests/test_hip_v1.py's


@pytest.mark.parametrize("name", V2_CASES)
def test_fp32_mode_matches_reference_golden_and_oracle(MoGeModel, name, tmp_path_factory):
    """Every fixture, incl. the BASELINE-size ones (moge-2-vitl 518x518 T=3600, moge-2-vitb-normal, the 518x1036 / 1036x518 grids 42x85 / 85x42)."""
    from oracle import moge_oracle as O
    case, cfg, sd, x, gold, meta = load_case(name)
    model, _, _ = get_model(MoGeModel, None, None, None, tmp_path_factory, case=case)
    kw = dict(case["kwargs"]); kw["use_fp16"] = False
    model.onnx_compatible_mode = bool(case.get("onnx"))        # docs/onnx.md: fixtures "tiny_onnx_mode_*" were made with the flag set
    try:
        out = model.float().infer(x, **kw)
    finally:
        model.onnx_compatible_mode = False
    ill = not case["sane"]
    st = case.get("stride", 1)
    # (1) committed golden vectors of the real reference
    seen = check_fp32(sub(out, st), golden_infer(gold), ill=ill)
    print(f"[parity fp32] {name}: " + " ".join(f"{k}={v:.1e}" for k, v in seen.items()))
    # (2) the oracle, live, full resolution (bit-identical to the reference on these cases; the big ones take the GPU box's CPU too long)
    if name not in SLOW_CASES:
        ref = O.infer(cfg, sd, x, onnx_compatible_mode=bool(case.get("onnx")), **{k: v for k, v in kw.items() if k != "use_fp16"})
        check_fp32(out, ref, ill=ill)


SANE = [n for n in V2_CASES if CASE_BY_NAME[n]["sane"]]
BIG = [n for n in SANE if n in SLOW_CASES and n != "vits_house518"]


@pytest.mark.parametrize("name", SANE)
def test_fp16_mode_within_reference_fp16_band(MoGeModel, name, tmp_path_factory):
    """fp16 mode, both forms the reference has (.half() weights; fp32 weights + use_fp16=True), against the reference's fp32 golden inside
    1.6x (per-image numbers, mask flips: 2x) the reference's own fp16 drift on that case."""
    case, cfg, sd, x, gold, meta = load_case(name)
    model, _, _ = get_model(MoGeModel, None, None, None, tmp_path_factory, case=case)
    kw = dict(case["kwargs"]); kw["use_fp16"] = True
    st = case.get("stride", 1)
    band = {"autocast": fp16_band(meta, gold, "autocast"), "half": fp16_band(meta, gold, "half")}
    g = golden_infer(gold)
    model.onnx_compatible_mode = bool(case.get("onnx"))
    try:
        out = model.float().infer(x, **kw)             # fp32 weights + use_fp16 (autocast analogue: fp32 residual stream)
        out_h = model.half().infer(x, **kw)            # .half() weights (scripts/infer.py:83-84: the residual stream itself is fp16)
    finally:
        model.float()
        model.onnx_compatible_mode = False
    for tag, o in (("autocast", out), ("half", out_h)):
        seen = check_fp16(sub(o, st), g, band[tag])
        print(f"[gate fp16 {tag}] {name}: " + gate_line(seen, band[tag]))
    # the reference's own fp16 outputs are inside the same bands by construction; ours must not be further from them than 2 bands
    check_fp16(sub(out, st), golden_infer(gold, "infer16."), {k: 2 * v for k, v in band["autocast"].items()})
    check_fp16(sub(out_h, st), golden_infer(gold, "infer16half."), {k: 2 * v for k, v in band["half"].items()})


@pytest.mark.parametrize("name", BIG)
def test_fp16_throughput_kernels_in_the_model_match_reference_golden(MoGeModel, name, tmp_path_factory):
    """The BASELINE-size fixtures are single images, which the production dispatch sends to the latency-regime GEMM kernels.  Here the SAME
    forward is pushed through the throughput kernels the batch-32 bench runs - gemm_pp128m16_kernel (PP_MIN_TILES = 0) for qkv / proj / fc1 /
    fc2 / out-proj / conv-transpose GEMMs, then again with the image replicated to a batch that reaches them under the production dispatch - and
    must (a) stay inside the reference-fp16 band of the fixture and (b) reproduce the single-image result bit for bit (ATTN_KS = 0: the batch-invariant form of
    the one-image attention; the default form of a single image is pinned to the band by the golden tests above and to this one by
    test_single_image_key_split_attention_stays_within_half_a_band)."""
    from moge_amd import _lib as L
    case, cfg, sd, x, gold, meta = load_case(name)
    model, _, _ = get_model(MoGeModel, None, None, None, tmp_path_factory, case=case)
    kw = dict(case["kwargs"]); kw["use_fp16"] = True
    st = case.get("stride", 1)
    band, g = fp16_band(meta, gold, "half"), golden_infer(gold)
    try:
        model.half()
        with L.tuned(ATTN_KS=0):    # (a single image's attention otherwise splits its key range inside the workgroup: within the band, not bit-identical to a batch item - test_single_image_key_split_attention_...)
            base = model.infer(x, **kw)
            with L.tuned(PP_MIN_TILES=0):
                forced = model.infer(x, **kw)
            xb = x.expand(9, *x.shape[1:]).contiguous()        # 9 x 3601 rows = 127 row tiles x >= 3 column tiles: ping-pong regime, two half-batch streams
            batch = model.infer(xb, **kw)
    finally:
        model.float()
    check_fp16(sub(forced, st), g, band)
    for k in base:
        for other, what in ((forced[k], "forced ping-pong"), (batch[k][:1], "batch 9, item 0"), (batch[k][8:], "batch 9, item 8")):
            a, b = other, base[k]
            if a.dtype == torch.bool:
                assert torch.equal(a, b), (k, what)
            else:
                fin = torch.isfinite(b)
                assert torch.equal(fin, torch.isfinite(a)) and torch.equal(a[fin], b[fin]), f"{k}: {what} differs from the single-image result"


def _same(a, b, what):
    if a.dtype == torch.bool:
        assert torch.equal(a, b), what
    else:
        fin = torch.isfinite(b)
        assert torch.equal(fin, torch.isfinite(a)) and torch.equal(a[fin], b[fin]), what


def test_bench_batch_of_32_distinct_images_matches_its_single_image_results(MoGeModel, tmp_path_factory):
    """The bench workload itself (BASELINE configs[2]: moge-2-vitl, 32 DISTINCT 518x518 images, .half(), default tokens, two 16-image streams):
    items 0 / 15 / 16 / 31 - both ends of both half-batch streams - equal their single-image results bit for bit, and item 0 (the fixture's
    image: torch.rand(32, ...) with seed 0 draws it first) sits inside the reference-.half() band of the golden."""
    from moge_amd import _lib as L
    case, cfg, sd, x1, gold, meta = load_case("vitl_518_t3600")
    model, _, _ = get_model(MoGeModel, None, None, None, tmp_path_factory, case=case)
    x = torch.rand(32, 3, 518, 518, generator=torch.Generator().manual_seed(0))
    assert torch.equal(x[:1], x1)
    try:
        model.half()
        batch = model.infer(x)
        # race screen: the same batch three more times through the two-stream production path (persistent GEMMs with prefetch across tiles,
        # counted vmcnt waits, head / tail hand-overs): every run must reproduce the first bit for bit
        for rep in range(3):
            again = model.infer(x)
            for k in batch:
                _same(again[k], batch[k], f"{k}: run {rep + 2} of the same batch differs from run 1 (a race)")
        with L.tuned(ATTN_KS=0):     # the batch-invariant form of the one-image attention (the default splits a single image's key range inside the workgroup)
            for i in (0, 15, 16, 31):
                single = model.infer(x[i])
                for k in single:
                    _same(batch[k][i], single[k], f"{k}: item {i} of the batch of 32 differs from its single-image result")
    finally:
        model.float()
    check_fp16(sub({k: v[:1] for k, v in batch.items()}, case.get("stride", 1)), golden_infer(gold), fp16_band(meta, gold, "half"))


def test_fp32_image_into_half_model_equals_prehalved_image(MoGeModel, tmp_path_factory):
    """v2.py:229 `image.to(dtype=self.dtype)`: an fp32 image given to a .half() model is rounded to fp16 inside preprocess_kernel (img_dtype 3);
    the result must equal feeding the explicitly pre-rounded fp16 tensor (img_dtype 1) bit for bit."""
    model, cfg, sd = get_model(MoGeModel, "tiny-vits-normal", 0, True, tmp_path_factory)
    x = torch.rand(2, 3, 84, 112, generator=torch.Generator().manual_seed(21))
    try:
        model.half()
        a = model.infer(x, num_tokens=108)
        b = model.infer(x.half(), num_tokens=108)
    finally:
        model.float()
    for k in a:
        fin = torch.isfinite(b[k]) if b[k].dtype != torch.bool else torch.ones_like(b[k])
        assert torch.equal(a[k][fin], b[k][fin]), k


def test_stage_taps_match_oracle(MoGeModel, tmp_path_factory):
    """Stage boundaries of one forward (fp32 mode): LayerNorm'ed ViT taps, cls token, encoder features, every neck level."""
    from oracle import moge_oracle as O
    case, cfg, sd, x, gold, meta = load_case("tiny_b2_up")
    model, _, _ = get_model(MoGeModel, None, None, None, tmp_path_factory, case=case)
    model.float()
    fwd = model.forward(x, case["kwargs"]["num_tokens"])
    tr = {}
    ref = O.forward(cfg, sd, x, case["kwargs"]["num_tokens"], tr)
    B = x.shape[0]
    taps = torch.cat([t[:, 1:] for t in tr["taps"]], dim=-1).reshape(-1)
    assert rel_err(model.debug_tap("tapcat").cpu().numpy(), taps.numpy()) < 1e-4
    assert rel_err(model.debug_tap("cls").cpu().numpy(), tr["cls"].reshape(-1).numpy()) < 1e-4
    assert rel_err(model.debug_tap("features").cpu().numpy(), tr["features"].permute(0, 2, 3, 1).reshape(-1).numpy()) < 1e-4
    for l, n in enumerate(tr["neck"]):
        assert rel_err(model.debug_tap(f"neck{l}").cpu().numpy(), n.permute(0, 2, 3, 1).reshape(-1).numpy()) < 2e-4, l
    for k in ref:
        assert rel_err(fwd[k].cpu().numpy(), ref[k].numpy()) < 5e-4, k


def test_forward_of_a_half_model_returns_half_tensors(MoGeModel, tmp_path_factory):
    """v2.py:386-387: forward() of a `.half()` model returns fp16 tensors of the same shapes; they come from moge_cast_f16 on the launch
    stream (no torch op on the path) and stay within the fp16 band of the fp32 forward."""
    model, cfg, sd = get_model(MoGeModel, "tiny-vits-normal", 0, True, tmp_path_factory)
    x = torch.rand(2, 3, 84, 112, generator=torch.Generator().manual_seed(21))
    try:
        model.float()
        f32 = model.forward(x, 108)
        model.half()
        f16 = model.forward(x, 108)
        again = model.forward(x, 108)
    finally:
        model.float()
    assert set(f16) == set(f32)
    for k in f32:
        assert f16[k].dtype == torch.float16 and f16[k].shape == f32[k].shape and f16[k].is_cuda, k
        assert torch.equal(f16[k], again[k]), k
        assert rel_err(f16[k].float().cpu().numpy(), f32[k].cpu().numpy()) < 1e-1, k      # sanity only (random tiny net; the fp16 gate is check_fp16 on the goldens)


def test_error_behaviour_matches_reference(MoGeModel, tmp_path_factory):
    """scipy raises ValueError('Residuals are not finite in the initial point.') when the point map overflows."""
    from oracle import moge_oracle as O
    cfg = O.named_configs()["tiny-vits-normal"]
    sd = O.synth_state_dict(cfg, 0, True)
    sd["points_head.output_blocks.4.bias"][2] = 200.0        # exp(200) = inf in fp32
    path = os.path.join(str(tmp_path_factory.mktemp("ckpt")), "bad.pt")
    O.save_checkpoint(path, cfg, sd)
    model = MoGeModel.from_pretrained(path).to("cuda").eval()
    with pytest.raises(ValueError):
        model.infer(torch.rand(1, 3, 64, 64), num_tokens=64, use_fp16=False)


def test_properties_at_baseline_size(MoGeModel, tmp_path_factory):
    """BASELINE config sizes (518x518, T=3600, fp16, vitb) - size-independent properties: batch items are independent
    (sharding contract of SURVEY 8(e)), outputs are deterministic, re-projection is consistent with depth+intrinsics,
    masked pixels are inf / 0, normals are unit length."""
    model, cfg, sd = get_model(MoGeModel, "moge-2-vitb-normal", 0, True, tmp_path_factory)
    model.half()
    g = torch.Generator().manual_seed(0)
    x = torch.rand(3, 3, 518, 518, generator=g)
    out = model.infer(x)
    out2 = model.infer(x)
    for k in out:
        assert torch.equal(out[k], out2[k]), f"{k} not deterministic"
    from moge_amd import _lib as L
    with L.tuned(ATTN_KS=0):         # the batch-invariant form of the one-image attention
        single = model.infer(x[1])
    for k in out:
        a, b = out[k][1], single[k]
        if a.dtype == torch.bool:
            assert torch.equal(a, b)
        else:
            fin = torch.isfinite(a)
            assert torch.equal(fin, torch.isfinite(b)) and torch.equal(a[fin], b[fin]), f"{k}: batch item depends on its batch"
    m, d, p, K, n = out["mask"], out["depth"], out["points"], out["intrinsics"], out["normal"]
    assert torch.isinf(d[~m]).all() and torch.isinf(p[~m]).all() and (n[~m] == 0).all()
    assert (d[m] > 0).all() and torch.equal(p[..., 2][m], d[m])
    u = (torch.arange(518, device="cuda") + 0.5) / 518
    xx = (u[None, None, :] - 0.5) / K[:, 0, 0, None, None] * d
    assert torch.allclose(xx[m], p[..., 0][m], rtol=1e-5, atol=1e-6)
    assert torch.allclose(n[m].norm(dim=-1), torch.ones_like(d[m]), atol=1e-4)
    model.float()


def test_batch_split_streams_are_bit_identical(MoGeModel, tmp_path_factory):
    """The production path runs a batch >= 6 as two half batches on two internal streams (model_v2.hip forward_dispatch);
    every image is computed independently of its batch, so the split result must equal the single-stream result."""
    from moge_amd import _lib as L
    model, cfg, sd = get_model(MoGeModel, "tiny-vits-normal", 0, True, tmp_path_factory)
    try:
        for half in (False, True):
            if half:
                model.half()
            for B in (9, 6, 7):                     # 4 + 5, 3 + 3 (the smallest parts split_parts allows), 3 + 4
                x = torch.rand(B, 3, 84, 112, generator=torch.Generator().manual_seed(3 + B))
                with L.tuned(BATCH_SPLIT=0):
                    ref = model.infer(x, num_tokens=108)
                out = model.infer(x, num_tokens=108)
                for k in ref:
                    a, b = out[k], ref[k]
                    if a.dtype == torch.bool:
                        assert torch.equal(a, b), k
                    else:
                        fin = torch.isfinite(b)
                        assert torch.equal(fin, torch.isfinite(a)) and torch.equal(a[fin], b[fin]), f"{k}: split != single stream (B={B})"
    finally:
        model.float()


def test_fused_resamplers_change_the_fp16_result_by_less_than_the_band(MoGeModel, tmp_path_factory):
    """Round 6: the fp16 decoder runs ConvTranspose2d + 3x3 (modules.py:160-165) as one composed conv where Cin = 2 Cout (conv_pp.hip CT3; FUSE_CT3).  On the bench
    workload's fixture: the fused form is in use (the result differs from FUSE_CT3 = 0 - otherwise this test tests nothing), both sit inside the reference-.half() band
    of the golden (check_fp16 = the gate of the parity tests), and they differ from EACH OTHER by less than half of that band at the p99.9 pixel (observed 0.26: two fp16
    roundings of the same decoder - the fused form rounds the composed weights once where the pair rounds the intermediate map)."""
    from moge_amd import _lib as L
    from oracle import metrics as MX
    case, cfg, sd, x, gold, meta = load_case("vitl_518_t3600")
    model, _, _ = get_model(MoGeModel, None, None, None, tmp_path_factory, case=case)
    st = case.get("stride", 1)
    band = fp16_band(meta, gold, "half")
    try:
        model.half()
        with L.tuned(FUSE_CT3=0):
            pair = sub(model.infer(x), st)
        fused = sub(model.infer(x), st)
    finally:
        model.float()
    assert not np.array_equal(pair["points"], fused["points"]), "FUSE_CT3 changed nothing: the fused resamplers are not being used"
    check_fp16(pair, golden_infer(gold), band)
    check_fp16(fused, golden_infer(gold), band)
    for k in ("points", "depth"):
        e, nmis, n = MX.pixel_errors(k, fused[k], pair[k])
        assert nmis <= 4, (k, nmis)
        assert float(np.quantile(e, 0.999)) <= 0.5 * band[k], (k, float(np.quantile(e, 0.999)), band[k])


def test_single_image_key_split_attention_stays_within_half_a_band(MoGeModel, tmp_path_factory):
    """Round 6 (batch-1 latency): a launch of at most one attention workgroup per CU - a single image - runs attn_pp16ks_kernel: 8-wave workgroups, the key range split
    between the two wave groups and combined through LDS in a fixed order (attention_pp.hip; ATTN_KS).  The same fp32 terms summed in another order: the result is no
    longer bit-identical to the same image inside a large batch (ATTN_KS = 0 is), so the fp16 modes' contract is re-scoped the way VERDICT r05 item 4 states it - fp32
    bit-identical, fp16 within the band.  On the bench workload's fixture: the split form is in use (the outputs differ), deterministic, both forms sit inside the
    reference-.half() band of the golden, and they differ from each other by less than half of that band at the p99.9 pixel."""
    from moge_amd import _lib as L
    from oracle import metrics as MX
    case, cfg, sd, x, gold, meta = load_case("vitl_518_t3600")
    model, _, _ = get_model(MoGeModel, None, None, None, tmp_path_factory, case=case)
    st = case.get("stride", 1)
    band = fp16_band(meta, gold, "half")
    try:
        model.half()
        with L.tuned(ATTN_KS=0):
            plain = sub(model.infer(x), st)
        split = sub(model.infer(x), st)
        again = sub(model.infer(x), st)
    finally:
        model.float()
    assert not np.array_equal(plain["points"], split["points"]), "ATTN_KS changed nothing: the key-split attention is not being used"
    for k in split:
        assert np.array_equal(np.nan_to_num(split[k], posinf=-1.0), np.nan_to_num(again[k], posinf=-1.0)), f"{k}: not deterministic"
    check_fp16(plain, golden_infer(gold), band)
    check_fp16(split, golden_infer(gold), band)
    for k in ("points", "depth"):
        e, nmis, n = MX.pixel_errors(k, split[k], plain[k])
        assert nmis <= 4, (k, nmis)
        assert float(np.quantile(e, 0.999)) <= 0.5 * band[k], (k, float(np.quantile(e, 0.999)), band[k])


def test_head_streams_are_bit_identical(MoGeModel, tmp_path_factory):
    """Small batches run the decoder heads after the first on their own streams and scratch buffers (model_v2.hip forward_impl,
    HEAD_STREAMS); same kernels on the same inputs: the result must equal the one-stream result, alone and inside a split batch.
    HEAD_STREAMS_MAX_B defaults to 1, so the test raises it: B = 3 forks slot 0's streams with a 3-image plan, B = 9 = 4 + 5 forks the head
    streams, events and scratch triples of BOTH sub-plans (slots 0 and 1) under BATCH_SPLIT."""
    import ctypes as C
    from moge_amd import _lib as L
    model, cfg, sd = get_model(MoGeModel, "tiny-vits-normal", 0, True, tmp_path_factory)
    try:
        with L.tuned(HEAD_STREAMS_MAX_B=16):
            for B in (1, 3, 9):
                x = torch.rand(B, 3, 84, 112, generator=torch.Generator().manual_seed(11 + B))
                for half in (False, True):
                    model.half() if half else model.float()
                    with L.tuned(HEAD_STREAMS=0):
                        ref = model.infer(x, num_tokens=108)
                    for pipe in (0, 1, 1):                  # HEAD_PIPE 1 (default): every head on a side stream, released level by level behind the neck; 0: forked behind the whole neck.
                        with L.tuned(HEAD_STREAMS=1, HEAD_PIPE=pipe):      # (twice: the second call reuses streams, events and scratch of the first)
                            for _ in range(2):
                                out = model.infer(x, num_tokens=108)
                                for k in ref:
                                    _same(out[k], ref[k], f"{k}: head streams != one stream (B={B}, half={half}, HEAD_PIPE={pipe})")
            # a subset of the outputs (forward with only normal + mask requested: head 0 is skipped, the first REQUESTED head is not head index 0)
            model.float()
            x = torch.rand(2, 3, 84, 112, generator=torch.Generator().manual_seed(5)).cuda()
            full = model.forward(x, 108)
            for hs, pipe in ((0, 1), (1, 0), (1, 1)):
                with L.tuned(HEAD_STREAMS=hs, HEAD_PIPE=pipe):
                    o = L.Outputs()
                    nrm = torch.empty_like(full["normal"]); mp = torch.empty_like(full["mask"])
                    o.normal, o.mask_prob = nrm.data_ptr(), mp.data_ptr()
                    L.check(L.lib.moge_forward(model._handle, x.data_ptr(), 0, 2, 84, 112, 9, 12, C.byref(o), L.stream_ptr()))
                    torch.cuda.synchronize()
                    assert torch.equal(nrm, full["normal"]) and torch.equal(mp, full["mask"]), f"subset of outputs, HEAD_STREAMS={hs}, HEAD_PIPE={pipe}"
    finally:
        model.float()


def test_eval_plugin_runs_through_the_click_loader(tmp_path_factory):
    """the reference's harness does `Baseline.load.main(args, standalone_mode=False)` then
    `infer_for_evaluation(image, intrinsics)` (moge/scripts/eval_baseline.py:40-42,65-71)."""
    import importlib.util
    from oracle import moge_oracle as O
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    cfg = O.named_configs()["tiny-vits-normal"]
    sd = O.synth_state_dict(cfg, 0, True)
    path = os.path.join(str(tmp_path_factory.mktemp("ckpt")), "model.pt")
    O.save_checkpoint(path, cfg, sd)
    plug = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "baselines", "moge_mi355x.py")
    spec = importlib.util.spec_from_file_location("moge_mi355x_plugin", plug)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    base = mod.Baseline.load.main(["--pretrained", path, "--num_tokens", "108", "--device", "cuda:0", "--version", "v2"], standalone_mode=False)
    x = torch.rand(3, 84, 112, generator=torch.Generator().manual_seed(5)).cuda()
    K = torch.tensor([[0.9, 0.0, 0.5], [0.0, 1.2, 0.5], [0.0, 0.0, 1.0]], device="cuda")
    out = base.infer_for_evaluation(x, K)
    assert set(out) == {"points_metric", "depth_metric", "intrinsics"}                          # baselines/moge.py:77-82: exactly these keys
    ref = O.infer(cfg, sd, x.cpu(), num_tokens=108, fov_x=float(mod._fov_x_degrees(K.cpu())), apply_mask=False)
    assert rel_err(out["depth_metric"].cpu().numpy(), ref["depth"].numpy()) < FP32_TOL
    assert rel_err(out["intrinsics"].cpu().numpy(), ref["intrinsics"].numpy()) < FP32_TOL
    # `--fp16` is autocast on fp32 weights in the plugin (baselines/moge.py:69), never model.half(); infer() ignores the flag (:47)
    base16 = mod.Baseline.load.main(["--pretrained", path, "--num_tokens", "108", "--version", "v2", "--fp16"], standalone_mode=False)
    assert base16.use_fp16 and base16.model.dtype == torch.float32
    same = base16.model.infer(x, fov_x=mod._fov_x_degrees(K), apply_mask=False, num_tokens=108, use_fp16=True)
    got = base16.infer_for_evaluation(x, K)
    assert torch.equal(got["depth_metric"], same["depth"])
    masked = base.infer(x, K)                                                                   # apply_mask=True, the model's default use_fp16=True
    want = base.model.infer(x, fov_x=mod._fov_x_degrees(K), apply_mask=True, num_tokens=108)
    assert torch.equal(torch.nan_to_num(masked["depth_metric"], posinf=-1.0), torch.nan_to_num(want["depth"], posinf=-1.0))


def test_eval_plugin_defaults_to_the_v1_model_like_the_reference(tmp_path_factory):
    """baselines/moge.py:35 - `--version` defaults to v1 and v1 reports the scale-invariant keys (:49-54, :71-76)."""
    import importlib.util
    from oracle import moge_oracle_v1 as O1
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    cfg = O1.named_configs()["tiny-v1-vits"]
    sd = O1.synth_state_dict(cfg, 1, True)
    path = os.path.join(str(tmp_path_factory.mktemp("ckpt1")), "model.pt")
    O1.save_checkpoint(path, cfg, sd)
    plug = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "baselines", "moge_mi355x.py")
    spec = importlib.util.spec_from_file_location("moge_mi355x_plugin", plug)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    base = mod.Baseline.load.main(["--pretrained", path, "--num_tokens", "108"], standalone_mode=False)
    assert base.version == "v1" and type(base.model).__module__.endswith("model.v1")
    x = torch.rand(3, 84, 112, generator=torch.Generator().manual_seed(6)).cuda()
    out = base.infer_for_evaluation(x)
    assert set(out) == {"points_scale_invariant", "depth_scale_invariant", "intrinsics"}
    ref = O1.infer(cfg, sd, x.cpu(), num_tokens=108, apply_mask=False)
    assert rel_err(out["depth_scale_invariant"].cpu().numpy(), ref["depth"].numpy()) < FP32_TOL


def test_master_blob_cache_is_bit_identical_to_the_checkpoint_load(MoGeModel, tmp_path_factory):
    """save_blob -> from_blob and the from_pretrained sidecar reproduce the .pt-loaded model bit for bit (fp32 and fp16 mode)."""
    from oracle import moge_oracle as O
    cfg = O.named_configs()["tiny-vits-normal"]
    sd = O.synth_state_dict(cfg, 3, True)
    d = str(tmp_path_factory.mktemp("blob"))
    path = os.path.join(d, "model.pt")
    O.save_checkpoint(path, cfg, sd)
    m0 = MoGeModel.from_pretrained(path).to("cuda").eval()
    x = torch.rand(2, 3, 84, 112, generator=torch.Generator().manual_seed(11)).cuda()
    ref32 = m0.infer(x, num_tokens=108, use_fp16=False)
    ref16 = m0.infer(x, num_tokens=108, use_fp16=True)
    blob = os.path.join(d, "model.blob")
    m0.save_blob(blob)
    header, off = MoGeModel.read_blob_header(blob)
    assert header["model_config"]["encoder"]["backbone"] == cfg["encoder"]["backbone"] and off % 4096 == 0
    m1 = MoGeModel.from_blob(blob).to("cuda").eval()
    assert m0.cache_blob() == path + ".mi355x-blob"
    m2 = MoGeModel.from_pretrained(path)                       # now served by the sidecar: no state dict on the host
    assert m2._state is None and m2._blob_path == path + ".mi355x-blob"
    m2 = m2.to("cuda").eval()
    for m in (m1, m2):
        o32 = m.infer(x, num_tokens=108, use_fp16=False)
        o16 = m.infer(x, num_tokens=108, use_fp16=True)
        for k in ref32:
            assert torch.equal(o32[k], ref32[k]), k
            assert torch.equal(o16[k], ref16[k]), k
    # a stale sidecar (checkpoint rewritten later) is ignored
    os.utime(path + ".mi355x-blob", (1, 1))
    assert MoGeModel.from_pretrained(path)._state is not None


@pytest.mark.parametrize("shape,tokens", [((37, 211), 96), ((300, 100), 147), ((64, 64), 16), ((97, 131), 300), ((518, 130), 120)])
def test_odd_shapes_and_token_grids_match_the_oracle_fp32(MoGeModel, tmp_path_factory, shape, tokens):
    """Ragged sizes either side of the resampler: down- AND up-sampling in the same image (37x211 -> 5x30 grid), a 1:3 portrait strip,
    the smallest grids, a prime-sized image, a 4:1 strip of the BASELINE height; token grid = Python half-to-even rounding (v2.py:147)."""
    from oracle import moge_oracle as O
    model, cfg, sd = get_model(MoGeModel, "tiny-vits-normal", 0, True, tmp_path_factory)
    H, W = shape
    x = torch.rand(2, 3, H, W, generator=torch.Generator().manual_seed(H * 1000 + W))
    out = model.infer(x, num_tokens=tokens, use_fp16=False)
    ref = O.infer(cfg, sd, x, num_tokens=tokens)
    assert out["mask"].shape == (2, H, W) and out["points"].shape == (2, H, W, 3)
    check_fp32(out, ref)


def _sweep_cases():
    """Seeded random (B, H, W, options) for the tiny model: extremes of size and aspect, every infer() option, per-image fov_x."""
    import random
    rng = random.Random(20260922)
    cases = []
    for i in range(12):
        B = rng.choice([1, 1, 2, 3, 5])
        H, W = rng.choice([(14, 14), (15, 400), (400, 15), (29, 31), (200, 333), (333, 200), (128, 128), (57, 601), (99, 98), (250, 250), (41, 183), (183, 41)])
        opts = dict(apply_mask=rng.random() < 0.7, force_projection=rng.random() < 0.7)
        if rng.random() < 0.5:
            opts["num_tokens"] = rng.choice([16, 30, 64, 100, 150, 256, 333])
        else:
            opts["resolution_level"] = rng.choice([0, 3, 5, 9])
        fov = rng.choice([None, "scalar", "tensor", "tensor"])
        cases.append((i, B, H, W, opts, fov))
    return cases


@pytest.mark.parametrize("i,B,H,W,opts,fov", _sweep_cases())
def test_random_shape_and_option_sweep_matches_the_oracle_fp32(MoGeModel, tmp_path_factory, i, B, H, W, opts, fov):
    """A seeded sweep over what the fixtures hold fixed: batch sizes 1-5, 14-pixel to 600-pixel sides, 1:27 aspect ratios either way, `num_tokens` or
    `resolution_level`, `apply_mask` / `force_projection` on and off, `fov_x` absent / a number / one value per image (v2.py:194-303).  fp32 mode against the
    CPU oracle: every pixel within 1e-3, mask bit-exact (check_fp32)."""
    from oracle import moge_oracle as O
    model, cfg, sd = get_model(MoGeModel, "tiny-vits-normal", 0, True, tmp_path_factory)
    g = torch.Generator().manual_seed(1000 + i)
    x = torch.rand(B, 3, H, W, generator=g)
    kw = dict(opts)
    if fov == "scalar":
        kw["fov_x"] = 55.0
    elif fov == "tensor":
        kw["fov_x"] = torch.tensor([40.0 + 7.0 * b for b in range(B)])
    out = model.infer(x, use_fp16=False, **kw)
    trace = {}
    ref = O.infer(cfg, sd, x, trace=trace, **kw)
    assert out["points"].shape == (B, H, W, 3) and out["mask"].shape == (B, H, W)
    # Knife-edge pixels: the mask is `sigmoid > 0.5 and z + shift > 0` (v2.py:253,268).  Over 10^6 random pixels a few land within float rounding of a
    # threshold (the first run of this sweep: one pixel of 171 285 with the mask logit at 0.5 +- 1e-7), where 1e-7 of forward noise - or the
    # reference's own thread count - decides.  Those pixels, identified from the ORACLE's own margins, are exempt; there must be next to none of them.
    prob = trace["forward"]["mask"].reshape(B, H, W)
    z = trace["forward"]["points"].reshape(B, H, W, 3)[..., 2] + trace["shift"].reshape(B, 1, 1)
    knife = ((prob - 0.5).abs() < 2e-6) | (z.abs() < 2e-6 * z.abs().median())
    assert int(knife.sum()) <= 3, int(knife.sum())
    out = {k: v.cpu().clone() for k, v in out.items()}
    for k in ("points", "depth", "mask", "normal"):
        if k in out:
            out[k][knife] = ref[k][knife]
    check_fp32(out, ref)


@pytest.mark.parametrize("kind", ["black", "white", "flat_gray"])
def test_fp16_mode_on_constant_images_stays_in_band(MoGeModel, tmp_path_factory, kind):
    """Degenerate inputs for the folded LayerNorm (fp16 path: row statistics from partial sums, raw residual in fp16): a constant image gives
    every patch the same embedding, so the token rows differ by the position embedding only.  Outputs must stay finite and within (twice) the fp16 band
    the reference shows on an ordinary image with the same model."""
    from oracle import moge_oracle as O
    model, cfg, sd = get_model(MoGeModel, "tiny-vits-normal", 0, True, tmp_path_factory)
    val = {"black": 0.0, "white": 1.0, "flat_gray": 0.5}[kind]
    x = torch.full((2, 3, 84, 112), val)
    model.half()
    try:
        out = model.infer(x, num_tokens=108, apply_mask=False)
    finally:
        model.float()
    ref = O.infer(cfg, sd, x, num_tokens=108, apply_mask=False)
    for k in ("points", "depth", "intrinsics"):
        a = out[k].float().cpu().numpy()
        assert np.isfinite(a).all(), k
    _c = load_case("tiny_b2_up")
    band = fp16_band(_c[5], _c[4])            # same model: the reference's fp16 drift measured on an ordinary image
    check_fp16({k: out[k] for k in ref}, ref, {k: 2 * v for k, v in band.items()})
