"""GPU: MoGe-1 (`moge.model.v1.MoGeModel`) through the v1 mirror -> `moge_create_v1 / moge_v1_forward / moge_v1_infer`
against the committed fixtures of the REAL reference v1 class (tests/golden/v1_*.npz) and the live CPU oracle (oracle/moge_oracle_v1.py).
Same gates as the MoGe-2 parity tests: fp32 mode every pixel within 1e-3 and the mask bit-exact; fp16 mode inside 1.6x (per-image numbers, mask flips: 2x) the reference's own
fp16-vs-fp32 drift."""
import os

import pytest
import torch

from tests.golden_util import gate_line, CASE_BY_NAME, SLOW_CASES, check_fp16, check_fp32, fp16_band, load_case, rel_err, subsample

pytestmark = pytest.mark.gpu
V1 = [n for n, c in CASE_BY_NAME.items() if c.get("version") == "v1"]
_models = {}


def get_model(case, tmp_path_factory):
    from moge_amd.model import import_model_class_by_version
    from oracle import moge_oracle_v1 as O1
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    key = (case["config"], case["seed"])
    if key not in _models:
        cfg = O1.named_configs()[case["config"]]
        sd = O1.synth_state_dict(cfg, case["seed"], case["sane"])
        path = os.path.join(str(tmp_path_factory.mktemp("ckpt")), "model.pt")
        O1.save_checkpoint(path, cfg, sd)
        _models[key] = import_model_class_by_version("v1").from_pretrained(path).to("cuda").eval()
    return _models[key]


def sub(out, st):
    return {k: subsample(k, v.cpu().numpy(), st) for k, v in out.items()}


@pytest.mark.parametrize("name", V1)
def test_v1_fp32_mode_matches_reference_golden_and_oracle(name, tmp_path_factory):
    from oracle import moge_oracle_v1 as O1
    case, cfg, sd, x, gold, meta = load_case(name)
    model = get_model(case, tmp_path_factory)
    kw = dict(case["kwargs"]); kw["use_fp16"] = False
    out = model.float().infer(x, **kw)
    st = case.get("stride", 1)
    g = {k[6:]: v for k, v in gold.items() if k.startswith("infer.")}
    seen = check_fp32(sub(out, st), g)
    print(f"[parity v1 fp32] {name}: " + " ".join(f"{k}={v:.1e}" for k, v in seen.items()))
    if name not in SLOW_CASES:
        ref = O1.infer(cfg, sd, x, **{k: v for k, v in kw.items() if k != "use_fp16"})
        check_fp32(out, ref)
        # raw forward outputs (points after the remap, mask without activation: v1.py:289-297)
        nt = kw.get("num_tokens") or int(cfg["num_tokens_range"][0] + (kw.get("resolution_level", 9) / 9) * (cfg["num_tokens_range"][1] - cfg["num_tokens_range"][0]))
        xb = x if x.dim() == 4 else x[None]
        fwd = model.forward(xb, nt)
        rf = O1.forward(cfg, sd, xb, nt)
        for k in rf:
            assert rel_err(fwd[k].cpu().numpy(), rf[k].numpy()) < 5e-4, k


@pytest.mark.parametrize("name", V1)
def test_v1_fp16_mode_within_reference_fp16_band(name, tmp_path_factory):
    case, cfg, sd, x, gold, meta = load_case(name)
    model = get_model(case, tmp_path_factory)
    kw = dict(case["kwargs"]); kw["use_fp16"] = True
    st = case.get("stride", 1)
    bands = {"autocast": fp16_band(meta, gold, "autocast"), "half": fp16_band(meta, gold, "half")}      # the reference's own drift, per fp16 form
    g = {k[6:]: v for k, v in gold.items() if k.startswith("infer.")}
    try:
        out = model.float().infer(x, **kw)
        out_h = model.half().infer(x, **kw)
    finally:
        model.float()
    for tag, o in (("autocast", out), ("half", out_h)):
        band = bands[tag]
        seen = check_fp16(sub(o, st), g, band)
        print(f"[gate v1 fp16 {tag}] {name}: " + gate_line(seen, band))


REDRAWN = [n for n in V1 if os.path.exists(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", n + ".redraws.json"))]


@pytest.mark.parametrize("name", REDRAWN)
def test_v1_fp16_forward_noise_against_the_reference_redraws(name, tmp_path_factory):
    """Fixtures whose focal / shift solve is ill-conditioned (v1_vitl_518) take their infer() band from the widest of the reference's own re-draws
    (golden_util.fp16_band) - a wide band.  The NETWORK in front of the solve is therefore gated here on a statistic that does not move from draw to draw: the raw
    point map of forward() in the .half() form against the reference's fp32 forward, mean |diff| / mean |points|, at most FP16_FACTOR x the same number of the
    reference's own .half() forward (its re-draws agree to 1 %: 9.0e-4 on v1_vitl_518; the library: 8.4e-4) - with the batch-invariant attention and with the
    key-split form at three split points (four draws of the library's own rounding noise), which must also agree with each other to 5 %."""
    import numpy as np
    from moge_amd import _lib as L
    from tests.golden_util import FP16_FACTOR
    case, cfg, sd, x, gold, meta = load_case(name)
    model = get_model(case, tmp_path_factory)
    st = case.get("stride", 1)
    kw = case["kwargs"]
    nt = kw.get("num_tokens") or int(cfg["num_tokens_range"][0] + (kw.get("resolution_level", 9) / 9) * (cfg["num_tokens_range"][1] - cfg["num_tokens_range"][0]))
    ref_noise = [r["half"]["forward_points_noise"] for r in meta["redraws16"]]
    assert max(ref_noise) <= 1.15 * min(ref_noise), ref_noise          # the statistic is stable on the reference's side
    gf = gold["forward.points"].astype(np.float64)
    xb = x if x.dim() == 4 else x[None]
    seen = []
    try:
        model.half()
        for ks, mid in ((0, 0), (1, 0), (1, 9), (1, 25)):
            with L.tuned(ATTN_KS=ks, ATTN_KS_MID=mid):
                f = model.forward(xb, nt)["points"].float().cpu().numpy()[:, ::st, ::st].astype(np.float64)
            seen.append(float(np.abs(f - gf).mean() / np.abs(gf).mean()))
    finally:
        model.float()
    print(f"[gate v1 fp16 half forward] {name}: library " + " / ".join(f"{v:.2e}" for v in seen) + f" reference {min(ref_noise):.2e} ... {max(ref_noise):.2e}")
    assert max(seen) <= FP16_FACTOR * float(np.median(ref_noise)), (seen, ref_noise)
    assert max(seen) <= 1.05 * min(seen), seen


def test_v1_properties_and_errors(tmp_path_factory):
    case = CASE_BY_NAME["v1_tiny_b2"]
    model = get_model(case, tmp_path_factory)
    x = torch.rand(3, 3, 84, 112, generator=torch.Generator().manual_seed(2))
    a = model.infer(x, num_tokens=100)
    b = model.infer(x, num_tokens=100)
    for k in a:
        assert torch.equal(a[k], b[k]), f"{k} not deterministic"
    one = model.infer(x[1], num_tokens=100)
    for k in a:
        u, v = a[k][1], one[k]
        fin = torch.isfinite(u) if u.dtype != torch.bool else torch.ones_like(u)
        assert torch.equal(u[fin], v[fin]), f"{k}: batch item depends on its batch"
    assert set(a) == {"points", "intrinsics", "depth", "mask"} and a["mask"].dtype == torch.bool
    assert torch.isinf(a["depth"][~a["mask"]]).all()
    with pytest.raises(ValueError):
        model.infer(x, num_tokens=100, fov_x=torch.tensor([50.0, 60.0]))
    from moge_amd import _lib as L
    import ctypes as C
    o = L.Outputs()
    assert L.lib.moge_forward(model._handle, x.cuda().data_ptr(), 0, 3, 84, 112, 6, 8, C.byref(o), None) == -1      # v2 entry point on a v1 handle


def test_panorama_view_batching_matches_per_view_infer(tmp_path_factory):
    """infer_panorama.py:97-104 with the v1 model (the script's default): batches of 4 views with a per-view fov_x tensor."""
    import numpy as np
    from moge_amd.panorama import infer_panorama_views, intrinsics_to_fov_x_deg
    model = get_model(CASE_BY_NAME["v1_tiny_b2"], tmp_path_factory)
    rng = np.random.default_rng(3)
    views = [(rng.random((64, 64, 3)) * 255).astype(np.uint8) for _ in range(6)]
    Ks = [np.array([[0.5 + 0.05 * i, 0, 0.5], [0, 0.5 + 0.05 * i, 0.5], [0, 0, 1.0]]) for i in range(6)]
    dist, masks = infer_panorama_views(model, views, Ks, batch_size=4, num_tokens=64)
    assert len(dist) == len(masks) == 6 and dist[0].shape == (64, 64) and masks[0].dtype == bool
    assert abs(float(intrinsics_to_fov_x_deg(Ks[0])[0]) - 90.0) < 1e-4
    for i in (0, 5):
        x = torch.tensor(views[i] / 255, dtype=torch.float32).permute(2, 0, 1)
        one = model.infer(x, fov_x=float(intrinsics_to_fov_x_deg(Ks[i])[0]), apply_mask=False, num_tokens=64)
        assert np.array_equal(one["points"].norm(dim=-1).cpu().numpy(), dist[i]) and np.array_equal(one["mask"].cpu().numpy(), masks[i])


def test_panorama_pipeline_runs_end_to_end_on_the_gpu(tmp_path_factory):
    """scripts/infer_panorama.py:86-121 through moge_amd.panorama.infer_panorama with the real (tiny, synthetic) v1 model on the GPU: 12 views
    in batches of 5, merge, resize.  The synthetic weights make the geometry meaningless; what is checked is the plumbing - the per-view maps
    are what infer() returns for those views, and the merged map is finite, positive and at the panorama's size (the merge itself is pinned
    against an analytic scene in tests/test_panorama_cpu.py)."""
    import numpy as np
    from moge_amd import panorama as P
    model = get_model(CASE_BY_NAME["v1_tiny_b2"], tmp_path_factory)
    H, W = 96, 192
    d = P.spherical_uv_to_directions(P._uv_grid(H, W))
    pano = np.clip((d * 0.5 + 0.5) * 255, 0, 255).astype(np.uint8)
    out = P.infer_panorama(model, pano, resolution=64, batch_size=5, merge_size=(128, 64), num_tokens=64)
    assert out["distance"].shape == (H, W) and out["distance"].dtype == np.float32 and out["points"].shape == (H, W, 3)
    assert out["mask"].shape == (H, W) and out["mask"].dtype == bool
    assert np.isfinite(out["distance"]).all() and (out["distance"] > 0).all()
    assert len(out["views"]) == len(out["view_distance"]) == len(out["view_mask"]) == 12
    E, Ks = P.get_panorama_cameras()
    x = torch.tensor(out["views"][7] / 255, dtype=torch.float32).permute(2, 0, 1)
    one = model.infer(x, fov_x=90.0, apply_mask=False, num_tokens=64)
    assert np.array_equal(one["points"].norm(dim=-1).cpu().numpy(), out["view_distance"][7])


@pytest.mark.parametrize("fp16", [False, True])
def test_v1_infer_uint8_equals_infer_of_the_callers_float_tensor(tmp_path_factory, fp16):
    """scripts/infer.py:98 with --version v1: `torch.tensor(image / 255, dtype=torch.float32).permute(2, 0, 1)` then infer(); infer_uint8 does the
    division, layout change and dtype cast on the device (moge_v1_infer img_dtype 2) - bit-identical outputs, batch and single image."""
    import numpy as np
    model = get_model(CASE_BY_NAME["v1_tiny_b2"], tmp_path_factory)
    rng = np.random.default_rng(11)
    imgs = (rng.random((2, 84, 112, 3)) * 255).astype(np.uint8)
    x = torch.stack([torch.tensor(im / 255, dtype=torch.float32).permute(2, 0, 1) for im in imgs]).cuda()
    try:
        m = model.half() if fp16 else model.float()
        ref = m.infer(x, num_tokens=100, use_fp16=fp16)
        out = m.infer_uint8(torch.from_numpy(imgs), num_tokens=100, use_fp16=fp16)
        one = m.infer_uint8(torch.from_numpy(imgs[1]), num_tokens=100, use_fp16=fp16)
    finally:
        model.float()
    assert set(out) == set(ref) == {"points", "depth", "intrinsics", "mask"}
    for k in ref:
        assert torch.equal(out[k], ref[k]), k
        assert torch.equal(one[k], ref[k][1]), k
    with pytest.raises(ValueError):
        model.infer_uint8(torch.zeros(3, 70, 98, dtype=torch.uint8))


def test_cli_runs_the_v1_model(tmp_path, tmp_path_factory):
    """`moge infer --version v1` (scripts/infer.py:22, 82): the CLI picks the class by version; --show is accepted (no viewer here) and warns."""
    import numpy as np
    from PIL import Image
    from click.testing import CliRunner
    from moge_amd import io as IO
    from moge_amd.scripts.infer import main as cli
    from oracle import moge_oracle_v1 as O1
    cfg = O1.named_configs()["tiny-v1-vits"]
    ckpt = str(tmp_path / "model.pt")
    O1.save_checkpoint(ckpt, cfg, O1.synth_state_dict(cfg, 0, True))
    rng = np.random.default_rng(6)
    src = tmp_path / "in"
    src.mkdir()
    im = (rng.random((84, 112, 3)) * 255).astype(np.uint8)
    Image.fromarray(im).save(src / "a.png")
    out = tmp_path / "out"
    with pytest.warns(UserWarning, match="no viewer"):
        r = CliRunner().invoke(cli, ["-i", str(src), "-o", str(out), "--pretrained", ckpt, "--version", "v1", "--num_tokens", "100", "--maps", "--ply", "--show"],
                               catch_exceptions=False)
    assert r.exit_code == 0, r.output
    d = out / "a"
    for f in ("image.jpg", "depth_vis.png", "depth.exr", "points.exr", "mask.png", "fov.json", "pointcloud.ply"):
        assert (d / f).exists(), f
    assert not (d / "normal.png").exists() and not (d / "mesh.glb").exists()          # MoGe-1 has no normal head; --glb was not asked for
    model = get_model(CASE_BY_NAME["v1_tiny_b2"], tmp_path_factory)                   # same config and seed as the checkpoint above
    ref = model.float().infer_uint8(torch.from_numpy(im), num_tokens=100, use_fp16=False)
    assert np.array_equal(IO.read_exr(d / "depth.exr"), ref["depth"].cpu().numpy())
