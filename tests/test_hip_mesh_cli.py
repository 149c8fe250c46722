"""The export commands write the same bytes whether the mesh is built on the GPU (moge_amd.mesh, the default) or on the host (`--host_mesh`,
moge_amd.io.build_mesh_from_map): `moge_amd.scripts.infer` on two images of different sizes (plus a third that shares a batch with the
first), `moge_amd.scripts.infer_baseline` on one and `moge_amd.scripts.infer_panorama` on one small equirectangular image (tiny MoGe-1
checkpoint; the command takes about half a second with it), driven through click with the tiny synthetic checkpoints the way
tests/test_caller_side.py drives them.

The synthetic checkpoint's depth is noise, which the default edge threshold removes to the last pixel (an empty mesh on both paths proves
little), so the commands run with `--threshold 1e9`: then only the neighbours of masked-out pixels are edges, about a third of the image is
left, and each compared file holds thousands of vertices.
"""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ckpt(tmp_path_factory):
    from oracle import moge_oracle as O
    cfg = O.named_configs()["tiny-vits-normal"]
    path = str(tmp_path_factory.mktemp("ckpt") / "model.pt")
    O.save_checkpoint(path, cfg, O.synth_state_dict(cfg, 0, True))
    return path


def test_infer_writes_the_same_files_with_the_device_and_the_host_mesh(tmp_path, ckpt):
    from PIL import Image
    from click.testing import CliRunner
    from moge_amd.scripts.infer import main as cli
    rng = np.random.default_rng(11)
    src = tmp_path / "in"
    (src / "sub").mkdir(parents=True)
    imgs = {"a.png": (84, 112), "b.png": (84, 112), "sub/c.png": (70, 98)}
    for name, (h, w) in imgs.items():
        Image.fromarray((rng.random((h, w, 3)) * 255).astype(np.uint8)).save(src / name)
    outs = {}
    for key, extra in (("device", []), ("host", ["--host_mesh"])):
        outs[key] = tmp_path / key
        args = ["-i", str(src), "-o", str(outs[key]), "--pretrained", ckpt, "--num_tokens", "108", "--batch", "2", "--glb", "--ply", "--threshold", "1e9"] + extra
        r = CliRunner().invoke(cli, args, catch_exceptions=False)
        assert r.exit_code == 0, r.output
    for name in imgs:
        for f in ("mesh.glb", "pointcloud.ply"):
            a, b = ((outs[k] / name[:-4] / f).read_bytes() for k in ("device", "host"))
            assert len(a) > 20000 and a == b, (name, f, len(a), len(b))


def test_infer_baseline_writes_the_same_files_with_the_device_and_the_host_mesh(tmp_path, ckpt):
    from PIL import Image
    from click.testing import CliRunner
    from moge_amd.scripts.infer_baseline import main as cli
    src = tmp_path / "in"
    src.mkdir()
    Image.fromarray((np.random.default_rng(12).random((84, 112, 3)) * 255).astype(np.uint8)).save(src / "a.png")
    plug = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "baselines", "moge_mi355x.py")
    outs = {}
    for key, extra in (("device", []), ("host", ["--host_mesh"])):
        outs[key] = tmp_path / key
        args = ["--baseline", plug, "-i", str(src), "-o", str(outs[key]), "--ply", "--glb", "--threshold", "1e9"] + extra + ["--pretrained", ckpt, "--version", "v2", "--num_tokens", "108"]
        r = CliRunner().invoke(cli, args, catch_exceptions=False)
        assert r.exit_code == 0, r.output
    for f in ("mesh.glb", "mesh.ply"):
        a, b = ((outs[k] / "a" / f).read_bytes() for k in ("device", "host"))
        assert len(a) > 20000 and a == b, (f, len(a), len(b))


def test_infer_panorama_writes_the_same_files_with_the_device_and_the_host_mesh(tmp_path):
    from PIL import Image
    from click.testing import CliRunner
    from moge_amd.scripts.infer_panorama import main as cli
    from oracle import moge_oracle_v1 as O1
    cfg = O1.named_configs()["tiny-v1-vits"]
    ckpt = str(tmp_path / "v1.pt")
    O1.save_checkpoint(ckpt, cfg, O1.synth_state_dict(cfg, 0, True))
    yy, xx = np.meshgrid(np.linspace(0, 1, 96), np.linspace(0, 1, 192), indexing="ij")
    src = tmp_path / "in"
    src.mkdir()
    Image.fromarray((np.stack([xx, yy, 0.5 + 0.5 * np.sin(6 * xx)], -1) * 255).astype(np.uint8)).save(src / "p.png")
    outs = {}
    for key, extra in (("device", []), ("host", ["--host_mesh"])):
        outs[key] = tmp_path / key
        args = ["-i", str(src), "-o", str(outs[key]), "--pretrained", ckpt, "--version", "v1", "--glb", "--ply", "--threshold", "1e9"] + extra
        r = CliRunner().invoke(cli, args, catch_exceptions=False)
        assert r.exit_code == 0, r.output
    for f in ("mesh.glb", "mesh.ply"):
        a, b = ((outs[k] / "p" / f).read_bytes() for k in ("device", "host"))
        assert len(a) > 20000 and a == b, (f, len(a), len(b))
