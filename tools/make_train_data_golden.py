"""Golden fixtures of the training data loader's geometric warp (tests/golden/train_*.npz) from the reference's unmodified
`moge.train.dataloader.TrainDataLoaderPipeline._process_instance`, run on the CPU with `image_augmentation = []`.

    python tools/make_train_data_golden.py          (build machine: needs the reference checkout of oracle/make_golden.py)

The method is called on an instance made with `__new__` (the uninstalled `pipeline` and `torchvision` packages are only stubbed).  Beside the
stubs of oracle.make_golden.install_stubs, the un-vendored functions it calls are supplied here:
  * utils3d.np / utils3d: the stand-ins of moge_amd.evaluation (unproject_cv, rotation_matrix_from_vectors, ray_intersection,
    intrinsics_from_focal_center, uv_map, masked_nearest_resize) and moge_amd.train_data (intrinsics_to_fov, focal_to_fov, fov_to_focal);
    depth_map_to_normal_map and depth_map_edge are the numpy references of tests/train_data_reference.py;
  * cv2.warpPerspective: tests/train_data_reference.py `warp_perspective` (float coordinates from the inverted matrix, constant-0 border,
    exact float bilinear and Lanczos-4 weights, nearest at rint).
Pillow's LANCZOS and numpy's nanquantile are the real ones.  Besides the outputs, a fixture keeps the sampled view (tgt_intrinsics, R, flip), the
two pre-resize sizes, max_depth, the bilinear-branch map and the knife-edge pixels (tests/train_data_fixtures.py `knife_map`), of which a
case may have at most 1 %."""
from __future__ import annotations

import json
import os
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from moge_amd import evaluation as E                                                                   # noqa: E402
from moge_amd import train_data as T                                                                   # noqa: E402
from tests import train_data_reference as R                                                            # noqa: E402
from tests.train_data_fixtures import GOLDEN_DIR, build_instance, instance_digest, knife_map           # noqa: E402

KNIFE_CAP = 0.01
REC: dict = {}


def install():
    from oracle.make_golden import install_stubs
    install_stubs()
    cv2 = sys.modules["cv2"]
    cv2.INTER_NEAREST, cv2.INTER_LINEAR, cv2.INTER_LANCZOS4 = R.INTER_NEAREST, R.INTER_LINEAR, R.INTER_LANCZOS4

    def warp_perspective(src, M, dsize, flags=R.INTER_LINEAR, **_):
        out = R.warp_perspective(src, M, dsize, flags=flags)
        REC.setdefault("warps", []).append((flags, src.shape, out))
        return out

    cv2.warpPerspective = warp_perspective
    u, npm = sys.modules["utils3d"], sys.modules["utils3d.np"]

    def depth_map_to_normal_map(depth, intrinsics=None, mask=None, edge_threshold=None, **_):
        assert (mask == np.isfinite(depth)).all()
        return R.normal_map(depth, intrinsics, edge_threshold)

    def depth_map_edge(depth, mask=None, kernel_size=3, ltol=None, **_):
        assert (mask == np.isfinite(depth)).all()
        return mask & ~R.depth_edge(depth, kernel_size, ltol)[0].astype(bool)

    def masked_nearest_resize(image, mask=None, size=None):
        out = E.masked_nearest_resize(image, mask, size)
        REC["nearest_size"] = out[0].shape
        return out

    npm.depth_map_to_normal_map, npm.depth_map_edge, npm.masked_nearest_resize = depth_map_to_normal_map, depth_map_edge, masked_nearest_resize
    npm.unproject_cv = lambda uv, depth, intrinsics=None, **_: E.unproject_cv(uv, depth, intrinsics)
    npm.rotation_matrix_from_vectors = E.rotation_matrix_from_vectors
    npm.ray_intersection = E.ray_intersection
    npm.intrinsics_from_focal_center = E.intrinsics_from_focal_center
    npm.uv_map = lambda *size: E.uv_map(*(size[0] if len(size) == 1 else size))
    npm.intrinsics_to_fov, npm.focal_to_fov, npm.fov_to_focal = T.intrinsics_to_fov, T.focal_to_fov, T.fov_to_focal
    u.focal_to_fov, u.fov_to_focal = T.focal_to_fov, T.fov_to_focal
    for name in ("pipeline", "torchvision", "torchvision.transforms", "torchvision.transforms.v2", "torchvision.transforms.v2.functional"):
        sys.modules.setdefault(name, types.ModuleType(name))


def cases():
    def K(fx, fy, cx, cy):
        return np.array([[fx, 0, cx], [0, fy, cy], [0, 0, 1]], np.float32)

    base = dict(curve=0.05, step_col=0, step_factor=1.0, nan_mod=0, nan_box=[0, 0, 0, 0], inf_rows=0, all_nan=0)
    cfg = dict(center_augmentation=0.5, fov_range_absolute=[1, 179], fov_range_relative=[0.6, 0.97], clamp_max_depth=1000.0, depth_unit=None,
               finite_depth_mask=None)
    out = []
    # (a) up-scale: neither pre-resize runs
    out.append(dict(base, name="upscale", H=32, W=40, tgt_H=48, tgt_W=64, K=K(0.83, 1.07, 0.5, 0.5), image_coef=[[3, 1, 2], [1, 2, 3], [2, 5, 1]],
                    plane=[2.0, 0.06, -0.04], seed=11, config=dict(cfg)))
    # (b) strong down-scale: the Lanczos and the masked-nearest pre-resize run
    out.append(dict(base, name="downscale", H=120, W=160, tgt_H=24, tgt_W=32, K=K(0.91, 1.19, 0.5, 0.5), image_coef=[[5, 3, 4], [2, 7, 2], [7, 1, 5]],
                    plane=[3.0, -0.3, 0.3], nan_mod=29, seed=5, config=dict(cfg)))
    # (c) a scale between 0.8 and 1: the masked-nearest pre-resize runs without Lanczos
    out.append(dict(base, name="mild", H=38, W=50, tgt_H=30, tgt_W=40, K=K(0.88, 1.15, 0.5, 0.5), image_coef=[[1, 4, 3], [6, 1, 1], [3, 3, 2]],
                    plane=[1.5, 0.03, 0.05], nan_mod=23, seed=3, config=dict(cfg, center_augmentation=0.2, fov_range_relative=[0.86, 0.93])))
    # (d) NaN holes, an inf sky band and a step: edge pixels take the nearest branch, NaN and inf survive the clamp; clamp_max_depth cuts
    out.append(dict(base, name="holes", H=36, W=48, tgt_H=30, tgt_W=40, K=K(0.8, 1.05, 0.5, 0.5), image_coef=[[9, 2, 2], [4, 9, 3], [1, 1, 1]],
                    plane=[2.5, 0.05, 0.03], step_col=27, step_factor=2.2, nan_mod=17, nan_box=[18, 30, 6, 17], inf_rows=7, seed=21, config=dict(cfg, clamp_max_depth=1.3)))
    # (e) off-centre principal point with center_augmentation = 1: R far from identity
    out.append(dict(base, name="offcentre", H=40, W=52, tgt_H=36, tgt_W=36, K=K(0.62, 0.81, 0.41, 0.57), image_coef=[[2, 2, 2], [3, 1, 4], [1, 5, 3]],
                    plane=[4.0, 0.15, -0.1], step_col=30, step_factor=1.3, seed=8, config=dict(cfg, center_augmentation=1.0, fov_range_relative=[0.35, 0.6])))
    # (f) one seed that flips and one that does not
    for name, seed in (("flip_yes", None), ("flip_no", None)):
        out.append(dict(base, name=name, H=30, W=44, tgt_H=26, tgt_W=38, K=K(0.9, 1.3, 0.48, 0.52), image_coef=[[7, 3, 1], [2, 6, 2], [5, 1, 3]],
                        plane=[1.2, 0.03, 0.02], nan_mod=37, inf_rows=3, seed=seed, config=dict(cfg)))
    # (g) all-NaN depth: the fallback
    out.append(dict(base, name="allnan", H=24, W=32, tgt_H=20, tgt_W=28, K=K(0.9, 1.2, 0.5, 0.5), image_coef=[[2, 3, 2], [3, 1, 1], [1, 5, 3]],
                    plane=[1.0, 0.0, 0.0], all_nan=1, seed=2, config=dict(cfg)))
    # (h) depth_unit with finite_depth_mask = "only_known": the masks differ on the sky band
    out.append(dict(base, name="metric", H=34, W=46, tgt_H=28, tgt_W=40, K=K(0.86, 1.1, 0.5, 0.5), image_coef=[[4, 1, 2], [1, 3, 1], [6, 2, 3]],
                    plane=[1800.0, 40.0, 30.0], curve=30.0, nan_mod=19, nan_box=[20, 29, 28, 40], inf_rows=6, seed=13, config=dict(cfg, depth_unit=0.001, finite_depth_mask="only_known")))
    # the flip is the fourth draw of the instance's generator: take the first seeds from 100 on that flip / do not
    for c in out:
        if c["seed"] is None:
            want = c["name"] == "flip_yes"
            seed = 100
            while True:
                rng = np.random.default_rng(seed)
                rng.uniform(), rng.uniform(), rng.uniform()
                if bool(rng.choice([True, False])) == want:
                    break
                seed += 1
            c["seed"] = seed
    return out


def main():
    install()
    import torch  # noqa: F401  (the reference module imports it)
    from moge.train.dataloader import TrainDataLoaderPipeline
    from moge.utils.data_augmentation import sample_perspective
    os.makedirs(GOLDEN_DIR, exist_ok=True)
    total = 0
    for case in cases():
        cfg = case.pop("config")
        rec = {k: (np.asarray(v) if not isinstance(v, str) else np.array(v)) for k, v in case.items()}
        rec["config_json"] = np.array(json.dumps(cfg))
        inst = build_instance(rec)
        obj = TrainDataLoaderPipeline.__new__(TrainDataLoaderPipeline)
        obj.clamp_max_depth = cfg["clamp_max_depth"]
        obj.center_augmentation, obj.fov_range_absolute, obj.fov_range_relative = cfg["center_augmentation"], cfg["fov_range_absolute"], cfg["fov_range_relative"]
        obj.image_augmentation = []
        obj.datasets = {"d": {k: cfg[k] for k in ("depth_unit", "finite_depth_mask") if cfg[k] is not None}}
        REC.clear()
        orig = np.nanquantile

        def nanquantile(*a, **k):
            REC["quantile"] = orig(*a, **k)
            return REC["quantile"]

        np.nanquantile = nanquantile
        try:
            with np.errstate(all="ignore"):
                res = TrainDataLoaderPipeline._process_instance(obj, {"image": inst["image"].copy(), "depth": inst["depth"].copy(), "intrinsics": inst["intrinsics"].copy(),
                                                                      "label_type": "synthetic", "dataset": "d", "seed": inst["seed"], "width": inst["width"],
                                                                      "height": inst["height"]})
        finally:
            np.nanquantile = orig
        geo = T.warp_geometry(*inst["depth"].shape, inst["intrinsics"], inst["width"], inst["height"], inst["seed"], center_augmentation=cfg["center_augmentation"],
                              fov_range_absolute=cfg["fov_range_absolute"], fov_range_relative=cfg["fov_range_relative"])
        warps = REC["warps"]                                    # image, eligibility, nearest depth, disparity, normal
        assert [w[0] for w in warps] == [R.INTER_LANCZOS4, R.INTER_LINEAR, R.INTER_NEAREST, R.INTER_LINEAR, R.INTER_LINEAR]
        image_size, nearest_size = warps[0][1][:2], warps[2][1][:2]
        branch = warps[1][2] == 1.0
        # the view and the flip as the reference's own functions draw them from this seed
        rng = np.random.default_rng(inst["seed"])
        ref_K, ref_R = sample_perspective(inst["intrinsics"], inst["width"] / inst["height"], cfg["center_augmentation"], cfg["fov_range_absolute"],
                                          cfg["fov_range_relative"], rng)
        flip = bool(rng.choice([True, False]))
        assert np.array_equal(ref_K, res["intrinsics"].numpy())
        warped_image = warps[0][2][:, ::-1] if flip else warps[0][2]
        assert np.array_equal(res["image"].numpy(), (warped_image.astype(np.float32) / 255.0).transpose(2, 0, 1))
        if flip:
            branch = branch[:, ::-1]
        knife = knife_map(inst, geo)
        invalid = res["label_type"] == "invalid"
        share = 0.0 if invalid else float(knife.mean())
        assert share <= KNIFE_CAP, f"{case['name']}: {share:.2%} knife-edge pixels; change the case"
        depth = res["depth"].numpy()
        z = {f"recipe_{k}": v for k, v in rec.items()}
        z.update(digest=np.array(instance_digest(inst)), tgt_intrinsics=res["intrinsics"].numpy(), R=np.asarray(ref_R), flip=np.array(flip),
                 image_size=np.array(image_size), nearest_size=np.array(nearest_size),
                 image=(res["image"].numpy().transpose(1, 2, 0) * 255).round().astype(np.uint8), depth=depth, normal=res["normal"].numpy(),
                 depth_mask_fin=np.packbits(res["depth_mask_fin"].numpy()), depth_mask_inf=np.packbits(res["depth_mask_inf"].numpy()),
                 bilinear=np.packbits(branch), knife=np.packbits(knife), invalid=np.array(invalid), is_metric=np.array(bool(res["is_metric"])),
                 max_depth=np.array(np.float32(REC["quantile"]) * np.float32(cfg["clamp_max_depth"]), np.float32))
        path = os.path.join(GOLDEN_DIR, f"train_{case['name']}.npz")
        np.savez_compressed(path, **z)
        total += os.path.getsize(path)
        print(f"{case['name']}: image {tuple(image_size)}, nearest {tuple(nearest_size)}, flip {flip}, knife {int(knife.sum())} ({share:.2%}), bilinear "
              f"{branch.mean():.0%}, finite {np.isfinite(depth).mean():.0%}, invalid {invalid}, max_depth {float(z['max_depth']):.6g}, {os.path.getsize(path) / 1e3:.0f} kB")
    print(f"total {total / 1e6:.2f} MB")


if __name__ == "__main__":
    main()
