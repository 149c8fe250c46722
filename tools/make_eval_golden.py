"""Golden fixtures of the evaluation data loader's view warp (tests/golden/eval_*.npz) from the reference's unmodified
`moge.test.dataloader.EvalDataLoaderPipeline._process_instance`, run on the CPU.

    python tools/make_eval_golden.py          (build machine: needs the reference checkout of oracle/make_golden.py)

The method is called on an instance made with `__new__` (the uninstalled `pipeline` package is only stubbed).  Beside the stubs of
oracle.make_golden.install_stubs, the un-vendored functions it calls are supplied here:
  * utils3d.np: the stand-ins of moge_amd.evaluation (unproject_cv, rotation_matrix_from_vectors, ray_intersection,
    intrinsics_from_focal_center, uv_map, uv_to_pixel, depth_map_to_point_map, masked_nearest_resize);
  * cv2: resize(INTER_NEAREST) as resizeNN (floor(d / (out / in)), clamped) and remap with a constant-0 border: INTER_LINEAR with exact float
    weights (the panorama goldens' convention, no INTER_BITS fixed point), INTER_NEAREST at rint (half to even).
Pillow's LANCZOS and numpy's nanquantile are the real ones.  Besides the outputs, the fixture keeps the Lanczos image (sha256 and a crop), the masked nearest
depth (as the reference passes them on), max_depth, and the knife-edge pixels: those whose remap coordinate lies within 1e-4 px of a
nearest-rounding boundary."""
from __future__ import annotations

import hashlib
import json
import os
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from moge_amd import evaluation as E                                                    # noqa: E402
from tests.eval_fixtures import GOLDEN_DIR, build_instance, instance_digest            # noqa: E402

KNIFE = 1e-4
REC: dict = {}


def _remap_linear(src, mx, my):
    H, W = src.shape[:2]
    img = src.astype(np.float32).reshape(H, W, -1)
    fx0, fy0 = np.floor(mx), np.floor(my)
    fx, fy = (mx - fx0)[..., None], (my - fy0)[..., None]
    x0, y0 = fx0.astype(np.int64), fy0.astype(np.int64)

    def tap(yy, xx):
        inside = (xx >= 0) & (xx < W) & (yy >= 0) & (yy < H)
        return img[np.clip(yy, 0, H - 1), np.clip(xx, 0, W - 1)] * inside[..., None].astype(np.float32)

    one = np.float32(1)
    out = (tap(y0, x0) * (one - fx) + tap(y0, x0 + 1) * fx) * (one - fy) + (tap(y0 + 1, x0) * (one - fx) + tap(y0 + 1, x0 + 1) * fx) * fy
    return np.clip(np.rint(out), 0, 255).astype(np.uint8).reshape(mx.shape + src.shape[2:])


def _remap_nearest(src, mx, my):
    H, W = src.shape[:2]
    rx, ry = np.rint(mx), np.rint(my)
    inside = (rx >= 0) & (rx <= W - 1) & (ry >= 0) & (ry <= H - 1)
    out = src[np.clip(ry, 0, H - 1).astype(np.int64), np.clip(rx, 0, W - 1).astype(np.int64)]
    return np.where(inside, out, np.zeros((), src.dtype))


def _knife(m):
    f = m - np.floor(m)
    return np.abs(f - 0.5) < KNIFE


def install():
    from oracle.make_golden import install_stubs
    install_stubs()
    cv2 = sys.modules["cv2"]
    cv2.INTER_NEAREST, cv2.INTER_LINEAR, cv2.INTER_LANCZOS4 = 0, 1, 4

    def resize(src, dsize, interpolation=1, **_):
        assert interpolation == cv2.INTER_NEAREST
        w, h = dsize
        H, W = src.shape[:2]
        sx = np.minimum(np.floor(np.arange(w) * (1.0 / (w / W))).astype(np.int64), W - 1)
        sy = np.minimum(np.floor(np.arange(h) * (1.0 / (h / H))).astype(np.int64), H - 1)
        return src[sy][:, sx]

    def remap(src, mx, my, interpolation, **_):
        if interpolation == cv2.INTER_LINEAR:
            REC["lanczos"] = src.copy()
            REC["knife"] = _knife(mx) | _knife(my)
            return _remap_linear(src, mx, my)
        return _remap_nearest(src, mx, my)

    cv2.resize, cv2.remap = resize, remap
    npm = sys.modules["utils3d.np"]

    def masked_nearest_resize(image, mask, size):
        out = E.masked_nearest_resize(image, mask, size)
        REC["mnr_depth"], REC["mnr_mask"] = out[0].copy(), out[1].copy()
        return out

    npm.unproject_cv = lambda uv, depth, intrinsics=None, **_: E.unproject_cv(uv, depth, intrinsics)
    npm.rotation_matrix_from_vectors = E.rotation_matrix_from_vectors
    npm.ray_intersection = E.ray_intersection
    npm.intrinsics_from_focal_center = E.intrinsics_from_focal_center
    npm.uv_map = E.uv_map
    npm.uv_to_pixel = E.uv_to_pixel
    npm.depth_map_to_point_map = lambda depth, intrinsics=None, **_: E.depth_map_to_point_map(depth, intrinsics)
    npm.masked_nearest_resize = masked_nearest_resize
    sys.modules.setdefault("pipeline", types.ModuleType("pipeline"))


def cases():
    def K(fx, fy, cx, cy):
        return np.array([[fx, 0, cx], [0, fy, cy], [0, 0, 1]], np.float32)

    rng = np.random.default_rng(7)
    out = []
    base = dict(nan_mod=0, inf_mod=0, all_invalid=0)
    cfg = dict(drop_max_depth=1000.0, depth_unit=1.0, include_segmentation=False, max_segments=100, min_seg_area=1000, has_sharp_boundary=False)
    # 1. NYU-like: centred intrinsics, same size
    out.append(dict(base, name="nyu", H=240, W=320, tgt_H=240, tgt_W=320, K=K(0.9, 1.2, 0.5, 0.5), image_coef=[[3, 1, 5], [1, 2, 3], [2, 5, 4]],
                    depth_grid=np.round(rng.uniform(1, 8, (6, 8)), 2).astype(np.float16), nan_mod=53, config=dict(cfg)))
    # 2. KITTI-like: off-centre principal point (R != I), raw 1216 x 352 -> 750 x 375, NaN and inf depth, a drop_max_depth that cuts
    out.append(dict(base, name="kitti", H=352, W=1216, tgt_H=375, tgt_W=750, K=K(0.595, 2.05, 0.53, 0.46), image_coef=[[5, 3, 4], [2, 7, 2], [7, 1, 5]],
                    depth_grid=np.round(rng.uniform(4, 60, (5, 16)), 2).astype(np.float16), nan_mod=31, inf_mod=89,
                    config=dict(cfg, drop_max_depth=3.0)))
    # 3. iBims-like: 120 labels incl. sky / background; max_segments and min_seg_area both cut
    ex = np.concatenate([[0], np.sort(rng.choice(np.arange(4, 316), 11, replace=False)), [320]])
    ey = np.concatenate([[0], np.sort(rng.choice(np.arange(4, 236), 9, replace=False)), [240]])
    ids = rng.permutation(np.arange(1, 121)).reshape(10, 12).astype(np.uint8)
    names = {f"obj{i:03d}": int(i) for i in range(1, 121)}
    names["sky"], names["background"] = names.pop("obj007"), names.pop("obj042")
    names = dict(sorted(names.items(), key=lambda kv: kv[1] * 37 % 121))          # label order unrelated to ids or areas
    out.append(dict(base, name="ibims", H=240, W=320, tgt_H=240, tgt_W=320, K=K(0.85, 1.13, 0.5, 0.5), image_coef=[[1, 4, 3], [6, 1, 1], [3, 3, 5]],
                    depth_grid=np.round(rng.uniform(1, 6, (8, 8)), 2).astype(np.float16), nan_mod=97, seg_x=ex, seg_y=ey, seg_ids=ids,
                    labels_json=json.dumps(names), config=dict(cfg, include_segmentation=True, max_segments=80, min_seg_area=300)))
    # 4. x3 downscale at a reduced ETH3D aspect (1512 x 1008 -> 504 x 336), depth_unit None, uint16 labels
    ex = np.arange(7) * 1512 // 6
    ey = np.arange(5) * 1008 // 4
    ids = (np.arange(24).reshape(4, 6) * 1111 + 300).astype(np.uint16)
    names = {f"part{i}": int(v) for i, v in enumerate(ids.ravel())}
    out.append(dict(base, name="eth3d", H=1008, W=1512, tgt_H=336, tgt_W=504, K=K(0.62, 0.93, 0.51, 0.495), image_coef=[[9, 2, 5], [4, 9, 3], [1, 1, 6]],
                    depth_grid=np.round(rng.uniform(2, 30, (12, 18)), 2).astype(np.float16), nan_mod=41, seg_x=ex, seg_y=ey, seg_ids=ids,
                    labels_json=json.dumps(names), config=dict(cfg, depth_unit=None, include_segmentation=True, min_seg_area=2000)))
    # 5. all-invalid depth: the label_type 'invalid' fallback
    out.append(dict(base, name="invalid", H=120, W=160, tgt_H=120, tgt_W=160, K=K(0.9, 1.2, 0.5, 0.5), image_coef=[[2, 2, 2], [3, 1, 4], [1, 5, 3]],
                    depth_grid=np.ones((2, 2), np.float16), all_invalid=1, config=dict(cfg)))
    return out


def main():
    install()
    import torch  # noqa: F401  (the reference module imports it)
    from moge.test.dataloader import EvalDataLoaderPipeline
    os.makedirs(GOLDEN_DIR, exist_ok=True)
    total = 0
    for case in cases():
        cfg = case.pop("config")
        rec = {k: (np.asarray(v) if not isinstance(v, str) else np.array(v)) for k, v in case.items()}
        rec["config_json"] = np.array(json.dumps(cfg))
        inst = build_instance(rec)
        digest = instance_digest(inst)
        obj = EvalDataLoaderPipeline.__new__(EvalDataLoaderPipeline)
        for k, v in cfg.items():
            setattr(obj, k, v)
        REC.clear()
        orig = np.nanquantile

        def nanquantile(*a, **k):
            REC["max_depth_q"] = orig(*a, **k)
            return REC["max_depth_q"]

        np.nanquantile = nanquantile
        try:
            res = EvalDataLoaderPipeline._process_instance(obj, dict(inst))
        finally:
            np.nanquantile = orig
        geo = E.warp_geometry(inst["image"].shape[0], inst["image"].shape[1], inst["intrinsics"], inst["width"], inst["height"])
        depth = res["depth"].numpy()
        z = {f"recipe_{k}": v for k, v in rec.items()}
        z.update(
            digest=np.array(digest),
            lanczos_sha256=np.array(hashlib.sha256(np.ascontiguousarray(REC["lanczos"]).tobytes()).hexdigest()), lanczos_crop=REC["lanczos"][:64, :96],
            mnr_depth=REC["mnr_depth"], mnr_mask=np.packbits(REC["mnr_mask"]),
            image_rows=(res["image"].numpy().transpose(1, 2, 0) * 255).round().astype(np.uint8)[::2],
            depth_rows=depth[::6], depth_mask=np.packbits(res["depth_mask"].numpy()), points_sub=res["points"].numpy()[::6, ::6],
            knife=np.packbits(REC["knife"]),
            max_depth=np.array(np.float32(REC["max_depth_q"]) * np.float32(cfg["drop_max_depth"]), np.float32),
            tgt_intrinsics=res["intrinsics"].numpy(), transform=geo["transform"], rescaled_size=np.array(REC["lanczos"].shape[:2]),
            segmentation_labels=np.array(json.dumps(res.get("segmentation_labels"))),
            label_type=np.array(res.get("label_type", "")),
        )
        assert (z["rescaled_size"] == np.array(geo["rescaled_size"])).all()
        path = os.path.join(GOLDEN_DIR, f"eval_{case['name']}.npz")
        np.savez_compressed(path, **z)
        total += os.path.getsize(path)
        print(f"{case['name']}: rescaled {tuple(z['rescaled_size'])}, knife {int(REC['knife'].sum())}, label_type {z['label_type']}, "
              f"{os.path.getsize(path) / 1e3:.0f} kB")
    print(f"total {total / 1e6:.2f} MB")


if __name__ == "__main__":
    main()
