"""Plain numpy references of the training-data kernels (csrc/traindata.hip), written from the conventions of DESIGN.md section 16 and vectorised
over whole maps.  `warp_perspective` below is also the `cv2.warpPerspective` stand-in under which tools/make_train_data_golden.py runs the
reference's `_process_instance`, so tests/test_train_data_cpu.py pins these functions to the reference's results.

Everything is float32 with numpy's operation order (no fused multiply-add), so the kernels can agree bit for bit except where they call
logf / sin / cos."""
from __future__ import annotations

import warnings

import numpy as np
from PIL import Image

from moge_amd import evaluation as E
from moge_amd import train_data as T

F = np.float32
INTER_NEAREST, INTER_LINEAR, INTER_LANCZOS4 = 0, 1, 4


def _norm(v):
    return np.sqrt((v[..., 0] * v[..., 0] + v[..., 1] * v[..., 1]) + v[..., 2] * v[..., 2])


# ------------------------------------------------------------------------------------------------------------------------------------------
# normal map and depth edge
# ------------------------------------------------------------------------------------------------------------------------------------------
def normal_map(depth: np.ndarray, intrinsics: np.ndarray, edge_threshold: float = 88.0, return_angles: bool = False):
    """-> (normal (H, W, 3) with NaN where no face counts, mask); return_angles adds the (H, W, 4) face angles in degrees (NaN where a face
    has an invalid corner)"""
    depth = np.asarray(depth, F)
    H, W = depth.shape
    K = np.asarray(intrinsics, F)
    u = (np.arange(W, dtype=F) + F(0.5)) / F(W)
    v = (np.arange(H, dtype=F) + F(0.5)) / F(H)
    with np.errstate(all="ignore"):
        p = np.stack([(u[None, :] - K[0, 2]) / K[0, 0] * depth, (v[:, None] - K[1, 2]) / K[1, 1] * depth, depth], axis=-1)
        valid = np.isfinite(depth)
        pad = np.pad(p, ((1, 1), (1, 1), (0, 0)), constant_values=0)
        vpad = np.pad(valid, 1, constant_values=False)
        shifts = [(0, 1), (1, 0), (2, 1), (1, 2)]                    # up, left, down, right as offsets into the padded maps
        edges = [pad[a:a + H, b:b + W] - p for a, b in shifts]
        ok = [vpad[a:a + H, b:b + W] & valid for a, b in shifts]
        lp = _norm(p)
        acc = np.zeros((H, W, 3), F)
        faces = np.zeros((H, W), np.int32)
        cos_thr = F(np.cos(np.float64(F(edge_threshold)) * np.pi / 180.0))
        angles = np.full((H, W, 4), np.nan)
        for k in range(4):
            a, b = edges[k], edges[(k + 1) % 4]
            n = np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                          a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], axis=-1)
            ln = _norm(n)
            c = -((n[..., 0] * p[..., 0] + n[..., 1] * p[..., 1]) + n[..., 2] * p[..., 2]) / (ln * lp)
            corners = ok[k] & ok[(k + 1) % 4]
            counted = corners & (c > cos_thr)
            acc = acc + np.where(counted[..., None], n / ln[..., None], F(0))
            faces += counted
            angles[..., k] = np.where(corners, np.degrees(np.arccos(np.clip(c.astype(np.float64), -1, 1))), np.nan)
        mask = faces > 0
        normal = np.where(mask[..., None], acc / _norm(acc)[..., None], F(np.nan)).astype(F)
    return (normal, mask, angles) if return_angles else (normal, mask)


def depth_edge(depth: np.ndarray, kernel_size: int = 5, ltol: float = 0.01, return_spread: bool = False):
    """-> (eligible = isfinite & ~edge as float32 0 / 1, known = ~isnan as uint8); return_spread adds max(log d) - min(log d) of the window"""
    depth = np.asarray(depth, F)
    H, W = depth.shape
    r = kernel_size // 2
    valid = np.isfinite(depth)
    hi = np.pad(np.where(valid, depth, F(-np.inf)), r, constant_values=-np.inf)
    lo = np.pad(np.where(valid, depth, F(np.inf)), r, constant_values=np.inf)
    mx, mn = np.full((H, W), -np.inf, F), np.full((H, W), np.inf, F)
    for a in range(kernel_size):
        for b in range(kernel_size):
            mx, mn = np.maximum(mx, hi[a:a + H, b:b + W]), np.minimum(mn, lo[a:a + H, b:b + W])
    with np.errstate(all="ignore"):
        spread = np.log(mx) - np.log(mn)
    edge = valid & (spread > F(ltol))
    out = ((valid & ~edge).astype(F), (~np.isnan(depth)).astype(np.uint8))
    return out + (np.where(valid, spread, np.nan),) if return_spread else out


# ------------------------------------------------------------------------------------------------------------------------------------------
# the warp: coordinates and the three interpolation rules
# ------------------------------------------------------------------------------------------------------------------------------------------
def source_coords(minv: np.ndarray, height: int, width: int):
    """(sx, sy) float32 of every target pixel: Minv (x, y, 1) in float32, then the division"""
    m = np.asarray(minv, F).ravel()
    x = np.arange(width, dtype=F)[None, :]
    y = np.arange(height, dtype=F)[:, None]
    with np.errstate(all="ignore"):
        X = (m[0] * x + m[1] * y) + m[2]
        Y = (m[3] * x + m[4] * y) + m[5]
        Z = (m[6] * x + m[7] * y) + m[8]
        return (X / Z).astype(F), (Y / Z).astype(F)


def lanczos4_weights(t: np.ndarray) -> np.ndarray:
    """OpenCV's Lanczos-4 weights of the fractions t (...,) -> (..., 8) float32 for taps -3 .. +4"""
    t = np.asarray(t, F)
    s45 = 0.70710678118654752440084436210485
    cs = np.array([[1, 0], [-s45, -s45], [0, 1], [s45, -s45], [-1, 0], [s45, s45], [0, -1], [-s45, s45]])
    t64 = t.astype(np.float64)
    y0 = -(t64 + 3) * np.pi * 0.25
    s0, c0 = np.sin(y0), np.cos(y0)
    w = np.empty(t.shape + (8,), F)
    total = np.zeros(t.shape, F)
    with np.errstate(all="ignore"):
        for i in range(8):
            y = -(t64 + 3 - i) * np.pi * 0.25
            w[..., i] = ((cs[i, 0] * s0 + cs[i, 1] * c0) / (y * y)).astype(F)
            total = total + w[..., i]
        w = w * (F(1) / total)[..., None]
    unit = np.zeros(8, F)
    unit[3] = 1
    return np.where((t < np.finfo(F).eps)[..., None], unit, w).astype(F)


def sample_lanczos4(src: np.ndarray, sx: np.ndarray, sy: np.ndarray) -> np.ndarray:
    """uint8 (H, W, C) -> uint8 (h, w, C)"""
    H, W, Cn = src.shape
    img = src.astype(F)
    with np.errstate(invalid="ignore"):
        near = (sx > -5) & (sx < W + 4) & (sy > -5) & (sy < H + 4)
    fx0, fy0 = np.floor(np.where(near, sx, 0)), np.floor(np.where(near, sy, 0))
    wx, wy = lanczos4_weights(np.where(near, sx, 0) - fx0), lanczos4_weights(np.where(near, sy, 0) - fy0)
    x0, y0 = fx0.astype(np.int64) - 3, fy0.astype(np.int64) - 3
    acc = np.zeros(sx.shape + (Cn,), F)
    for r in range(8):
        yy = y0 + r
        for c in range(8):
            xx = x0 + c
            inside = near & (yy >= 0) & (yy < H) & (xx >= 0) & (xx < W)
            tap = np.where(inside[..., None], img[np.clip(yy, 0, H - 1), np.clip(xx, 0, W - 1)], F(0))
            acc = acc + tap * (wy[..., r] * wx[..., c])[..., None]
    return np.clip(np.rint(acc), 0, 255).astype(np.uint8)


def sample_bilinear(src: np.ndarray, sx: np.ndarray, sy: np.ndarray) -> np.ndarray:
    """float32 (H, W) or (H, W, C); constant-0 border; NaN and inf of an in-image tap propagate, also at weight 0"""
    H, W = src.shape[:2]
    img = np.asarray(src, F).reshape(H, W, -1)
    with np.errstate(all="ignore"):
        near = (sx > -2) & (sx < W + 1) & (sy > -2) & (sy < H + 1)
        cx, cy = np.where(near, sx, F(0)), np.where(near, sy, F(0))
        flx, fly = np.floor(cx), np.floor(cy)
        fx, fy = (cx - flx)[..., None], (cy - fly)[..., None]
        x0, y0 = flx.astype(np.int64), fly.astype(np.int64)

        def tap(yy, xx):
            inside = near & (xx >= 0) & (xx < W) & (yy >= 0) & (yy < H)
            return np.where(inside[..., None], img[np.clip(yy, 0, H - 1), np.clip(xx, 0, W - 1)], F(0))

        one = F(1)
        out = (tap(y0, x0) * (one - fx) + tap(y0, x0 + 1) * fx) * (one - fy) + (tap(y0 + 1, x0) * (one - fx) + tap(y0 + 1, x0 + 1) * fx) * fy
    return out.astype(F).reshape(sx.shape + src.shape[2:])


def sample_nearest(src: np.ndarray, sx: np.ndarray, sy: np.ndarray) -> np.ndarray:
    H, W = src.shape[:2]
    with np.errstate(invalid="ignore"):
        rx, ry = np.rint(sx), np.rint(sy)
        inside = (rx >= 0) & (rx <= W - 1) & (ry >= 0) & (ry <= H - 1)
    ix, iy = np.where(inside, rx, 0).astype(np.int64), np.where(inside, ry, 0).astype(np.int64)
    return np.where(inside, src[iy, ix], np.zeros((), src.dtype))


def warp_perspective(src: np.ndarray, M: np.ndarray, dsize, flags: int = INTER_LINEAR, **_) -> np.ndarray:
    """cv2.warpPerspective(src, M, (width, height), flags=interpolation) with the conventions of DESIGN.md section 16 (no INTER_BITS fixed
    point): the float64 inverse of M rounded to float32, float32 coordinates, constant-0 border."""
    width, height = dsize
    minv = np.linalg.inv(np.asarray(M, np.float64)).astype(F)
    sx, sy = source_coords(minv, height, width)
    if flags == INTER_LANCZOS4:
        assert src.dtype == np.uint8 and src.ndim == 3
        return sample_lanczos4(src, sx, sy)
    if flags == INTER_LINEAR:
        return sample_bilinear(src, sx, sy)
    assert flags == INTER_NEAREST
    return sample_nearest(src, sx, sy)


# ------------------------------------------------------------------------------------------------------------------------------------------
# finish and the whole instance
# ------------------------------------------------------------------------------------------------------------------------------------------
def finish(depth: np.ndarray, count: int, depth_unit, clamp_max_depth: float, only_known: bool, q: float = 0.01):
    """-> (depth, mask_fin, mask_inf, invalid, max_depth)"""
    depth = np.array(depth, F)
    invalid = bool(np.float64(count) / np.float64(depth.size) < 0.001)
    if invalid:
        depth = np.ones_like(depth)
    if depth_unit is not None:
        depth = depth * F(depth_unit)
    finite = np.isfinite(depth)
    with np.errstate(all="ignore"), warnings.catch_warnings():
        warnings.simplefilter("ignore")                      # "All-NaN slice" when nothing is finite
        max_depth = F(np.nanquantile(np.where(finite, depth, F(np.nan)), F(q)) * F(clamp_max_depth))
        depth = np.where(finite, np.minimum(np.maximum(depth, F(0)), max_depth), depth).astype(F)
    inf = np.isinf(depth)
    return depth, (np.isfinite(depth) if only_known else ~inf), inf, invalid, max_depth


def warp_maps(image, nearest, raw_depth, eligible, normal, mats, out_h, out_w, flip):
    """The fused warp of moge_train_warp -> (image_u8, depth, normal, bilinear branch, count)"""
    mats = np.asarray(mats, F)
    sx, sy = source_coords(mats[0:9], out_h, out_w)
    img = sample_lanczos4(image, sx, sy)
    sx, sy = source_coords(mats[18:27], out_h, out_w)
    el = sample_bilinear(eligible, sx, sy)
    with np.errstate(all="ignore"):
        bil = F(1) / sample_bilinear(F(1) / np.asarray(raw_depth, F), sx, sy)
        nrm = sample_bilinear(normal, sx, sy)
        sx, sy = source_coords(mats[9:18], out_h, out_w)
        near = sample_nearest(np.asarray(nearest, F), sx, sy)
        branch = el == F(1)
        warped = np.where(branch, bil, near)
        u = ((np.arange(out_w, dtype=F) + F(0.5)) / F(out_w))[None, :]
        v = ((np.arange(out_h, dtype=F) + F(0.5)) / F(out_h))[:, None]
        zr = mats[36:39]
        depth = (warped / ((u * zr[0] + v * zr[1]) + zr[2])).astype(F)
        R = mats[27:36].reshape(3, 3)
        rot = np.stack([(nrm[..., 0] * R[k, 0] + nrm[..., 1] * R[k, 1]) + nrm[..., 2] * R[k, 2] for k in range(3)], axis=-1).astype(F)
    if flip:
        img, depth, branch = img[:, ::-1], depth[:, ::-1], branch[:, ::-1]
        rot = rot[:, ::-1] * np.array([-1, 1, 1], F)
    return np.ascontiguousarray(img), np.ascontiguousarray(depth), np.ascontiguousarray(rot), np.ascontiguousarray(branch), int(np.isfinite(depth).sum())


def warp_train_sample(image, depth, intrinsics, width, height, seed, *, center_augmentation, fov_range_absolute, fov_range_relative, clamp_max_depth,
                      depth_unit=None, finite_depth_mask=None):
    """moge_amd.train_data.warp_train_sample on the host: the numpy pieces above, real Pillow for the Lanczos pre-resize and the masked nearest
    resize of moge_amd.evaluation."""
    H, W = depth.shape
    geo = T.warp_geometry(H, W, intrinsics, width, height, seed, center_augmentation=center_augmentation, fov_range_absolute=fov_range_absolute,
                          fov_range_relative=fov_range_relative)
    normal, _ = normal_map(depth, intrinsics, T.EDGE_THRESHOLD)
    eligible, known = depth_edge(depth, T.EDGE_KERNEL, T.EDGE_LTOL)
    (ih, iw), (nh, nw) = geo["image_size"], geo["nearest_size"]
    src_image = np.array(Image.fromarray(image).resize((iw, ih), Image.Resampling.LANCZOS)) if (ih, iw) != (H, W) else image
    nearest = E.masked_nearest_resize(depth, known.astype(bool), (nh, nw))[0] if (nh, nw) != (H, W) else depth
    img, d, nrm, branch, count = warp_maps(src_image, nearest, depth, eligible, normal, geo["mats"], height, width, geo["flip"])
    d, fin, inf, invalid, max_depth = finish(d, count, depth_unit, clamp_max_depth, finite_depth_mask == "only_known")
    return {"geometry": geo, "image_u8": img, "image": (img.astype(F) / F(255)).transpose(2, 0, 1), "depth": d, "depth_mask_fin": fin, "depth_mask_inf": inf,
            "normal": nrm, "bilinear": branch, "count": count, "invalid": invalid, "max_depth": max_depth, "raw_normal": normal, "eligible": eligible,
            "nearest_depth": nearest, "resized_image": src_image}
