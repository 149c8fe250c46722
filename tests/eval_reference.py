"""Plain numpy references of the evaluation kernels (csrc/metrics.hip, csrc/evaldata.hip), written from the documented formulas.

Each function restates one operation in float32 numpy in the kernel's stated operation order (sums and counts in float64 / int64), so a
kernel can be compared with it bit for bit where the contract says exact.  tests/test_metrics_cpu.py and tests/test_evaluation_cpu.py pin
these restatements to the reference project's stored results (tests/golden/); the GPU sweeps (tests/test_hip_*_kernels.py) then compare
the kernels with them at the sizes and values the fixtures never reach.  Nothing here needs a GPU."""
from __future__ import annotations

import math
import warnings

import numpy as np
import torch

F = np.float32
EPS = F(1e-6)                                    # rel_depth / rel_point eps (metrics.py:25-48)
# boundary thresholds: what `rel > 1 + t` compares an fp32 tensor against for t in torch.linspace(0.05, 0.25, 10) (fp32 t, Python 1 + t)
BOUNDARY_T = torch.linspace(0.05, 0.25, 10).tolist()
BOUNDARY_THR = [F(1 + t) for t in BOUNDARY_T]


# ---------------------------------------------------------------------------------------------------------------------------------------
# fp32 helpers
# ---------------------------------------------------------------------------------------------------------------------------------------
def fma32(a, b, c):
    """Correctly rounded fp32 fma(a, b, c), elementwise.  a * b is exact in float64 (24 + 24 bits); the float64 sum is made round-to-odd
    (truncate toward zero, set the last bit when inexact), which then rounds to fp32 exactly like one fused operation."""
    a, b, c = (np.asarray(v, F) for v in (a, b, c))
    p = a.astype(np.float64) * b.astype(np.float64)
    c64 = c.astype(np.float64)
    with np.errstate(all="ignore"):
        s = p + c64
        bb = s - p
        e = (p - (s - bb)) + (c64 - bb)                      # exact error of the float64 sum (TwoSum)
        inexact = np.isfinite(s) & (e != 0)
        away = inexact & ((s > 0) != (e > 0))                # s was rounded away from zero: step back toward zero
        t = np.where(away, np.nextafter(s, 0.0), s)
        bits = t.view(np.uint64) | inexact.astype(np.uint64)
        return bits.view(np.float64).astype(F)


def norm3_fma(x, y, z):
    """torch.norm(dim=-1) of a 3-vector on the CPU: sqrt(fma(z, z, fma(y, y, x * x)))"""
    x, y, z = (np.asarray(v, F) for v in (x, y, z))
    return np.sqrt(fma32(z, z, fma32(y, y, x * x)))


def norm3_plain(x, y, z):
    """numpy's norm of a 3-vector without contraction: sqrt((x x + y y) + z z)"""
    return np.sqrt((x * x + y * y) + z * z)


def f2ord(v):
    """the order-preserving int32 of fp32 bits (the bbox / masked-max keys of csrc/metrics.hip)"""
    i = np.asarray(v, F).view(np.int32)
    return np.where(i >= 0, i, i ^ np.int32(0x7FFFFFFF)).astype(np.int32)


def ord2f(i):
    i = np.asarray(i, np.int32)
    return np.where(i >= 0, i, i ^ np.int32(0x7FFFFFFF)).astype(np.int32).view(F)


def same_bits(a, b) -> bool:
    """fp32 arrays equal bit for bit, any NaN matching any NaN"""
    a, b = np.asarray(a, F), np.asarray(b, F)
    if a.shape != b.shape:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(na, nb) and np.array_equal(a[~na].view(np.uint32), b[~nb].view(np.uint32)))


# ---------------------------------------------------------------------------------------------------------------------------------------
# metrics: error pass (metrics.py:25-48, modes of moge_metrics_error)
# ---------------------------------------------------------------------------------------------------------------------------------------
def _xform(mode, p, s, t, c):
    if mode == 0:
        return p * s
    if mode == 1:
        return p * s + t
    if mode == 2:
        return p + t
    v = p * s + t
    return F(1) / np.where(v < c, c, v)                 # clamp_min: NaN stays NaN


def error_pass_ref(pred, gt, mask, params, dim):
    """(K, 3) float64: per params row (mode, s, t0, t1, t2, c) the sum of rel, the delta1 count and the mask count over mask."""
    mask = np.asarray(mask, bool).reshape(-1)
    params = np.asarray(params, F).reshape(-1, 6)
    out = np.zeros((params.shape[0], 3))
    with np.errstate(all="ignore"):
        if dim == 1:
            p, g = np.asarray(pred, F).reshape(-1)[mask], np.asarray(gt, F).reshape(-1)[mask]
            for k, (mode, s, t0, _, _, c) in enumerate(params):
                q = _xform(int(mode), p, s, t0, c)
                rel = np.abs(q - g) / (g + EPS)
                d1 = np.maximum(g / q, q / g) < F(1.25)          # torch.maximum: NaN propagates and compares false
                out[k] = rel.astype(np.float64).sum(), d1.sum(), mask.sum()
        else:
            p, g = np.asarray(pred, F).reshape(-1, 3)[mask], np.asarray(gt, F).reshape(-1, 3)[mask]
            dist_gt = norm3_fma(g[:, 0], g[:, 1], g[:, 2])
            for k, (mode, s, t0, t1, t2, _) in enumerate(params):
                q = [_xform(int(mode), p[:, a], s, t, F(0)) for a, t in enumerate((t0, t1, t2))]
                err = norm3_fma(q[0] - g[:, 0], q[1] - g[:, 1], q[2] - g[:, 2])
                rel = err / (dist_gt + EPS)
                dq = norm3_fma(*q)
                d1 = err < F(0.25) * np.minimum(dist_gt, dq)     # torch.minimum: NaN propagates and compares false
                out[k] = rel.astype(np.float64).sum(), d1.sum(), mask.sum()
    return out


def masked_max_ref(x, mask):
    """max(x[mask]) with the kernel's contract: -inf for an empty mask, NaN as soon as one masked value is NaN
    (either sign; like torch.max), and +0.0 above -0.0."""
    v = np.asarray(x, F).reshape(-1)[np.asarray(mask, bool).reshape(-1)]
    if v.size == 0:
        return F(-np.inf)
    if np.isnan(v).any():
        return F(np.nan)
    return ord2f(f2ord(v).max())


# ---------------------------------------------------------------------------------------------------------------------------------------
# metrics: boundary F1 (metrics.py:63-92) with shifted slices
# ---------------------------------------------------------------------------------------------------------------------------------------
def boundary_counts_ref(pred, gt, mask, r):
    """(10, 3) int64 (TP, gt-label, pred-label) for radius r: centres in the interior [r:-r, r:-r], neighbours with dx^2 + dy^2 <= r^2 + 1e-5,
    valid = mask[centre] & mask[neighbour], labels v[n] / v[c] > fp32(1 + t) in fp32."""
    pred, gt, mask = np.asarray(pred, F), np.asarray(gt, F), np.asarray(mask, bool)
    H, W = mask.shape
    out = np.zeros((10, 3), np.int64)
    if H <= 2 * r or W <= 2 * r:
        return out
    ci = (slice(r, H - r), slice(r, W - r))
    pc, gc, mc = pred[ci], gt[ci], mask[ci]
    with np.errstate(all="ignore"):
        for dy in range(-r, r + 1):
            for dx in range(-r, r + 1):
                if dx * dx + dy * dy > r * r + 1e-5:
                    continue
                ni = (slice(r + dy, H - r + dy), slice(r + dx, W - r + dx))
                pr, gr = pred[ni] / pc, gt[ni] / gc
                valid = mc & mask[ni]
                for t, thr in enumerate(BOUNDARY_THR):
                    pl, gl = (pr > thr) & valid, (gr > thr) & valid
                    out[t] += (pl & gl).sum(), gl.sum(), pl.sum()
    return out


def boundary_f1_ref(counts):
    """metrics.py:79-92 from the (10, 3) counts: fp32 precision / recall / F1, weighted average in Python floats."""
    f1s = []
    for tp, gl, pl in np.asarray(counts):
        tp, gl, pl = F(tp), F(gl), F(pl)
        precision = tp / max(gl, F(1e-12))
        recall = tp / max(pl, F(1e-12))
        f1s.append(float(F(2) * precision * recall / max(precision + recall, F(1e-12))))
    return sum(w * f for w, f in zip(BOUNDARY_T, f1s)) / sum(BOUNDARY_T)


# ---------------------------------------------------------------------------------------------------------------------------------------
# metrics: local points (metrics.py:283-311)
# ---------------------------------------------------------------------------------------------------------------------------------------
def segments_ref(seg, mask, gt, labels, lr_mask, lr_index):
    """Per label u of `labels` (sorted): bbox (6,) int32 ordered keys of gt over (seg == u) & mask (min xyz, max xyz; empty: INT_MAX /
    INT_MIN), diameter (fp32 max over xyz of max - min; NaN when empty), the low-resolution count and the row-major flat source indices of
    the low-resolution samples of u (the packing order of src / tgt).  Pixels whose id is not in `labels` count nowhere."""
    seg2d = np.asarray(seg)
    W = seg2d.shape[1]
    seg_f, mask_f = seg2d.reshape(-1), np.asarray(mask, bool).reshape(-1)
    keys = f2ord(np.asarray(gt, F).reshape(-1, 3))
    rows, cols = (np.asarray(v).reshape(-1).astype(np.int64) for v in lr_index)
    lm = np.asarray(lr_mask, bool).reshape(-1)
    lr_ids = seg2d[rows, cols]
    out = []
    for u in labels:
        sel = (seg_f == u) & mask_f
        if sel.any():
            k = keys[sel]
            bbox = np.concatenate([k.min(0), k.max(0)]).astype(np.int32)
            ext = ord2f(bbox[3:]) - ord2f(bbox[:3])
            diam = F(np.nan) if np.isnan(ext).any() else F(ext.max())
        else:
            bbox = np.array([0x7FFFFFFF] * 3 + [-0x80000000] * 3, np.int32)
            diam = F(np.nan)
        lsel = lm & (lr_ids == u)
        out.append({"bbox": bbox, "diameter": diam, "lr_count": int(lsel.sum()), "lr_flat": rows[lsel] * W + cols[lsel]})
    return out


def segment_error_ref(seg, mask, pred, gt, label, scale, shift, diameter):
    """(sum err / diameter, delta1 count, pixel count) of one segment after pred * scale + shift (fp32, no contraction; fma norm)."""
    sel = (np.asarray(seg).reshape(-1) == label) & np.asarray(mask, bool).reshape(-1)
    p, g = np.asarray(pred, F).reshape(-1, 3)[sel], np.asarray(gt, F).reshape(-1, 3)[sel]
    q = p * F(scale) + np.asarray(shift, F)
    err = norm3_fma(q[:, 0] - g[:, 0], q[:, 1] - g[:, 1], q[:, 2] - g[:, 2])
    d = F(diameter)
    return float((err / d).astype(np.float64).sum()), int((err < F(0.25) * d).sum()), int(sel.sum())


# ---------------------------------------------------------------------------------------------------------------------------------------
# evaluation data: Lanczos (Pillow Resample.c fixed point), nearest resize, distance, remap, quantile cut, unproject
# ---------------------------------------------------------------------------------------------------------------------------------------
def _lz_coeffs(in_size, out_size):
    scale = float(np.float32(in_size)) / out_size
    fs = max(scale, 1.0)
    support = 3.0 * fs
    ksize = int(math.ceil(support)) * 2 + 1

    def filt(x):
        def sinc(v):
            if v == 0.0:
                return 1.0
            v = v * math.pi
            return math.sin(v) / v
        return sinc(x) * sinc(x / 3) if -3.0 <= x < 3.0 else 0.0

    bounds, kk = [], np.zeros((out_size, ksize), np.int64)
    for xx in range(out_size):
        center = 0.0 + (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        xmax = min(int(center + support + 0.5), in_size) - xmin
        w = [filt((x + xmin - center + 0.5) / fs) for x in range(xmax)]
        ww = sum(w)
        for x in range(xmax):
            v = w[x] / ww if ww != 0.0 else w[x]
            kk[xx, x] = int(-0.5 + v * (1 << 22)) if v < 0 else int(0.5 + v * (1 << 22))
        bounds.append((xmin, xmax))
    return bounds, kk


def _lz_pass(src, bounds, kk):
    """src (N, in, C) uint8 -> (N, out, C) along axis 1"""
    out = np.zeros((src.shape[0], len(bounds), src.shape[2]), np.uint8)
    for xx, (xmin, xmax) in enumerate(bounds):
        acc = (1 << 21) + np.einsum("nkc,k->nc", src[:, xmin:xmin + xmax].astype(np.int64), kk[xx, :xmax])
        out[:, xx] = np.clip(acc >> 22, 0, 255)
    return out


def lanczos_np(img, h, w):
    """Pillow's two-pass fixed-point Lanczos as csrc/evaldata.hip states it (horizontal first, over the rows the vertical pass reads)"""
    H, W = img.shape[:2]
    if (H, W) == (h, w):
        return img.copy()
    bh, kh = _lz_coeffs(W, w)
    bv, kv = _lz_coeffs(H, h)
    first, last = bv[0][0], bv[-1][0] + bv[-1][1]
    if W != w:
        img = _lz_pass(img[first:last] if H != h else img, bh, kh)
        bv = [(a - first, b) for a, b in bv] if H != h else bv
    if H != h:
        img = _lz_pass(img.transpose(1, 0, 2), bv, kv).transpose(1, 0, 2)
    return img


def resize_nearest_ref(src, h, w):
    """cv2.resize(INTER_NEAREST): source index min(floor(d * (1 / (out / in))), in - 1) in float64, per axis"""
    H, W = src.shape
    sx = np.minimum(np.floor(np.arange(w) * (1.0 / (w / W))).astype(np.int64), W - 1)
    sy = np.minimum(np.floor(np.arange(h) * (1.0 / (h / H))).astype(np.int64), H - 1)
    return src[sy[:, None], sx[None, :]]


def uv_grid(h, w):
    u = (np.arange(w, dtype=F) + F(0.5)) / F(w)
    v = (np.arange(h, dtype=F) + F(0.5)) / F(h)
    return np.broadcast_to(u[None, :], (h, w)), np.broadcast_to(v[:, None], (h, w))


def distance_ref(depth, K):
    """|(x, y, depth)| of depth_map_to_point_map at pixel centres, fp32, numpy's norm order"""
    depth = np.asarray(depth, F)
    h, w = depth.shape
    u, v = uv_grid(h, w)
    fx, fy, cx, cy = F(K[0, 0]), F(K[1, 1]), F(K[0, 2]), F(K[1, 2])
    x = (u - cx) / fx * depth
    y = (v - cy) / fy * depth
    return norm3_plain(x, y, depth)


def _affine_uv(M, u, v):
    M = np.asarray(M, F).reshape(3, 3)
    return [u * M[r, 0] + v * M[r, 1] + M[r, 2] for r in range(3)]


def remap_ref(image, distance, mask, seg, T, Kinv, OH, OW):
    """remap_kernel restated in fp32 numpy: the homography T of target uv, bilinear image with constant-0 border (rint, clip), nearest
    distance / mask / labels at rint (half to even), ray length |[u, v, 1] Kinv^T| and depth = distance / (ray + 1e-12).
    -> dict image (OH, OW, 3) uint8, mask bool, seg int32 or None, depth fp32"""
    image = np.asarray(image, np.uint8)
    h, w = image.shape[:2]
    u, v = uv_grid(OH, OW)
    p0, p1, p2 = _affine_uv(T, u, v)
    with np.errstate(all="ignore"):
        den = p2 + F(1e-12)
        px = p0 / den * F(w) - F(0.5)
        py = p1 / den * F(h) - F(0.5)
        near = (px > F(-2)) & (px < F(w) + F(1)) & (py > F(-2)) & (py < F(h) + F(1))
        flx, fly = np.floor(np.where(near, px, 0)), np.floor(np.where(near, py, 0))
        x0, y0 = flx.astype(np.int64), fly.astype(np.int64)
        fx, fy = np.where(near, px, 0) - flx, np.where(near, py, 0) - fly
        taps = []
        for q in range(4):
            xx, yy = x0 + (q & 1), y0 + (q >> 1)
            inside = near & (xx >= 0) & (xx < w) & (yy >= 0) & (yy < h)
            taps.append(np.where(inside[..., None], image[np.clip(yy, 0, h - 1), np.clip(xx, 0, w - 1)].astype(F), F(0)))
        fx3, fy3 = fx[..., None], fy[..., None]
        acc = (taps[0] * (F(1) - fx3) + taps[1] * fx3) * (F(1) - fy3) + (taps[2] * (F(1) - fx3) + taps[3] * fx3) * fy3
        acc = np.where(near[..., None], acc, F(0))
        out_u8 = np.clip(np.rint(acc), 0, 255).astype(np.uint8)
        rx, ry = np.rint(px), np.rint(py)
        inside = (rx >= 0) & (rx <= F(w - 1)) & (ry >= 0) & (ry <= F(h - 1))
        iy, ix = np.where(inside, ry, 0).astype(np.int64), np.where(inside, rx, 0).astype(np.int64)
        dist = np.where(inside, np.asarray(distance, F)[iy, ix], F(0))
        out_mask = inside & (np.asarray(mask)[iy, ix] > 0)
        out_seg = None if seg is None else np.where(inside, np.asarray(seg).astype(np.int32)[iy, ix], 0).astype(np.int32)
        a, b, c = _affine_uv(Kinv, u, v)
        ray = norm3_plain(a, b, c)
        depth = dist / (ray + F(1e-12))
    return {"image": out_u8, "mask": out_mask, "seg": out_seg, "depth": depth.astype(F)}


def nanquantile32(values, q):
    """np.nanquantile of float32 values (linear method, in float32) as a float32; NaN when nothing is left"""
    with warnings.catch_warnings(), np.errstate(all="ignore"):
        warnings.simplefilter("ignore")
        return F(np.nanquantile(np.asarray(values, F), q)) if np.asarray(values).size else F(np.nan)


def quantile_cut_ref(depth, mask, q, drop, unit=None):
    """dataloader.py:167-172 at quantile q -> (max_depth fp32, mask bool, depth fp32, count)"""
    depth, mask = np.asarray(depth, F).reshape(-1), np.asarray(mask, bool).reshape(-1)
    md = nanquantile32(np.where(mask, depth, F(np.nan)), q) * F(drop)
    with np.errstate(invalid="ignore"):
        m = mask & (depth <= md)
    d = np.nan_to_num(depth)
    if unit is not None:
        d = d * F(unit)
    return md, m, d, int(m.sum())


def unproject_ref(depth, mask, Kinv, count):
    """dataloader.py:173-180: an empty mask turns into all ones (mask and depth); points = [u, v, 1] Kinv^T * depth"""
    depth, mask = np.asarray(depth, F), np.asarray(mask, bool)
    if count == 0:
        depth, mask = np.ones_like(depth), np.ones_like(mask)
    h, w = depth.shape
    u, v = uv_grid(h, w)
    pts = np.stack([c * depth for c in _affine_uv(Kinv, u, v)], -1)
    return depth, mask, pts
