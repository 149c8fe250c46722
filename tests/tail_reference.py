"""float64 numpy references, with per-element error bounds, for the kernels of the inference tail (csrc/post.hip: head_final*, mlp_layer, recover +
finalize through moge_postprocess; csrc/elementwise.hip: layernorm, ln_raw, ln_finalize, fold_ln, resize_bilinear_uv, u8hwc_to_chw).

Every reference is written from the definition of the operation (the reference model's modules), not from the kernel, and is checked on the CPU against
an independent torch float64 formulation in tests/test_tail_reference_cpu.py.  tests/test_hip_tail_kernels.py compares element by element:
|got - ref| <= bound(element).

How the bounds are derived
--------------------------
u = 2^-24 is the unit roundoff of fp32, ulp32(v) the spacing of fp32 at |v|.  Inputs are rounded to the storage type (fp16 or fp32) BEFORE the
reference runs; both storage types accumulate in fp32, so they get the same bound.

Sums.  A sum of n fp32 terms in which every term passes through at most d additions is off by at most d u sum|terms| (Higham, Accuracy and Stability of
Numerical Algorithms, section 4.2: any summation order).  For the channel dot products of the head (C <= 64 per input) d is the fully sequential
worst case.  For the long rows (LayerNorm D <= 1024, mlp K <= 1024, fold_ln K <= 1024) the bound admits any blocked / tree summation of depth
SUM_DEPTH(n) = 2 ceil(log2 n) + 2: a wave-per-row or block-per-row reduction is at most that deep; a fully sequential sum of 1024 floats is not
what it admits.  SUM_DEPTH and the "+ 8" of the head are allowances for a class of summation orders, not counts of one kernel's additions (at K = 4
the depth is 6 where 3 additions exist); what they leave unused on an MI355X is recorded in EXPERIMENTS.md R7.2 (fp32 paths: 0.12 - 0.40 of the bound).

Bilinear taps.  Source coordinate and lerp weights in float32 exactly as ATen computes them (UpSample.h area_pixel_compute_source_index +
guard_index_and_lambda): scale = f32(in) / f32(out), src = max(scale * (dst + 0.5) - 0.5, 0), i0 = min(int(src), in - 1), i1 = i0 + (i0 < in - 1),
l1 = src - i0, l0 = 1 - l1.  Everything after that is float64.

Head (head_final / head_final_k3 / head_final_dot).  pre = bias + sum_taps wt (sum_c w_c x_c [+ sum_c w2_c n4_c]) with the conv evaluated at the low
resolution (3x3: replicate padding).  Magnitude A = |bias| + sum_taps wt sum_c |w_c x_c| (both inputs' terms when n4 is given: A roughly doubles).
  e_pre = (n_terms + 8) u A + (ulp32(sy + 0.5) + ulp32(sx + 0.5)) spread
n_terms = channel products per tap (C, 2 C with n4, 9 C for the 3x3 conv, 1 or 2 for head_final_dot); + 8 = two roundings of a lerp weight (1 - l,
the product), the tap multiply, three tap additions, the weight multiply, the bias addition.  The second term is the source coordinate: the compiler may
contract scale * (dst + 0.5) - 0.5 into one FMA and ATen does not, which moves src by up to one ulp of the product (magnitude src + 0.5) per axis; the
output moves by that times the slope between taps, bounded by `spread` = max - min of the conv output over the taps and their lower neighbours (a
coordinate that sits on a cell border may fall into the cell below).
Through the activation, first order in e_pre (|pre| <= 4 in the tests: second order is below 1e-12), K_ULP = 4 ulp for expf / sinhf:
  linear / raw : e_pre
  sinh         : cosh(z) e + K_ULP ulp32(sinh z)
  exp          : z' = e^z: e^z e_z + K_ULP ulp32(e^z);  x' = x e^z: e^z e_x + |x| (e^z e_z + K_ULP ulp32(e^z)) + ulp32(x e^z)
  normal       : n = o / max(|o|, 1e-12): (e_j + |n_j| sum_k |n_k| e_k) / |o| + 10 u |n_j|   (5 ops of the squared norm, sqrt, divide)
  sigmoid      : s = 1 / (1 + e^-o): s (1 - s) (e + K_ULP 2^-23) + 2 ulp32(s)

mlp_layer.  A = |bias| + sum_k |in_k W_k|; e = (SUM_DEPTH(K) + 2) u A; relu keeps it, exp: e^s e + K_ULP ulp32(e^s).

LayerNorm (eps 1e-6, biased variance, two-pass).  With a = x - mean, q = sum a^2, d = SUM_DEPTH(D):
  e_mean = (d + 1) u mean|x|                       e_a = e_mean + u |a|
  e_q    = sum(2 |a| e_a + e_a^2) + (d + 2) u q    e_var = e_q / D + 2 u (var + eps)
  e_rstd = rstd (0.5 e_var / (var + eps) + 4 u)    (rsqrtf: 1 ulp on gfx9; 4 u covers it and the addition of eps)
  e_y    = |w| (rstd e_a + |a| e_rstd + u |a| rstd) + 2 u (|a rstd w| + |b|)      [+ 2^-11 |y| + 2^-25 when the output is stored as fp16]
A one-pass variance (E[x^2] - mean^2) on rows with mean 50, sigma 0.1 is off by u 2500 / 0.01 = 1.5 % of the variance per operation - two orders
above e_var - which is what the large-mean rows of the tests are for.

ln_finalize.  The reference is the kernel's stated formula on the given partials: mean = s1 / D, var = max(s2 / D - mean^2, 0), rstd = 1 / sqrt(var + eps).
  e_mean = NP u sum|p1| / D + 2 u |mean|
  e_var  = (NP + 3) u s2 / D + 2 |mean| e_mean + 2 u mean^2        (first term: summation, 1 / D, the product and the cancellation term u s2 / D)
and rstd is carried through rsqrt EXACTLY, not linearised (the clamp at 0 makes the derivative unbounded relative to eps): the bound is the distance
from rstd to the ends of [1 / sqrt(var + e_var + eps), 1 / sqrt(max(var - e_var, 0) + eps)], + 4 u rstd.

fold_ln.  Wf = fp16(fp32(g w)): bit-exact.  c = sum of the ROUNDED Wf: SUM_DEPTH(K) u sum|Wf|.  bf = b + sum beta w: (SUM_DEPTH(K) + 3) u (|b| + sum|beta w|).

resize_bilinear_uv.  A = sum_taps wt |x|; e = 8 u A + the coordinate term above [+ 2^-11 |ref| + 2^-25 for fp16 storage].  uv channels: torch.linspace in
fp32 (start + step i below the middle, end - step (n - 1 - i) above): 3 ulp32 of the range end covers a contracted multiply-add.

u8 ingest, the fp16 copies, padding, masks and INF fills are bit-exact.

Post-processing (recover + finalize).  `postprocess` restates v2.py:246-289 / v1.py:358 from the oracle's pieces; `finalize_f32` is the float32
arithmetic of the same lines from a GIVEN shift and intrinsics (adds, multiplies, divides: nothing to contract), compared within 2 ulp.
"""
import math

import numpy as np

U32 = 2.0 ** -24
K_ULP = 4.0
REMAPS = ("linear", "sinh", "exp", "sinh_exp")


def ulp32(v):
    return np.spacing(np.abs(np.asarray(v, dtype=np.float64)).astype(np.float32)).astype(np.float64)


def sum_depth(n):
    return 2 * math.ceil(math.log2(max(n, 2))) + 2


def to_storage(x, prec):
    """fp32 values as the kernel sees them after the conversion to its storage type (prec 1 = fp16), as float64."""
    x = np.asarray(x, dtype=np.float32)
    return (x.astype(np.float16) if prec == 1 else x).astype(np.float64)


def bilinear_taps(n_in, n_out):
    """ATen's float32 source index: (i0, i1, l0, l1, src) for every destination index."""
    scale = np.float32(n_in) / np.float32(n_out)
    dst = np.arange(n_out, dtype=np.float32)
    src = np.maximum(scale * (dst + np.float32(0.5)) - np.float32(0.5), np.float32(0))
    i0 = np.minimum(src.astype(np.int64), n_in - 1)
    i1 = i0 + (i0 < n_in - 1)
    l1 = np.clip(src - i0.astype(np.float32), np.float32(0), np.float32(1))
    l0 = np.float32(1) - l1
    assert src.dtype == l1.dtype == l0.dtype == np.float32
    return i0, i1, l0.astype(np.float64), l1.astype(np.float64), src.astype(np.float64)


def resize(t, a, H, W):
    """Bilinear resize of t (B,Hd,Wd,K) float64 to (B,H,W,K); `a` (same shape) is the magnitude map resized with the same weights.
    Returns (value, magnitude, coordinate term)."""
    B, Hd, Wd, _ = t.shape
    y0, y1, ly0, ly1, sy = bilinear_taps(Hd, H)
    x0, x1, lx0, lx1, sx = bilinear_taps(Wd, W)

    def blend(m):
        top = m[:, y0][:, :, x0] * lx0[None, None, :, None] + m[:, y0][:, :, x1] * lx1[None, None, :, None]
        bot = m[:, y1][:, :, x0] * lx0[None, None, :, None] + m[:, y1][:, :, x1] * lx1[None, None, :, None]
        return top * ly0[None, :, None, None] + bot * ly1[None, :, None, None]

    ys = [np.maximum(y0 - 1, 0), y0, y1]
    xs = [np.maximum(x0 - 1, 0), x0, x1]
    nb = np.stack([t[:, yy][:, :, xx] for yy in ys for xx in xs])
    spread = nb.max(0) - nb.min(0)
    coord = (ulp32(sy + 0.5)[None, :, None, None] + ulp32(sx + 0.5)[None, None, :, None]) * spread
    return blend(t), blend(a), coord


def conv_lowres(x, w):
    """1x1 (w (CO,C)) or 3x3 replicate-padded (w (CO,C,3,3)) conv of x (B,Hd,Wd,C), float64: (value, magnitude sum |w x|)."""
    if w.ndim == 2:
        return x @ w.T, np.abs(x) @ np.abs(w).T
    B, Hd, Wd, C = x.shape
    xp = np.pad(x, ((0, 0), (1, 1), (1, 1), (0, 0)), mode="edge")
    t = np.zeros((B, Hd, Wd, w.shape[0]))
    a = np.zeros_like(t)
    for dy in range(3):
        for dx in range(3):
            win = xp[:, dy:dy + Hd, dx:dx + Wd]
            t += win @ w[:, :, dy, dx].T
            a += np.abs(win) @ np.abs(w[:, :, dy, dx]).T
    return t, a


def activate(pre, e, kind, remap):
    """kind 0 points (+ remap), 1 unit normal, 2 sigmoid, 3 raw; pre / e (..., CO) float64 -> (ref, bound)."""
    if kind == 3:
        return pre, e
    if kind == 2:
        s = 1.0 / (1.0 + np.exp(-pre))
        return s, s * (1 - s) * (e + K_ULP * 2.0 ** -23) + 2 * ulp32(s)
    if kind == 1:
        nrm = np.maximum(np.sqrt((pre * pre).sum(-1, keepdims=True)), 1e-12)
        assert nrm.min() > 1e-3, "the test inputs must keep the normal away from 0"
        n = pre / nrm
        return n, (e + np.abs(n) * (np.abs(n) * e).sum(-1, keepdims=True)) / nrm + 10 * U32 * np.abs(n)
    mode = REMAPS[remap]
    ref, b = pre.copy(), e.copy()
    if mode == "linear":
        return ref, b

    def sinh(z, ez):
        return np.sinh(z), np.cosh(z) * ez + K_ULP * ulp32(np.sinh(z))

    def exp(z, ez):
        return np.exp(z), np.exp(z) * ez + K_ULP * ulp32(np.exp(z))

    if mode == "sinh":
        return sinh(pre, e)
    ref[..., 2], b[..., 2] = exp(pre[..., 2], e[..., 2])
    if mode == "sinh_exp":
        ref[..., :2], b[..., :2] = sinh(pre[..., :2], e[..., :2])
    else:
        z, bz = ref[..., 2:3], b[..., 2:3]
        ref[..., :2] = pre[..., :2] * z
        b[..., :2] = z * e[..., :2] + np.abs(pre[..., :2]) * bz + ulp32(ref[..., :2])
    return ref, b


def head_final(x, w, bias, H, W, kind, remap=0, n4=None, w2=None):
    """out = activation(resize(conv(x) [+ conv(n4; w2)] + bias)): x (B,Hd,Wd,C) float64 already rounded to storage, w (CO,C) or (CO,C,3,3).
    Returns (ref, bound, pre-activation)."""
    x, w, bias = (np.asarray(v, dtype=np.float64) for v in (x, w, bias))
    t, a = conv_lowres(x, w)
    n_terms = x.shape[-1] * (9 if w.ndim == 4 else 1)
    if n4 is not None:
        t2, a2 = conv_lowres(np.asarray(n4, dtype=np.float64), np.asarray(w2, dtype=np.float64))
        t, a, n_terms = t + t2, a + a2, 2 * n_terms
    v, A, coord = resize(t, a, H, W)
    pre = v + bias
    e = (n_terms + 8) * U32 * (A + np.abs(bias)) + coord
    ref, bound = activate(pre, e, kind, remap)
    return ref, bound, pre


def head_final_dot(y, z, zoff, bias, H, W, kind, remap=0):
    """head_final on the maps of the fused output conv: y (B,Hd,Wd,4), z (B,Hd,Wd,zld) or None; channel 3 of a tap is not part of a 3-channel kind."""
    CO = 3 if kind in (0, 1) else 1
    y = np.asarray(y, dtype=np.float64)[..., :CO]
    t, a, n_terms = y, np.abs(y), 1
    if z is not None:
        zz = np.asarray(z, dtype=np.float64)[..., zoff:zoff + CO]
        t, a, n_terms = t + zz, a + np.abs(zz), 2
    bias = np.asarray(bias, dtype=np.float64)[:CO]
    v, A, coord = resize(t, a, H, W)
    pre = v + bias
    e = (n_terms + 8) * U32 * (A + np.abs(bias)) + coord
    ref, bound = activate(pre, e, kind, remap)
    return ref, bound, pre


def mlp_layer(x, W, bias, act):
    x, W, bias = (np.asarray(v, dtype=np.float64) for v in (x, W, bias))
    s = x @ W.T + bias
    e = (sum_depth(x.shape[1]) + 2) * U32 * (np.abs(x) @ np.abs(W).T + np.abs(bias))
    if act == 1:
        return np.maximum(s, 0), e
    if act == 2:
        return np.exp(s), np.exp(s) * e + K_ULP * ulp32(np.exp(s))
    return s, e


def layernorm(x, w, b, eps=1e-6, out_fp16=False):
    """Rows of x (rows, D) float64 (already rounded to the stream's type).  Returns dict(y, e_y, mean, e_mean, rstd, e_rstd)."""
    x, w, b = (np.asarray(v, dtype=np.float64) for v in (x, w, b))
    D = x.shape[1]
    d = sum_depth(D)
    mean = x.mean(-1, keepdims=True)
    a = x - mean
    q = (a * a).sum(-1, keepdims=True)
    var = q / D
    rstd = 1.0 / np.sqrt(var + eps)
    y = a * rstd * w + b
    e_mean = (d + 1) * U32 * np.abs(x).mean(-1, keepdims=True)
    e_a = e_mean + U32 * np.abs(a)
    e_q = (2 * np.abs(a) * e_a + e_a * e_a).sum(-1, keepdims=True) + (d + 2) * U32 * q
    e_var = e_q / D + 2 * U32 * (var + eps)
    e_rstd = rstd * (0.5 * e_var / (var + eps) + 4 * U32)
    e_y = np.abs(w) * (rstd * e_a + np.abs(a) * e_rstd + U32 * np.abs(a) * rstd) + 2 * U32 * (np.abs(a * rstd * w) + np.abs(b))
    if out_fp16:
        e_y = e_y + 2.0 ** -11 * np.abs(y) + 2.0 ** -25
    return dict(y=y, e_y=e_y, mean=mean[:, 0], e_mean=e_mean[:, 0], rstd=rstd[:, 0], e_rstd=e_rstd[:, 0])


def ln_finalize(part, D, eps=1e-6):
    """part (rows, NP, 2) fp32 (sum, sum of squares) partials -> (mean, e_mean, rstd, e_rstd): the stated formula on the given partials."""
    p = np.asarray(part, dtype=np.float64)
    NP = p.shape[1]
    s1, s2 = p[..., 0].sum(-1), p[..., 1].sum(-1)
    mean = s1 / D
    var = np.maximum(s2 / D - mean * mean, 0.0)
    rstd = 1.0 / np.sqrt(var + eps)
    e_mean = NP * U32 * np.abs(p[..., 0]).sum(-1) / D + 2 * U32 * np.abs(mean)
    e_var = (NP + 3) * U32 * s2 / D + 2 * np.abs(mean) * e_mean + 2 * U32 * mean * mean
    hi = 1.0 / np.sqrt(np.maximum(var - e_var, 0.0) + eps)
    lo = 1.0 / np.sqrt(var + e_var + eps)
    e_rstd = np.maximum(hi - rstd, rstd - lo) + 4 * U32 * rstd
    return mean, e_mean, rstd, e_rstd


def fold_ln(W, g, beta, b):
    """W (N,K), g / beta (K), b (N) fp32 -> Wf (fp16 values as float64, exact), c, e_c, bf, e_bf."""
    W32, g32 = np.asarray(W, dtype=np.float32), np.asarray(g, dtype=np.float32)
    Wf = (g32[None, :] * W32).astype(np.float16).astype(np.float64)
    K = W32.shape[1]
    d = sum_depth(K)
    W64, beta64, b64 = W32.astype(np.float64), np.asarray(beta, dtype=np.float64), np.asarray(b, dtype=np.float64)
    c = Wf.sum(-1)
    e_c = d * U32 * np.abs(Wf).sum(-1)
    bf = b64 + (beta64[None, :] * W64).sum(-1)
    e_bf = (d + 3) * U32 * (np.abs(b64) + np.abs(beta64[None, :] * W64).sum(-1))
    return Wf, c, e_c, bf, e_bf


def resize_bilinear_uv(x, OH, OW, out_fp16=False):
    """x (B,hs,ws,C) float64 (rounded to storage) -> the C resized channels (B,OH,OW,C) and their bound."""
    x = np.asarray(x, dtype=np.float64)
    v, A, coord = resize(x, np.abs(x), OH, OW)
    e = 8 * U32 * A + coord
    if out_fp16:
        e = e + 2.0 ** -11 * np.abs(v) + 2.0 ** -25
    return v, e


def u8_ingest(img):
    """uint8 (B,H,W,3) -> float32 (B,3,H,W) = image / 255: the division in float64, one rounding to float32."""
    return np.ascontiguousarray((np.asarray(img, dtype=np.uint8).astype(np.float64) / 255.0).astype(np.float32).transpose(0, 3, 1, 2))


# ---------------------------------------------------------------------------------------------------------------------
# post-processing half of infer()
# ---------------------------------------------------------------------------------------------------------------------
def postprocess(points, normal, mask_prob, metric, fov_x, flags, v1=False, mask_thr=0.5):
    """v2.py:246-289 (v1: v1.py:358, no `depth > 0` term in the mask) on forward outputs, torch fp32, from the oracle's own pieces.
    points (B,H,W,3), normal (B,H,W,3) or None, mask_prob (B,H,W), metric (B,) or None, fov_x (B,) degrees or None; flags bit 0 force_projection,
    bit 1 apply_mask.  Returns a dict of torch tensors (focal, shift, intrinsics, points, depth, mask, normal)."""
    import torch
    from oracle import moge_oracle as O
    B, H, W, _ = points.shape
    aspect = W / H
    mask_b = mask_prob > mask_thr
    if fov_x is None:
        focal, shift = O.recover_focal_shift(points, mask_b)
    else:
        fov = torch.as_tensor(fov_x, dtype=points.dtype)
        focal = aspect / (1 + aspect ** 2) ** 0.5 / torch.tan(torch.deg2rad(fov / 2))
        _, shift = O.recover_focal_shift(points, mask_b, focal=focal)
    fx = focal / 2 * (1 + aspect ** 2) ** 0.5 / aspect
    fy = focal / 2 * (1 + aspect ** 2) ** 0.5
    K = O._intrinsics(fx, fy)
    pts = points.clone()
    pts[..., 2] += shift[:, None, None]
    if not v1:
        mask_b = mask_b & (pts[..., 2] > 0)
    depth = pts[..., 2].clone()
    if flags & 1:
        pts = O._depth_to_points(depth, K)
    if metric is not None:
        pts = pts * metric[:, None, None, None]
        depth = depth * metric[:, None, None]
    if flags & 2:
        inf = torch.tensor(float("inf"), dtype=torch.float32)
        pts = torch.where(mask_b[..., None], pts, inf)
        depth = torch.where(mask_b, depth, inf)
        if normal is not None:
            normal = torch.where(mask_b[..., None], normal, torch.zeros_like(normal))
    return dict(focal=focal, shift=shift, intrinsics=K, points=pts, depth=depth, mask=mask_b, normal=normal)


def finalize_f32(points, normal, mask_prob, metric, shift, intr, flags, v1=False, mask_thr=0.5):
    """The same lines after the solve, in float32 numpy, from a GIVEN shift (B,) and intrinsics (B,3,3)."""
    f = np.float32
    points, mask_prob, shift, intr = (np.asarray(v, dtype=f) for v in (points, mask_prob, shift, intr))
    B, H, W, _ = points.shape
    x, y = points[..., 0].copy(), points[..., 1].copy()
    z = points[..., 2] + shift[:, None, None]
    m = mask_prob > f(mask_thr)
    if not v1:
        m = m & (z > 0)
    depth = z.copy()
    if flags & 1:
        u = ((np.arange(W, dtype=f) + f(0.5)) / f(W))[None, None, :]
        v = ((np.arange(H, dtype=f) + f(0.5)) / f(H))[None, :, None]
        x = (u - intr[:, 0, 2, None, None]) / intr[:, 0, 0, None, None] * depth
        y = (v - intr[:, 1, 2, None, None]) / intr[:, 1, 1, None, None] * depth
    if metric is not None:
        s = np.asarray(metric, dtype=f)[:, None, None]
        x, y, z, depth = x * s, y * s, z * s, depth * s
    pts = np.stack([x, y, z], -1).astype(f)
    nrm = None if normal is None else np.asarray(normal, dtype=f).copy()
    if flags & 2:
        pts[~m] = np.inf
        depth = np.where(m, depth, f(np.inf))
        if nrm is not None:
            nrm[~m] = 0
    return dict(points=pts, depth=depth.astype(f), mask=m, normal=nrm)
