"""float64 numpy restatement of the normal-guided depth refinement, written from the formulas, not from the reference's
code or the kernel's: the independent side of tests/test_hip_refine.py.  tests/test_refine_reference_cpu.py checks it against the outputs of the
reference's unmodified function (tests/golden/refine_*.npz).

    r = k // 2, x0 = log(max(depth, eps)), uv at pixel centres, Kinv = inverse(K), duv[a, b] = ((b - r) / W, (a - r) / H)
    g      = -(n_xy . Kinv[:2,:2]) / (n_z + n_xy . (Kinv[:2,:2] uv + Kinv[:2,2]))                    (row vector times matrix)
    w[p,t] = exp(-((x0[p+t] - x0[p]) / max(|duv[t]|, eps) / 10)^2)                                   interior pixels p, window taps t
    tot[p] = max(sum_t w, eps),   lap[p] = clamp(sum_t w[p,t] (g[p+t] + g[p]) . duv[t] / 2, -0.1, 0.1)
    x[p]  <- 0.1 x[p] + 0.9 (damp x0[p] - lap[p] + sum_t w[p,t] x[p+t]) / (tot[p] + damp)            Jacobi; the ring of width r keeps x0
    out    = exp(x)

With a mask: a tap on a masked-out pixel is left out of all three sums (it is skipped, so whatever the pixel holds never enters the arithmetic),
a masked-out pixel is never updated and is returned as its input depth, a masked-in ring pixel as exp(x0)."""
import numpy as np


def refine(depth, normal, K, iterations=10, damp=1e-3, eps=1e-12, kernel_size=5, mask=None):
    """One image: depth (H, W), normal (H, W, 3), K (3, 3), mask (H, W) bool or None -> refined depth (H, W) float64."""
    depth = np.asarray(depth, np.float64)
    normal = np.asarray(normal, np.float64)
    Kinv = np.linalg.inv(np.asarray(K, np.float64))
    H, W = depth.shape
    k, r = kernel_size, kernel_size // 2
    valid = np.ones((H, W), bool) if mask is None else np.asarray(mask, bool)
    x0 = np.zeros((H, W))
    x0[valid] = np.log(np.maximum(depth[valid], eps))
    v, u = np.meshgrid((np.arange(H) + 0.5) / H, (np.arange(W) + 0.5) / W, indexing="ij")
    g = np.zeros((H, W, 2))
    with np.errstate(all="ignore"):
        nx, ny, nz = normal[..., 0], normal[..., 1], normal[..., 2]
        den = nz + nx * (Kinv[0, 0] * u + Kinv[0, 1] * v + Kinv[0, 2]) + ny * (Kinv[1, 0] * u + Kinv[1, 1] * v + Kinv[1, 2])
        gx = -(nx * Kinv[0, 0] + ny * Kinv[1, 0]) / den
        gy = -(nx * Kinv[0, 1] + ny * Kinv[1, 1]) / den
    g[valid, 0], g[valid, 1] = gx[valid], gy[valid]                  # values under the mask are never read below
    hi, wi = H - 2 * r, W - 2 * r
    ctr = (slice(r, H - r), slice(r, W - r))
    taps = []                                                        # (window slice, weight, validity of the tap) per tap
    tot = np.zeros((hi, wi))
    lap = np.zeros((hi, wi))
    for a in range(k):
        for b in range(k):
            win = (slice(a, a + hi), slice(b, b + wi))
            du, dv = (b - r) / W, (a - r) / H
            ok = valid[win] & valid[ctr]
            w = np.where(ok, np.exp(-((x0[win] - x0[ctr]) / max(np.hypot(du, dv), eps) / 10) ** 2), 0.0)
            tot += w
            lap += w * ((g[win][..., 0] + g[ctr][..., 0]) * du + (g[win][..., 1] + g[ctr][..., 1]) * dv) / 2
            taps.append((win, w))
    tot = np.maximum(tot, eps)
    lap = np.clip(lap, -0.1, 0.1)
    x = x0.copy()
    for _ in range(iterations):
        s = np.zeros((hi, wi))
        for win, w in taps:
            s += w * x[win]
        new = 0.1 * x[ctr] + 0.9 * (damp * x0[ctr] - lap + s) / (tot + damp)
        x[ctr] = np.where(valid[ctr], new, x[ctr])
    return np.where(valid, np.exp(x), depth)


def refine_batch(depth, normal, K, mask=None, **kw):
    """Leading batch dims: depth (..., H, W), normal (..., H, W, 3), K (..., 3, 3), mask (..., H, W) or None."""
    depth = np.asarray(depth)
    H, W = depth.shape[-2:]
    d, n, k = depth.reshape(-1, H, W), np.asarray(normal).reshape(-1, H, W, 3), np.asarray(K).reshape(-1, 3, 3)
    m = None if mask is None else np.asarray(mask).reshape(-1, H, W)
    out = np.stack([refine(d[i], n[i], k[i], mask=None if m is None else m[i], **kw) for i in range(d.shape[0])])
    return out.reshape(depth.shape)
