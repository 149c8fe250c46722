"""Golden fixtures of the normal-guided depth refinement (tests/golden/refine_*.npz) from the reference's unmodified
`moge.utils.geometry_torch.refine_depth_with_normal` on the CPU.

    python tools/make_refine_golden.py          (build machine: needs the reference checkout of oracle/make_golden.py)

The reference calls three utils3d functions that are not vendored; beside oracle.make_golden.install_stubs() (which also supplies the empty cv2)
this file supplies them, in the conventions of this repository's other utils3d stand-ins:
  * sliding_window(x, window_size, stride, dim) / sliding_window_2d: stride-1 windows by `unfold` over the two given dims, window dims appended;
  * uv_map((H, W)): pixel centres in [0, 1], u right / v down, (H, W, 2) (moge_amd.io.uv_map).
Scenes (camera frame, pinhole K with an off-centre principal point, one with skew): a tilted plane, two planes meeting in a depth step, a smooth
bumpy surface; exact normals, depth with 1 % multiplicative noise.  Every scene keeps |n_z + n_xy . (Kinv[:2,:2] uv + Kinv[:2,2])| >= 0.05 and
depth in [0.3, 30] (asserted), so the reference alone is finite.  Normals are stored as fp16 (the inputs ARE those rounded values).  A fixture
holds depth / normal / intrinsics, the reference's float64 and fp32 outputs at the defaults (k = 5, 10 iterations), ref32_err = max |log out32 -
log out64|, and for the small scenes float64 outputs at other (k, iterations) under out64_k<k>_i<iterations>."""
from __future__ import annotations

import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

EXTRA = [(3, 0), (3, 2), (3, 11), (5, 1), (7, 1), (7, 10)]          # (k, iterations) beside the default, small scenes only


def _stub_sliding_window(x, window_size, stride=1, dim=(-2, -1)):
    assert stride == 1 and len(dim) == 2
    d0, d1 = (d % x.dim() for d in dim)
    return x.unfold(d0, window_size, 1).unfold(d1, window_size, 1)


def _stub_uv_map(size, device=None, dtype=None):
    H, W = size
    u = (torch.arange(W, device=device, dtype=dtype) + 0.5) / W
    v = (torch.arange(H, device=device, dtype=dtype) + 0.5) / H
    return torch.stack(torch.meshgrid(u, v, indexing="xy"), dim=-1)


def install():
    from oracle.make_golden import install_stubs
    install_stubs()
    pt = sys.modules["utils3d"].pt
    pt.sliding_window = _stub_sliding_window
    pt.sliding_window_2d = _stub_sliding_window
    pt.uv_map = _stub_uv_map


def rays(H, W, K):
    v, u = np.meshgrid((np.arange(H) + 0.5) / H, (np.arange(W) + 0.5) / W, indexing="ij")
    return np.stack([u, v, np.ones_like(u)], -1) @ np.linalg.inv(K).T, u, v


def plane(H, W, K, n, c):
    """depth and normal of the plane n . P = c seen through K"""
    n = np.asarray(n, np.float64) / np.linalg.norm(n)
    ray, _, _ = rays(H, W, K)
    return c / (ray @ n), np.broadcast_to(n, (H, W, 3)).copy()


def bumpy(H, W, K):
    """z(u, v) smooth; normal = dP/du x dP/dv of P = z ray"""
    ray, u, v = rays(H, W, K)
    Kinv = np.linalg.inv(K)
    z = 3.0 + 0.4 * np.sin(5.0 * u + 0.3) * np.cos(4.0 * v) + 0.8 * u - 0.5 * v
    zu = 0.4 * 5.0 * np.cos(5.0 * u + 0.3) * np.cos(4.0 * v) + 0.8
    zv = -0.4 * 4.0 * np.sin(5.0 * u + 0.3) * np.sin(4.0 * v) - 0.5
    pu = zu[..., None] * ray + z[..., None] * Kinv[:, 0]
    pv = zv[..., None] * ray + z[..., None] * Kinv[:, 1]
    n = np.cross(pu, pv)
    return z, n / np.linalg.norm(n, axis=-1, keepdims=True)


def scene(name, H, W, kind, K, seed):
    rng = np.random.default_rng(seed)
    K = np.asarray(K, np.float64)
    if kind == "plane":
        depth, normal = plane(H, W, K, (0.25, -0.35, -0.9), -2.5)
    elif kind == "step":
        d0, n0 = plane(H, W, K, (0.3, 0.1, -0.95), -2.0)
        d1, n1 = plane(H, W, K, (-0.2, 0.25, -0.94), -4.5)
        right = np.broadcast_to(np.arange(W)[None, :] >= (W + 1) // 2, (H, W))
        depth, normal = np.where(right, d1, d0), np.where(right[..., None], n1, n0)
    else:
        depth, normal = bumpy(H, W, K)
    depth = (depth * (1.0 + 0.01 * rng.standard_normal((H, W)))).astype(np.float32)
    normal = normal.astype(np.float16)
    K32 = K.astype(np.float32)
    Kinv = np.linalg.inv(K32.astype(np.float64))
    _, u, v = rays(H, W, K32.astype(np.float64))
    n = normal.astype(np.float64)
    den = n[..., 2] + n[..., 0] * (Kinv[0, 0] * u + Kinv[0, 1] * v + Kinv[0, 2]) + n[..., 1] * (Kinv[1, 0] * u + Kinv[1, 1] * v + Kinv[1, 2])
    assert np.abs(den).min() >= 0.05, (name, np.abs(den).min())
    assert depth.min() >= 0.3 and depth.max() <= 30, (name, depth.min(), depth.max())
    return depth, normal, K32


CASES = [("plane_5x5", 5, 5, "plane", [[0.9, 0, 0.45], [0, 0.9, 0.56], [0, 0, 1]]),
         ("step_5x9", 5, 9, "step", [[0.8, 0, 0.52], [0, 1.4, 0.47], [0, 0, 1]]),
         ("bumpy_12x7", 12, 7, "bumpy", [[1.3, 0.04, 0.55], [0, 0.75, 0.44], [0, 0, 1]]),           # skew
         ("step_37x53", 37, 53, "step", [[0.85, 0, 0.46], [0, 1.2, 0.53], [0, 0, 1]]),
         ("bumpy_70x131", 70, 131, "bumpy", [[0.7, 0, 0.54], [0, 1.3, 0.48], [0, 0, 1]])]


def main():
    install()
    from moge.utils.geometry_torch import refine_depth_with_normal as ref
    os.makedirs(GOLDEN, exist_ok=True)
    for seed, (name, H, W, kind, K) in enumerate(CASES):
        depth, normal, K32 = scene(name, H, W, kind, K, 100 + seed)

        def run(dtype, **kw):
            out = ref(torch.from_numpy(depth).to(dtype).clone(), torch.from_numpy(normal).to(dtype), torch.from_numpy(K32).to(dtype), **kw)
            assert bool(torch.isfinite(out).all()), (name, kw)
            return out.numpy()

        out64, out32 = run(torch.float64), run(torch.float32)
        data = {"depth": depth, "normal": normal, "intrinsics": K32, "out64": out64, "out32": out32,
                "ref32_err": np.float64(np.abs(np.log(out32.astype(np.float64)) - np.log(out64)).max())}
        if H * W < 1000:
            for k, it in EXTRA:
                if H >= k and W >= k:
                    data[f"out64_k{k}_i{it}"] = run(torch.float64, kernel_size=k, iterations=it)
        path = os.path.join(GOLDEN, f"refine_{name}.npz")
        np.savez_compressed(path, **data)
        size = os.path.getsize(path)
        assert size < 200 * 1024, (path, size)
        print(f"{path}: {size} bytes, ref32_err {data['ref32_err']:.3e}")


if __name__ == "__main__":
    main()
