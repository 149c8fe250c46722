"""Deterministic inputs shared by tests/test_tail_reference_cpu.py and tests/test_hip_tail_kernels.py."""
import numpy as np
import torch

import tail_reference as TR

# (Hd, Wd) -> (H, W): single pixel, broadcast, one row, identity (weights exactly 0 and 1), up (top clamp sy < 0 and bottom clamp y0 = Hd - 1), down, mixed
HEAD_SHAPES = [((1, 1), (1, 1)), ((1, 1), (5, 3)), ((1, 6), (4, 17)), ((5, 7), (5, 7)), ((4, 4), (13, 11)), ((16, 16), (5, 9)), ((3, 2), (2, 7))]
ACTS = [(0, 0), (0, 1), (0, 2), (0, 3), (1, 0), (2, 0), (3, 0)]          # (kind, remap)


def head_inputs(seed, B, Hd, Wd, C, ld, choff, kind, prec, n4, ksize=1, H=None, W=None):
    """Signed, channel-asymmetric inputs (a different scale per channel and per output: a permuted channel, output or tap changes the result),
    conditioned so that |pre-activation| stays below 4.  x / n4 are (B,Hd,Wd,ld) fp32 with channels [choff, choff + C) the kernel's input and a
    large finite value in the rest (a wrong slice is visible).  Returns a dict of numpy arrays; xs / n4s are the slices rounded to storage."""
    rng = np.random.default_rng(seed)
    CO = 3 if kind in (0, 1) else 1
    ch = 0.5 + np.arange(C) / max(C - 1, 1)                        # per-channel scale 0.5 ... 1.5
    oscale = 0.4 * (1 + np.arange(CO))[:, None]                    # per-output scale

    def fmap():
        m = np.full((B, Hd, Wd, ld), 1000.0, dtype=np.float32)
        m[..., choff:choff + C] = (rng.standard_normal((B, Hd, Wd, C)) * ch + 0.1).astype(np.float32)
        return m

    def weights():
        shape = (CO, C) if ksize == 1 else (CO, C, 3, 3)
        w = rng.standard_normal(shape) / np.sqrt(C * (9 if ksize == 3 else 1))
        if ksize == 3:
            w = w * (1 + 0.25 * np.arange(9).reshape(3, 3))        # asymmetric in (dy, dx)
            oscale_ = oscale[:, :, None, None]
        else:
            oscale_ = oscale
        return (w * oscale_).astype(np.float32)

    d = dict(x=fmap(), w=weights(), bias=np.array([0.3, -0.2, 0.5][:CO], dtype=np.float32), n4=None, w2=None)
    if n4:
        d["n4"], d["w2"] = fmap(), weights()
    d["xs"] = TR.to_storage(d["x"][..., choff:choff + C], prec)
    d["n4s"] = TR.to_storage(d["n4"][..., choff:choff + C], prec) if n4 else None
    pre = TR.head_final(d["xs"], d["w"], d["bias"], H or Hd, W or Wd, 3 if CO == 1 else 0, 0, d["n4s"], d["w2"])[2]
    top = float(np.abs(pre).max())
    if top > 3.0:                                                  # condition on the inputs: exp cannot overflow, the reference stays inside its bound
        for k in ("w", "w2", "bias"):
            if d[k] is not None:
                d[k] = (d[k] * np.float32(3.0 / top)).astype(np.float32)
    return d


def pinhole_scene(B, H, W, seed=11, thr=0.5):
    """A synthetic pin-hole scene as in test_recover_matches_oracle_lm, with mask_prob at least 0.05 away from `thr` and z + shift away from 0:
    points (B,H,W,3), normal (B,H,W,3) unit, mask_prob (B,H,W), metric (B,), fov (B,) degrees - torch fp32 on the CPU."""
    from oracle import moge_oracle as O
    g = torch.Generator().manual_seed(seed)
    uv = O.view_plane_uv(W, H)
    z = 1.0 + 2.0 * torch.rand(B, H, W, generator=g)
    f_true = torch.tensor([0.7, 1.1, 1.6])[:B].view(B, 1, 1, 1)
    s_true = torch.tensor([0.2, -0.3, 0.05])[:B].view(B, 1, 1)
    xy = uv[None] * (z + s_true)[..., None] / f_true + 0.01 * torch.randn(B, H, W, 2, generator=g)
    pts = torch.cat([xy, z[..., None]], dim=-1)
    iy, ix = torch.arange(64) * H // 64, torch.arange(64) * W // 64
    sampled = torch.zeros(H, W, dtype=torch.bool)
    sampled[iy[:, None], ix[None, :]] = True                      # the 64 x 64 nearest sub-sample the solve reads (geometry_torch.py:140)
    # points behind the camera after the shift (the `depth > 0` term of v2), only where the solve does not look: it stays well-posed
    far = (torch.rand(B, H, W, generator=g) < 0.15) & ~sampled
    pts[..., 2] = torch.where(far, -1.0 - torch.rand(B, H, W, generator=g), pts[..., 2])
    r = torch.rand(B, H, W, generator=g)
    side = torch.rand(B, H, W, generator=g) > 0.3
    mask_prob = torch.where(side, thr + 0.05 + (0.95 - thr) * r * 0.9, (thr - 0.05) * r)
    nrm = torch.nn.functional.normalize(torch.randn(B, H, W, 3, generator=g), dim=-1)
    metric = torch.tensor([1.7, 0.6, 2.3])[:B]
    fov = torch.tensor([55.0, 80.0, 40.0])[:B]
    return dict(points=pts.contiguous(), normal=nrm.contiguous(), mask_prob=mask_prob.contiguous(), metric=metric, fov=fov)
