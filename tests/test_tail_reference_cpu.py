"""CPU: every float64 numpy reference of tests/tail_reference.py against an independent torch formulation of the same operation, so that a wrong
reference cannot pass a wrong kernel in tests/test_hip_tail_kernels.py.  Where torch can run the operation in float32 too, that result must sit
inside the derived bound: a bound a correct fp32 implementation misses would be useless."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import tail_fixtures as TF
import tail_reference as TR


def _aten_matrix(n_in, n_out):
    """(n_out, n_in) bilinear weights as ATen itself computes them in float32: the resize of the identity (products with 0 and 1 are exact)."""
    eye = torch.eye(n_in, dtype=torch.float32).view(1, n_in, n_in, 1)
    return F.interpolate(eye, size=(n_out, 1), mode="bilinear", align_corners=False)[0, :, :, 0].T.double()


def _torch_remap(p, kind, remap):
    from oracle import moge_oracle as O
    if kind == 0:
        return O.remap_points(p, TR.REMAPS[remap])
    if kind == 1:
        return F.normalize(p, dim=-1)
    return torch.sigmoid(p) if kind == 2 else p


@pytest.mark.parametrize("ksize,C,n4", [(1, 8, False), (1, 32, True), (3, 8, False)])
@pytest.mark.parametrize("shape", TF.HEAD_SHAPES)
def test_head_reference_matches_torch(shape, ksize, C, n4):
    (Hd, Wd), (H, W) = shape
    for kind, remap in TF.ACTS:
        d = TF.head_inputs(3, 2, Hd, Wd, C, C, 0, kind, 0, n4, ksize, H, W)
        ref, bound, pre = TR.head_final(d["xs"], d["w"], d["bias"], H, W, kind, remap, d["n4s"], d["w2"])
        assert np.abs(pre).max() < 4 and (bound > 0).all()

        def conv(x, w, dtype):
            x = torch.from_numpy(np.asarray(x)).to(dtype).permute(0, 3, 1, 2)
            w = torch.from_numpy(w).to(dtype)
            if ksize == 3:
                return F.conv2d(F.pad(x, (1, 1, 1, 1), mode="replicate"), w)
            return F.conv2d(x, w[:, :, None, None])

        def low(dtype):
            t = conv(d["xs"], d["w"], dtype)
            if n4:
                t = t + conv(d["n4s"], d["w2"], dtype)
            return t + torch.from_numpy(d["bias"]).to(dtype)[None, :, None, None]

        # float64 conv, ATen's own float32 lerp weights (the resize of the identity).  ATen's CPU build may contract the source coordinate into an
        # FMA where numpy does not: that is the coordinate term of the bound, and the only difference allowed here
        low64 = low(torch.float64)
        coord = TR.resize(low64.permute(0, 2, 3, 1).numpy(), np.abs(low64.permute(0, 2, 3, 1).numpy()), H, W)[2]
        My, Mx = _aten_matrix(Hd, H), _aten_matrix(Wd, W)
        want_pre = torch.einsum("oh,bchw,pw->bopc", My, low64, Mx).numpy()
        assert (np.abs(pre - want_pre) <= coord + 1e-12).all(), float(np.abs(pre - want_pre).max())
        if (Hd, Wd) == (H, W):
            assert (np.abs(pre - low64.permute(0, 2, 3, 1).numpy()) <= 1e-13).all()              # identity: weights exactly 0 and 1
        np.testing.assert_allclose(ref, _torch_remap(torch.from_numpy(pre), kind, remap).numpy(), rtol=1e-12, atol=1e-12)
        # F.interpolate(F.conv2d(...)) end to end: in float64 it differs by its float64 source coordinate only, in float32 it is an fp32 implementation
        e2e = F.interpolate(low64, size=(H, W), mode="bilinear", align_corners=False).permute(0, 2, 3, 1).numpy()
        assert (np.abs(pre - e2e) <= 3 * coord + 1e-12).all(), float(np.abs(pre - e2e).max())
        f32 = _torch_remap(F.interpolate(low(torch.float32), size=(H, W), mode="bilinear", align_corners=False).permute(0, 2, 3, 1), kind, remap)
        assert (np.abs(f32.double().numpy() - ref) <= bound).all(), (shape, kind, remap, float((np.abs(f32.double().numpy() - ref) / bound).max()))


def test_head_dot_reference_is_the_head_with_unit_weights():
    rng = np.random.default_rng(0)
    y, z = rng.standard_normal((2, 4, 5, 4)), rng.standard_normal((2, 4, 5, 12))
    y[..., 3] = 1e4
    bias = np.array([0.3, -0.2, 0.5])
    for kind, remap in TF.ACTS:
        CO = 3 if kind in (0, 1) else 1
        ref, bound, _ = TR.head_final_dot(y, z, 4, bias, 9, 13, kind, remap)
        want = TR.head_final(np.concatenate([y[..., :CO], z[..., 4:4 + CO]], -1), np.concatenate([np.eye(CO), np.eye(CO)], 1), bias[:CO], 9, 13, kind, remap)[0]
        np.testing.assert_allclose(ref, want, rtol=1e-13, atol=1e-13)
        assert np.isfinite(bound).all()


@pytest.mark.parametrize("K,N,act", [(4, 1, 0), (252, 3, 1), (1024, 5, 2)])
def test_mlp_reference_matches_torch(K, N, act):
    g = torch.Generator().manual_seed(K)
    x, W, b = torch.randn(3, K, generator=g), torch.randn(N, K, generator=g) / K ** 0.5, torch.randn(N, generator=g)
    ref, bound = TR.mlp_layer(x.numpy(), W.numpy(), b.numpy(), act)
    f = [lambda t: t, torch.relu, torch.exp][act]
    np.testing.assert_allclose(ref, f(F.linear(x.double(), W.double(), b.double())).numpy(), rtol=1e-12, atol=1e-13)
    assert (np.abs(f(F.linear(x, W, b)).double().numpy() - ref) <= bound).all()


@pytest.mark.parametrize("D", [128, 384, 640, 1024])
def test_layernorm_reference_matches_torch(D):
    g = torch.Generator().manual_seed(D)
    x = torch.randn(9, D, generator=g)
    x[1] = 50 + 0.1 * torch.randn(D, generator=g)                    # mean >> spread
    x[2] = 0.75                                                      # constant row
    w, b = 1 + 0.3 * torch.randn(D, generator=g), 0.2 * torch.randn(D, generator=g)
    r = TR.layernorm(x.numpy(), w.numpy(), b.numpy())
    want = F.layer_norm(x.double(), (D,), w.double(), b.double(), eps=1e-6)
    np.testing.assert_allclose(r["y"], want.numpy(), rtol=1e-9, atol=1e-9)
    np.testing.assert_allclose(r["mean"], x.double().mean(-1).numpy(), rtol=1e-13)
    np.testing.assert_allclose(r["rstd"], (x.double().var(-1, unbiased=False) + 1e-6).rsqrt().numpy(), rtol=1e-12)
    got32 = F.layer_norm(x, (D,), w, b, eps=1e-6).double().numpy()
    assert (np.abs(got32 - r["y"]) <= r["e_y"]).all(), float((np.abs(got32 - r["y"]) / r["e_y"]).max())
    # a one-pass variance in float32 must NOT fit the bound on the large-mean row: that row is what separates the two
    m32 = x.mean(-1, keepdim=True)
    one_pass = ((x - m32) * ((x * x).mean(-1, keepdim=True) - m32 * m32 + 1e-6).clamp_min(1e-12).rsqrt() * w + b).double().numpy()
    assert (np.abs(one_pass[1] - r["y"][1]) > r["e_y"][1]).any()


@pytest.mark.parametrize("NP", [4, 12, 24, 32])
def test_ln_finalize_reference_matches_the_moments_of_the_data(NP):
    D = 32 * NP
    x = np.random.default_rng(NP).standard_normal((7, D)) * 0.7 + 0.3
    part = np.stack([x.reshape(7, NP, 32).sum(-1), (x * x).reshape(7, NP, 32).sum(-1)], -1)          # exact float64 partials
    mean, e_mean, rstd, e_rstd = TR.ln_finalize(part, D)
    xt = torch.from_numpy(x)
    np.testing.assert_allclose(mean, xt.mean(-1).numpy(), rtol=1e-12)
    np.testing.assert_allclose(rstd, (xt.var(-1, unbiased=False) + 1e-6).rsqrt().numpy(), rtol=1e-10)
    const = np.zeros((1, NP, 2))
    const[..., 0], const[..., 1] = 16.0, 8.0                          # 32 values of 0.5
    mean, e_mean, rstd, e_rstd = TR.ln_finalize(const, D)
    assert mean[0] == 0.5 and rstd[0] == 1.0 / np.sqrt(1e-6) and e_rstd[0] > 0


@pytest.mark.parametrize("N,K", [(1, 4), (5, 72), (2, 1024)])
def test_fold_ln_reference_matches_torch(N, K):
    g = torch.Generator().manual_seed(K)
    W, gam, beta, b = torch.randn(N, K, generator=g), 1 + 0.3 * torch.randn(K, generator=g), 0.3 * torch.randn(K, generator=g), torch.randn(N, generator=g)
    Wf, c, e_c, bf, e_bf = TR.fold_ln(W.numpy(), gam.numpy(), beta.numpy(), b.numpy())
    want = (gam[None] * W).half()
    assert np.array_equal(Wf, want.double().numpy())
    np.testing.assert_allclose(c, want.double().sum(-1).numpy(), rtol=1e-13)
    if K == 72:                 # the sum of the rounded weights and the sum of g w are told apart by the bound
        assert np.abs(c - (gam[None].double() * W.double()).sum(-1).numpy()).max() > 10 * e_c.max()
    np.testing.assert_allclose(bf, (b.double() + (beta.double()[None] * W.double()).sum(-1)).numpy(), rtol=1e-12, atol=1e-13)


@pytest.mark.parametrize("hs,ws,OH,OW", [(4, 4, 13, 11), (16, 16, 5, 9), (5, 7, 5, 7), (1, 6, 4, 17), (3, 1, 2, 7)])
def test_resize_reference_matches_torch(hs, ws, OH, OW):
    x = np.random.default_rng(hs).standard_normal((2, hs, ws, 4))
    v, e = TR.resize_bilinear_uv(x, OH, OW)
    want = torch.einsum("oh,bhwc,pw->bopc", _aten_matrix(hs, OH), torch.from_numpy(x), _aten_matrix(ws, OW))
    coord = TR.resize(x, np.abs(x), OH, OW)[2]
    assert (np.abs(v - want.numpy()) <= coord + 1e-13).all()          # ATen's CPU build may contract the source coordinate: the coordinate term, nothing else
    if (hs, ws) == (OH, OW):
        assert np.array_equal(v, x)
    f32 = F.interpolate(torch.from_numpy(x).float().permute(0, 3, 1, 2), size=(OH, OW), mode="bilinear", align_corners=False).permute(0, 2, 3, 1)
    assert (np.abs(f32.double().numpy() - TR.resize_bilinear_uv(torch.from_numpy(x).float().numpy(), OH, OW)[0]) <= e + 1e-7).all()


def test_u8_ingest_reference_matches_the_callers_expression():
    img = np.random.default_rng(0).integers(0, 256, (2, 7, 37, 3), dtype=np.uint8)
    img.reshape(-1, 3)[:256] = np.arange(256, dtype=np.uint8)[:, None]
    want = torch.stack([torch.tensor(i / 255, dtype=torch.float32).permute(2, 0, 1) for i in img])
    assert np.array_equal(TR.u8_ingest(img), want.numpy())


@pytest.mark.parametrize("flags", [0, 1, 2, 3])
@pytest.mark.parametrize("use_fov", [False, True])
def test_postprocess_restatement_matches_the_oracles_infer(flags, use_fov, monkeypatch):
    from oracle import moge_oracle as O
    from oracle import moge_oracle_v1 as O1
    B, H, W = 2, 33, 70
    img = torch.zeros(B, 3, H, W)
    for v1, thr in ((False, 0.5), (True, 0.3)):
        s = TF.pinhole_scene(B, H, W, thr=thr)
        fov = s["fov"] if use_fov else None
        kw = dict(force_projection=bool(flags & 1), apply_mask=bool(flags & 2), fov_x=fov, num_tokens=100)
        if v1:
            monkeypatch.setattr(O1, "forward", lambda *a, **k: {"points": s["points"].clone(), "mask": s["mask_prob"].clone()})
            want = O1.infer({**O1.named_configs()["tiny-v1-vits"], "mask_threshold": thr}, {}, img, **kw)
            got = TR.postprocess(s["points"], None, s["mask_prob"], None, fov, flags, True, thr)
        else:
            monkeypatch.setattr(O, "forward", lambda *a, **k: {"points": s["points"].clone(), "normal": s["normal"].clone(), "mask": s["mask_prob"].clone(),
                                                               "metric_scale": s["metric"].clone()})
            want = O.infer(O.named_configs()["tiny-vits-normal"], {}, img, **kw)
            got = TR.postprocess(s["points"], s["normal"], s["mask_prob"], s["metric"], fov, flags, False, thr)
        for k, v in want.items():
            assert torch.equal(got[k], v), (v1, k)
        # ... and the float32 numpy form of the lines after the solve agrees with it to the last bits
        f = TR.finalize_f32(s["points"].numpy(), None if v1 else s["normal"].numpy(), s["mask_prob"].numpy(), None if v1 else s["metric"].numpy(),
                            got["shift"].numpy(), got["intrinsics"].numpy(), flags, v1, thr)
        assert np.array_equal(f["mask"], got["mask"].numpy())
        assert (got["mask"] != (s["mask_prob"] > thr)).any() != v1              # the scene exercises the `depth > 0` term
        for k in ("points", "depth"):
            a, b = f[k], got[k].numpy()
            assert np.array_equal(np.isinf(a), np.isinf(b))
            fin = np.isfinite(b)
            assert (np.abs(a[fin] - b[fin]) <= 2 * np.spacing(np.abs(b[fin]))).all(), k
