"""moge_amd.refine (csrc/refine.hip) against the float64 restatement of tests/refine_reference.py, which tests/test_refine_reference_cpu.py ties
to the reference's unmodified function.  The gate is |log got - log ref64| per element with

    bound = max(4 x ref32_err of the case, 16 fp32 ulps of max |log depth|)

ref32_err being the reference's own fp32-against-float64 error on that fixture (the margin of 4 covers another summation order over up to 49
taps and the hardware exp at 1-2 ulp against libm, times at most 10 non-amplifying iterations); scenes that are not fixtures have no ref32_err
and get the 16-ulp term alone.  Exact properties (masked-out pixels, all-true mask = no mask, batch = alone, run = rerun) are checked bit for bit.

The kernel's tile is moge_amd.refine.TILE = 32 (square): TILE_SHAPES sits on it, a pixel under and a pixel over in each dimension, and 70 x 67 is
more than two tiles both ways.

Worst observed error / bound per group, measured on an MI355X (40 passed, 3.7 s for the module; `pytest -s` prints the table of the run at hand):
  fixtures k=3 0.096   fixtures k=5 0.069   fixtures k=7 0.068   (25 / 25 / 15 cases: five scenes x 0, 1, 2, 10, 11 iterations)
  tile edges k=3 0.079   tile edges k=5 0.072   tile edges k=7 0.068   single pixel k=7 0.054   batch 0.065   zeros 0.018
  mask k=3 0.070   mask k=5 0.064   mask k=7 0.061
Nearly all of it is the fp32 rounding of log(depth) itself (half an ulp of x0 = 1/32 of a 16-ulp bound, and the exp back): the iteration sums
w (x[p+t] - x[p]), so its own rounding scales with the update, not with |x| sum w.  Summing w x[p+t] directly used 0.12 - 0.75 of the bound
(EXPERIMENTS.md R8.1)."""
import ctypes as C
import glob
import os

import numpy as np
import pytest
import torch

import refine_reference as RR

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FIXTURES = sorted(os.path.basename(p)[len("refine_"):-len(".npz")] for p in glob.glob(os.path.join(GOLDEN, "refine_*.npz")))
TILE = 32
TILE_SHAPES = [(32, 32), (31, 33), (33, 31), (70, 67)]
ITERATIONS = [0, 1, 2, 10, 11]
WORST = {}


@pytest.fixture(scope="module")
def R():
    import moge_amd.refine as refine
    assert refine.TILE == TILE
    yield refine
    print("\nworst error / bound per group:")
    for k in sorted(WORST):
        print(f"  {k:24s} {WORST[k][0]:8.4f}   ({WORST[k][1]} cases)")


def ulp16(depth, eps=1e-12):
    return 16 * float(np.spacing(np.float32(np.abs(np.log(np.maximum(depth.astype(np.float64), eps))).max())))


def check(group, got, ref, bound, what, where=None):
    got = got.detach().cpu().double().numpy() if torch.is_tensor(got) else np.asarray(got, np.float64)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    if where is not None:
        got, ref = got[where], ref[where]
    assert np.isfinite(got).all(), what
    ratio = np.abs(np.log(got) - np.log(ref)) / bound
    worst = float(ratio.max())
    w = WORST.setdefault(group, [0.0, 0])
    w[0], w[1] = max(w[0], worst), w[1] + 1
    assert worst <= 1.0, f"{group} {what}: error / bound = {worst:.3f} (bound {bound:.3e})"


def cuda(*arrays):
    return tuple(torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in arrays)


def load(name):
    z = np.load(os.path.join(GOLDEN, f"refine_{name}.npz"))
    return z["depth"], z["normal"].astype(np.float32), z["intrinsics"], float(z["ref32_err"])


def scene(H, W, seed, batch=()):
    """Two noisy planes meeting in a depth step, one K per image (off-centre principal point, skew): |den| >= 0.05, depth in [0.3, 30]."""
    rng = np.random.default_rng(seed)
    n_img = int(np.prod(batch, dtype=np.int64))
    depth, normal, Ks = [], [], []
    v, u = np.meshgrid((np.arange(H) + 0.5) / H, (np.arange(W) + 0.5) / W, indexing="ij")
    for _ in range(n_img):
        K = np.array([[rng.uniform(0.7, 1.3), rng.uniform(-0.03, 0.03), rng.uniform(0.44, 0.56)], [0, rng.uniform(0.7, 1.3), rng.uniform(0.44, 0.56)], [0, 0, 1]])
        ray = np.stack([u, v, np.ones_like(u)], -1) @ np.linalg.inv(K).T
        planes = []
        for c in (rng.uniform(1.5, 2.5), rng.uniform(4.0, 6.0)):
            n = np.array([rng.uniform(-0.2, 0.2), rng.uniform(-0.2, 0.2), -1.0])
            n /= np.linalg.norm(n)
            planes.append((-c / (ray @ n), n))
        right = (u + 0.3 * v > rng.uniform(0.5, 0.8))
        d = np.where(right, planes[1][0], planes[0][0]) * (1 + 0.01 * rng.standard_normal((H, W)))
        nm = np.where(right[..., None], planes[1][1], planes[0][1]).astype(np.float32)
        K32 = K.astype(np.float32)
        rayk = np.stack([u, v, np.ones_like(u)], -1) @ np.linalg.inv(K32.astype(np.float64)).T
        assert np.abs((rayk * nm).sum(-1)).min() >= 0.05 and d.min() >= 0.3 and d.max() <= 30
        depth.append(d.astype(np.float32)); normal.append(nm); Ks.append(K32)
    return np.stack(depth).reshape(batch + (H, W)), np.stack(normal).reshape(batch + (H, W, 3)), np.stack(Ks).reshape(batch + (3, 3))


# ------------------------------------------------------------------------------------------------------------------ accuracy
@pytest.mark.parametrize("k", [3, 5, 7])
@pytest.mark.parametrize("name", FIXTURES)
def test_fixtures(R, name, k):
    """Every fixture at every window that fits and at 0, 1, 2, 10, 11 iterations (none, one launch, both ping-pong parities).  plane_5x5 at k = 5 is
    a single interior pixel."""
    depth, normal, K, ref32_err = load(name)
    if min(depth.shape) < k:
        with pytest.raises(ValueError):
            R.refine_depth_with_normal(*cuda(depth, normal, K), kernel_size=k)
        return
    bound = max(4 * ref32_err, ulp16(depth))
    d, n, kk = cuda(depth, normal, K)
    for it in ITERATIONS:
        got = R.refine_depth_with_normal(d, n, kk, iterations=it, kernel_size=k)
        check(f"fixtures k={k}", got, RR.refine(depth, normal, K, iterations=it, kernel_size=k), bound, f"{name} it={it}")


def test_single_interior_pixel_k7(R):
    depth, normal, K = scene(7, 7, 3)
    for it in (1, 10):
        got = R.refine_depth_with_normal(*cuda(depth, normal, K), iterations=it, kernel_size=7)
        ref = RR.refine(depth, normal, K, iterations=it, kernel_size=7)
        check("single pixel k=7", got, ref, ulp16(depth), f"it={it}")
        ring = np.ones((7, 7), bool)
        ring[3, 3] = False
        assert np.abs(ref[3, 3] / depth[3, 3] - 1) > 1e-4 and np.allclose(ref[ring], depth[ring], rtol=1e-12)


@pytest.mark.parametrize("k", [3, 5, 7])
@pytest.mark.parametrize("shape", TILE_SHAPES)
def test_tile_edges(R, shape, k):
    depth, normal, K = scene(*shape, seed=shape[0] * 100 + shape[1])
    d, n, kk = cuda(depth, normal, K)
    for it in (1, 10, 11):
        got = R.refine_depth_with_normal(d, n, kk, iterations=it, kernel_size=k)
        check(f"tile edges k={k}", got, RR.refine(depth, normal, K, iterations=it, kernel_size=k), ulp16(depth), f"{shape} it={it}")


@pytest.mark.parametrize("batch", [(), (3,), (2, 2)])
def test_batch_shapes(R, batch):
    depth, normal, K = scene(37, 45, 11, batch)
    got = R.refine_depth_with_normal(*cuda(depth, normal, K), iterations=3)
    assert got.shape == depth.shape and got.dtype == torch.float32
    check("batch", got, RR.refine_batch(depth, normal, K, iterations=3), ulp16(depth), str(batch))


def test_alone_equals_in_batch_and_rerun(R):
    depth, normal, K = scene(45, 70, 12, (4,))
    mask = np.random.default_rng(0).random(depth.shape) > 0.1
    for m in (None, mask):
        args = cuda(depth, normal, K)
        mt = None if m is None else torch.from_numpy(m).cuda()
        a = R.refine_depth_with_normal(*args, iterations=5, mask=mt)
        b = R.refine_depth_with_normal(*args, iterations=5, mask=mt)
        alone = R.refine_depth_with_normal(args[0][2], args[1][2], args[2][2], iterations=5, mask=None if m is None else mt[2])
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
        assert torch.equal(a[2].view(torch.int32), alone.view(torch.int32))


def test_zero_iterations(R):
    """exp(log(max(depth, eps))) within 2 fp32 ulp, the log rounded to fp32 as the x0 plane holds it"""
    depth, normal, K = scene(33, 47, 13)
    depth[3, 4], depth[10, 11], depth[0, 0] = 0.0, 1e-20, 29.9
    got = R.refine_depth_with_normal(*cuda(depth, normal, K), iterations=0).cpu().numpy()
    x0 = np.log(np.maximum(depth.astype(np.float64), 1e-12)).astype(np.float32)
    want = np.exp(x0.astype(np.float64))
    assert (np.abs(got.astype(np.float64) - want) <= 2 * np.spacing(want.astype(np.float32))).all()


def test_zeros_and_tiny_depth(R):
    depth, normal, K = scene(33, 47, 14)
    depth[5, 6], depth[20, 30], depth[21, 30], depth[0, 46] = 0.0, 1e-20, 1e-13, 0.0
    got = R.refine_depth_with_normal(*cuda(depth, normal, K), iterations=10)
    ref = RR.refine(depth, normal, K, iterations=10)
    check("zeros", got, ref, ulp16(depth), "zeros and values below eps")


# ------------------------------------------------------------------------------------------------------------------ mask
def masks(H, W):
    rng = np.random.default_rng(5)
    holes = rng.random((H, W)) > 0.12
    holes[10:15, 7:19] = False
    band = np.ones((H, W), bool)
    band[:3], band[-2:], band[:, :4], band[:, -1:] = False, False, False, False
    island = np.zeros((H, W), bool)
    island[20, 33] = True
    return {"holes": holes, "border band": band, "island": island}


@pytest.mark.parametrize("k", [3, 5, 7])
def test_mask(R, k):
    depth, normal, K = scene(41, 67, 15)
    d, n, kk = cuda(depth, normal, K)
    a = R.refine_depth_with_normal(d, n, kk, iterations=4, kernel_size=k)
    b = R.refine_depth_with_normal(d, n, kk, iterations=4, kernel_size=k, mask=torch.ones(depth.shape, dtype=torch.bool, device="cuda"))
    assert torch.equal(a.view(torch.int32), b.view(torch.int32)), "an all-true mask is mask=None"
    for what, m in masks(*depth.shape).items():
        d_bad, n_bad = depth.copy(), normal.copy()
        out_idx = np.argwhere(~m)
        d_bad[~m] = np.where(np.arange(len(out_idx)) % 3 == 0, np.inf, np.where(np.arange(len(out_idx)) % 3 == 1, np.nan, -1.0))
        n_bad[~m] = np.nan
        mt = torch.from_numpy(m).cuda()
        for it in (0, 1, 10):
            ref = RR.refine(depth, normal, K, iterations=it, kernel_size=k, mask=m)
            for dd, nn in ((depth, normal), (d_bad, n_bad)):
                got = R.refine_depth_with_normal(*cuda(dd, nn, K), iterations=it, kernel_size=k, mask=mt)
                check(f"mask k={k}", got, ref, ulp16(depth), f"{what} it={it}", where=m)
                assert np.array_equal(got.cpu().numpy().view(np.int32)[~m], dd.view(np.int32)[~m]), f"{what}: masked-out pixels are the input's bits"


# ------------------------------------------------------------------------------------------------------------------ interface
def test_interface(R):
    depth, normal, K = scene(20, 26, 17, (2,))
    d, n, kk = cuda(depth, normal, K)
    depth[0, 2, 3] = 0.0
    d = torch.from_numpy(depth).cuda()
    before = d.clone()
    want = R.refine_depth_with_normal(d, n, kk)
    assert torch.equal(d, before), "the caller's depth is not clamped in place"
    n_chw = n.permute(0, 3, 1, 2).contiguous()                                   # (..., 3, H, W) storage viewed as (..., H, W, 3)
    view = n_chw.permute(0, 2, 3, 1)
    assert not view.is_contiguous()
    assert torch.equal(R.refine_depth_with_normal(d, view, kk), want)
    assert torch.equal(R.refine_depth_with_normal(d.transpose(-1, -2).contiguous().transpose(-1, -2), n, kk), want)
    half = R.refine_depth_with_normal(d.half(), n, kk)
    assert half.dtype == torch.float16 and half.shape == d.shape
    assert torch.equal(half, R.refine_depth_with_normal(d.half().float(), n, kk).half())
    with pytest.raises(RuntimeError):
        R.refine_depth_with_normal(d.cpu(), n.cpu(), kk.cpu())
    with pytest.raises(RuntimeError):
        R.refine_depth_with_normal(d, n, kk.cpu())
    for k in (4, 9):
        with pytest.raises(ValueError):
            R.refine_depth_with_normal(d, n, kk, kernel_size=k)
    with pytest.raises(ValueError):
        R.refine_depth_with_normal(d[:, :4], n[:, :4], kk, kernel_size=5)
    with pytest.raises(ValueError):
        R.refine_depth_with_normal(d[:, :, :6], n[:, :, :6], kk, kernel_size=7)


def test_c_call_rejects_bad_arguments(R):
    from moge_amd import _lib as L
    depth, normal, K = scene(20, 26, 18, (1,))
    d, n, kk = cuda(depth, normal, K)
    nbytes = C.c_int64(-1)
    assert L.lib.moge_refine_depth_workspace(1, 20, 26, C.byref(nbytes)) == 0 and nbytes.value == 4 * 20 * 26 * 4
    assert L.lib.moge_refine_depth_workspace(1, 20, 26, None) != 0
    assert L.lib.moge_refine_depth_workspace(-1, 20, 26, C.byref(nbytes)) != 0
    ws = torch.empty(nbytes.value if nbytes.value > 0 else 4 * 20 * 26 * 4, dtype=torch.uint8, device="cuda")
    out = torch.full_like(d, -7.0)
    p = lambda t: C.c_void_p(t.data_ptr())                                       # noqa: E731
    st = L.stream_ptr()

    def call(depth=p(d), normal=p(n), intr=p(kk), H=20, W=26, k=5, it=2, ws_=p(ws), out_=p(out)):
        return L.lib.moge_refine_depth(depth, normal, intr, None, 1, H, W, k, it, 1e-3, 1e-12, ws_, out_, st)

    for bad in (dict(k=4), dict(k=9), dict(k=1), dict(H=4), dict(W=4), dict(H=6, k=7), dict(it=-1), dict(depth=None), dict(normal=None), dict(intr=None),
                dict(ws_=None), dict(out_=None)):
        assert call(**bad) != 0, bad
        assert L.lib.moge_last_error()
    torch.cuda.synchronize()
    assert bool((out == -7.0).all()), "a rejected call launches nothing"
    assert call() == 0
    torch.cuda.synchronize()
    assert torch.equal(out, R.refine_depth_with_normal(d, n, kk, iterations=2))


# ------------------------------------------------------------------------------------------------------------------ model
def test_model_refine_depth(R, tmp_path):
    import copy
    from moge_amd.model import import_model_class_by_version
    from oracle import moge_oracle as O
    M = import_model_class_by_version("v2")
    cfg = O.named_configs()["tiny-vits-normal"]
    path = str(tmp_path / "model.pt")
    O.save_checkpoint(path, cfg, O.synth_state_dict(cfg, 0, True))
    model = M.from_pretrained(path).to("cuda").eval()
    img = torch.rand(2, 3, 84, 112, generator=torch.Generator().manual_seed(0)).cuda()
    for image in (img, img[0]):
        out = model.infer(image, num_tokens=108)
        new = model.refine_depth(out, iterations=3)
        mask = out["mask"]
        assert mask.any()
        direct = R.refine_depth_with_normal(out["depth"], out["normal"], out["intrinsics"], iterations=3, mask=mask)
        assert torch.equal(new["depth"].view(torch.int32), direct.view(torch.int32))
        assert set(new) == set(out) and new["normal"] is out["normal"] and new["depth"] is not out["depth"]
        assert torch.equal(new["depth"][~mask].view(torch.int32), out["depth"][~mask].view(torch.int32))
        assert torch.equal(new["points"][~mask].view(torch.int32), out["points"][~mask].view(torch.int32))
        assert not torch.equal(new["depth"][mask], out["depth"][mask])
        z, want = new["points"][..., 2][mask].double(), new["depth"][mask].double()
        assert ((z - want).abs() <= 4 * 2.0 ** -24 * want.abs()).all()             # z * (new / old): two roundings on top of z == old depth
        ratio = (new["depth"] / out["depth"])[mask]
        assert torch.allclose(new["points"][mask][:, 0], out["points"][mask][:, 0] * ratio, rtol=1e-6, atol=0)
    with pytest.raises(ValueError):
        model.refine_depth({k: v for k, v in out.items() if k != "normal"})
    zero = {k: v.clone() for k, v in out.items()}                                  # a masked-in depth of 0 has no ratio: its point stays as it is
    at = tuple(t[0] for t in torch.where(mask))
    zero["depth"][at] = 0.0
    new = model.refine_depth(zero, iterations=3)
    assert torch.isfinite(new["points"][mask]).all() and torch.equal(new["points"][at], zero["points"][at])
    cfg2 = copy.deepcopy(cfg)
    cfg2.pop("normal_head")
    path2 = str(tmp_path / "model_no_normal.pt")
    O.save_checkpoint(path2, cfg2, O.synth_state_dict(cfg2, 0, True))
    plain = M.from_pretrained(path2).to("cuda").eval()
    out2 = plain.infer(img, num_tokens=108)
    assert "normal" not in out2
    with pytest.raises(ValueError):
        plain.refine_depth(out2)
    model._release(); plain._release()
