"""moge_amd.panorama_gpu (csrc/panorama.hip) against the host module moge_amd/panorama.py, stage by stage, and against the reference's own
outputs (tests/golden/panorama_ref.npz).  Inputs are the seeded `make_panorama_golden.merge_inputs` / `split_input` (importing that module does not
touch the reference).  Shapes: panorama 72 x 36 with 24-pixel views (one level, width no multiple of 64), 264 x 132 with 40-pixel views (just
over 256: the coarse-to-fine start and the resize run), and the golden cases m128 / m256 / m512.

Bounds, each from the arithmetic it covers and none from what the kernels give:
  split      1 LSB on uint8 (what the host path itself is held to, tests/test_panorama_reference.py), 0.255 absolute on the float32 image
  system     row masks and `seen` equal; bx, by within 16 fp32 ulps of max |log distance| of the case, bl within 32: a warped log value carries at
             most 3 ulps (one for the log, two for the blend), a difference 2 * 3 + 1, the Laplacian (1 + 1 + 1 + 1 + 4) * 3 plus its own additions,
             and the masked mean is a convex combination
  operator   per element 11 * 2^-53 * (|A| |v|): at most 11 terms, each rounded once; the adjoint identity <A v, u> = <v, A^T u> to
             24 * 2^-53 * |u|^T |A| |v| (both products at 11, and one rounding per term of each exactly summed dot product)
  solver     fixed iteration count K = 10, 40 (atol = btol = conlim = 0), on the HOST's right-hand side so that only the solver differs:
             max |dx| <= 1e-12 against scipy, itn == K, istop == 7.  scipy's own result moves by 1e-16 ... 7e-16 when only the order of its sums
             changes and one iteration moves x by 7.5e-3 ... 2e-2: 1e-12 passes any correct summation order and fails any wrong sign, weight, scalar
             or off-by-one
  converged  against the reference's golden maps: masks equal, max |d log distance| < 5e-5, the LOG_TOL every implementation of this function is held
             to here.  No tighter gate against scipy's converged answer: that answer itself moves by 1.5e-7 ... 2.6e-5 under a reordering of its
             sums.  GPU-vs-host max |d log| and both iteration counts are printed, ungated (host values for the single-level cases only: the
             host's m512 merge alone takes longer than this whole module)
Exact properties (run = rerun, any polling interval, masked-out views, edge cases) are checked bit for bit or against the host's behaviour.
`pytest -s` prints worst value / bound per group at module teardown.

Worst value / bound per group, measured on an MI355X (22 passed, 5.0 s for the module):
  split u8 vs host 0 LSB, vs reference 1 LSB (the host's own distance)   split f32 vs host 0, vs reference 0.003
  system bx 0.06   by 0.13   bl 0.25   operator A v 0.33   A^T u 0.33   adjoint 0.005   lsmr K=10 0.01   K=40 0.0005
  converged vs reference 0.24   vs host (72 x 36, 264 x 132) 0.05   edge cases vs host 0.03   pipeline 0.005   cli depth.exr 0.005
  iteration counts equal to scipy's on every system: 527 (m128), 822 (m256), 347 (72 x 36), 315 (264 x 132 from the resized coarse solution)"""
import ctypes as C
import math
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(ROOT, "tests", "golden", "panorama_ref.npz")
LOG_TOL = 5e-5
SMALL = [("p72", 72, 36, 24), ("p264", 264, 132, 40)]
WORST = {}
REPORT = []


def note(group, value, bound):
    r = float(value) / bound
    w = WORST.get(group, (0.0, 0))
    WORST[group] = (max(w[0], r), w[1] + 1)
    print(f"[pano] {group}: {float(value):.3e} / {bound:.3e}")


@pytest.fixture(scope="module")
def G():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    import moge_amd.panorama_gpu as gpu
    yield gpu
    print("\nworst value / bound per group:")
    for k in sorted(WORST):
        print(f"  {k:28s} {WORST[k][0]:8.4f}   ({WORST[k][1]} cases)")
    print("converged solves (ungated): case, GPU itn per level, host itn, max |log GPU - log host|")
    for line in REPORT:
        print("  " + line)


@pytest.fixture(scope="module")
def P():
    from moge_amd import panorama
    return panorama


@pytest.fixture(scope="module")
def MG():
    import make_panorama_golden
    return make_panorama_golden


def cuda_views(dist, masks):
    return torch.from_numpy(np.stack(dist)).cuda(), torch.from_numpy(np.stack(masks)).cuda()


def layout(P, width, height, bx, by, bl, rx, ry, rl):
    """The host's planes in the kernels' row order -> (b (M,) float64, rows (M,) bool)"""
    by2, ry2 = by.reshape(height - 1, width), ry.reshape(height - 1, width)
    b = np.concatenate([bx.reshape(-1), by2.reshape(-1), by2[:, 0], bl.reshape(-1)]).astype(np.float64)
    rows = np.concatenate([rx, ry, ry2[:, 0], rl])
    return np.where(rows, b, 0.0), rows


def full_operator(P, width, height, rows):
    import scipy.sparse as sp
    Dx, Dy, Lap = P._difference_operators(width, height)
    col0 = np.arange(height - 1) * width
    A = sp.vstack([Dx, Dy, Dy[col0], Lap], format="csr").astype(np.float64)
    return sp.diags(rows.astype(np.float64)) @ A


@pytest.fixture(scope="module")
def host(P, MG):
    """Per small case, computed once: inputs, the host's system of the fine level (and of the coarse one), scipy's solves."""
    from scipy.sparse.linalg import lsmr
    out = {}
    for name, w, h, res in SMALL:
        E, Ks, dist, masks = MG.merge_inputs(P, res, seed=w)
        c = {"w": w, "h": h, "E": E, "Ks": Ks, "dist": dist, "masks": masks, "logmax": float(np.abs(np.log(np.stack(dist))).max()), "x0": None, "coarse": None}
        if max(w, h) > 256:
            c["coarse"] = P.merge_system(w // 2, h // 2, dist, masks, E, Ks)
            xc = lsmr(c["coarse"][7], c["coarse"][8], atol=1e-5, btol=1e-5)[0]
            c["x0"] = np.log(P._resize_bilinear(np.exp(xc).reshape(h // 2, w // 2).astype(np.float32), h, w)).reshape(-1).astype(np.float64)
        c["sys"] = P.merge_system(w, h, dist, masks, E, Ks)
        sol = lsmr(c["sys"][7], c["sys"][8], atol=1e-5, btol=1e-5, x0=c["x0"])
        c["x"], c["itn"] = sol[0], sol[2]
        out[name] = c
    return out


# ---------------------------------------------------------------------------------------------------------------------------------------
# 1. split
# ---------------------------------------------------------------------------------------------------------------------------------------
def test_split_matches_the_host_and_the_reference(G, P, MG):
    E, Ks = P.get_panorama_cameras()
    gold = np.load(GOLDEN)
    rng = np.random.default_rng(5)
    small = (rng.random((37, 75, 3)) * 255).astype(np.uint8)
    img = MG.split_input(P)
    for tag, image, res in (("37x75", small, 24), ("split_input", img, 64)):
        got = G.split_panorama_image(torch.from_numpy(image).cuda(), E, Ks, res)
        assert got.shape == (12, res, res, 3) and got.dtype == torch.uint8
        want = np.stack(P.split_panorama_image(image, E, Ks, res))
        d = np.abs(got.cpu().numpy().astype(np.int32) - want.astype(np.int32)).max()
        note("split u8 vs host (LSB)", d, 1.0)
        assert d <= 1, tag
    d = np.abs(got.cpu().numpy().astype(np.int32) - gold["split_u8"].astype(np.int32)).max()
    note("split u8 vs reference (LSB)", d, 1.0)
    assert d <= 1
    gotf = G.split_panorama_image(torch.from_numpy(img.astype(np.float32)).cuda(), E[:3], Ks[:3], 32)
    assert gotf.shape == (3, 32, 32, 3) and gotf.dtype == torch.float32
    wantf = np.stack(P.split_panorama_image(img.astype(np.float32), E[:3], Ks[:3], 32))
    for tag, ref in (("host", wantf), ("reference", gold["split_f32"])):
        d = np.abs(gotf.cpu().numpy() - ref).max()
        note(f"split f32 vs {tag}", d, 0.255)
        assert d <= 0.255, tag
    # a strided view of a larger tensor is accepted (made contiguous), and a single camera
    big = torch.zeros((37, 80, 3), dtype=torch.uint8, device="cuda")
    big[:, :75] = torch.from_numpy(small).cuda()
    one = G.split_panorama_image(big[:, :75], E[4:5], Ks[4:5], 24)
    assert torch.equal(one[0], G.split_panorama_image(torch.from_numpy(small).cuda(), E, Ks, 24)[4])


# ---------------------------------------------------------------------------------------------------------------------------------------
# 2. system assembly
# ---------------------------------------------------------------------------------------------------------------------------------------
def check_system(G, tag, s, hs, logmax):
    bx, by, bl, rx, ry, rl, seen = hs[:7]
    ulp = float(np.spacing(np.float32(logmax)))
    assert np.array_equal(s.rx.cpu().numpy(), rx) and np.array_equal(s.ry.cpu().numpy(), ry) and np.array_equal(s.rl.cpu().numpy(), rl), tag
    assert np.array_equal(s.seen.cpu().numpy(), seen), tag
    H, W = seen.shape
    col0 = s.rows[W * H + (H - 1) * W: W * H + (H - 1) * W + (H - 1)].bool().cpu().numpy()
    assert np.array_equal(col0, ry.reshape(H - 1, W)[:, 0]), tag
    extra = s.b[W * H + (H - 1) * W: W * H + (H - 1) * W + (H - 1)]
    assert torch.equal(extra, s.by[:, 0]), tag                              # the duplicated column-0 equations carry the same bits
    for nm, got, want, k in (("bx", s.bx, bx, 16), ("by", s.by, by, 16), ("bl", s.bl, bl, 32)):
        d = np.abs(got.cpu().numpy() - want).max()
        note(f"system {nm}", d, k * ulp)
        assert d <= k * ulp, (tag, nm)


def test_system_matches_the_host_merge_system(G, host):
    for name, c in host.items():
        dist, masks = cuda_views(c["dist"], c["masks"])
        check_system(G, name, G.merge_system(c["w"], c["h"], dist, masks, c["E"], c["Ks"]), c["sys"], c["logmax"])
        if c["coarse"] is not None:
            check_system(G, name + " coarse", G.merge_system(c["w"] // 2, c["h"] // 2, dist, masks, c["E"], c["Ks"]), c["coarse"], c["logmax"])
    # lists of maps are accepted like the stacked tensors
    c = host["p72"]
    a = G.merge_system(72, 36, [torch.from_numpy(d).cuda() for d in c["dist"]], [torch.from_numpy(m).cuda() for m in c["masks"]], c["E"], c["Ks"])
    b = G.merge_system(72, 36, *cuda_views(c["dist"], c["masks"]), c["E"], c["Ks"])
    assert torch.equal(a.b, b.b) and torch.equal(a.rows, b.rows) and torch.equal(a.seen, b.seen)


# ---------------------------------------------------------------------------------------------------------------------------------------
# 3. operator
# ---------------------------------------------------------------------------------------------------------------------------------------
def apply(width, height, rows, vec, transpose):
    from moge_amd import _lib as L
    import moge_amd.panorama_gpu as gpu
    M, N = gpu.system_rows(width, height), width * height
    out = torch.full((N if transpose else M,), float("nan"), dtype=torch.float64, device="cuda")
    assert vec.numel() == (M if transpose else N)
    L.check(L.lib.moge_test_pano_apply(width, height, rows.data_ptr(), int(transpose), vec.data_ptr(), out.data_ptr(), L.stream_ptr(out.device)))
    return out


@pytest.mark.parametrize("name", ["p72", "p264", "w2", "h2"])
def test_operator_and_its_adjoint_match_the_host_sparse_matrix(G, P, host, name):
    rng = np.random.default_rng(17)
    if name in host:
        c = host[name]
        w, h = c["w"], c["h"]
        _, rows = layout(P, w, h, *c["sys"][:6])
    else:
        w, h = (2, 5) if name == "w2" else (70, 2)
        rows = rng.random(G.system_rows(w, h)) > 0.3
    A = full_operator(P, w, h, rows)
    absA = abs(A)
    v, u = rng.normal(size=w * h), rng.normal(size=A.shape[0])
    rows_t = torch.from_numpy(rows.astype(np.uint8)).cuda()
    Av = apply(w, h, rows_t, torch.from_numpy(v).cuda(), False).cpu().numpy()
    Atu = apply(w, h, rows_t, torch.from_numpy(u).cuda(), True).cpu().numpy()
    eps = 11 * 2.0 ** -53
    for tag, got, want, bound in (("A v", Av, A @ v, eps * (absA @ np.abs(v))), ("A^T u", Atu, A.T @ u, eps * (absA.T @ np.abs(u)))):
        assert np.isfinite(got).all() and got.shape == want.shape, tag
        assert np.array_equal(got[bound == 0], want[bound == 0]), tag                 # zero rows / untouched pixels are exactly zero
        nz = bound > 0
        r = (np.abs(got - want)[nz] / bound[nz]).max()
        note("operator " + tag, r, 1.0)
        assert r <= 1.0, (name, tag)
    scale = 24 * 2.0 ** -53 * float(np.abs(u) @ (absA @ np.abs(v)))
    d = abs(math.fsum(Av * u) - math.fsum(v * Atu))
    note("operator adjoint", d, scale)
    assert d <= scale, name


# ---------------------------------------------------------------------------------------------------------------------------------------
# 4. recurrences at a fixed iteration count
# ---------------------------------------------------------------------------------------------------------------------------------------
def device_system(G, P, c):
    b, rows = layout(P, c["w"], c["h"], *c["sys"][:6])
    assert np.array_equal(b[rows], c["sys"][8])                                       # the host's right-hand side, bit for bit
    return G.PanoSystem(c["w"], c["h"], torch.from_numpy(b).cuda(), torch.from_numpy(rows.astype(np.uint8)).cuda(), torch.from_numpy(c["sys"][6]).cuda())


@pytest.mark.parametrize("K", [10, 40])
@pytest.mark.parametrize("name,start", [("p72", False), ("p264", False), ("p264", True)])
def test_lsmr_recurrences_match_scipy_at_a_fixed_iteration_count(G, P, host, name, start, K):
    from scipy.sparse.linalg import lsmr
    c = host[name]
    x0 = c["x0"] if start else None
    assert not start or x0 is not None
    want = lsmr(c["sys"][7], c["sys"][8], atol=0, btol=0, conlim=0, maxiter=K, x0=x0)
    got = G.lsmr(device_system(G, P, c), x0=torch.from_numpy(x0).cuda() if start else None, atol=0, btol=0, conlim=0, maxiter=K)
    d = np.abs(got[0].cpu().numpy() - want[0]).max()
    note(f"lsmr K={K} max |dx|", d, 1e-12)
    print(f"[pano] {name} start={start} K={K}: normr {got[3]:.15e} / {want[3]:.15e}  normA {got[5]:.15e} / {want[5]:.15e}  normx {got[7]:.15e} / {want[7]:.15e}")
    assert got[2] == K == want[2] and got[1] == 7 == want[1]
    assert d <= 1e-12
    for i in (3, 4, 5, 6, 7):                                                         # normr, normar, normA, condA, normx: scipy's estimates
        assert abs(got[i] - want[i]) <= 1e-9 * max(abs(want[i]), 1e-300), i


# ---------------------------------------------------------------------------------------------------------------------------------------
# 5. converged solve against the reference
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,width,height,res", [("m128", 128, 64, 48), ("m256", 256, 128, 64), ("m512", 512, 256, 96)])
def test_converged_merge_matches_the_reference_golden(G, P, MG, name, width, height, res):
    from scipy.sparse.linalg import lsmr
    assert (name, width, height, res) in MG.MERGE_CASES
    gold = np.load(GOLDEN)
    E, Ks, dist, masks = MG.merge_inputs(P, res, seed=width)
    itns = []
    got, seen = G.merge_panorama_depth(width, height, *cuda_views(dist, masks), E, Ks, iterations=itns)
    assert got.shape == (height, width) and got.dtype == torch.float32 and seen.shape == (height, width) and seen.dtype == torch.bool
    assert len(itns) == (2 if width > 256 else 1)
    assert np.array_equal(seen.cpu().numpy(), gold[name + "_mask"])
    lg = np.log(got.cpu().numpy().astype(np.float64))
    d = np.abs(lg - np.log(gold[name + "_depth"].astype(np.float64))).max()
    note("converged vs reference", d, LOG_TOL)
    line = f"{name}: GPU itn {itns}"
    if width <= 256:                                                                  # one level: the host's solve is a second or two
        *_, A, b = P.merge_system(width, height, dist, masks, E, Ks)
        sol = lsmr(A, b, atol=1e-5, btol=1e-5)
        line += f", host itn {sol[2]}, max |d log| {np.abs(lg.reshape(-1) - sol[0]).max():.2e}"
    REPORT.append(line)
    assert d < LOG_TOL


def test_converged_small_cases_report(G, P, host):
    """72 x 36 and 264 x 132 against the reference contract through the host (which sits 1.2e-5 or closer to the reference): printed, and held to
    the same LOG_TOL against the host's own converged answer."""
    for name, c in host.items():
        itns = []
        got, seen = G.merge_panorama_depth(c["w"], c["h"], *cuda_views(c["dist"], c["masks"]), c["E"], c["Ks"], iterations=itns)
        assert np.array_equal(seen.cpu().numpy(), c["sys"][6])
        d = np.abs(np.log(got.cpu().numpy().astype(np.float64)).reshape(-1) - c["x"]).max()
        REPORT.append(f"{name}: GPU itn {itns}, host itn (fine level) {c['itn']}, max |d log| {d:.2e}")
        note("converged vs host (small)", d, LOG_TOL)
        assert d < LOG_TOL, name


# ---------------------------------------------------------------------------------------------------------------------------------------
# 6. exact properties
# ---------------------------------------------------------------------------------------------------------------------------------------
def test_two_runs_and_any_polling_interval_give_the_same_bits(G, P, host):
    for name, c in host.items():
        s = device_system(G, P, c)
        x0 = torch.from_numpy(c["x0"]).cuda() if c["x0"] is not None else None
        a = G.lsmr(s, x0=x0)
        b = G.lsmr(s, x0=x0)
        assert torch.equal(a[0], b[0]) and a[1:] == b[1:], name
        assert a[1] in (1, 2) and 0 < a[2] < min(int(s.rows.sum()), c["w"] * c["h"])
        for poll in (1, 64):
            p = G.lsmr(s, x0=x0, poll=poll)
            assert torch.equal(a[0], p[0]) and a[1:] == p[1:], (name, poll)
        dist, masks = cuda_views(c["dist"], c["masks"])
        m1 = G.merge_panorama_depth(c["w"], c["h"], dist, masks, c["E"], c["Ks"])
        m2 = G.merge_panorama_depth(c["w"], c["h"], dist, masks, c["E"], c["Ks"], poll=1)
        assert torch.equal(m1[0], m2[0]) and torch.equal(m1[1], m2[1]), name


def test_fully_masked_views_contribute_nothing(G, host):
    c = host["p72"]
    assert not c["masks"][9].any()
    dist, masks = cuda_views(c["dist"], c["masks"])
    poisoned = dist.clone()
    poisoned[9] = float("nan")
    a, b = G.merge_system(72, 36, dist, masks, c["E"], c["Ks"]), G.merge_system(72, 36, poisoned, masks, c["E"], c["Ks"])
    assert torch.equal(a.b, b.b) and torch.equal(a.rows, b.rows) and torch.equal(a.seen, b.seen)
    m1, m2 = G.merge_panorama_depth(72, 36, dist, masks, c["E"], c["Ks"]), G.merge_panorama_depth(72, 36, poisoned, masks, c["E"], c["Ks"])
    assert torch.equal(m1[0], m2[0]) and torch.equal(m1[1], m2[1]) and bool(torch.isfinite(m1[0]).all())


def test_edge_cases_behave_as_the_host_does(G, P, host):
    c = host["p72"]
    E, Ks = c["E"], c["Ks"]
    dist, masks = cuda_views(c["dist"], c["masks"])
    # all 12 masks false: the host returns distance 1 everywhere and an empty mask (no equations, x = 0)
    none = torch.zeros_like(masks)
    hd, hm = P.merge_panorama_depth(72, 36, c["dist"], [np.zeros_like(m) for m in c["masks"]], E, Ks)
    assert (hd == 1).all() and not hm.any()
    gd, gm = G.merge_panorama_depth(72, 36, dist, none, E, Ks)
    assert bool((gd == 1).all()) and not bool(gm.any())
    s = G.merge_system(72, 36, dist, none, E, Ks)
    assert not bool(s.rows.any()) and not bool(s.b.any())
    x, istop, itn, *_ = G.lsmr(s)
    assert istop == 0 and itn == 0 and not bool(x.any())
    # ... and above 256 pixels, where the coarse level is empty too
    gd, gm = G.merge_panorama_depth(264, 132, dist, none, E, Ks)
    assert bool((gd == 1).all()) and not bool(gm.any())
    # a single view, height 2, a width off the workgroup's span, width 2: the host's system, scipy's iterates at a fixed count, the converged map.
    # Width 2 (72 unknowns) is not a converged comparison: scipy itself runs into maxiter there (istop 7) and its answer moves by
    # 2.7e-5 ... 8e-4 when only the rows of A are permuted (six permutations, measured with scipy alone) - so that map is printed, not gated,
    # and the fixed-count iterates carry the check.
    from scipy.sparse.linalg import lsmr
    for tag, w, h, sl, converges in (("single view", 72, 36, slice(0, 1), True), ("height 2", 72, 2, slice(None), True), ("70 x 35", 70, 35, slice(None), True),
                                     ("width 2", 2, 36, slice(None), False)):
        hv = (c["dist"][sl], c["masks"][sl], E[sl], Ks[sl])
        gv = (dist[sl], masks[sl], E[sl], Ks[sl])
        hs = P.merge_system(w, h, *hv)
        check_system(G, tag, G.merge_system(w, h, *gv), hs, c["logmax"])
        want = lsmr(hs[7], hs[8], atol=0, btol=0, conlim=0, maxiter=10)
        got = G.lsmr(device_system(G, P, {"w": w, "h": h, "sys": hs}), atol=0, btol=0, conlim=0, maxiter=10)
        d = np.abs(got[0].cpu().numpy() - want[0]).max()
        note("lsmr K=10 max |dx|", d, 1e-12)
        assert d <= 1e-12 and got[1:3] == (7, 10), tag
        hd, hm = P.merge_panorama_depth(w, h, *hv)
        gd, gm = G.merge_panorama_depth(w, h, *gv)
        assert np.array_equal(gm.cpu().numpy(), hm), tag
        d = np.abs(np.log(gd.cpu().numpy().astype(np.float64)) - np.log(hd.astype(np.float64))).max()
        if converges:
            note("edge cases vs host", d, LOG_TOL)
            assert d < LOG_TOL, tag
        else:
            REPORT.append(f"{tag} ({w} x {h}): max |d log| {d:.2e} against a host solve that stops at maxiter")
    # what is refused
    for w, h in ((1, 36), (72, 1), (0, 36), (72, 0)):
        with pytest.raises(ValueError):
            G.merge_panorama_depth(w, h, dist, masks, E, Ks)
        with pytest.raises(ValueError):
            G.merge_system(w, h, dist, masks, E, Ks)
    with pytest.raises(ValueError):
        G.merge_panorama_depth(72, 36, dist[:0], masks[:0], E[:0], Ks[:0])
    with pytest.raises(ValueError):
        G.merge_panorama_depth(72, 36, dist, masks[:, :, :5], E, Ks)
    with pytest.raises(ValueError):
        G.merge_panorama_depth(72, 36, dist, masks, E[:5], Ks[:5])
    with pytest.raises(ValueError):
        G.merge_panorama_depth(72, 36, dist.double(), masks, E, Ks)
    with pytest.raises(ValueError):
        G.split_panorama_image(torch.zeros(8, 16, 4, dtype=torch.uint8, device="cuda"), E, Ks, 8)
    with pytest.raises(RuntimeError, match="GPU tensors only"):
        G.merge_panorama_depth(72, 36, dist.cpu(), masks.cpu(), E, Ks)


def test_resizes_match_the_host(G, P):
    rng = np.random.default_rng(2)
    src = rng.random((36, 72)).astype(np.float32) + 0.5
    msk = rng.random((36, 72)) > 0.5
    for oh, ow in ((72, 144), (50, 131), (36, 72), (20, 33)):
        got = G._resize_bilinear(torch.from_numpy(src).cuda(), oh, ow).cpu().numpy()
        want = P._resize_bilinear(src, oh, ow)
        d = np.abs(got - want).max()
        note("resize bilinear (ulps of 1.5)", d / float(np.spacing(np.float32(1.5))), 2.0)        # the same fp32 expression: at most the weights' last bit
        assert d <= 2 * float(np.spacing(np.float32(1.5)))
        gm = G._resize_nearest(torch.from_numpy(msk).cuda(), oh, ow).cpu().numpy()
        assert np.array_equal(gm, P._resize_nearest(msk.astype(np.uint8), oh, ow) > 0)


# ---------------------------------------------------------------------------------------------------------------------------------------
# 7. pipeline
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def v1_checkpoint(tmp_path_factory):
    from oracle import moge_oracle_v1 as O1
    cfg = O1.named_configs()["tiny-v1-vits"]
    path = str(tmp_path_factory.mktemp("pano_ckpt") / "v1.pt")
    O1.save_checkpoint(path, cfg, O1.synth_state_dict(cfg, 0, True))
    return path


def test_infer_panorama_on_the_device_matches_the_host_pipeline(G, P, v1_checkpoint):
    from moge_amd.model import import_model_class_by_version
    model = import_model_class_by_version("v1").from_pretrained(v1_checkpoint).to("cuda").eval()
    yy, xx = np.meshgrid(np.linspace(0, 1, 64), np.linspace(0, 1, 128), indexing="ij")
    image = (np.stack([xx, yy, 0.5 + 0.5 * np.sin(6 * xx)], -1) * 255).astype(np.uint8)
    out = G.infer_panorama(model, torch.from_numpy(image).cuda(), resolution=64, merge_size=(128, 64), num_tokens=64)
    assert set(out) == {"distance", "mask", "points", "views", "view_distance", "view_mask"} and all(v.is_cuda for v in out.values())
    for k, shape, dtype in (("distance", (64, 128), torch.float32), ("mask", (64, 128), torch.bool), ("points", (64, 128, 3), torch.float32),
                            ("views", (12, 64, 64, 3), torch.uint8), ("view_distance", (12, 64, 64), torch.float32), ("view_mask", (12, 64, 64), torch.bool)):
        assert out[k].shape == shape and out[k].dtype == dtype, k
    E, Ks = P.get_panorama_cameras()
    views = out["views"].cpu().numpy()
    vd, vm = P.infer_panorama_views(model, list(views), Ks, batch_size=4, num_tokens=64)          # infer(view / 255), the host caller's form
    assert np.array_equal(np.stack(vd), out["view_distance"].cpu().numpy()) and np.array_equal(np.stack(vm), out["view_mask"].cpu().numpy())
    # (why the pipeline does not use infer_uint8: with float32 weights and use_fp16=True it stages the bytes in fp16 - printed, not gated)
    fov = torch.tensor(P.intrinsics_to_fov_x_deg(np.array(Ks[:4])), device="cuda")
    u8 = model.infer_uint8(out["views"][:4], fov_x=fov, apply_mask=False, num_tokens=64)["points"].norm(dim=-1)
    REPORT.append(f"infer_uint8 against infer(view / 255), autocast form: max relative difference {float(((u8 - out['view_distance'][:4]).abs() / out['view_distance'][:4]).max()):.2e}")
    hd, hm = P.merge_panorama_depth(128, 64, vd, vm, E, Ks)
    assert np.array_equal(out["mask"].cpu().numpy(), hm)
    got = out["distance"].cpu().numpy()
    d = np.abs(np.log(got.astype(np.float64)) - np.log(hd.astype(np.float64))).max()
    note("pipeline merged vs host", d, LOG_TOL)
    assert d < LOG_TOL
    want_points = got[:, :, None] * P.spherical_uv_to_directions(P._uv_grid(64, 128)).astype(np.float32)
    assert np.allclose(out["points"].cpu().numpy(), want_points, rtol=1e-6, atol=1e-7 * float(got.max()))


def test_cli_gpu_merge_writes_the_same_files(G, tmp_path, v1_checkpoint):
    from PIL import Image
    from click.testing import CliRunner
    from moge_amd import io as IO
    from moge_amd.scripts.infer_panorama import main as cli
    yy, xx = np.meshgrid(np.linspace(0, 1, 96), np.linspace(0, 1, 192), indexing="ij")
    src = tmp_path / "in"
    src.mkdir()
    Image.fromarray((np.stack([xx, yy, 0.5 + 0.5 * np.sin(6 * xx)], -1) * 255).astype(np.uint8)).save(src / "p.png")
    outs = {}
    for key, extra in (("host", []), ("gpu", ["--gpu_merge"])):
        outs[key] = tmp_path / key
        args = ["-i", str(src), "-o", str(outs[key]), "--pretrained", v1_checkpoint, "--version", "v1", "--maps", "--glb", "--ply", "--threshold", "1e9"] + extra
        r = CliRunner().invoke(cli, args, catch_exceptions=False)
        assert r.exit_code == 0, r.output
    files = {k: sorted(str(p.relative_to(outs[k])) for p in outs[k].rglob("*") if p.is_file()) for k in outs}
    assert files["host"] == files["gpu"] and {"p/depth.exr", "p/points.exr", "p/mask.png", "p/mesh.glb", "p/mesh.ply", "p/image.jpg"} <= set(files["gpu"])
    mh, mg = (np.asarray(Image.open(outs[k] / "p" / "mask.png")) for k in ("host", "gpu"))
    assert np.array_equal(mh, mg)
    dh, dg = (IO.read_exr(outs[k] / "p" / "depth.exr").astype(np.float64) for k in ("host", "gpu"))
    keep = mh > 0
    d = np.abs(np.log(dh[keep]) - np.log(dg[keep])).max() if keep.any() else 0.0
    note("cli depth.exr vs host", d, LOG_TOL)
    assert d < LOG_TOL
