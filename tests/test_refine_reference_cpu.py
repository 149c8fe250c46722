"""tests/refine_reference.py (the float64 restatement the GPU tests of moge_amd.refine compare against) checked on the CPU: against the outputs of
the reference's unmodified refine_depth_with_normal (tests/golden/refine_*.npz, tools/make_refine_golden.py), on the fixed point the conventions
imply, and for the mask extension's two defining properties."""
import glob
import os

import numpy as np
import pytest

import refine_reference as RR

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FIXTURES = sorted(os.path.basename(p)[len("refine_"):-len(".npz")] for p in glob.glob(os.path.join(GOLDEN, "refine_*.npz")))


def load(name):
    z = np.load(os.path.join(GOLDEN, f"refine_{name}.npz"))
    return {k: z[k] for k in z.files}


def test_fixture_set():
    assert FIXTURES == ["bumpy_12x7", "bumpy_70x131", "plane_5x5", "step_37x53", "step_5x9"]


@pytest.mark.parametrize("name", FIXTURES)
def test_restatement_matches_reference(name):
    z = load(name)
    depth, normal, K = z["depth"], z["normal"].astype(np.float32), z["intrinsics"]
    assert depth.min() >= 0.3 and depth.max() <= 30 and depth.nbytes + normal.nbytes < 200 * 1024
    runs = [("out64", 5, 10)] + [(k, int(k.split("_")[1][1:]), int(k.split("_")[2][1:])) for k in z if k.startswith("out64_k")]
    for key, k, it in runs:
        got = RR.refine(depth, normal, K, iterations=it, kernel_size=k)
        err = np.abs(np.log(got) - np.log(z[key])).max()
        assert err <= 1e-12, (name, key, err)
    assert z["ref32_err"] == np.abs(np.log(z["out32"].astype(np.float64)) - np.log(z["out64"])).max()
    assert z["ref32_err"] < 1e-5


def clean_plane(H, W):
    K = np.array([[0.9, 0.02, 0.45], [0, 1.1, 0.56], [0, 0, 1]])
    n = np.array([0.1, -0.15, -0.98])
    n /= np.linalg.norm(n)
    v, u = np.meshgrid((np.arange(H) + 0.5) / H, (np.arange(W) + 0.5) / W, indexing="ij")
    ray = np.stack([u, v, np.ones_like(u)], -1) @ np.linalg.inv(K).T
    return -2.5 / (ray @ n), np.broadcast_to(n, (H, W, 3)).copy(), K


@pytest.mark.parametrize("k", [3, 5, 7])
def test_clean_plane_is_a_fixed_point(k):
    """The relaxation integrates g by the trapezoid rule, (g[p+t] + g[p]) . duv / 2, exact for a log-depth that is quadratic in uv.  The log-depth of
    a plane is -log(n . ray): the rule's third-order remainder grows with the cube of the tilt and the square of the window, so "fixed point" holds
    to 1e-6 for a moderate tilt (this plane, 11 degrees: 7e-9 / 5e-8 / 1.4e-7 after 100 iterations at k = 3 / 5 / 7), not for any plane (the 25-degree
    plane of the golden scenes: 5.8e-7 / 3.3e-6 / 8.5e-6).  A wrong sign or a swapped uv convention leaves a first-order term, 1e-2 and more."""
    depth, normal, K = clean_plane(40, 56)
    out = RR.refine(depth, normal, K, iterations=100, kernel_size=k)
    assert np.abs(np.log(out) - np.log(depth)).max() < 1e-6


def test_noise_shrinks():
    depth, normal, K = clean_plane(40, 56)
    noisy = depth * (1 + 0.01 * np.random.default_rng(0).standard_normal(depth.shape))
    out = RR.refine(noisy, normal, K, iterations=10)
    inner = (slice(8, -8), slice(8, -8))
    assert np.abs(np.log(out / depth))[inner].std() < 0.25 * np.abs(np.log(noisy / depth))[inner].std()


@pytest.mark.parametrize("name", FIXTURES)
def test_all_true_mask_is_the_unmasked_formula(name):
    z = load(name)
    a = RR.refine(z["depth"], z["normal"], z["intrinsics"], iterations=3)
    b = RR.refine(z["depth"], z["normal"], z["intrinsics"], iterations=3, mask=np.ones(z["depth"].shape, bool))
    assert np.array_equal(a, b)


@pytest.mark.parametrize("k", [3, 5, 7])
def test_values_under_the_mask_do_not_matter(k):
    z = load("step_37x53")
    depth, normal, K = z["depth"].astype(np.float64), z["normal"].astype(np.float64), z["intrinsics"]
    rng = np.random.default_rng(1)
    mask = rng.random(depth.shape) > 0.15
    mask[10:14, 20:31] = False
    mask[:, :2] = False
    d_bad, n_bad = depth.copy(), normal.copy()
    hole = np.argwhere(~mask)
    d_bad[~mask] = np.where(np.arange(len(hole)) % 2 == 0, np.inf, np.nan)
    n_bad[~mask] = np.nan
    d_any = np.where(mask, depth, 7.25)
    got = RR.refine(d_bad, n_bad, K, iterations=10, kernel_size=k, mask=mask)
    want = RR.refine(d_any, normal, K, iterations=10, kernel_size=k, mask=mask)
    assert np.isfinite(got[mask]).all()
    assert np.array_equal(got[mask], want[mask])
    assert np.array_equal(got[~mask], d_bad[~mask], equal_nan=True)
    unmasked = RR.refine(depth, normal, K, iterations=10, kernel_size=k)
    assert np.abs(np.log(got[mask]) - np.log(unmasked[mask])).max() > 1e-6        # the mask does change the masked-in result
