"""How the stateless ops are called (moge_amd._lib `device_of` / `on` / `ptr`): one call per module at the smallest valid shape.  For each op

  1. every stream it hands to the library is asked for with the device of its inputs, never the thread's current device (`stream_ptr(None)`);
  2. inside `torch.cuda.stream(side)` it runs on `side` and gives the bits of the default-stream run;
  3. with inputs on cuda:1 while cuda:0 is current it gives the cuda:0 bits (skipped on a box with one GPU).

The CPU half (the helpers on stand-in objects) is tests/test_lib_calls_cpu.py."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _mask(shape, g):
    m = torch.rand(shape, generator=g) > 0.25
    m.view(-1)[:2] = True
    return m


# ---- inputs: built on the host from a seed, so that every device gets the same values ------------------------------------------------------
def _in_align(g):
    return dict(x=torch.randn(3, 40, generator=g), y=torch.randn(3, 40, generator=g), w=torch.rand(3, 40, generator=g) + 0.1)


def _in_points(g):
    src = torch.randn(2, 12, 3, generator=g)
    return dict(src=src, tgt=0.8 * src + 0.1 + 0.05 * torch.randn(2, 12, 3, generator=g), w=torch.rand(2, 12, generator=g) + 0.1)


def _in_maps(g):
    gt = torch.rand(9, 11, generator=g) + 0.5
    return dict(pred=gt * (1 + 0.1 * torch.randn(9, 11, generator=g)), gt=gt, mask=_mask((9, 11), g),
                params=torch.tensor([[0.0, 1.1, 0.0, 0.0, 0.0, 0.0], [1.0, 0.9, 0.05, 0.0, 0.0, 0.0]]))       # (mode, s, t0, t1, t2, c): scale, affine


def _in_eval(g):
    return dict(image=torch.randint(0, 256, (9, 11, 3), generator=g, dtype=torch.uint8), seg=torch.randint(0, 5, (9, 11), generator=g, dtype=torch.uint8),
                depth=torch.rand(9, 11, generator=g) + 0.5, mask=_mask((9, 11), g))


def _in_refine(g):
    n = 0.1 * torch.randn(5, 5, 3, generator=g) + torch.tensor([0.0, 0.0, -1.0])
    return dict(depth=torch.rand(5, 5, generator=g) + 1.0, normal=n / n.norm(dim=-1, keepdim=True),
                K=torch.tensor([[1.0, 0.0, 0.5], [0.0, 1.0, 0.5], [0.0, 0.0, 1.0]]))


def _in_mesh(g):
    return dict(points=torch.randn(4, 5, 3, generator=g), mask=_mask((4, 5), g))


def _in_split(g):
    return dict(image=torch.randint(0, 256, (8, 16, 3), generator=g, dtype=torch.uint8))


def _in_merge(g):
    return dict(dist=torch.rand(2, 4, 4, generator=g) + 1.0, masks=torch.ones(2, 4, 4, dtype=torch.bool))


def _cameras(n=2):
    from moge_amd.panorama import get_panorama_cameras
    E, Ks = get_panorama_cameras()
    return E[:n], Ks[:n]


K_EVAL = np.array([[0.9, 0.0, 0.5], [0.0, 1.2, 0.5], [0.0, 0.0, 1.0]], np.float32)


# ---- the ops: name -> (inputs, call) -------------------------------------------------------------------------------------------------------
def _ops():
    from moge_amd import alignment as A, evaluation as E, mesh as MS, metrics as M, panorama_gpu as PG, refine as R

    def merge_and_solve(t):
        s = PG.merge_system(8, 4, t["dist"], t["masks"], *_cameras())
        return (s.b, s.rows, s.seen) + tuple(PG.lsmr(s, maxiter=3))

    return {
        "alignment.align": (_in_align, lambda t: A.align(t["x"], t["y"], t["w"])),
        "alignment.align_trunc": (_in_align, lambda t: A.align_trunc(t["x"], t["y"], t["w"], 0.1)),
        "alignment.align_points_scale_xyz_shift": (_in_points, lambda t: A.align_points_scale_xyz_shift(t["src"], t["tgt"], t["w"])),
        "metrics.boundary_counts": (_in_maps, lambda t: M.boundary_counts(t["pred"], t["gt"], t["mask"])),
        "metrics.masked_max": (_in_maps, lambda t: M.masked_max(t["gt"], t["mask"])),
        "metrics.error_pass": (_in_maps, lambda t: M.error_pass(t["pred"], t["gt"], t["mask"], t["params"])),
        "metrics.masked_nearest_resize": (_in_maps, lambda t: M.masked_nearest_resize(t["gt"], mask=t["mask"], size=(4, 4), return_index=True)),
        "evaluation.lanczos_resize": (_in_eval, lambda t: E.lanczos_resize(t["image"], 5, 6)),
        "evaluation.resize_nearest": (_in_eval, lambda t: E.resize_nearest(t["seg"], (5, 6))),
        "evaluation.masked_nearest_resize_distance": (_in_eval, lambda t: E.masked_nearest_resize_distance(t["depth"], t["mask"], (5, 6), K_EVAL)),
        "refine.refine_depth_with_normal": (_in_refine, lambda t: R.refine_depth_with_normal(t["depth"], t["normal"], t["K"], iterations=2, kernel_size=3)),
        "mesh.build_mesh_from_map": (_in_mesh, lambda t: MS.build_mesh_from_map(t["points"], mask=t["mask"])),
        "panorama_gpu.split_panorama_image": (_in_split, lambda t: PG.split_panorama_image(t["image"], *_cameras(), 4)),
        "panorama_gpu.merge_system+lsmr": (_in_merge, merge_and_solve),
    }


NAMES = ["alignment.align", "alignment.align_trunc", "alignment.align_points_scale_xyz_shift", "metrics.boundary_counts", "metrics.masked_max",
         "metrics.error_pass", "metrics.masked_nearest_resize", "evaluation.lanczos_resize", "evaluation.resize_nearest",
         "evaluation.masked_nearest_resize_distance", "refine.refine_depth_with_normal", "mesh.build_mesh_from_map",
         "panorama_gpu.split_panorama_image", "panorama_gpu.merge_system+lsmr"]


def _inputs(name, device):
    make, _ = _ops()[name]
    return {k: v.to(device) for k, v in make(_gen(NAMES.index(name))).items()}


def _bits(out):
    """the result as host bytes (tensors) and plain values (the solver's scalars), nesting flattened"""
    if isinstance(out, torch.Tensor):
        return [out.detach().contiguous().cpu().numpy().tobytes()]
    if isinstance(out, (tuple, list)):
        return [b for o in out for b in _bits(o)]
    return [np.float64(out).tobytes()]


@pytest.fixture(scope="module")
def default_bits():
    """name -> bits of the run on cuda:0's default stream, computed once"""
    cache = {}

    def get(name):
        if name not in cache:
            assert _ops().keys() == set(NAMES)
            out = _ops()[name][1](_inputs(name, "cuda:0"))
            torch.cuda.synchronize()
            cache[name] = _bits(out)
        return cache[name]
    return get


@pytest.fixture
def streams_asked(monkeypatch):
    """records (device argument, returned stream) of every _lib.stream_ptr call"""
    from moge_amd import _lib as L
    calls, real = [], L.stream_ptr

    def recorder(device=None):
        st = real(device)
        calls.append((device, st))
        return st
    monkeypatch.setattr(L, "stream_ptr", recorder)
    return calls


@pytest.mark.parametrize("name", NAMES)
def test_stream_is_taken_from_the_device_of_the_inputs(name, streams_asked, default_bits):
    t = _inputs(name, "cuda:0")
    dev = next(iter(t.values())).device
    out = _ops()[name][1](t)
    torch.cuda.synchronize()
    assert len(streams_asked) >= 1
    for asked, _ in streams_asked:
        assert asked is not None and torch.device(asked) == dev, (name, asked)
    assert _bits(out) == default_bits(name)


@pytest.mark.parametrize("name", NAMES)
def test_side_stream_is_honoured_and_gives_the_same_bits(name, streams_asked, default_bits):
    want = default_bits(name)
    t = _inputs(name, "cuda:0")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    del streams_asked[:]
    with torch.cuda.stream(side):
        out = _ops()[name][1](t)
    torch.cuda.synchronize()
    assert len(streams_asked) >= 1 and all(st == side.cuda_stream for _, st in streams_asked), name
    assert _bits(out) == want


@pytest.mark.parametrize("name", NAMES)
def test_inputs_on_another_gpu_give_the_same_bits(name, streams_asked, default_bits):
    if torch.cuda.device_count() < 2:
        pytest.skip("needs two GPUs")
    want = default_bits(name)
    other = torch.device("cuda", 1)
    t = _inputs(name, other)
    del streams_asked[:]
    with torch.cuda.device(0):
        out = _ops()[name][1](t)
        assert torch.cuda.current_device() == 0
    torch.cuda.synchronize(other)
    assert len(streams_asked) >= 1 and all(torch.device(asked) == other for asked, _ in streams_asked), name
    assert all(o.device == other for o in (out if isinstance(out, (tuple, list)) else [out]) if isinstance(o, torch.Tensor))
    assert _bits(out) == want
