"""GPU: the trainable Linear (moge_amd.linear, csrc/linear_grad.hip) against the float64 references of tests/linear_reference.py.

Gate: |got - ref| <= bound element by element, for y, dx, dw and db in both storage types; every output is filled with NaN before the call and must
come back finite.  Shapes are the tile edges (128 x 128 output tiles, 64 x 64 per wave, K tiles of 64 fp16 / 32 fp32 elements), not the workload;
(1370, 384, 1536) and a shape at which the weight gradient splits M run once each.  Inputs are rounded to the storage type before the reference
runs, so the figures are the kernels' own error.  Every test prints its figures before it asserts.

Measured worst error / bound on an MI355X: fp32 y 0.333, dx 0.367, dw 0.332, db 0.085 at the edges (all at sums of 4 terms) and at
most 0.057 at the larger shapes; fp16 y 0.990, dx 0.990, dw 0.999, db 0.960 - the fp16 bound is dominated by the store's h |ref| with h the unit
roundoff, which one correct rounding of a value just above a power of two uses up, so a fraction close to 1 is the store, not the sum.  The block
through autograd: at most 7.3e-7 plain and 6.1e-4 under fp16 autocast."""
import copy

import numpy as np
import pytest
import torch
from torch import nn
from torch.nn import functional as F

import linear_reference as LR
from tests.test_attention_module_cpu import StandInAttention
from tests.test_linear_module_cpu import StandInMlp, model_of

pytestmark = pytest.mark.gpu

DTYPES = [torch.float32, torch.float16]
PREC = {torch.float32: 0, torch.float16: 1}
NAMES = ("y", "dx", "dw", "db")
BAND = {False: 2e-5, True: 1e-2}           # the project's bands for the path through autograd: plain, fp16 autocast


@pytest.fixture(scope="module")
def Lin():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from moge_amd import linear
    return linear


def gpu(c, dtype):
    return tuple(torch.from_numpy(c[n]).to("cuda", dtype) for n in ("x", "w", "b", "dy"))


def nan(*shape, dtype):
    return torch.full(shape, float("nan"), dtype=dtype, device="cuda")


def run(Lin, x, w, b, dy, outs=None):
    """Forward and backward through the low-level calls into NaN-filled outputs (`outs`: views to write instead) -> {name: tensor}."""
    (M, K), N = x.shape, w.shape[0]
    o = outs or {"y": nan(M, N, dtype=x.dtype), "dx": nan(M, K, dtype=x.dtype), "dw": nan(N, K, dtype=x.dtype), "db": nan(N, dtype=x.dtype)}
    assert Lin.forward(x, w, b, out=o["y"]) is o["y"]
    Lin.backward(x, w, dy, o["dx"], o["dw"], o["db"])
    return o


def check(got, ref, what):
    frac = {}
    for n in NAMES:
        r, bound = ref[n]
        g = got[n].double().cpu().numpy()
        assert np.isfinite(g).all(), (what, n)
        frac[n] = float((np.abs(g - r) / bound).max())
    print(what, " ".join(f"{n}={f:.3f}" for n, f in frac.items()), "(worst error / bound)")
    for n in NAMES:
        assert frac[n] <= 1.0, (what, n, frac[n])


def same_bits(a, b, names=NAMES):
    return all(torch.equal(a[n], b[n]) for n in names)


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "fp16"])
@pytest.mark.parametrize("kn", range(5))
@pytest.mark.parametrize("M", LR.SWEEP_M)
def test_tile_edges_against_float64(Lin, M, kn, dtype):
    K, N = LR.sweep_kn(PREC[dtype])[kn]
    for family in ("random", "offset"):
        c = LR.case(M, K, N, family, PREC[dtype])
        check(run(Lin, *gpu(c, dtype)), c["ref"], f"edges M{M} K{K} N{N} {family} {dtype}")


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "fp16"])
@pytest.mark.parametrize("M,K,N", [LR.LARGE, LR.SPLIT], ids=["large", "split"])
def test_larger_shapes_against_float64(Lin, M, K, N, dtype):
    split = Lin.workspace_bytes(M, N, K, dtype) // (4 * N * K)
    assert split > 1                                    # both shapes split M in the weight gradient
    c = LR.case(M, K, N, "random", PREC[dtype])
    check(run(Lin, *gpu(c, dtype)), c["ref"], f"large M{M} K{K} N{N} split {split} {dtype}")


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "fp16"])
@pytest.mark.parametrize("M,K,N", [(129, 136, 264), (33, 72, 136)])
def test_slices_of_nan_padded_allocations_give_the_same_bits(Lin, M, K, N, dtype):
    """x, w, dy and every output as [:rows, :cols] slices of allocations with NaN rows and NaN columns behind: nothing outside is read, nothing
    outside is written."""
    c = LR.case(M, K, N, "random", PREC[dtype])
    x, w, b, dy = gpu(c, dtype)
    base = run(Lin, x, w, b, dy)
    pad = 2 * LR.CR.chunk(PREC[dtype])

    def padded(t):
        big = nan(t.shape[0] + 3, t.shape[1] + pad, dtype=dtype)
        big[:t.shape[0], :t.shape[1]] = t
        return big, big[:t.shape[0], :t.shape[1]]

    bigs = {n: nan(r + 3, cols + pad, dtype=dtype) for n, (r, cols) in (("y", (M, N)), ("dx", (M, K)), ("dw", (N, K)))}
    outs = {n: bigs[n][:r, :cols] for n, (r, cols) in (("y", (M, N)), ("dx", (M, K)), ("dw", (N, K)))}
    outs["db"] = nan(N + pad, dtype=dtype)[:N]
    xs, ws, dys = padded(x)[1], padded(w)[1], padded(dy)[1]
    assert not xs.is_contiguous() and Lin._rows(xs).data_ptr() == xs.data_ptr()
    got = run(Lin, xs, ws, b, dys, outs)
    assert same_bits(got, base)
    for n, big in bigs.items():                         # the padding of the outputs is untouched
        r, cols = outs[n].shape
        assert torch.isnan(big[r:]).all() and torch.isnan(big[:, cols:]).all(), n


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "fp16"])
def test_deterministic_and_a_row_is_the_row_it_is_alone(Lin, dtype):
    c = LR.case(129, 136, 264, "random", PREC[dtype])
    x, w, b, dy = gpu(c, dtype)
    first, second = run(Lin, x, w, b, dy), run(Lin, x, w, b, dy)
    assert same_bits(first, second)
    alone = run(Lin, x[:1], w, b, dy[:1])
    assert torch.equal(alone["y"], first["y"][:1]) and torch.equal(alone["dx"], first["dx"][:1])
    c = LR.case(*LR.SPLIT, "random", PREC[dtype])       # ... and with the split of M
    x, w, b, dy = gpu(c, dtype)
    assert same_bits(run(Lin, x, w, b, dy), run(Lin, x, w, b, dy))


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "fp16"])
def test_the_public_function_equals_the_low_level_calls_and_skips_what_is_not_needed(Lin, dtype):
    c = LR.case(129, 136, 264, "random", PREC[dtype])
    x, w, b, dy = gpu(c, dtype)
    base = run(Lin, x, w, b, dy)

    def through_autograd(need):
        xl, wl, bl = (t.clone().requires_grad_(n) for t, n in zip((x, w, b), need))
        y = Lin.linear(xl.view(3, 43, 136), wl, bl)
        assert y.shape == (3, 43, 264) and y.dtype == dtype
        y.backward(dy.view(3, 43, 264))
        return {"y": y.detach().view(129, 264), "dx": xl.grad if xl.grad is None else xl.grad.view(129, 136), "dw": wl.grad, "db": bl.grad}

    assert same_bits(through_autograd((True, True, True)), base)
    for skip in range(3):                               # each gradient skipped alone: it is None, the others keep their bits
        need = tuple(i != skip for i in range(3))
        got = through_autograd(need)
        assert got[NAMES[1 + skip]] is None
        assert same_bits(got, base, [n for i, n in enumerate(NAMES) if i != 1 + skip])
    y = Lin.linear(x, w)                                # no bias, no gradient
    assert not y.requires_grad and torch.equal(y, Lin.forward(x, w))
    out = {"dx": nan(129, 136, dtype=dtype)}            # the low-level call with one output: the others cost nothing and need nothing
    Lin.backward(None, w, dy, dx=out["dx"])
    assert torch.equal(out["dx"], base["dx"])
    db = nan(264, dtype=dtype)
    Lin.backward(None, None, dy, db=db)
    assert torch.equal(db, base["db"])


def test_the_packed_attention_gradient_is_the_dy_of_the_qkv_projection_without_a_copy(Lin):
    from moge_amd import attention as A
    torch.manual_seed(0)
    x = torch.randn(2, 65, 128, device="cuda")
    w = (torch.randn(384, 128, device="cuda") / 11).requires_grad_(True)
    b = torch.randn(384, device="cuda").requires_grad_(True)
    qkv = Lin.linear(x, w, b)
    seen = []
    qkv.register_hook(seen.append)
    A.attention_qkv_packed(qkv, 2).sum().backward()
    (g,) = seen
    assert g.shape == (2, 65, 384) and g.is_contiguous()
    dy = Lin._rows(g)
    assert dy.data_ptr() == g.data_ptr() and dy.shape == (130, 384)          # read in place
    dw, db = nan(384, 128, dtype=torch.float32), nan(384, dtype=torch.float32)
    Lin.backward(x.view(130, 128), None, dy, dw=dw, db=db)
    assert torch.equal(dw, w.grad) and torch.equal(db, b.grad)


def test_autocast(Lin):
    x = torch.randn(33, 64, device="cuda", requires_grad=True)
    lin = Lin.wrap_linear(nn.Linear(64, 72).cuda())
    with torch.autocast("cuda", dtype=torch.bfloat16):
        with pytest.raises(NotImplementedError, match="bfloat16"):
            lin(x)
    with torch.autocast("cuda", dtype=torch.float16):
        y = lin(x)
    assert y.dtype == torch.float16
    y.backward(torch.ones_like(y))
    assert x.grad.dtype == lin.weight.grad.dtype == lin.bias.grad.dtype == torch.float32          # fp32 tensors receive fp32 gradients through the cast
    want = F.linear(x.detach().half(), lin.weight.detach().half(), lin.bias.detach().half())
    assert float((y.detach().float() - want.float()).abs().max()) <= 2.0 ** -10 * float(want.float().abs().max())
    xg = x.detach().requires_grad_(True)                 # double backward is not built: once_differentiable refuses it
    yg = lin(xg)
    (g,) = torch.autograd.grad(yg, xg, grad_outputs=torch.ones_like(yg).requires_grad_(True), create_graph=True)
    with pytest.raises(RuntimeError, match="once_differentiable"):
        g.sum().backward()


class LayerScale(nn.Module):
    def __init__(self, dim):
        super().__init__()
        self.gamma = nn.Parameter(0.25 + torch.rand(dim))

    def forward(self, x):
        return x * self.gamma


class StandInBlock(nn.Module):
    """dinov2/layers/block.py: x + ls1(attn(norm1(x))), then x + ls2(mlp(norm2(x)))."""

    def __init__(self, dim=128, heads=2, hidden=512):
        super().__init__()
        self.norm1, self.attn, self.ls1 = nn.LayerNorm(dim), StandInAttention(dim, heads), LayerScale(dim)
        self.norm2, self.mlp, self.ls2 = nn.LayerNorm(dim), StandInMlp(dim, hidden), LayerScale(dim)

    def forward(self, x):
        x = x + self.ls1(self.attn(self.norm1(x)))
        return x + self.ls2(self.mlp(self.norm2(x)))


@pytest.mark.parametrize("autocast", [False, True], ids=["fp32", "autocast-fp16"])
def test_a_block_trains_a_step_through_this_library(Lin, autocast, monkeypatch):
    from moge_amd import attention as A
    torch.manual_seed(5)
    block = StandInBlock()
    with torch.no_grad():
        for p in list(block.norm1.parameters()) + list(block.norm2.parameters()):
            p.add_(0.1 * torch.randn_like(p))
    x, gy = torch.randn(2, 65, 128), torch.randn(2, 65, 128)
    ref_block = copy.deepcopy(block).double()
    xr = x.double().requires_grad_(True)
    yr = ref_block(xr)
    yr.backward(gy.double())
    want = {"y": yr.detach(), "x": xr.grad, **{n: p.grad for n, p in ref_block.named_parameters()}}

    model = Lin.use_hip_linear(A.use_hip_attention(model_of(block.cuda())))
    block = model.encoder.backbone.blocks[0]

    def refuse(*a, **k):
        raise AssertionError("torch's own linear / attention was called inside the block")

    monkeypatch.setattr(F, "linear", refuse)
    monkeypatch.setattr(F, "scaled_dot_product_attention", refuse)
    xg = x.cuda().requires_grad_(True)
    with torch.autocast("cuda", dtype=torch.float16, enabled=autocast):
        y = block(xg)
    y.backward(gy.cuda().to(y.dtype))
    monkeypatch.undo()
    got = {"y": y.detach(), "x": xg.grad, **{n: p.grad for n, p in block.named_parameters()}}
    assert set(got) == set(want) and len(want) == 2 + 14
    err = {n: float((got[n].double().cpu() - want[n]).abs().max() / want[n].abs().max()) for n in want}
    print(f"block autocast={autocast}", " ".join(f"{n}={e:.3e}" for n, e in err.items()))
    for n in want:
        assert got[n].dtype == torch.float32 and err[n] < BAND[autocast], (n, err[n])
