"""GPU: the trainable attention (moge_amd.attention, csrc/attention_grad.hip) against the float64 reference of tests/attention_reference.py.

Gate: max|got - ref| / max|ref| per tensor (o, lse, dq, dk, dv) below 2e-5 in fp32 and 1e-2 in fp16 - the bands the forward attention of the
infer() path is held to (tests/test_hip_kernels.py::test_attention).  Shapes are the tile edges (32-query / 32-key waves, 64-key and 32- or
64-query tiles, 128-row workgroups), not the workload; (1, 2, 1370) and (1, 1, 3601) run once each.  Inputs are rounded to the storage type
before the reference runs, so the figures are the kernels' own error.  Every test prints its figures before it asserts."""
import functools

import pytest
import torch
from torch import nn

from tests.attention_reference import reference
from tests.test_attention_module_cpu import StandInAttention

pytestmark = pytest.mark.gpu

BAND = {torch.float32: 2e-5, torch.float16: 1e-2}
DTYPES = [torch.float32, torch.float16]
EDGES = [1, 2, 31, 32, 33, 63, 64, 65, 127, 128, 129, 200, 257]
NAMES = ("o", "lse", "dq", "dk", "dv")


@pytest.fixture(scope="module")
def A():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from moge_amd import attention
    return attention


@functools.lru_cache(maxsize=None)
def case(B, nh, N, dtype, qmul=1.5):
    """Seeded inputs in the storage type (CPU) and their float64 reference; shared by every test that asks for the same case, never modified."""
    g = torch.Generator().manual_seed(N)
    q, k, v, do = (torch.randn(B, nh, N, 64, generator=g) for _ in range(4))
    q = q * qmul
    v[:, :, N // 2] += 5.0                       # asymmetric values: a transposed / permuted key order cannot pass
    do[:, :, N // 3] += 5.0                      # ... nor a permuted query order
    q, k, v, do = (t.to(dtype) for t in (q, k, v, do))
    return (q, k, v, do), reference(q, k, v, do)


def run(A, q, k, v, do):
    """Forward and backward through the low-level calls; q, k, v, do: (B, nh, N, 64) GPU tensors or views.  -> dict of (B, nh, N, ...) results,
    the gradients as slices of one packed buffer."""
    B, nh, N, _ = q.shape
    out, ws = A.forward(q, k, v)
    assert out.shape == (B, N, nh, 64) and out.is_contiguous() and ws.shape == (2, B, nh, N) and ws.dtype == torch.float32
    packed = torch.empty(B, N, 3, nh, 64, dtype=q.dtype, device="cuda")
    dq, dk, dv = (packed[:, :, i].permute(0, 2, 1, 3) for i in range(3))
    A.backward(q, k, v, out, do, ws, dq, dk, dv)
    return {"o": out.permute(0, 2, 1, 3), "lse": ws[0].clone(), "dq": dq, "dk": dk, "dv": dv}


def errors(got, ref, inputs):
    """max|got - ref| / max|ref| per tensor.  With a single key P = 1 and dS = P (dO V^T - D) is identically 0, so dq and dk are 0 and have no
    scale of their own (the float64 reference holds 1e-13 of summation noise, or 0): there the scale is that of the two terms that cancel,
    max|dO V^T| max|K| / 8 for dq and max|dO V^T| max|Q| / 8 for dk."""
    scale = {n: float(ref[n].abs().max()) for n in NAMES}
    q, k, v, do = (t.double() for t in inputs)
    if q.shape[2] == 1:
        cancel = float((do * v).sum(-1).abs().max())
        scale["dq"], scale["dk"] = cancel * float(k.abs().max()) / 8.0, cancel * float(q.abs().max()) / 8.0
    return {n: float((got[n].double().cpu() - ref[n]).abs().max()) / scale[n] for n in NAMES}


def check(got, ref, dtype, what, inputs):
    err = errors(got, ref, inputs)
    print(what, str(dtype), " ".join(f"{n}={e:.3e}" for n, e in err.items()))
    for n in NAMES:
        assert torch.isfinite(got[n]).all(), (what, n)
        assert err[n] < BAND[dtype], (what, n, err[n])


def same_bits(a, b):
    return all(torch.equal(a[n], b[n]) for n in NAMES)


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "fp16"])
@pytest.mark.parametrize("B,nh,N", [(b, h, n) for (b, h) in ((1, 1), (2, 3)) for n in EDGES] + [(1, 2, 1370), (1, 1, 3601)])
def test_against_float64(A, B, nh, N, dtype):
    (q, k, v, do), ref = case(B, nh, N, dtype)
    check(run(A, q.cuda(), k.cuda(), v.cuda(), do.cuda()), ref, dtype, f"edges B{B} nh{nh} N{N}", (q, k, v, do))


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "fp16"])
@pytest.mark.parametrize("B,nh,N", [(2, 3, 65), (1, 2, 257)])
def test_saturated_softmax(A, B, nh, N, dtype):
    """q *= 8: score differences of tens of units, most probabilities exactly 0 - the rescale across key tiles in the forward and
    exp(S - lse) in the backward."""
    (q, k, v, do), ref = case(B, nh, N, dtype, 1.5 * 8)
    check(run(A, q.cuda(), k.cuda(), v.cuda(), do.cuda()), ref, dtype, f"saturated B{B} nh{nh} N{N}", (q, k, v, do))


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "fp16"])
@pytest.mark.parametrize("B,nh,N", [(2, 3, 65), (1, 2, 200)])
def test_layouts_give_the_same_bits(A, B, nh, N, dtype):
    (q, k, v, do), _ = case(B, nh, N, dtype)
    q, k, v, do = q.cuda(), k.cuda(), v.cuda(), do.cuda()
    base = run(A, q, k, v, do)
    # the packed (B, N, 3, nh, 64) projection, read in place
    packed = torch.stack([t.permute(0, 2, 1, 3) for t in (q, k, v)], dim=2).contiguous()
    qs, ks, vs = (packed[:, :, i].permute(0, 2, 1, 3) for i in range(3))
    assert qs.data_ptr() == packed.data_ptr() and not qs.is_contiguous()
    assert same_bits(run(A, qs, ks, vs, do), base)
    # slices of a longer allocation whose extra rows are NaN: nothing past N is read
    def padded(t):
        big = torch.full((B, nh, N + 7, 64), float("nan"), dtype=dtype, device="cuda")
        big[:, :, :N] = t
        return big[:, :, :N]
    assert same_bits(run(A, padded(q), padded(k), padded(v), padded(do)), base)
    # through the public function: the same forward bits, and the same gradients
    ql, kl, vl = (t.clone().requires_grad_(True) for t in (qs, ks, vs))
    o = A.scaled_dot_product_attention(ql, kl, vl)
    assert o.shape == (B, nh, N, 64) and o.permute(0, 2, 1, 3).is_contiguous()
    o.backward(do)
    assert torch.equal(o.detach(), base["o"]) and torch.equal(ql.grad, base["dq"]) and torch.equal(kl.grad, base["dk"]) and torch.equal(vl.grad, base["dv"])


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "fp16"])
def test_deterministic_and_independent_of_the_batch(A, dtype):
    (q, k, v, do), _ = case(2, 3, 129, dtype)
    q, k, v, do = q.cuda(), k.cuda(), v.cuda(), do.cuda()
    first, second = run(A, q, k, v, do), run(A, q, k, v, do)
    assert same_bits(first, second)
    alone = run(A, q[:1].contiguous(), k[:1].contiguous(), v[:1].contiguous(), do[:1].contiguous())
    assert all(torch.equal(alone[n], first[n][:1]) for n in NAMES)


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "fp16"])
@pytest.mark.parametrize("B,nh,N", [(2, 3, 129), (1, 2, 257)])
def test_forward_agrees_with_the_inference_kernels(A, B, nh, N, dtype):
    from tests import hip_util
    (q, k, v, do), ref = case(B, nh, N, dtype)
    out, _ = A.forward(q.cuda(), k.cuda(), v.cuda())
    other = hip_util.attention({torch.float32: 0, torch.float16: 1}[dtype], q.float(), k.float(), v.float()).view(B, N, nh, 64)
    err = float((out.double() - other.double()).abs().max() / ref["o"].abs().max())
    print(f"vs infer kernels B{B} nh{nh} N{N} {dtype}: {err:.3e}")
    assert err < BAND[dtype]


class Float64Attention(nn.Module):
    """The stand-in module's arithmetic spelled out in float64: softmax(Q K^T / 8) V between the two projections."""

    def __init__(self, src):
        super().__init__()
        self.num_heads = src.num_heads
        self.qkv, self.proj = nn.Linear(128, 384), nn.Linear(128, 128)
        self.load_state_dict({k: v for k, v in src.state_dict().items()})
        self.double()

    def forward(self, x):
        B, N, C = x.shape
        q, k, v = self.qkv(x).reshape(B, N, 3, self.num_heads, 64).permute(2, 0, 3, 1, 4)
        p = torch.softmax(q @ k.transpose(-1, -2) / 8.0, dim=-1)
        return self.proj((p @ v).permute(0, 2, 1, 3).reshape(B, N, C))


@pytest.mark.parametrize("autocast", [False, True], ids=["fp32", "autocast-fp16"])
@pytest.mark.parametrize("N", [65, 257])
def test_through_autograd_in_a_dinov2_attention_module(A, N, autocast):
    torch.manual_seed(N)
    mod = StandInAttention(128, 2)
    x = torch.randn(2, N, 128)
    gy = torch.randn(2, N, 128)
    gy = gy.half().float() if autocast else gy            # the incoming gradient in the dtype the module's output has
    ref_mod = Float64Attention(mod)
    xr = x.double().requires_grad_(True)
    yr = ref_mod(xr)
    yr.backward(gy.double())
    want = {"y": yr.detach(), "x": xr.grad, "qkv.weight": ref_mod.qkv.weight.grad, "qkv.bias": ref_mod.qkv.bias.grad, "proj.weight": ref_mod.proj.weight.grad}

    mod = A.wrap_dinov2_attention(mod.cuda())
    xg = x.cuda().requires_grad_(True)
    with torch.autocast("cuda", dtype=torch.float16, enabled=autocast):
        y = mod(xg)
    assert y.dtype == (torch.float16 if autocast else torch.float32)
    y.backward(gy.cuda().to(y.dtype))
    got = {"y": y.detach(), "x": xg.grad, "qkv.weight": mod.qkv.weight.grad, "qkv.bias": mod.qkv.bias.grad, "proj.weight": mod.proj.weight.grad}
    band = BAND[torch.float16 if autocast else torch.float32]
    err = {n: float((got[n].double().cpu() - want[n]).abs().max() / want[n].abs().max()) for n in want}
    print(f"module N{N} autocast={autocast}", " ".join(f"{n}={e:.3e}" for n, e in err.items()))
    for n in want:
        assert got[n].dtype == (torch.float16 if autocast and n == "y" else torch.float32) and err[n] < band, (n, err[n])


def test_packed_gradient_is_one_tensor_and_the_graph_is_freed(A):
    qkv = torch.randn(2, 65, 384, device="cuda").requires_grad_(True)
    seen = []
    inner = (qkv * 1.0)
    inner.register_hook(seen.append)
    y = A.attention_qkv_packed(inner, 2)
    assert y.shape == (2, 65, 128)
    y.sum().backward()
    assert len(seen) == 1 and seen[0].shape == (2, 65, 384) and seen[0].is_contiguous() and torch.isfinite(seen[0]).all()
    y = A.attention_qkv_packed(qkv, 2)
    y.sum().backward()
    with pytest.raises(RuntimeError, match="backward through the graph a second time"):
        y.sum().backward()


def test_bf16_autocast_is_refused(A):
    q = torch.randn(1, 2, 33, 64, device="cuda")
    with torch.autocast("cuda", dtype=torch.bfloat16):
        with pytest.raises(NotImplementedError, match="bfloat16"):
            A.scaled_dot_product_attention(q, q, q)
        with pytest.raises(NotImplementedError, match="bfloat16"):
            A.attention_qkv_packed(torch.randn(1, 33, 384, device="cuda"), 2)
    with torch.autocast("cuda", dtype=torch.float16):
        assert A.scaled_dot_product_attention(q, q, q).dtype == torch.float16
