"""GPU: the trainable attention (moge_amd.attention, csrc/attention_grad.hip) against the float64 reference of tests/attention_reference.py.

Gate: |got - ref| <= bound on EVERY element of o, lse, D, dq, dk and dv, the bound counted from the kernels' roundings (derivation: the docstring of
tests/attention_reference.py; its power: tests/test_attention_reference_cpu.py), plus isfinite.  D, the second half of the workspace, is also held to
rowsum(dO o O) of the `out` the forward itself returned, with the 65 u of the delta kernel alone ("D|out").  Beside it the older gate stays:
max|got - ref| / max|ref| per tensor (o, lse, dq, dk, dv) below 2e-5 in fp32 and 1e-2 in fp16, on the inputs it was set on (the random and the
saturated family).  It is printed but not asserted in the offset and neg_scores families: there D is large and dP - D cancels, and the honest float64
emulation of the CPU tests, which rounds every sum ONCE, already gives 2.1e-5 for dq at (2, 3, 97) in fp32; the kernels measure 8.0e-5 (dq, (2, 3, 257))
at 0.012 of their bound.

The sweep (test_against_float64: random, offset, neg_scores; test_saturated_softmax: saturated) runs (B, nh) in ((1, 1), (2, 3)) x N in 1, 2, 31, 32, 33, 63,
64, 65, 95, 96, 97, 127, 128, 129, 200, 255, 256, 257 - the tile edges (32-query / 32-key waves, 64-key and 32- or 64-query tiles, 128-row workgroups),
not the workload; (1, 2, 1370) and (1, 1, 3601) run once each, random only.  It goes through the C entry points on buffers this module owns, every byte of
out, of both halves of the workspace and of the gradient destination 0xFF before each launch (run_poisoned): a store a kernel skips is a NaN, not the
previous call's answer out of the caching allocator.  test_nothing_else_is_written adds gaps, margins and over-allocation and finds them untouched;
test_poisoned_entry_gives_the_bits_of_the_python_calls ties this way in to A.forward / A.backward.  Inputs are rounded to the storage type before the
reference runs, so the figures are the kernels' own error.  Every test prints its figures before it asserts.

Measured on an MI355X (pytest -s, 172 tests, 7.9 s for the module, slowest test 0.9 s), worst error / bound over the sweep and the two large shapes:

    fp32         o      lse    D      dq     dk     dv     D|out        fp16         o      lse    D      dq     dk     dv     D|out
    random       0.070  0.074  0.028  0.012  0.010  0.015  0.078        random       0.577  0.039  0.181  0.514  0.503  0.664  0.079
    offset       0.077  0.074  0.019  0.018  0.015  0.014  0.078        offset       0.593  0.039  0.135  0.347  0.376  0.673  0.083
    neg_scores   0.039  0.051  0.033  0.022  0.037  0.028  0.080        neg_scores   0.594  0.027  0.140  0.333  0.506  0.698  0.079
    saturated    0.096  0.065  0.028  0.033  0.024  0.042  0.052        saturated    0.608  0.031  0.149  0.246  0.422  0.629  0.079

No figure was above 1 on the first run and no term was added to a bound after it.  The fp16 worst cases are mostly at N = 2 (dq, dk, dv) and N = 32 / 33 (o) (few terms:
the fp16 roundings of P, dS and the store are all there is, and the bound allows each its worst case); they equal the CPU emulation's (0.608 / 0.514 /
0.506 / 0.698) to three digits.  fp32 uses a tenth of a bound that admits N sequential roundings."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch
from torch import nn

from tests import attention_reference as AR
from tests.test_attention_module_cpu import StandInAttention

pytestmark = pytest.mark.gpu

BAND = {torch.float32: 2e-5, torch.float16: 1e-2}
DTYPES = [torch.float32, torch.float16]
PREC = {torch.float32: 0, torch.float16: 1}
NAMES = ("o", "lse", "dq", "dk", "dv")                  # the tensors of the band; the bounds hold AR.NAMES, with D
SWEEP_FAMILIES = ("random", "offset", "neg_scores")
BAND_FAMILIES = ("random", "saturated")                 # the inputs the band was set on; see the module docstring for the other two


@pytest.fixture(scope="module")
def A():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from moge_amd import attention
    return attention


@functools.lru_cache(maxsize=None)
def case(B, nh, N, dtype, family="random"):
    """Seeded inputs in the storage type (CPU) and their float64 reference (attention_reference.case, shared with the CPU tests); never modified."""
    c = AR.case(B, nh, N, family, PREC[dtype])
    return tuple(torch.from_numpy(t).to(dtype) for t in c["inputs"]), {n: torch.from_numpy(r) for n, (r, _) in c["ref"].items()}


def run(A, q, k, v, do):
    """Forward and backward through the low-level calls; q, k, v, do: (B, nh, N, 64) GPU tensors or views.  -> dict of (B, nh, N, ...) results,
    the gradients as slices of one packed buffer."""
    B, nh, N, _ = q.shape
    out, ws = A.forward(q, k, v)
    assert out.shape == (B, N, nh, 64) and out.is_contiguous() and ws.shape == (2, B, nh, N) and ws.dtype == torch.float32
    packed = torch.empty(B, N, 3, nh, 64, dtype=q.dtype, device="cuda")
    dq, dk, dv = (packed[:, :, i].permute(0, 2, 1, 3) for i in range(3))
    lse = ws[0].clone()
    A.backward(q, k, v, out, do, ws, dq, dk, dv)
    assert torch.equal(ws[0], lse)                       # the backward leaves the first half alone
    return {"o": out.permute(0, 2, 1, 3), "lse": lse, "D": ws[1], "dq": dq, "dk": dk, "dv": dv}


def poisoned(numel, dtype):
    """A buffer of `numel` elements whose every byte is 0xFF: NaN in fp16 and in fp32."""
    return torch.full((numel * torch.empty((), dtype=dtype).element_size(),), 0xFF, dtype=torch.uint8, device="cuda").view(dtype)


def all_ff(t):
    return bool((t.contiguous().view(torch.uint8) == 0xFF).all())


def grad_views(buf, B, nh, N, ts, margin):
    """dq, dk, dv (B, nh, N, 64) inside buf: `margin` elements, then B N tokens of `ts` >= 3 nh 64 elements each (q | k | v | gap)."""
    tok = buf[margin:margin + B * N * ts].view(B, N, ts)
    return tuple(tok[:, :, i * nh * 64:(i + 1) * nh * 64].unflatten(-1, (nh, 64)).permute(0, 2, 1, 3) for i in range(3))


def strides(t):
    return (C.c_int64 * 3)(t.stride(0), t.stride(1), t.stride(2))


def run_poisoned(q, k, v, do, gap=0, margin=0, over=0):
    """The same through L.lib.moge_attn_forward / _backward on buffers this test owns: out, both halves of the workspace and the gradient destination are
    0xFF bytes before each launch, so a store the kernel skips is a NaN and not the previous call's answer out of the caching allocator.  gap: elements between
    the tokens of the gradient destination, margin: before and after it, over: past the end of out and of the workspace; all of them must still be 0xFF
    afterwards."""
    from moge_amd import _lib as L
    B, nh, N, _ = q.shape
    dt, n_out, n_ws, ts = q.dtype, B * N * nh * 64, 2 * B * nh * N, 3 * nh * 64 + gap
    out_buf, ws_buf, g_buf = poisoned(n_out + over, dt), poisoned(n_ws + over, torch.float32), poisoned(2 * margin + B * N * ts, dt)
    out = out_buf[:n_out].view(B, N, nh, 64)
    o = out.permute(0, 2, 1, 3)
    dq, dk, dv = grad_views(g_buf, B, nh, N, ts, margin)
    with L.on(q.device) as st:
        L.check(L.lib.moge_attn_forward(L.FP16 if dt == torch.float16 else L.FP32, L.ptr(q), strides(q), L.ptr(k), strides(k), L.ptr(v), strides(v), L.ptr(out_buf),
                                        L.ptr(ws_buf), B, nh, N, st))
        lse = ws_buf[:n_ws // 2].view(B, nh, N).clone()
        assert all_ff(ws_buf[n_ws // 2:]), "the forward wrote past the lse half of the workspace"
        L.check(L.lib.moge_attn_backward(L.FP16 if dt == torch.float16 else L.FP32, L.ptr(q), strides(q), L.ptr(k), strides(k), L.ptr(v), strides(v), L.ptr(o), strides(o),
                                         L.ptr(do), strides(do), L.ptr(ws_buf), L.ptr(dq), strides(dq), L.ptr(dk), strides(dk), L.ptr(dv), strides(dv), B, nh, N, st))
    assert torch.equal(ws_buf[:n_ws // 2].view(B, nh, N), lse)
    assert all_ff(out_buf[n_out:]) and all_ff(ws_buf[n_ws:]), "bytes past the end of out / the workspace were written"
    if gap or margin:
        rest = g_buf.clone()
        for t in grad_views(rest.view(torch.int16 if dt == torch.float16 else torch.int32), B, nh, N, ts, margin):
            t.fill_(-1)                                   # what the three views cover, back to 0xFF: everything else must never have left it
        assert all_ff(rest), "bytes outside the dq / dk / dv views were written"
    return {"o": o, "lse": lse, "D": ws_buf[n_ws // 2:n_ws].view(B, nh, N), "dq": dq, "dk": dk, "dv": dv}


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


def fractions(got, B, nh, N, dtype, family, inputs):
    """Worst |got - ref| / bound per tensor of AR.NAMES, and "D|out": the D the backward left against rowsum(dO o O) of the out the forward returned,
    which holds the delta kernel alone to its 65 u."""
    bounds = AR.case(B, nh, N, family, PREC[dtype])["ref"]
    host = {n: got[n].double().cpu().numpy() for n in AR.NAMES}
    fr = {n: float((np.abs(host[n] - bounds[n][0]) / bounds[n][1]).max()) for n in AR.NAMES}
    ref, bound = AR.d_from_out(host["o"], inputs[3])
    fr["D|out"] = float((np.abs(host["D"] - ref) / np.maximum(bound, AR.FLUSH)).max())
    return fr


def check(got, dtype, what, B, nh, N, family="random"):
    inputs, ref = case(B, nh, N, dtype, family)
    err = errors(got, ref, inputs)
    fr = fractions(got, B, nh, N, dtype, family, inputs)
    print(what, family, str(dtype), "band", " ".join(f"{n}={e:.3e}" for n, e in err.items()), "| error / bound", " ".join(f"{n}={x:.3f}" for n, x in fr.items()))
    for n in AR.NAMES:
        assert torch.isfinite(got[n]).all(), (what, family, n)
    if family in BAND_FAMILIES:
        for n in NAMES:
            assert err[n] < BAND[dtype], (what, family, n, err[n])
    for n, x in fr.items():
        assert x <= 1.0, (what, family, n, x)
    return fr


def same_bits(a, b):
    return all(torch.equal(a[n], b[n]) for n in AR.NAMES)


def sweep(B, nh, N, dtype, family, what):
    q, k, v, do = (t.cuda() for t in case(B, nh, N, dtype, family)[0])
    return check(run_poisoned(q, k, v, do), dtype, f"{what} B{B} nh{nh} N{N}", B, nh, N, family)


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "fp16"])
@pytest.mark.parametrize("B,nh,N", AR.SMALL + AR.LARGE)
def test_against_float64(A, B, nh, N, dtype):
    """Every element of o, lse, D, dq, dk, dv within its bound, in the random, offset and neg_scores families (the two large shapes: random only)."""
    for family in SWEEP_FAMILIES if (B, nh, N) in AR.SMALL else SWEEP_FAMILIES[:1]:
        sweep(B, nh, N, dtype, family, "edges")


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "fp16"])
@pytest.mark.parametrize("B,nh,N", AR.SMALL + [(1, 2, 257)])
def test_saturated_softmax(A, B, nh, N, dtype):
    """q x 12: score differences of tens of units, most probabilities exactly 0 - the rescale across key tiles in the forward and
    exp(S - lse) in the backward."""
    sweep(B, nh, N, dtype, "saturated", "saturated")


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "fp16"])
def test_poisoned_entry_gives_the_bits_of_the_python_calls(A, dtype):
    q, k, v, do = (t.cuda() for t in case(2, 3, 129, dtype)[0])
    first = run(A, q, k, v, do)
    check(first, dtype, "python calls B2 nh3 N129", 2, 3, 129)
    assert same_bits(first, run_poisoned(q, k, v, do))


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "fp16"])
@pytest.mark.parametrize("B,nh,N", [(2, 3, 65), (1, 2, 129)])
def test_nothing_else_is_written(A, B, nh, N, dtype):
    """dq, dk and dv into a destination with gaps: a token stride larger than 3 nh 64 and a margin before and after, out and the workspace over-allocated,
    all 0xFF.  Afterwards every byte outside the results still is (run_poisoned asserts it), and the results are the bits of the packed layout."""
    q, k, v, do = (t.cuda() for t in case(B, nh, N, dtype)[0])
    got = run_poisoned(q, k, v, do, gap=40, margin=64, over=96)
    assert got["dq"].stride(2) == 3 * nh * 64 + 40
    check(got, dtype, f"gaps B{B} nh{nh} N{N}", B, nh, N)
    assert same_bits(got, run_poisoned(q, k, v, do))


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
