"""CPU: the float64 reference of the trainable attention (tests/attention_reference.py) against torch's own float64 autograd of
F.scaled_dot_product_attention.  The GPU tests (tests/test_hip_attention_grad.py) measure the HIP kernels against this reference."""
import pytest
import torch
import torch.nn.functional as F

from tests.attention_reference import reference


@pytest.mark.parametrize("B,nh,N", [(1, 1, 1), (2, 3, 65), (1, 2, 257)])
def test_reference_is_torch_float64_autograd(B, nh, N):
    g = torch.Generator().manual_seed(100 + N)
    q, k, v, do = (torch.randn(B, nh, N, 64, generator=g, dtype=torch.float64) for _ in range(4))
    q = q * 1.5
    v[:, :, N // 2] += 5.0
    ref = reference(q, k, v, do)
    ql, kl, vl = (t.clone().requires_grad_(True) for t in (q, k, v))
    o = F.scaled_dot_product_attention(ql, kl, vl)
    o.backward(do)
    lse = torch.logsumexp(q @ k.transpose(-1, -2) / 8.0, dim=-1)
    for name, want in (("o", o.detach()), ("lse", lse), ("dq", ql.grad), ("dk", kl.grad), ("dv", vl.grad)):
        err = float((ref[name] - want).abs().max() / want.abs().max())
        assert err < 1e-12, (name, err)
        assert ref[name].dtype == torch.float64 and ref[name].shape == want.shape
