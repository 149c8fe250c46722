import torch, torch.nn.functional as F, sys
sys.path.insert(0, '.')
from tests import hip_util as H
from moge_amd import _lib as L
for scale in (1.0, 3.0, 8.0):
    g = torch.Generator().manual_seed(0)
    B, nh, N = 2, 4, 3601
    q, k, v = (torch.randn(B, nh, N, 64, generator=g) for _ in range(3))
    q = q * scale
    # slowly growing logits along the key axis: the running max rises a little every tile (stale max stress)
    k = k + torch.linspace(0, 2.0, N)[None, None, :, None] * q.mean(dim=2, keepdim=True) / q.mean(dim=2, keepdim=True).norm(dim=-1, keepdim=True)
    ref = F.scaled_dot_product_attention(q.double().cuda(), k.double().cuda(), v.double().cuda()).permute(0, 2, 1, 3).reshape(B, N, nh * 64)
    for kern in (0, 1):
        with L.tuned(ATTN_KERN=kern):
            o = H.attention(1, q, k, v).double()
        e = (o - ref).abs()
        print(f"scale {scale} kern {kern}: max {float(e.max()):.3e} mean {float(e.mean()):.3e} p999 {float(torch.quantile(e.flatten()[:4000000].float(), 0.999)):.3e} refmax {float(ref.abs().max()):.2f}")
