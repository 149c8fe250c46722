"""float64 reference of the trainable attention (moge_amd.attention), written from the formulas and not from the
kernels: per (batch, head), with S = Q K^T / 8,

    lse = log sum_j exp(S_ij)      P = exp(S - lse)      O = P V
    D = rowsum(dO o O)             dV = P^T dO           dS = P o (dO V^T - D) / 8       dQ = dS K       dK = dS^T Q

tests/test_attention_reference_cpu.py checks it against torch's float64 autograd of F.scaled_dot_product_attention."""
import torch


def reference(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, do: torch.Tensor) -> dict:
    """q, k, v, do (B, nh, N, 64) of any float dtype -> float64 CPU tensors o, dq, dk, dv (B, nh, N, 64) and lse (B, nh, N).  One (batch, head)
    at a time, so that N = 3601 needs one N x N matrix at a time."""
    q, k, v, do = (t.detach().to("cpu", torch.float64) for t in (q, k, v, do))
    B, nh, N, _ = q.shape
    res = {name: torch.empty_like(q) for name in ("o", "dq", "dk", "dv")}
    res["lse"] = torch.empty(B, nh, N, dtype=torch.float64)
    for b in range(B):
        for h in range(nh):
            Q, K, V, dO = q[b, h], k[b, h], v[b, h], do[b, h]
            S = Q @ K.T / 8.0
            m = S.max(dim=1, keepdim=True).values
            lse = m + torch.log(torch.exp(S - m).sum(dim=1, keepdim=True))
            P = torch.exp(S - lse)
            O = P @ V
            D = (dO * O).sum(dim=1, keepdim=True)
            dS = P * (dO @ V.T - D) / 8.0
            res["o"][b, h], res["lse"][b, h] = O, lse[:, 0]
            res["dv"][b, h], res["dq"][b, h], res["dk"][b, h] = P.T @ dO, dS @ K, dS.T @ Q
    return res
