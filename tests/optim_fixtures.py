"""The shared fixture of the optimizer tests (moge_amd.optim, csrc/optim.hip): a list of small tensors placed around the kernel's chunk
(MOGE_OPTIM_CHUNK elements per workgroup, 4 per thread and round), two parameter groups and T steps of gradients.  Everything is seeded on the
host and held in float32 values, so the float64 reference, torch's own fp32 run and the GPU start from the same numbers.  Fewer than 10 chunks of
elements in all."""
import functools
from typing import Dict, List, Optional, Tuple

import torch

from moge_amd._lib import OPTIM_CHUNK as C

T = 6
# (name, shape, kind): kind "view" = a view starting one element into its storage (not 16-byte aligned), "nograd" = its grad is always None
TENSORS: List[Tuple[str, Tuple[int, ...], str]] = [
    ("n1", (1,), ""), ("n3", (3,), ""), ("n4", (4,), ""), ("n5", (5,), ""), ("n63", (63,), ""), ("n64", (64,), ""), ("n65", (65,), ""),
    ("c_minus", (C - 1,), ""), ("c", (C,), ""), ("c_plus", (C + 1,), ""), ("two_c", (2 * C + 3,), ""), ("matrix", (7, 9), ""), ("empty", (0,), ""),
    ("view", (C + 2,), "view"), ("nograd", (10,), "nograd")]
NAMES = [t[0] for t in TENSORS]
INDEX = {name: i for i, name in enumerate(NAMES)}
GROUPS = [dict(lr=1e-4, weight_decay=0.01, betas=(0.9, 0.999), eps=1e-8), dict(lr=1e-5, weight_decay=0.0, betas=(0.8, 0.99), eps=1e-6)]
GROUP_OF = [i % 2 for i in range(len(TENSORS))]         # even tensors in group 0, odd ones in group 1
assert sum(int(torch.Size(s).numel()) for _, s, _ in TENSORS) < 10 * C


@functools.lru_cache(maxsize=None)
def _values() -> Tuple[Tuple[torch.Tensor, ...], Tuple[Tuple[Optional[torch.Tensor], ...], ...]]:
    gen = torch.Generator().manual_seed(20261019)
    params = tuple(torch.randn(shape, generator=gen, dtype=torch.float32) for _, shape, _ in TENSORS)
    grads = tuple(tuple(None if kind == "nograd" else torch.randn(shape, generator=gen, dtype=torch.float32) * (10.0 if t % 2 == 0 else 0.01)
                        for _, shape, kind in TENSORS) for t in range(T))
    return params, grads


def initial(dtype=torch.float32, device="cpu", aligned_view: bool = False) -> List[torch.Tensor]:
    """Fresh parameter tensors (leaves that do not require grad; the tests set .grad themselves).  The "view" tensor starts one element into a
    storage of its own unless aligned_view."""
    out = []
    for (name, shape, kind), value in zip(TENSORS, _values()[0]):
        if kind == "view" and not aligned_view:
            base = torch.zeros(value.numel() + 1, dtype=dtype, device=device)
            t = base[1:]
            t.copy_(value)
        else:
            t = value.to(dtype=dtype, device=device, copy=True)
        out.append(t)
    return out


def gradients(t: int, dtype=torch.float32, device="cpu", scale: float = 1.0, poison: Optional[Dict[str, Tuple[int, float]]] = None) -> List[Optional[torch.Tensor]]:
    """The gradients of step t (alternately large, so that clipping at 1 engages, and small), times `scale`; poison: {tensor name: (flat
    index, value)} overwrites single elements."""
    out = []
    for name, g in zip(NAMES, _values()[1][t]):
        if g is None:
            out.append(None)
            continue
        g = (g.to(torch.float64) * scale).to(dtype)
        if poison and name in poison:
            at, value = poison[name]
            g.view(-1)[at] = value
        out.append(g.to(device))
    return out


def param_groups(params: List[torch.Tensor]) -> List[dict]:
    return [{"params": [p for p, gi in zip(params, GROUP_OF) if gi == k], **GROUPS[k]} for k in range(len(GROUPS))]


def group_order() -> List[int]:
    """Fixture indices in the optimizer's parameter order (group by group)."""
    return [i for k in range(len(GROUPS)) for i, gi in enumerate(GROUP_OF) if gi == k]
