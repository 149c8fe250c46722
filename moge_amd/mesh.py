"""Image mesh and masked point cloud on the MI355X: the device twins of `moge_amd.io.build_mesh_from_map` and `moge_amd.io.masked_point_cloud`
(the host functions are the specification: the results here equal theirs bit for bit), calling the stream-compaction kernels of
`csrc/mesh.hip` through the C ABI (`moge_image_mesh_workspace` / `_count` / `_fill`).  DESIGN.md section 13 has the algorithm and the launches.

    from moge_amd.mesh import export_mesh
    out = model.infer(image)
    clean = model.depth_edge_mask(out["depth"], out["mask"], rtol=0.04)
    faces, vertices, vertex_colors, vertex_uvs, vertex_normals = export_mesh(out["points"], image_u8, clean, out["normal"])   # or model.image_mesh(out, image_u8)

Every tensor must live on the GPU (`cuda`); there is no CPU path here (`moge_amd.io` is the host form).  Maps are float32, or uint8 (an image),
which becomes float32 `x / 255`.  Because the output sizes depend on the mask, every call reads the per-image counts (8 bytes per image) back
to the host once; nothing else synchronises."""
from __future__ import annotations

import ctypes as C
from typing import List, Optional, Sequence, Tuple

import torch

from . import _lib as L
from ._lib import ptr

BLOCK_PX = L.MESH_BLOCK_PX          # include/moge_hip.h MOGE_MESH_BLOCK_PX: consecutive pixels one workgroup of the scan ranks
SCAN_SPAN = L.MESH_SCAN_SPAN        # MOGE_MESH_SCAN_SPAN: workgroup totals one workgroup of the second scan level covers (the tests place shapes on both)
MAX_MAPS = L.MESH_MAX_MAPS

_FLIP_YZ = ((1.0, -1.0, -1.0), None)                   # vertices, normals: OpenGL convention (x right, y up, z backward), scripts/infer.py:146-149
_FLIP_V = ((1.0, -1.0), (0.0, 1.0))                    # uv: (0, 0) = left-bottom of the texture
UV = "uv"                                              # in place of a map: texture coordinates generated in the gather (= moge_amd.io.uv_map)


def workspace_bytes(B: int, H: int, W: int) -> int:
    """moge_image_mesh_workspace: pure arithmetic, no GPU call."""
    n = C.c_int64(0)
    L.check(L.lib.moge_image_mesh_workspace(int(B), int(H), int(W), C.byref(n)))
    return n.value


def _prepare(maps: Sequence, mask: Optional[torch.Tensor], batched: Optional[bool]):
    """-> (batched, B, H, W, device, [(tensor (B, H, W, C) contiguous or None for UV, C, dtype code)], mask (B, H, W) u8 or None)"""
    tensors = [m for m in maps if not isinstance(m, str)] + ([mask] if mask is not None else [])
    if not tensors:
        raise ValueError("need at least one map or a mask")
    dev = L.device_of("mesh", *tensors, host="moge_amd.io", tensors_only=True)
    if len(maps) > MAX_MAPS:
        raise ValueError(f"at most {MAX_MAPS} maps per call, got {len(maps)}")
    if batched is None:                                 # a mask says it; without one a 3-D map is (H, W, C), as in the host function
        batched = mask.dim() == 3 if mask is not None else tensors[0].dim() == 4
    lead = 3 if batched else 2
    ref = mask if mask is not None else tensors[0]
    if ref.dim() < lead:
        raise ValueError(f"expected {'(B, H, W' if batched else '(H, W'}, ...), got {tuple(ref.shape)}")
    shape = tuple(ref.shape[:lead])
    if mask is not None and mask.dim() != lead:
        raise ValueError(f"mask {tuple(mask.shape)} must be {'(B, H, W)' if batched else '(H, W)'}")
    B, H, W = shape if batched else (1,) + shape
    if H < 1 or W < 1 or H * W >= 2 ** 31 or B > 65535:                  # the limits of the C calls (one grid row per image)
        raise ValueError(f"need H, W >= 1, H * W < 2^31 and at most 65535 images, got {B} x {H} x {W}")
    specs = []
    for m in maps:
        if isinstance(m, str):
            if m != UV:
                raise ValueError(f"unknown generated map {m!r}")
            specs.append((None, 2, L.MESH_UV))
            continue
        if m.dim() not in (lead, lead + 1) or tuple(m.shape[:lead]) != shape:
            raise ValueError(f"map {tuple(m.shape)} does not match {shape} (+ an optional channel axis)")
        ch = m.shape[lead] if m.dim() == lead + 1 else 1
        if not 1 <= ch <= 4:
            raise ValueError(f"a map has 1 ... 4 channels, got {ch}")
        if m.dtype not in (torch.float32, torch.uint8):
            raise ValueError(f"maps are float32 or uint8, got {m.dtype}")
        specs.append((m.reshape(B, H, W, ch).contiguous(), ch, L.MESH_F32 if m.dtype == torch.float32 else L.MESH_U8))
    mk = None
    if mask is not None:
        if mask.dtype not in (torch.bool, torch.uint8):
            raise ValueError(f"mask must be bool (or uint8), got {mask.dtype}")
        mk = mask.reshape(B, H, W).contiguous().view(torch.uint8)
    return batched, B, H, W, dev, specs, mk


def _compact(maps: Sequence, mask, tri: Optional[bool], points: bool, transforms: Optional[Sequence] = None, batched: Optional[bool] = None):
    """The two C calls.  -> (batched, [(faces or None, [attributes])] per image)"""
    batched, B, H, W, dev, specs, mk = _prepare(maps, mask, batched)
    transforms = transforms or [(None, None)] * len(specs)
    faces_w = 3 if tri else 4
    if B == 0:
        return batched, []
    ws = torch.empty(workspace_bytes(B, H, W), device=dev, dtype=torch.uint8)
    counts = torch.empty((B, 2), device=dev, dtype=torch.int32)
    offsets = torch.empty((B, 2), device=dev, dtype=torch.int64)
    with L.on(dev) as st:
        L.check(L.lib.moge_image_mesh_count(ptr(mk), B, H, W, 1 if points else 0, ptr(ws), ptr(counts), ptr(offsets), st))
        cnt = counts.cpu().tolist()                     # the one host read-back: the outputs' sizes
        V, Q = sum(c[0] for c in cnt), sum(c[1] for c in cnt)
        outs = [torch.empty((V, ch), device=dev, dtype=torch.float32) for _, ch, _ in specs]
        faces = None if tri is None else torch.empty(((2 if tri else 1) * Q, faces_w), device=dev, dtype=torch.int32)
        if V > 0 and (specs or tri is not None):        # an empty result launches nothing
            arr = (L.MeshMap * max(1, len(specs)))()
            for a, (t, ch, code), o, (scale, offset) in zip(arr, specs, outs, transforms):
                a.data, a.out, a.channels, a.dtype = ptr(t), ptr(o), ch, code
                a.has_scale, a.has_offset = int(scale is not None), int(offset is not None)
                for k in range(ch):
                    a.scale[k] = scale[k] if scale is not None else 1.0
                    a.offset[k] = offset[k] if offset is not None else 0.0
            L.check(L.lib.moge_image_mesh_fill(B, H, W, ptr(ws), arr, len(specs), L.MESH_NO_FACES if tri is None else int(bool(tri)), ptr(faces), ptr(offsets), st))
    res, v0, q0 = [], 0, 0
    per = 2 if tri else 1
    for v, q in cnt:
        res.append((None if faces is None else faces[per * q0:per * (q0 + q)], [o[v0:v0 + v] for o in outs]))
        v0, q0 = v0 + v, q0 + q
    return batched, res


def build_mesh_from_map(*maps: torch.Tensor, mask: Optional[torch.Tensor] = None, tri: bool = True):
    """`moge_amd.io.build_mesh_from_map` on the device, same call shape and result: grid mesh over an (H, W) image, one quad per 2x2 pixel block
    whose four pixels are inside `mask` (None: all), split into two triangles when `tri`; vertices no face references are dropped and the faces
    re-indexed.  maps: CUDA tensors (H, W, C) with C = 1 ... 4, or (H, W); float32, whose values keep their bits (NaN, inf, -0.0), or uint8 (an
    image), returned as float32 `x / 255`; non-contiguous views are accepted; `moge_amd.mesh.UV` in place of a map generates
    `moge_amd.io.uv_map(H, W)`.  -> (faces int32 (2Q, 3) or (Q, 4), *attributes float32 (N, C)), CUDA tensors (slices of one buffer each).

    Batch: maps (B, H, W[, C]) with mask (B, H, W) return a list of B such tuples, image b's equal to that image alone.  Without a mask a 3-D map
    is read as (H, W, C), like the host function does, and a 4-D one as a batch.

    The call makes ONE host read-back, of the per-image (vertices, quads) counts that size the outputs; nothing else synchronises.  CPU tensors
    raise RuntimeError (no CPU path here); mismatched shapes, more than 4 channels, more than 8 maps, more than 65535 images and other dtypes raise ValueError."""
    if not maps:
        raise ValueError("build_mesh_from_map needs at least one map")
    batched, res = _compact(maps, mask, bool(tri), points=False)
    tuples = [(f,) + tuple(a) for f, a in res]
    return tuples if batched else tuples[0]


def masked_point_cloud(points: torch.Tensor, mask: torch.Tensor, image: Optional[torch.Tensor] = None, normal: Optional[torch.Tensor] = None):
    """`moge_amd.io.masked_point_cloud` on the device: vertices (N, 3), colours (N, 3) in [0, 1] (a uint8 image / 255) or None, normals or None of
    EVERY pixel inside `mask`, in the export convention (x right, y up, z backward) - the same scan as the mesh, with the mask itself as the
    flag.  (B, H, W) masks return a list.  One host read-back of the counts, as build_mesh_from_map."""
    if mask is None:
        raise ValueError("masked_point_cloud needs a mask")
    maps = [points] + [m for m in (image, normal) if m is not None]
    tr = [_FLIP_YZ] + ([(None, None)] if image is not None else []) + ([_FLIP_YZ] if normal is not None else [])
    for name, t in (("points", points), ("normal", normal), ("image", image)):
        if t is not None and isinstance(t, torch.Tensor) and t.shape[-1:] != (3,):
            raise ValueError(f"{name} must be (..., H, W, 3), got {tuple(t.shape)}")
    batched, res = _compact(maps, mask, None, points=True, transforms=tr)

    def unpack(a):
        a = list(a)
        v = a.pop(0)
        c = a.pop(0) if image is not None else None
        n = a.pop(0) if normal is not None else None
        return v, c, n
    out = [unpack(a) for _, a in res]
    return out if batched else out[0]


def export_mesh(points: torch.Tensor, image_u8: torch.Tensor, mask: Optional[torch.Tensor], normal: Optional[torch.Tensor] = None, tri: bool = True):
    """What the export scripts need, in one call: -> faces, vertices, vertex_colors, vertex_uvs[, vertex_normals] of the image mesh over `mask`,
    already in the export convention - vertices and normals * [1, -1, -1], uvs * [1, -1] + [0, 1] with the uvs generated in the gather
    (`moge_amd.io.uv_map`), colours = image / 255 (a float32 image passes through).  Each value equals the scripts' float64 host expression
    rounded once to float32, which is what the writers store.  points (H, W, 3) float32, image_u8 (H, W, 3) uint8, mask (H, W) bool or None, normal
    (H, W, 3) or None; with a leading batch axis on all of them a list of B tuples.  One host read-back of the counts, as build_mesh_from_map."""
    for name, t in (("points", points), ("image", image_u8), ("normal", normal)):
        if t is not None and isinstance(t, torch.Tensor) and t.shape[-1:] != (3,):
            raise ValueError(f"{name} must be (..., H, W, 3), got {tuple(t.shape)}")
    maps = [points, image_u8, UV] + ([normal] if normal is not None else [])
    tr = [_FLIP_YZ, (None, None), _FLIP_V] + ([_FLIP_YZ] if normal is not None else [])
    batched, res = _compact(maps, mask, bool(tri), points=False, transforms=tr, batched=isinstance(points, torch.Tensor) and points.dim() == 4)
    tuples = [(f,) + tuple(a) for f, a in res]
    return tuples if batched else tuples[0]
