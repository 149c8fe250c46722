"""CPU: the image-mesh entry points of the C ABI (include/moge_hip.h, csrc/mesh.hip) are exported and bound, the workspace size is the documented
arithmetic, and bad arguments come back as MOGE_ERR_INVALID with a message, before anything touches a GPU.  No GPU call is made here: every
call below either is pure arithmetic or is rejected by the argument checks."""
import ctypes as C
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["moge_image_mesh_workspace", "moge_image_mesh_count", "moge_image_mesh_fill"]
INVALID = -1


def last_error(L):
    return (L.lib.moge_last_error() or b"").decode()


def documented_bytes(B, H, W, block_px, span):
    nblk = -(-H * W // block_px)
    nspan = -(-nblk // span)
    return B * (8 * (nblk + nspan + 1) + 5 * H * W)


def test_symbols_are_declared_exported_and_bound():
    from moge_amd import _lib as L
    hdr = open(os.path.join(ROOT, "include", "moge_hip.h")).read()
    for name in NAMES:
        assert re.search(r"\bint\s+" + name + r"\s*\(", hdr), name
        assert name in L.EXPORTS and getattr(L.lib, name).argtypes is not None, name
    assert L.lib.moge_abi_version() == 5                                   # purely additive
    for macro, value in (("MOGE_MESH_MAX_MAPS", L.MESH_MAX_MAPS), ("MOGE_MESH_BLOCK_PX", L.MESH_BLOCK_PX), ("MOGE_MESH_SCAN_SPAN", L.MESH_SCAN_SPAN)):
        assert int(re.search(r"#define\s+" + macro + r"\s+(\d+)", hdr).group(1)) == value, macro
    assert C.sizeof(L.MeshMap) == 2 * C.sizeof(C.c_void_p) + 4 * 4 + 8 * 4
    import moge_amd.mesh as M
    assert (M.BLOCK_PX, M.SCAN_SPAN, M.MAX_MAPS) == (L.MESH_BLOCK_PX, L.MESH_SCAN_SPAN, L.MESH_MAX_MAPS) == (1024, 256, 8)


def test_workspace_is_the_documented_arithmetic():
    from moge_amd import _lib as L
    import moge_amd.mesh as M
    n = C.c_int64(-1)
    for B, H, W in ((1, 70, 67), (3, 1080, 1920), (2, 5, 52429), (1, 1, 1), (0, 4, 4)):
        assert L.lib.moge_image_mesh_workspace(B, H, W, C.byref(n)) == 0
        assert n.value == documented_bytes(B, H, W, M.BLOCK_PX, M.SCAN_SPAN) == M.workspace_bytes(B, H, W), (B, H, W)
    assert documented_bytes(1, 70, 67, 1024, 256) == 8 * (5 + 1 + 1) + 5 * 4690
    assert documented_bytes(3, 1080, 1920, 1024, 256) == 3 * (8 * (2025 + 8 + 1) + 5 * 2073600)
    assert L.lib.moge_image_mesh_workspace(1, 46340, 46340, C.byref(n)) == 0 and n.value > 5 * 46340 * 46340       # the largest square below 2^31 pixels


def test_bad_arguments_are_rejected_with_a_message():
    from moge_amd import _lib as L
    n = C.c_int64(7)
    assert L.lib.moge_image_mesh_workspace(1, 4, 4, None) == INVALID and "null" in last_error(L)
    for B, H, W in ((-1, 4, 4), (1, 0, 4), (1, 4, 0), (1, -3, 4), (65536, 4, 4), (1, 46341, 46341), (1, 65536, 32768), (1, 2 ** 31 - 1, 2)):
        assert L.lib.moge_image_mesh_workspace(B, H, W, C.byref(n)) == INVALID, (B, H, W)
        assert n.value == 0 and "2^31" in last_error(L)
        # the same sizes through the two working calls: rejected by the size check, which comes before any pointer is looked at
        assert L.lib.moge_image_mesh_count(None, B, H, W, 0, None, None, None, None) == INVALID and "moge_image_mesh_count" in last_error(L)
        assert L.lib.moge_image_mesh_fill(B, H, W, None, None, 0, 1, None, None, None) == INVALID and "moge_image_mesh_fill" in last_error(L)
    # good sizes, null pointers (host scratch stands in for device memory: nothing is launched, so nothing dereferences it)
    buf = (C.c_int64 * 64)()
    p = C.addressof(buf)
    assert L.lib.moge_image_mesh_count(None, 1, 4, 4, 0, None, p, p, None) == INVALID and "null" in last_error(L)
    assert L.lib.moge_image_mesh_count(None, 1, 4, 4, 0, p, None, p, None) == INVALID
    assert L.lib.moge_image_mesh_count(None, 1, 4, 4, 0, p, p, None, None) == INVALID
    maps = (L.MeshMap * 9)()
    for m in maps:
        m.data, m.out, m.channels, m.dtype = p, p, 3, L.MESH_F32

    def fill(n_maps=1, tri=1, ws=p, faces=p, offsets=p, arr=maps):
        return L.lib.moge_image_mesh_fill(1, 4, 4, ws, arr, n_maps, tri, faces, offsets, None)
    assert fill(ws=None) == INVALID and "null" in last_error(L)
    assert fill(faces=None) == INVALID and fill(offsets=None) == INVALID and fill(arr=None) == INVALID
    assert fill(n_maps=9) == INVALID and "n_maps" in last_error(L)
    assert fill(n_maps=-1) == INVALID and fill(tri=2) == INVALID
    assert fill(n_maps=0, tri=L.MESH_NO_FACES, faces=None) == INVALID and "nothing to write" in last_error(L)
    for field, value, word in (("channels", 0, "channels"), ("channels", 5, "channels"), ("dtype", 3, "dtype"), ("out", None, "null"), ("data", None, "null")):
        old = getattr(maps[1], field)
        setattr(maps[1], field, value)
        assert fill(n_maps=2) == INVALID and word in last_error(L), field
        setattr(maps[1], field, old)
    maps[0].dtype, maps[0].channels = L.MESH_UV, 3
    assert fill() == INVALID and "uv" in last_error(L)
