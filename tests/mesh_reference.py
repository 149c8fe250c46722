"""An independent restatement of the image mesh and the masked point cloud for the tests of moge_amd.mesh: a plain double loop over the quads
that builds the faces, the used set and the attributes with no cumsum and no fancy indexing.  tests/test_mesh_reference_cpu.py ties it to
`moge_amd.io.build_mesh_from_map` / `masked_point_cloud` (the specification) on the shapes and masks below, so the yardstick of
tests/test_hip_mesh.py does not rest on one implementation.  Also here: those shapes and masks, shared by the CPU and the GPU module.

The shapes sit on the kernel's tiling constants (include/moge_hip.h; moge_amd.mesh exports them and the GPU module asserts they are these):
BLOCK_PX = 1024 consecutive pixels per workgroup of the scan, SCAN_SPAN = 256 workgroup totals per workgroup of the second level, so an image of
more than 256 * 1024 pixels is the smallest that needs the third level to add anything."""
import numpy as np

BLOCK_PX = 1024
SCAN_SPAN = 256

# one pixel under / on / over BLOCK_PX: as a near-square (31 x 33 = 1023, 32 x 32, 25 x 41 = 1025) and as few long rows - a row PAIR has an even
# pixel count, so (2, n) is 1022 / 1024 / 1026 and the odd counts come as 3 x 341 = 1023 and 5 x 205 = 1025
SMALL_SHAPES = [(2, 2), (1, 7), (7, 1), (3, 5), (2, 511), (2, 512), (2, 513), (3, 341), (5, 205), (31, 33), (32, 32), (25, 41), (70, 67)]
# 257 workgroups = the smallest count past one second-level pass (5 x 52429 = 262145 = 256 * 1024 + 1 pixels), and 256 workgroups, exactly one pass
SPAN_SHAPES = [(2, 131072), (5, 52429)]
SHAPES = SMALL_SHAPES + SPAN_SHAPES
assert [-(-h * w // BLOCK_PX) for h, w in SPAN_SHAPES] == [SCAN_SPAN, SCAN_SPAN + 1]


def masks(H, W, seed=0):
    """name -> mask (H, W) bool, or None for the mask=None case.  The boundary island needs a 2 x 2 block whose top row holds the flat indices
    BLOCK_PX - 1 and BLOCK_PX (the last pixel of one workgroup and the first of the next): shapes without one do not get that mask."""
    rng = np.random.default_rng(seed + 1000 * H + W)
    out = {"none": None, "all_true": np.ones((H, W), bool), "all_false": np.zeros((H, W), bool)}
    out["checkerboard"] = (np.add.outer(np.arange(H), np.arange(W)) % 2 == 0)
    for name, (i, j) in {"island_tl": (0, 0), "island_tr": (0, W - 2), "island_bl": (H - 2, 0), "island_br": (H - 2, W - 2)}.items():
        m = np.zeros((H, W), bool)
        m[max(i, 0):max(i, 0) + 2, max(j, 0):max(j, 0) + 2] = True
        out[name] = m
    i, j = divmod(BLOCK_PX - 1, W)
    if i + 1 < H and j + 1 < W:
        m = np.zeros((H, W), bool)
        m[i:i + 2, j:j + 2] = True
        out["island_on_block_boundary"] = m
    m = np.zeros((H, W), bool)
    m[::2] = True
    out["alternate_rows"] = m
    out["random_0.5"] = rng.random((H, W)) < 0.5
    out["random_0.97"] = rng.random((H, W)) < 0.97
    m = np.ones((H, W), bool)
    m[H // 2, W // 3] = False
    out["one_false_pixel"] = m
    return out


def image_mesh(maps, mask=None, tri=True):
    """(faces int32, *attributes) as moge_amd.io.build_mesh_from_map returns them, by loops."""
    H, W = maps[0].shape[:2]
    m = [[True] * W for _ in range(H)] if mask is None else np.asarray(mask).astype(bool).tolist()
    used = [[False] * W for _ in range(H)]
    quads = []
    for i in range(H - 1):
        for j in range(W - 1):
            if m[i][j] and m[i + 1][j] and m[i][j + 1] and m[i + 1][j + 1]:
                quads.append((i, j))
                used[i][j] = used[i + 1][j] = used[i][j + 1] = used[i + 1][j + 1] = True
    new, order = {}, []
    for i in range(H):
        for j in range(W):
            if used[i][j]:
                new[(i, j)] = len(order)
                order.append((i, j))
    corners = [(new[(i, j)], new[(i + 1, j)], new[(i + 1, j + 1)], new[(i, j + 1)]) for i, j in quads]
    if tri:
        rows = [(a, b, c) for a, b, c, d in corners] + [(a, c, d) for a, b, c, d in corners]
        faces = np.array(rows, dtype=np.int32).reshape(len(rows), 3)
    else:
        faces = np.array(corners, dtype=np.int32).reshape(len(corners), 4)
    return (faces,) + tuple(_rows(x, order) for x in maps)


def point_cloud(points, mask, image=None, normal=None):
    """(vertices, colors or None, normals or None) as moge_amd.io.masked_point_cloud returns them, by loops."""
    H, W = mask.shape
    m = np.asarray(mask).astype(bool).tolist()
    order = [(i, j) for i in range(H) for j in range(W) if m[i][j]]
    flip = np.array([1, -1, -1], dtype=np.float32)
    v = _rows(points, order).astype(np.float32) * flip
    c = None
    if image is not None:
        c = _rows(image, order)
        c = c.astype(np.float32) / np.float32(255) if image.dtype == np.uint8 else c.astype(np.float32)
    n = None if normal is None else _rows(normal, order).astype(np.float32) * flip
    return v, c, n


def _rows(x, order):
    """Rows (i, j) of an (H, W[, C]) map in the given order, copied as bytes (so every bit pattern survives)."""
    x = np.ascontiguousarray(x)
    W, C = x.shape[1], int(np.prod(x.shape[2:], dtype=np.int64))
    buf, size = x.tobytes(), C * x.dtype.itemsize
    picked = b"".join([buf[(i * W + j) * size:(i * W + j + 1) * size] for i, j in order])
    return np.frombuffer(picked, dtype=x.dtype).reshape(len(order), C).copy()


def bits(a):
    """float32 array -> its int32 bit patterns (what 'bit for bit' compares)."""
    a = np.ascontiguousarray(a)
    assert a.dtype == np.float32, a.dtype
    return a.view(np.int32)
