"""float64 numpy references, with per-element error bounds, for the kernels at the encoder's entrance (csrc/elementwise.hip: preprocess, posembed,
resize_bicubic_aa; csrc/gemm.hip: the EPI_PATCH, EPI_QKV and EPI_CONVT epilogues of the parity kernels).

Every reference is written from the definition of the operation (ATen's UpSampleKernel.cpp / UpSample.h for the resizes, the reference model's modules
for the rest), not from the kernel, and is tied on the CPU to an independent torch float64 formulation in tests/test_entrance_reference_cpu.py.
tests/test_hip_entrance_kernels.py compares element by element: |got - ref| <= bound(element).  Conventions (u = 2^-24, ulp32, rounding of the inputs
to the storage type BEFORE the reference runs, Higham's any-order summation bound) are those of tests/tail_reference.py.

Antialiased resize (F.interpolate(..., antialias=True), bilinear = triangle filter, interp_size 2; bicubic = cubic convolution a = -0.5, interp_size 4)
----------------------------------------------------------------------------------------------------------------------------------------------------
Per axis ATen forms, in the image's scalar type (float32 here: _compute_indices_min_size_weights_aa):
  scale = f32(in) / f32(out)      support = interp_size / 2 * max(scale, 1)      invscale = 1 / max(scale, 1)      center = scale * (o + 0.5)
  lo = max(int(center - support + 0.5), 0)      hi = min(int(center + support + 0.5), in)      w_j = filter((j + lo - center + 0.5) * invscale)
`aa_axis` does exactly that in float32.  Everything after it is float64: S = sum_j w_j, wn_j = w_j / S, out = sum_j wny_j sum_i wnx_i v_ji.
With A = sum_j |wny_j| sum_i |wnx_i| |v_ji| the bound of the resized value r is e_r = e_sum + e_coord (+ e_w for the cubic filter):

  e_sum = (ny + nx + 8) u A.  ny + nx: each pass accumulates its n taps in fp32, n u sum|terms| in any order.  + 8: per axis the product that forms the
      filter argument, the rounding of the filter value, the division by S and the product wn v (4 x 2 axes).  Two things this term does NOT derive and
      takes as ASSUMPTIONS: (i) the kernel sums S in fp32 where the reference sums it in float64 - up to (n - 1) u S more in the worst order - and that is
      taken to fit in the taps term with the accumulation (for the symmetric filters here the prefix sums of S average S / 2; the accumulation loses its
      full n u only when the first tap, the smallest of a range, carries the mass); (ii) the rounding of a float32 filter value is taken as relative to the
      value, which holds for the triangle 1 - |x| but for a cubic polynomial only as far as its Horner intermediates (up to 8 |a|) do not dwarf the value.
      The kernels' share of the bound on an MI355X (tests/test_hip_entrance_kernels.py's docstring) is the evidence that neither assumption is strained.
  e_w (cubic filters only; `weight_term=False` leaves it out and gives the plain three-part form above, which the tests also record): where (ii) fails.
      The reference and a kernel evaluate the same Horner form in float32 but the compiler may contract each of its three multiply-adds into an FMA, which
      drops the rounding of that product: at most u |product|, carried down the chain by the factors x <= 2 that follow.  With a = -0.5 the products are
      <= 1, 3, 2.1 on 1 <= |x| < 2 (4 u + 6 u + 2.1 u -> W_OUT = 12 u) and <= 1.5, 1.04, 1 on |x| < 1 (W_IN = 4 u); with A = -0.75 (position embedding)
      <= 1.5, 4.5, 3.1 (6 u + 9 u + 3.1 u -> W_OUT = 18 u) and W_IN = 4 u.  These are ABSOLUTE errors of a weight, so near the zeros of the filter they are
      not covered by a term relative to |w v|.  A weight error dw_j moves wn_j by dw_j / S - wn_j dS / S:
        e_w(axis) = sum_j W_j |v_j| / |S| + (sum_j W_j / |S|) sum_j |wn_j v_j|         (the other axis' |wn| applied on top)
      That a correct fp32 implementation needs it: torch's own float32 antialiased bicubic is 1.3 - 1.4 x the three-part form away from the reference when
      up-scaling (7 x 5 -> 14 x 14, 40 x 40 -> 62 x 63 and 54 x 54) and at 0.14 of the bound with e_w; torch's own float32 bicubic position embedding is up to 3.9 x the three-part form away from the
      reference at 60 x 60 (rows 0-2, 5, 6, where src + 0.5 < 1 makes the coordinate term vanish and 16 u A is all that is left), and inside the bound with
      e_w (tests/test_entrance_reference_cpu.py).  The triangle filter has no such term: 1 - |x| is one rounding of a value <= 1.
  e_coord: `scale * (o + 0.5)` feeds a subtraction (lo, hi, the filter argument), which the compiler may contract into one FMA: the centre moves by up to
      one ulp32(center).  In filter units that is ulp32(center) invscale, and the normalised weights re-distribute at most that share of the range of v:
      e_coord(axis) = ulp32(center) invscale spread,   spread = max - min of v over the 2-D tap window.
Normalisation o = (r - mean) / sd with the float32 constants: e_o = e_r / sd + 2 u |o| (the subtraction and the correctly rounded division).
An fp16 store adds 2^-11 |ref| + 2^-25 (half an ulp, or half the smallest subnormal).  round16 and an fp16 input round the image before the reference runs.
At scale 1 the two taps of an axis get the weights 1 and 0 EXACTLY (arguments 0 and 1): r = v, and o is two roundings away from the exact quotient - within
1 ulp32 of f32((v - mean) / sd).

preprocess, aa = 0 (onnx_compatible_mode): ATen's plain bilinear resize, two taps per axis: tail_reference.bilinear_taps / resize, e_r = 8 u A + its coordinate
term (tail_reference's docstring), then the normalisation above.

resize_bicubic_aa: the antialiased resize with the cubic filter, no normalisation; round16 rounds the input AND the stored result to fp16 (a .half()
MoGe-1 keeps the resized image in fp16): + 2^-11 |ref| + 2^-25.

Position embedding (vision_transformer.py:187-221)
--------------------------------------------------
Bicubic, A = -0.75, align_corners = False, taps clamped to the 37 x 37 grid.  In float32 as ATen does: src = rscale * (o + 0.5) - 0.5, i = floor(src), t = src - i,
weights cc2(t + 1), cc1(t), cc1(1 - t), cc2((1 - t) + 1) with cc1(x) = ((A + 2) x - (A + 3)) x x + 1, cc2(x) = ((A x - 5 A) x + 8 A) x - 4 A.  rscale as the launcher
and ATen compute it: plain mode f32(1 / ((n + 0.1) / 37)) - interpolate() is given scale_factor = (n + 0.1) / 37 as a double and uses f32(1 / scale_factor) -;
size mode f32(37) / f32(n).  float64 after that.  A = sum |wy| |wx| |v|:
  e = (4 + 4 + 8) u A + e_coord + e_w          (the same shape: taps of the two passes + 8, with assumption (ii) above for the float32 weights, A = -0.75)
  e_coord: the FMA moves src by ulp32(src + 0.5) per axis (no antialiasing: the inverse scale is 1):
      e_coord(axis) = ulp32(src + 0.5) spread, with the spread over taps i - 2 .. i + 2 of both axes (src may cross into the next cell).
  e_w as above with W = (18, 4, 4, 18) u for the four taps and S = 1 (the weights sum to 1 by construction: no normalisation term).
Row 0 (the cls position) and, in plain mode, the whole 37 x 37 grid are copies: bit-equal.

GEMM epilogues
--------------
Inputs rounded to the storage type first; the MFMA chain accumulates along K in fp32, K terms being the fully sequential worst case:
  patch   ref = sum_k a_k w_k + bias + pos[1 + p]     e = (K + 3) u (sum_k |a_k w_k| + |bias| + |pos|)         cls rows: f32(cls + pos[0]) exactly
  qkv     ref = sum_k a_k w_k + bias                  e = (K + 3) u (sum |a w| + |bias|); q: times qscale, + 1 u |q|; fp16 storage: + 2^-11 |ref| + 2^-25
  convt, uv at the input pixel (MoGe-1, v1.py:118-121): ref = sum_k a_k w_k + bias[n] + wu[n] u(x) + wv[n] v(y), u / v = torch.linspace in fp32
          e = (K + 6) u (sum |a w| + |bias| + |wu u| + |wv v|) + 3 (|wu| ulp32(max |u|) + |wv| ulp32(max |v|))      (linspace: tail_reference's 3 ulp)
"""
import numpy as np

from tail_reference import U32, resize, ulp32

MEAN = np.array([0.485, 0.456, 0.406], dtype=np.float32).astype(np.float64)
SD = np.array([0.229, 0.224, 0.225], dtype=np.float32).astype(np.float64)
PATCH_K = 3 * 14 * 14
F32 = np.float32

INTERP_SIZE = {"bilinear": 2, "bicubic": 4}
AA_W_IN, AA_W_OUT = 4.0, 12.0          # absolute error of a float32 cubic filter value (a = -0.5), in units of u: |x| < 1, 1 <= |x| < 2
POS_W = (18.0, 4.0, 4.0, 18.0)         # ... of the four bicubic weights at A = -0.75


def _cc1(x, A):
    F = type(A)
    return ((A + F(2)) * x - (A + F(3))) * x * x + F(1)


def _cc2(x, A):
    F = type(A)
    return ((A * x - F(5) * A) * x + F(8) * A) * x - F(4) * A


def _filter32(x, kind):
    """ATen's aa filters on a float32 array, in float32."""
    x = np.abs(x)
    F = x.dtype.type
    if kind == "bilinear":
        return np.where(x < F(1), F(1) - x, F(0)).astype(F)
    A = F(-0.5)
    return np.where(x < F(1), _cc1(x, A), np.where(x < F(2), _cc2(x, A), F(0))).astype(F)


def aa_axis(n_in, n_out, kind, form_dtype=np.float32):
    """One axis of ATen's antialiased resize: float32 range, centre and unnormalised weights.  Returns the (n_out, n_in) float64 matrix of normalised weights
    `Wn` and per output index lo, hi, n (taps), S, center, invscale (float64).
    form_dtype = np.float64 forms them the way ATen does for a double image (the CPU tie of the structure; no kernel test uses it)."""
    interp, T = INTERP_SIZE[kind], form_dtype
    scale = T(n_in) / T(n_out)
    support = T(interp * 0.5) * scale if scale >= 1 else T(interp * 0.5)
    invscale = T(1) / scale if scale >= 1 else T(1)
    o = np.arange(n_out, dtype=T)
    center = scale * (o + T(0.5))
    lo = np.maximum((center - support + T(0.5)).astype(np.int64), 0)
    hi = np.minimum((center + support + T(0.5)).astype(np.int64), n_in)
    n = hi - lo
    assert center.dtype == T and (n >= 1).all()
    j = np.arange(n_in)
    win = (j[None, :] >= lo[:, None]) & (j[None, :] < hi[:, None])
    arg = (j[None, :].astype(F32) - center[:, None] + T(0.5)) * invscale          # (j + lo) is the input index itself
    assert arg.dtype == T
    w = np.where(win, _filter32(arg, kind), T(0)).astype(np.float64)
    S = w.sum(-1)
    wabs = np.where(win, np.where(np.abs(arg) < 1, AA_W_IN, AA_W_OUT), 0.0) * U32 if kind == "bicubic" else np.zeros_like(w)
    return dict(Wn=w / S[:, None], Wabs=wabs / np.abs(S)[:, None], lo=lo, hi=hi, n=n.astype(np.float64), S=S, center=center.astype(np.float64), invscale=float(invscale))


def _window_spread(v, ay, ax):
    """max - min of v (B,C,H,W) over the tap window of every output pixel: (B,C,OH,OW)."""
    B, C, H, W = v.shape
    OH, OW = len(ay["lo"]), len(ax["lo"])
    cmax = np.empty((B, C, H, OW))
    cmin = np.empty((B, C, H, OW))
    for p in range(OW):
        s = v[..., ax["lo"][p]:ax["hi"][p]]
        cmax[..., p], cmin[..., p] = s.max(-1), s.min(-1)
    out = np.empty((B, C, OH, OW))
    for o in range(OH):
        out[:, :, o] = cmax[:, :, ay["lo"][o]:ay["hi"][o]].max(2) - cmin[:, :, ay["lo"][o]:ay["hi"][o]].min(2)
    return out


def aa_resize(v, OH, OW, kind, parts=False, form_dtype=np.float32, weight_term=True):
    """Antialiased resize of v (B,C,H,W) float64 (already rounded to what the kernel reads) to (B,C,OH,OW): (value, bound); parts: also (e_sum, e_coord,
    e_w).  weight_term=False: the three-part form e_sum + e_coord."""
    v = np.asarray(v, dtype=np.float64)
    ay, ax = aa_axis(v.shape[2], OH, kind, form_dtype), aa_axis(v.shape[3], OW, kind, form_dtype)

    def apply(my, m, mx):
        return np.einsum("oh,bchw,pw->bcop", my, m, mx, optimize=True)

    ref = apply(ay["Wn"], v, ax["Wn"])
    A = apply(np.abs(ay["Wn"]), np.abs(v), np.abs(ax["Wn"]))
    ny, nx = ay["n"][None, None, :, None], ax["n"][None, None, None, :]
    e_sum = (ny + nx + 8) * U32 * A
    cy, cx = ulp32(ay["center"]) * ay["invscale"], ulp32(ax["center"]) * ax["invscale"]
    e_coord = (cy[None, None, :, None] + cx[None, None, None, :]) * _window_spread(v, ay, ax)
    e_w = np.zeros_like(A)
    if kind == "bicubic" and weight_term:
        aWy, aWx, av = np.abs(ay["Wn"]), np.abs(ax["Wn"]), np.abs(v)
        e_w = (apply(aWy, av, ax["Wabs"]) + ax["Wabs"].sum(-1)[None, None, None, :] * A) + (apply(ay["Wabs"], av, aWx) + ay["Wabs"].sum(-1)[None, None, :, None] * A)
    if parts:
        return ref, e_sum + e_coord + e_w, e_sum, e_coord, e_w
    return ref, e_sum + e_coord + e_w


def normalise(r, e_r, out_fp16=False):
    """o = (r - mean) / sd per channel of (B,3,H,W), with the propagated bound."""
    m, s = MEAN[None, :, None, None], SD[None, :, None, None]
    o = (r - m) / s
    e = e_r / s + 2 * U32 * np.abs(o)
    if out_fp16:
        e = e + 2.0 ** -11 * np.abs(o) + 2.0 ** -25
    return o, e


def round_image(img, in_fp16=False, round16=False):
    """The image as the kernel reads it, float64."""
    img = np.asarray(img, dtype=np.float32)
    return (img.astype(np.float16) if (in_fp16 or round16) else img).astype(np.float64)


def preprocess(img, rows, cols, aa=True, in_fp16=False, round16=False, out_fp16=False):
    """modules.py:121-122: resize to (14 rows, 14 cols) (antialiased bilinear, or plain bilinear with aa = False) + ImageNet normalisation.
    img (B,3,H,W) fp32 -> (ref, bound) (B,3,14 rows,14 cols) float64."""
    v = round_image(img, in_fp16, round16)
    OH, OW = 14 * rows, 14 * cols
    if aa:
        r, e = aa_resize(v, OH, OW, "bilinear")
    else:
        t = v.transpose(0, 2, 3, 1)
        val, A, coord = resize(t, np.abs(t), OH, OW)
        r, e = val.transpose(0, 3, 1, 2), (8 * U32 * A + coord).transpose(0, 3, 1, 2)
    return normalise(r, e, out_fp16)


def patchify(x, ldk=PATCH_K, fill=0.0):
    """(B,3,14 rows,14 cols) -> the im2col matrix (B rows cols, ldk) of the 14 x 14 stride-14 patch embedding (patch_embed.py:75): row b Np + py cols + px,
    column c 196 + iy 14 + ix; columns [588, ldk) = fill."""
    B, C, OH, OW = x.shape
    rows, cols = OH // 14, OW // 14
    m = x.reshape(B, C, rows, 14, cols, 14).transpose(0, 2, 4, 1, 3, 5).reshape(B * rows * cols, C * 196)
    out = np.full((B * rows * cols, ldk), fill, dtype=x.dtype)
    out[:, :PATCH_K] = m
    return out


def unpatchify(m, B, rows, cols):
    """Inverse of patchify on the first 588 columns."""
    return m[:, :PATCH_K].reshape(B, rows, cols, 3, 14, 14).transpose(0, 3, 1, 4, 2, 5).reshape(B, 3, rows * 14, cols * 14)


def resize_bicubic_aa(img, OH, OW, in_fp16=False, round16=False, weight_term=True):
    """v1.py:275 on (B,3,H,W) fp32 -> (ref, bound)."""
    r, e = aa_resize(round_image(img, in_fp16, round16), OH, OW, "bicubic", weight_term=weight_term)
    if round16:
        e = e + 2.0 ** -11 * np.abs(r) + 2.0 ** -25
    return r, e


# ---------------------------------------------------------------------------------------------------------------------
# position embedding
# ---------------------------------------------------------------------------------------------------------------------
POS_M = 37


def pos_rscale(n, size_mode):
    return F32(POS_M) / F32(n) if size_mode else F32(1.0 / ((n + 0.1) / POS_M))


def _pos_axis(n, size_mode):
    rs = pos_rscale(n, size_mode)
    o = np.arange(n, dtype=np.float32)
    src = rs * (o + F32(0.5)) - F32(0.5)
    fl = np.floor(src)
    t = src - fl
    A = F32(-0.75)
    x2 = F32(1) - t
    w = np.stack([_cc2(t + F32(1), A), _cc1(t, A), _cc1(x2, A), _cc2(x2 + F32(1), A)], -1)
    assert src.dtype == t.dtype == w.dtype == np.float32
    i = fl.astype(np.int64)
    idx = np.clip(i[:, None] + np.arange(-1, 3)[None, :], 0, POS_M - 1)
    Wm = np.zeros((n, POS_M))
    for k in range(4):
        np.add.at(Wm, (np.arange(n), idx[:, k]), w[:, k].astype(np.float64))          # clamped taps may coincide: their weights add
    aW = np.zeros((n, POS_M))
    Wabs = np.zeros((n, POS_M))
    for k in range(4):
        np.add.at(aW, (np.arange(n), idx[:, k]), np.abs(w[:, k]).astype(np.float64))
        np.add.at(Wabs, (np.arange(n), idx[:, k]), POS_W[k] * U32)
    lo, hi = np.clip(i - 2, 0, POS_M - 1), np.clip(i + 2, 0, POS_M - 1) + 1
    return dict(W=Wm, aW=aW, Wabs=Wabs, lo=lo, hi=hi, src=src.astype(np.float64))


def posembed(pos, rows, cols, size_mode=False, weight_term=True):
    """pos (1 + 37 * 37, D) fp32 -> (ref, bound) (1 + rows cols, D) float64; the bound of the copied elements is 0.  weight_term=False: the three-part form."""
    pos32 = np.asarray(pos, dtype=np.float32)
    D = pos32.shape[1]
    ref = np.empty((1 + rows * cols, D))
    e = np.zeros_like(ref)
    ref[0] = pos32[0]
    if not size_mode and rows == POS_M and cols == POS_M:
        ref[1:] = pos32[1:]
        return ref, e
    g = pos32[1:].astype(np.float64).reshape(POS_M, POS_M, D).transpose(2, 0, 1)[None]          # (1, D, 37, 37)
    ay, ax = _pos_axis(rows, size_mode), _pos_axis(cols, size_mode)

    def apply(my, m, mx):
        return np.einsum("oh,bchw,pw->bcop", my, m, mx, optimize=True)

    val = apply(ay["W"], g, ax["W"])
    ag = np.abs(g)
    A = apply(ay["aW"], ag, ax["aW"])
    spread = _window_spread(g, ay, ax)
    cy = ulp32(ay["src"] + 0.5)
    cx = ulp32(ax["src"] + 0.5)
    e_w = apply(ay["aW"], ag, ax["Wabs"]) + apply(ay["Wabs"], ag, ax["aW"]) if weight_term else 0.0
    bound = 16 * U32 * A + e_w + (cy[None, None, :, None] + cx[None, None, None, :]) * spread
    ref[1:] = val[0].transpose(1, 2, 0).reshape(rows * cols, D)
    e[1:] = bound[0].transpose(1, 2, 0).reshape(rows * cols, D)
    return ref, e


# ---------------------------------------------------------------------------------------------------------------------
# GEMM epilogues
# ---------------------------------------------------------------------------------------------------------------------
def to_storage(x, prec):
    x = np.asarray(x, dtype=np.float32)
    return (x.astype(np.float16) if prec == 1 else x).astype(np.float64)


def gemm_mag(A, W, prec):
    """(sum_k a_k w_k, sum_k |a_k w_k|) in float64 of the inputs rounded to the storage type."""
    a, w = to_storage(A, prec), to_storage(W, prec)
    return a @ w.T, np.abs(a) @ np.abs(w).T


def patch_embed(A, W, bias, pos, cls, B, Np, Ntok, xres_fill, prec):
    """The fp32 residual stream (B Ntok, N) after the patch-embedding epilogue: (ref, bound); rows the epilogue does not own keep xres_fill with bound 0;
    the cls rows are the float32 sum cls + pos[0], bound 0."""
    acc, mag = gemm_mag(A, W, prec)
    K, N = np.shape(A)[1], np.shape(W)[0]
    bias64, pos32 = np.asarray(bias, dtype=np.float64), np.asarray(pos, dtype=np.float32)
    ref = np.array(xres_fill, dtype=np.float64).reshape(B * Ntok, N).copy()
    e = np.zeros_like(ref)
    for b in range(B):
        rows = slice(b * Ntok + 1, b * Ntok + 1 + Np)
        pe = pos32[1:1 + Np].astype(np.float64)
        ref[rows] = acc[b * Np:(b + 1) * Np] + bias64[None] + pe
        e[rows] = (K + 3) * U32 * (mag[b * Np:(b + 1) * Np] + np.abs(bias64)[None] + np.abs(pe))
        if cls is not None:
            ref[b * Ntok] = (np.asarray(cls, dtype=np.float32) + pos32[0]).astype(np.float64)
    return ref, e


def qkv(A, W, bias, B, Ntok, nh, qscale, prec):
    """q, k (B,nh,Ntok,64) and v^T (B,nh,64,Ntok) of attention.py:72-74 (q times qscale): dict name -> (ref, bound)."""
    acc, mag = gemm_mag(A, W, prec)
    K = np.shape(A)[1]
    b64 = np.asarray(bias, dtype=np.float64)
    val = (acc + b64[None]).reshape(B, Ntok, 3, nh, 64).transpose(2, 0, 3, 1, 4)
    e = ((K + 3) * U32 * (mag + np.abs(b64)[None])).reshape(B, Ntok, 3, nh, 64).transpose(2, 0, 3, 1, 4)
    qs = float(F32(qscale))
    out = {"q": (val[0] * qs, e[0] * qs + U32 * np.abs(val[0] * qs)), "k": (val[1], e[1]), "vT": (val[2].transpose(0, 1, 3, 2), e[2].transpose(0, 1, 3, 2))}
    if prec == 1:
        out = {k: (r, b + 2.0 ** -11 * np.abs(r) + 2.0 ** -25) for k, (r, b) in out.items()}
    return out


def linspace32(a, b, n):
    """torch.linspace(a, b, n) in float32 (ATen: start + step i below the middle, end - step (n - 1 - i) from it on, each ONE fused multiply-add: the
    product of two float32 numbers is exact in float64), as float64."""
    a, b = F32(a), F32(b)
    step = np.float64((b - a) / F32(n - 1)) if n > 1 else 0.0
    i = np.arange(n)
    lo = (np.float64(a) + step * i).astype(np.float32)
    hi = (np.float64(b) - step * (n - 1 - i)).astype(np.float32)
    return np.where((i < n // 2) | (n == 1), lo, hi).astype(np.float64)          # a single step is `start`


def convt_uv_in(A, W, bias, wu, wv, uv_range, B, pixH, pixW, Cout, prec):
    """ConvTranspose2d(k2, s2) of an input that carries the uv planes as two extra channels (v1.py:118-121), as the GEMM sees it: A (B pixH pixW, K),
    W (4 Cout, K) with row n = (dy 2 + dx) Cout + co, wu / wv (4 Cout) the weights of the two uv channels.  -> (ref, bound) (B, 2 pixH, 2 pixW, Cout)."""
    acc, mag = gemm_mag(A, W, prec)
    K = np.shape(A)[1]
    u0, u1, v0, v1 = uv_range
    u, v = linspace32(u0, u1, pixW), linspace32(v0, v1, pixH)
    b64, wu64, wv64 = (np.asarray(t, dtype=np.float64) for t in (bias, wu, wv))
    uu = np.broadcast_to(u[None, None, :], (B, pixH, pixW)).reshape(-1, 1)
    vv = np.broadcast_to(v[None, :, None], (B, pixH, pixW)).reshape(-1, 1)
    val = acc + b64[None] + wu64[None] * uu + wv64[None] * vv
    e = (K + 6) * U32 * (mag + np.abs(b64)[None] + np.abs(wu64[None] * uu) + np.abs(wv64[None] * vv))
    e = e + 3 * (np.abs(wu64)[None] * ulp32(max(abs(u0), abs(u1))) + np.abs(wv64)[None] * ulp32(max(abs(v0), abs(v1))))
    if prec == 1:
        e = e + 2.0 ** -11 * np.abs(val) + 2.0 ** -25

    def shuffle(t):
        return t.reshape(B, pixH, pixW, 2, 2, Cout).transpose(0, 1, 3, 2, 4, 5).reshape(B, 2 * pixH, 2 * pixW, Cout)

    return shuffle(val), shuffle(e)
