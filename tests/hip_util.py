"""ctypes helpers for the per-kernel C-ABI test entry points (tests only)."""
import contextlib

import torch

from moge_amd import _lib as L


@contextlib.contextmanager
def experiments_library():
    """Every helper here, L.tune and L.check call the --experiments copy of the library (built by build() beside the product one) inside
    the block, the product library again after it."""
    prev = L.lib
    L.lib = L.experiments_lib()
    try:
        yield
    finally:
        L.lib = prev


def _p(t):
    return None if t is None else t.data_ptr()


def _f(t):
    return t.detach().to("cuda", torch.float32).contiguous()


def st():
    return L.stream_ptr()


def gemm(prec, A, W, bias=None, act=0):
    A, W = _f(A), _f(W)
    bias = None if bias is None else _f(bias)
    M, K = A.shape
    N = W.shape[0]
    C = torch.empty((M, N), device="cuda", dtype=torch.float32)
    L.check(L.lib.moge_test_gemm(prec, _p(A), _p(W), _p(bias), _p(C), M, N, K, act, st()))
    return C


TG_STORE, TG_RESID, TG_QKV, TG_CONVT, TG_PATCH = 0, 1, 2, 3, 4


def gemm_ex(kind, A, W, bias, prec=1, act=0, ln_mr=None, ln_c=None, uv=None, pix=None, Cout=0, xres=None, gamma=None, want_x16=False,
            nh=0, Ntok=0, qscale=1.0, x16_stream=None, want_part=True, pos=None, cls=None, Np=0, v_prefill=None, uv_in=False, raw=False):
    """One GEMM through a fused epilogue (moge_test_gemm_ex).  All tensors fp32 on the GPU.  Returns a dict of outputs.
    TG_PATCH: xres (B Ntok, N) is the pre-filled residual stream, pos (1 + Np, N), cls (N) or None.  TG_QKV with v_prefill (B, nh, 64, Npad): the
    transposed V of the fp32 path, returned whole.  TG_CONVT with uv and uv_in: the uv term at the input pixel, wu / wv by GEMM column.
    raw=True returns the status code instead of raising."""
    import ctypes as C
    A, W = _f(A), _f(W)
    M, K = A.shape
    N = W.shape[0]
    a = L.TestGemmArgs()
    keep = [A, W]

    def dev(t):
        if t is None:
            return None
        t = _f(t)
        keep.append(t)
        return t.data_ptr()

    a.precision, a.kind, a.act, a.M, a.N, a.K = prec, kind, act, M, N, K
    a.A, a.W, a.bias = A.data_ptr(), W.data_ptr(), dev(bias)
    a.ln_mr, a.ln_c = dev(ln_mr), dev(ln_c)
    if pix is not None:
        a.pixW, a.pixH = pix
    if uv is not None:
        wu, wv, u0, u1, v0, v1 = uv
        a.wu, a.wv, a.u0, a.u1, a.v0, a.v1 = dev(wu), dev(wv), u0, u1, v0, v1
    out = {}
    if kind in (TG_STORE, TG_CONVT):
        out["out"] = torch.empty((M, N), device="cuda", dtype=torch.float32)
        a.out, a.Cout, a.uv_in = out["out"].data_ptr(), Cout, int(bool(uv_in))
    elif kind == TG_PATCH:
        out["xres"] = _f(xres).clone()
        a.xres, a.pos, a.cls, a.Np, a.Ntok = out["xres"].data_ptr(), dev(pos), dev(cls), Np, Ntok
    elif kind == TG_RESID and x16_stream is not None:
        # fp16 residual stream of a `.half()` model (EPK_RESID16): x16 in / out (fp32 values that are exact fp16 numbers), xres = NULL
        out["x16"] = _f(x16_stream).clone()
        a.x16_out, a.gamma = out["x16"].data_ptr(), dev(gamma)
        if want_part:
            out["ln_part"] = torch.full((M, N // 32, 2), float("nan"), device="cuda", dtype=torch.float32)      # the kernel writes the caller's buffer: a group it skips stays NaN
            a.ln_part_out = out["ln_part"].data_ptr()
    elif kind == TG_RESID:
        out["xres"] = _f(xres).clone()
        a.xres, a.gamma = out["xres"].data_ptr(), dev(gamma)
        if want_x16:
            out["x16"] = torch.empty((M, N), device="cuda", dtype=torch.float32)
            out["ln_part"] = torch.full((M, N // 32, 2), float("nan"), device="cuda", dtype=torch.float32)      # the kernel writes the caller's buffer: a group it skips stays NaN
            a.x16_out, a.ln_part_out = out["x16"].data_ptr(), out["ln_part"].data_ptr()
    elif kind == TG_QKV:
        B = M // Ntok
        for k in ("q", "k", "v"):
            out[k] = torch.empty((B, nh, Ntok, 64), device="cuda", dtype=torch.float32)
        if v_prefill is not None:
            assert tuple(v_prefill.shape) == (B, nh, 64, (Ntok + 63) // 64 * 64)
            out["v"], a.v_transposed = _f(v_prefill).clone(), 1
        a.q_out, a.k_out, a.v_out = out["q"].data_ptr(), out["k"].data_ptr(), out["v"].data_ptr()
        a.nh, a.Ntok, a.qscale = nh, Ntok, qscale
    rc = L.lib.moge_test_gemm_ex(C.byref(a), st())
    if raw:
        return rc
    L.check(rc)
    return out


def gemm_fused_ln(A, W, bias, gamma, stream, half_stream=True, bufs=None, raw=False):
    """The EPI_RESID GEMM with the LN statistics finalised inside the launch (moge_test_gemm_fused_ln).  `stream` (M, N) is the residual stream before the
    launch: the fp16 stream of a `.half()` model (half_stream) or the fp32 one.  bufs: the dict a previous call returned - its ln_part, ln_mr and counter
    buffers are handed to the kernel again as they are.  Returns dict(stream, x16, ln_part, ln_mr, cnt); cnt has two guard entries behind the counters."""
    A, W, bias, gamma = _f(A), _f(W), _f(bias), _f(gamma)
    M, K = A.shape
    N = W.shape[0]
    o = {}
    if bufs is None:
        o["ln_part"] = torch.full((M, N // 32, 2), float("nan"), device="cuda", dtype=torch.float32)
        o["ln_mr"] = torch.full((M, 2), float("nan"), device="cuda", dtype=torch.float32)
        o["cnt"] = torch.zeros(((M + 63) // 64 + 2,), device="cuda", dtype=torch.int32)
    else:
        o.update({k: bufs[k] for k in ("ln_part", "ln_mr", "cnt")})
    x = _f(stream).clone()
    if half_stream:
        xres, o["x16"] = None, x
    else:
        xres, o["x16"] = x, torch.full((M, N), float("nan"), device="cuda", dtype=torch.float32)
    o["stream"] = x
    rc = L.lib.moge_test_gemm_fused_ln(_p(A), _p(W), _p(bias), _p(gamma), _p(xres), _p(o["x16"]), _p(o["ln_part"]), _p(o["ln_mr"]), _p(o["cnt"]), M, N, K, st())
    if raw:
        return rc
    L.check(rc)
    return o


def layernorm(prec, x, w, b):
    x, w, b = _f(x), _f(w), _f(b)
    y = torch.empty_like(x)
    L.check(L.lib.moge_test_layernorm(prec, _p(x), _p(w), _p(b), _p(y), x.shape[0], x.shape[1], st()))
    return y


def attention(prec, q, k, v):
    q, k, v = _f(q), _f(k), _f(v)
    B, nh, N, _ = q.shape
    o = torch.empty((B, N, nh * 64), device="cuda", dtype=torch.float32)
    L.check(L.lib.moge_test_attention(prec, _p(q), _p(k), _p(v), _p(o), B, nh, N, st()))
    return o


def conv3x3(prec, x_nhwc, w, bias, relu_in=False, up2=False):
    x, w, bias = _f(x_nhwc), _f(w), _f(bias)
    B, H, W, Cin = x.shape
    Cout = w.shape[0]
    Ho, Wo = (2 * H, 2 * W) if up2 else (H, W)
    y = torch.empty((B, Ho, Wo, Cout), device="cuda", dtype=torch.float32)
    L.check(L.lib.moge_test_conv3x3(prec, _p(x), _p(w), _p(bias), _p(y), B, H, W, Cin, Cout, (1 if relu_in else 0) | (2 if up2 else 0), st()))
    return y


def convt2x2(prec, x_nhwc, w, bias):
    x, w, bias = _f(x_nhwc), _f(w), _f(bias)
    B, H, W, Cin = x.shape
    Cout = w.shape[1]
    y = torch.empty((B, 2 * H, 2 * W, Cout), device="cuda", dtype=torch.float32)
    L.check(L.lib.moge_test_convt2x2(prec, _p(x), _p(w), _p(bias), _p(y), B, H, W, Cin, Cout, st()))
    return y


def preprocess(img, rows, cols):
    img = _f(img)
    B, _, H, W = img.shape
    y = torch.empty((B, 3, rows * 14, cols * 14), device="cuda", dtype=torch.float32)
    L.check(L.lib.moge_test_preprocess(_p(img), _p(y), B, H, W, rows, cols, st()))
    return y


def posembed(pos, rows, cols):
    pos = _f(pos)
    D = pos.shape[-1]
    y = torch.empty((1 + rows * cols, D), device="cuda", dtype=torch.float32)
    L.check(L.lib.moge_test_posembed(_p(pos), _p(y), D, rows, cols, st()))
    return y


def posembed_ex(pos, rows, cols, size_mode):
    pos = _f(pos)
    D = pos.shape[-1]
    y = torch.full((1 + rows * cols, D), float("nan"), device="cuda", dtype=torch.float32)
    L.check(L.lib.moge_test_posembed_ex(_p(pos), _p(y), D, rows, cols, int(bool(size_mode)), st()))
    return y


def preprocess_ex(img, rows, cols, out_prefill, in_fp16=False, out_fp16=False, ldk=640, nchw_out=False, round16=False, aa=True, counters=None, zero_n=0,
                  raw=False):
    """preprocess_kernel as the model launches it (moge_test_preprocess_ex).  out_prefill: (B rows cols, ldk), or (B,3,14 rows,14 cols) with nchw_out;
    counters: int32 tensor (zero_n entries + a guard) or None.  Both are copied, handed to the kernel and returned whole."""
    img = _f(img)
    B, _, H, W = img.shape
    y = _f(out_prefill).clone()
    assert y.numel() == (B * 3 * rows * 14 * cols * 14 if nchw_out else B * rows * cols * max(ldk, 0))
    cnt = None if counters is None else counters.detach().to("cuda", torch.int32).contiguous().clone()
    assert cnt is None or cnt.numel() >= zero_n
    rc = L.lib.moge_test_preprocess_ex(int(bool(in_fp16)), int(bool(out_fp16)), _p(img), _p(y), _p(cnt), B, H, W, rows, cols, ldk, int(bool(nchw_out)),
                                       int(bool(round16)), int(bool(aa)), zero_n, st())
    if raw:
        return rc
    L.check(rc)
    return y, cnt


def resize_bicubic_aa_ex(img, OH, OW, in_fp16=False, round16=False):
    img = _f(img)
    B, _, H, W = img.shape
    y = torch.full((B, 3, OH, OW), float("nan"), device="cuda", dtype=torch.float32)
    L.check(L.lib.moge_test_resize_bicubic_aa_ex(int(bool(in_fp16)), _p(img), _p(y), B, H, W, OH, OW, int(bool(round16)), st()))
    return y


def recover(points, mask, focal=None):
    points = _f(points)
    B, H, W, _ = points.shape
    m = None if mask is None else mask.to("cuda", torch.uint8).contiguous()
    f_in = None if focal is None else _f(focal)
    f = torch.empty((B,), device="cuda", dtype=torch.float32)
    s = torch.empty((B,), device="cuda", dtype=torch.float32)
    status = torch.zeros((1,), device="cuda", dtype=torch.int32)
    L.check(L.lib.moge_test_recover(_p(points), _p(m), _p(f_in), B, H, W, _p(f), _p(s), _p(status), st()))
    return f, s, int(status.item())


def resize_bicubic_aa(img, OH, OW):
    img = _f(img)
    B, _, H, W = img.shape
    y = torch.empty((B, 3, OH, OW), device="cuda", dtype=torch.float32)
    L.check(L.lib.moge_test_resize_bicubic_aa(_p(img), _p(y), B, H, W, OH, OW, st()))
    return y


def groupnorm_relu(prec, x_nhwc, gamma, beta, groups):
    x, gamma, beta = _f(x_nhwc), _f(gamma), _f(beta)
    B, H, W, Cc = x.shape
    y = torch.empty_like(x)
    L.check(L.lib.moge_test_groupnorm_relu(prec, _p(x), _p(gamma), _p(beta), _p(y), B, H, W, Cc, groups, st()))
    return y


def norm_act(prec, x_nhwc, gamma, beta, groups, act, in_place=False):
    """act(norm(x)) of a v2 residual block: groups 0 = no norm, C = InstanceNorm2d (gamma = beta = None)."""
    x = _f(x_nhwc)
    B, H, W, Cc = x.shape
    y = torch.empty_like(x)
    g = _f(gamma) if gamma is not None else None
    b = _f(beta) if beta is not None else None
    L.check(L.lib.moge_test_norm_act(prec, _p(x), _p(g) if g is not None else None, _p(b) if b is not None else None, _p(y), B, H, W, Cc, groups, act, int(in_place), st()))
    return y


def conv_ex(x_nhwc, w, bias, prec=1, relu_in=False, act=0, add=None, side=None, side_w=None, uv=None, up2=False, w2=None, bias2=None, dot_w=None):
    """One 3x3 conv through the pieces the decoder fuses into it (moge_test_conv_ex).  uv = (wu, wv, u0, u1, v0, v1) at the OUTPUT resolution;
    w2 / bias2 select the fused residual block (conv_rb.hip)."""
    import ctypes as C
    keep = []

    def dev(t):
        if t is None:
            return None
        t = _f(t)
        keep.append(t)
        return t.data_ptr()

    x = _f(x_nhwc)
    B, H, W, Cin = x.shape
    Cout = w.shape[0]
    Ho, Wo = (2 * H, 2 * W) if up2 else (H, W)
    y = torch.empty((B, Ho, Wo, 4 if dot_w is not None else Cout), device="cuda", dtype=torch.float32)
    a = L.TestConvArgs()
    a.precision, a.B, a.H, a.W, a.Cin, a.Cout = prec, B, H, W, Cin, Cout
    a.relu_in, a.act, a.up2 = int(bool(relu_in)), act, int(bool(up2))
    a.x, a.w, a.bias = x.data_ptr(), dev(w), dev(bias)
    a.add, a.side, a.side_w = dev(add), dev(side), dev(side_w)
    if uv is not None:
        wu, wv, u0, u1, v0, v1 = uv
        a.wu, a.wv, a.u0, a.u1, a.v0, a.v1 = dev(wu), dev(wv), u0, u1, v0, v1
    a.w2, a.bias2 = dev(w2), dev(bias2)
    if dot_w is not None:
        a.dot_w, a.dot_rows = dev(dot_w), int(dot_w.shape[0])
    a.y = y.data_ptr()
    L.check(L.lib.moge_test_conv_ex(C.byref(a), st()))
    return y


def ct3(x_nhwc, wt, bt, w3, b3, side=None, side_w=None, uv=None, no_border=False):
    """ConvTranspose2d(k2, s2) + 3x3 replicate conv through the fused fp16 path (moge_test_ct3): x (B,H,W,Cin), wt (Cin,Cout,2,2), w3 (Cout,Cout,3,3)
    -> (B,2H,2W,Cout).  side (B,2H,2W,Cout) / side_w (Cout,Cout): the fused 1x1 input block; uv = (wu, wv, u0, u1, v0, v1) at the output resolution."""
    import ctypes as C
    keep = []

    def dev(t):
        if t is None:
            return None
        t = _f(t)
        keep.append(t)
        return t.data_ptr()

    x = _f(x_nhwc)
    B, H, W, Cin = x.shape
    Cout = w3.shape[0]
    y = torch.empty((B, 2 * H, 2 * W, Cout), device="cuda", dtype=torch.float32)
    a = L.TestCt3Args()
    a.precision, a.B, a.H, a.W, a.Cin, a.Cout, a.no_border = 1, B, H, W, Cin, Cout, int(bool(no_border))
    a.x, a.wt, a.bt, a.w3, a.b3 = x.data_ptr(), dev(wt), dev(bt), dev(w3), dev(b3)
    a.side, a.side_w = dev(side), dev(side_w)
    if uv is not None:
        wu, wv, u0, u1, v0, v1 = uv
        a.wu, a.wv, a.u0, a.u1, a.v0, a.v1 = dev(wu), dev(wv), u0, u1, v0, v1
    a.y = y.data_ptr()
    L.check(L.lib.moge_test_ct3(C.byref(a), st()))
    return y


def head_final(prec, kind, x, w, bias, H, W, remap=0, ksize=1, C=None, choff=0, n4=None, w2=None, n4_below=False, raw=False):
    """The decoder tail (moge_test_head_final): x (B,Hd,Wd,ld) with channels [choff, choff + C) the kernel's input, w (CO,C) or (CO,C,3,3).
    raw=True returns the status code instead of raising."""
    import ctypes as C_
    x, w, bias = _f(x), _f(w), _f(bias)
    B, Hd, Wd, ld = x.shape
    Cc = ld if C is None else C
    CO = 3 if kind in (0, 1) else 1
    out = torch.empty((B, H, W, CO), device="cuda", dtype=torch.float32)
    a = L.TestHeadArgs()
    a.precision, a.kind, a.remap, a.ksize = prec, kind, remap, ksize
    a.B, a.Hd, a.Wd, a.C, a.ld, a.choff, a.H, a.W = B, Hd, Wd, Cc, ld, choff, H, W
    a.n4_below = int(bool(n4_below))
    a.x, a.w, a.bias, a.out = x.data_ptr(), w.data_ptr(), bias.data_ptr(), out.data_ptr()
    keep = []
    if n4 is not None:
        keep += [_f(n4), _f(w2)]
        a.n4, a.w2 = keep[0].data_ptr(), keep[1].data_ptr()
    rc = L.lib.moge_test_head_final(C_.byref(a), st())
    if raw:
        return rc
    L.check(rc)
    return out


def head_final_dot(kind, y, bias, H, W, remap=0, z=None, zoff=0, raw=False):
    y, bias = _f(y), _f(bias)
    z = None if z is None else _f(z)
    B, Hd, Wd, _ = y.shape
    CO = 3 if kind in (0, 1) else 1
    out = torch.empty((B, H, W, CO), device="cuda", dtype=torch.float32)
    rc = L.lib.moge_test_head_final_dot(kind, remap, _p(y), _p(z), 0 if z is None else z.shape[-1], zoff, _p(bias), _p(out), B, Hd, Wd, H, W, st())
    if raw:
        return rc
    L.check(rc)
    return out


def mlp_layer(x, W, bias, act, raw=False):
    x, W, bias = _f(x), _f(W), _f(bias)
    B, K = x.shape
    N = W.shape[0]
    out = torch.empty((B, N), device="cuda", dtype=torch.float32)
    rc = L.lib.moge_test_mlp_layer(_p(x), _p(W), _p(bias), _p(out), B, K, N, act, st())
    if raw:
        return rc
    L.check(rc)
    return out


def layernorm_ex(prec, x, w, b, y_prefill, stream16=False, coloff=0, tap_mode=False, Ntok=0, cls_prefill=None, raw=False):
    """LayerNorm through the output modes of layernorm_kernel (moge_test_layernorm_ex): y_prefill (out rows, ldo) and cls_prefill (B, D) or None are
    copied, handed to the kernel and returned, so that what the kernel left alone can be checked."""
    x, w, b = _f(x), _f(w), _f(b)
    y = _f(y_prefill).clone()
    cls = None if cls_prefill is None else _f(cls_prefill).clone()
    rows, D = x.shape
    rc = L.lib.moge_test_layernorm_ex(prec, int(bool(stream16)), _p(x), _p(w), _p(b), _p(y), _p(cls), rows, D, y.shape[-1], coloff, int(bool(tap_mode)), Ntok, st())
    if raw:
        return rc
    L.check(rc)
    return y, cls


def ln_raw(x, raw=False):
    x = _f(x)
    rows, D = x.shape
    x16 = torch.empty_like(x)
    mr = torch.empty((rows, 2), device="cuda", dtype=torch.float32)
    rc = L.lib.moge_test_ln_raw(_p(x), _p(x16), _p(mr), rows, D, st())
    if raw:
        return rc
    L.check(rc)
    return x16, mr


def ln_finalize(part, D, raw=False):
    part = _f(part)
    rows, NP, _ = part.shape
    mr = torch.empty((rows, 2), device="cuda", dtype=torch.float32)
    rc = L.lib.moge_test_ln_finalize(_p(part), _p(mr), rows, NP, D, st())
    if raw:
        return rc
    L.check(rc)
    return mr


def fold_ln(W, g, beta, b):
    W, g, beta, b = _f(W), _f(g), _f(beta), _f(b)
    N, K = W.shape
    Wf = torch.empty_like(W)
    c = torch.empty((N,), device="cuda", dtype=torch.float32)
    bf = torch.empty((N,), device="cuda", dtype=torch.float32)
    L.check(L.lib.moge_test_fold_ln(_p(W), _p(g), _p(beta), _p(b), _p(Wf), _p(c), _p(bf), N, K, st()))
    return Wf, c, bf


def resize_bilinear_uv(prec, x, OH, OW, Cp, uv_range, raw=False):
    x = _f(x)
    B, hs, ws, Cc = x.shape
    out = torch.empty((B, OH, OW, Cp), device="cuda", dtype=torch.float32)
    u0, u1, v0, v1 = uv_range
    rc = L.lib.moge_test_resize_bilinear_uv(prec, _p(x), _p(out), B, hs, ws, Cc, OH, OW, Cp, u0, u1, v0, v1, st())
    if raw:
        return rc
    L.check(rc)
    return out


def u8_ingest(prec, img_u8):
    img = img_u8.to("cuda", torch.uint8).contiguous()
    B, H, W, _ = img.shape
    out = torch.empty((B, 3, H, W), device="cuda", dtype=torch.float32)
    L.check(L.lib.moge_test_u8_ingest(prec, _p(img), _p(out), B, H, W, st()))
    return out
