// Trainable bilinear resize (F.interpolate / nn.Upsample, mode bilinear, align_corners False, no antialias) and the narrow 1x1 convolution at the exit of
// a head (Cout <= 8), each with its gradients, on NHWC activations.  C ABI moge_resize_bilinear_* and moge_narrow_conv1x1_*, python mirror
// moge_amd/resample.py, DESIGN.md section 23.  Everything here is memory-bound: no MFMA, no LDS tiles beyond the narrow conv's weight.
//
// Resize, one axis with n_in input and n_out output samples and scale sigma (rs_coord, rs_tap):
//     s(o) = max(sigma (o + 0.5) - 0.5, 0)      i0 = min(floor s, n_in - 1)      i1 = min(i0 + 1, n_in - 1)      l1 = s - i0      l0 = 1 - l1
//     y [b,o,p,c] = l0H (l0W x[b,i0H,i0W,c] + l1W x[b,i0H,i1W,c]) + l1H (l0W x[b,i1H,i0W,c] + l1W x[b,i1H,i1W,c])
//     dx[b,r,q,c] = sum over the outputs (o, p) that have (r, q) among their taps of wH(o, r) wW(p, q) dy[b,o,p,c]
// i0 is non-decreasing in o, so first[r] = min{o : i0(o) >= r} (r = 0 ... n_in, first[n_in] = n_out; resize_table_kernel, a binary search with the same
// rs_coord) turns the transpose into a gather: input sample r takes l1(o) from o in [first[r-1], first[r]) and l0(o) from o in [first[r], first[r+1]); at
// r = n_in - 1 both taps of its own range are r itself, so it takes l0 + l1 there.  An empty range (down-sampling) is a gradient of exactly 0, written.
// One thread per (pixel, 16-byte chunk of channels) where C, the pointers and the pixel strides allow 16-byte accesses, per (pixel, channel) otherwise; both
// forms do the same arithmetic in the same order.  fp32 sums, rows outer and columns inner and both ascending in the gradient, one rounding of the result.
// No atomics: two calls give the same bits, and a pixel depends on its own image only.
//
// Narrow conv, M = B H W pixels, x (M, Cin), w (Cout, Cin), y and dy (M, Cout) with a pixel stride of Cout elements or more (scalar accesses):
//     y[m,o] = b[o] + sum_c x[m,c] w[o,c]          conv1x1n_kernel         a quad of lanes per pixel: lane l takes the chunks l, l + 4, ...; quad sum by DPP
//     dx[m,c] = sum_o dy[m,o] w[o,c]               conv1x1n_dgrad_kernel   a thread per (pixel, chunk)
//     dw[o,c] = sum_m dy[m,o] x[m,c], db[o]        conv1x1n_wgrad_kernel   a workgroup per slab of pixels: thread = (row lane, chunk), the row lanes added in
//                                                                           order through LDS; conv1x1n_reduce_kernel adds the slabs in slab order
// The whole weight (at most 8 x 256) lies in LDS as fp32.  db is not lin_colsum_kernel's: that kernel reads rows in 16-byte chunks, and a row of dy here has 1 or
// 3 elements; the wgrad kernel has every dy value in a register anyway.  The slab count is a function of the pixel count only.
#include <cmath>

#include "grad_host.h"

#pragma clang fp contract(off)        // every fused multiply-add below is written as one (__fmaf_rn); nothing else is contracted

namespace {

// ---- the source coordinate: the forward, the table and the gradient all read this one function.  Two roundings: o + 0.5 (exact below 2^23) and the fma.
__device__ __forceinline__ float rs_coord(int o, float sigma) { return fmaxf(__fmaf_rn(sigma, (float)o + 0.5f, -0.5f), 0.f); }
__device__ __forceinline__ int rs_floor(float s, int n_in) {
    const int i = (int)fminf(floorf(s), 1073741824.f);      // 2^30: above every n_in the entries admit, exact in fp32
    return i < n_in - 1 ? i : n_in - 1;
}
__device__ __forceinline__ int rs_i0(int o, float sigma, int n_in) { return rs_floor(rs_coord(o, sigma), n_in); }
struct RsTap { int i0, i1; float l0, l1; };
__device__ __forceinline__ RsTap rs_tap(int o, float sigma, int n_in) {
    const float s = rs_coord(o, sigma);
    RsTap t;
    t.i0 = rs_floor(s, n_in);
    t.i1 = t.i0 + 1 < n_in ? t.i0 + 1 : n_in - 1;
    t.l1 = s - (float)t.i0;
    t.l0 = 1.f - t.l1;
    return t;
}
// what input sample r takes from output sample o, o in [first[r-1], first[r+1]) and own = (o >= first[r])
__device__ __forceinline__ float rs_weight(const RsTap& t, bool own, bool last) { return own ? (last ? t.l0 + t.l1 : t.l0) : t.l1; }

// N channels of one pixel: a 16-byte chunk, or one element
template <typename T, bool VEC> struct RsIO {
    static constexpr int N = VEC ? TT<T>::CH : 1;
    static __device__ __forceinline__ void load(const T* p, float (&v)[N]) {
        if constexpr (VEC) {
            const typename Vec<T>::type h = __builtin_bit_cast(typename Vec<T>::type, ldg16(p));
#pragma unroll
            for (int e = 0; e < N; e++) v[e] = (float)h[e];
        } else {
            v[0] = (float)*p;
        }
    }
    static __device__ __forceinline__ void store(T* p, const float (&v)[N]) {
        if constexpr (VEC) {
            typename Vec<T>::type h;
#pragma unroll
            for (int e = 0; e < N; e++) h[e] = (T)v[e];
            *reinterpret_cast<typename Vec<T>::type*>(p) = h;
        } else {
            *p = (T)v[0];
        }
    }
};

// e = ((b n_h + i) n_w + j) cv + c -> the pixel's coordinates and the element offset of the thread's channels
struct RsPlace { int b, i, j, c; };
template <typename T, bool VEC> __device__ __forceinline__ RsPlace rs_place(long long e, int n_h, int n_w, int C) {
    const int cv = VEC ? C / TT<T>::CH : C;
    RsPlace p;
    p.c = (int)(e % cv) * RsIO<T, VEC>::N;
    const long long pix = e / cv, row = pix / n_w;
    p.j = (int)(pix - row * n_w);
    p.b = (int)(row / n_h);
    p.i = (int)(row - (long long)p.b * n_h);
    return p;
}

template <typename T, bool VEC>
__global__ __launch_bounds__(256) void resize_bilinear_kernel(const T* __restrict__ x, long long ldx, T* __restrict__ y, long long ldy, int Hin, int Win, int Hout, int Wout,
                                                              int C, float sh, float sw, long long total) {
    constexpr int N = RsIO<T, VEC>::N;
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    if (e >= total) return;
    const RsPlace at = rs_place<T, VEC>(e, Hout, Wout, C);
    const RsTap th = rs_tap(at.i, sh, Hin), tw = rs_tap(at.j, sw, Win);
    const long long r0 = ((long long)at.b * Hin + th.i0) * Win, r1 = ((long long)at.b * Hin + th.i1) * Win;
    float a[N], b[N], c[N], d[N], v[N];
    RsIO<T, VEC>::load(x + (r0 + tw.i0) * ldx + at.c, a);
    RsIO<T, VEC>::load(x + (r0 + tw.i1) * ldx + at.c, b);
    RsIO<T, VEC>::load(x + (r1 + tw.i0) * ldx + at.c, c);
    RsIO<T, VEC>::load(x + (r1 + tw.i1) * ldx + at.c, d);
#pragma unroll
    for (int k = 0; k < N; k++) {
        const float top = __fmaf_rn(tw.l1, b[k], tw.l0 * a[k]), bot = __fmaf_rn(tw.l1, d[k], tw.l0 * c[k]);
        v[k] = __fmaf_rn(th.l1, bot, th.l0 * top);
    }
    RsIO<T, VEC>::store(y + (((long long)at.b * Hout + at.i) * Wout + at.j) * ldy + at.c, v);
}

// first[r] of both axes: blockIdx.y = 0 the rows (tab_h, Hin + 1 ints), 1 the columns (tab_w, Win + 1 ints)
__global__ __launch_bounds__(256) void resize_table_kernel(int* __restrict__ tab_h, int* __restrict__ tab_w, int Hin, int Win, int Hout, int Wout, float sh, float sw) {
    const bool cols = blockIdx.y != 0;
    const int n_in = cols ? Win : Hin, n_out = cols ? Wout : Hout;
    const float sigma = cols ? sw : sh;
    const int r = blockIdx.x * 256 + threadIdx.x;
    if (r > n_in) return;
    int lo = 0, hi = n_out;              // the smallest o in [0, n_out] with i0(o) >= r; i0 is non-decreasing, and never reaches n_in
    while (lo < hi) {
        const int mid = lo + (hi - lo) / 2;
        if (rs_i0(mid, sigma, n_in) >= r) hi = mid;
        else lo = mid + 1;
    }
    (cols ? tab_w : tab_h)[r] = lo;
}

template <typename T, bool VEC>
__global__ __launch_bounds__(256) void resize_bilinear_grad_kernel(const T* __restrict__ dy, long long lddy, T* __restrict__ dx, long long lddx, const int* __restrict__ tab_h,
                                                                   const int* __restrict__ tab_w, int Hin, int Win, int Hout, int Wout, int C, float sh, float sw,
                                                                   long long total) {
    constexpr int N = RsIO<T, VEC>::N;
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    if (e >= total) return;
    const RsPlace at = rs_place<T, VEC>(e, Hin, Win, C);
    const int oa = tab_h[at.i > 0 ? at.i - 1 : 0], om = tab_h[at.i], ob = tab_h[at.i + 1];
    const int pa = tab_w[at.j > 0 ? at.j - 1 : 0], pm = tab_w[at.j], pb = tab_w[at.j + 1];
    const bool last_h = at.i == Hin - 1, last_w = at.j == Win - 1;
    float acc[N];
#pragma unroll
    for (int k = 0; k < N; k++) acc[k] = 0.f;
    for (int o = oa; o < ob; o++) {
        const float wh = rs_weight(rs_tap(o, sh, Hin), o >= om, last_h);
        const T* row = dy + ((long long)at.b * Hout + o) * Wout * lddy + at.c;
        float in[N];
#pragma unroll
        for (int k = 0; k < N; k++) in[k] = 0.f;
        for (int p = pa; p < pb; p++) {
            const float ww = rs_weight(rs_tap(p, sw, Win), p >= pm, last_w);
            float g[N];
            RsIO<T, VEC>::load(row + p * lddy, g);
#pragma unroll
            for (int k = 0; k < N; k++) in[k] = __fmaf_rn(ww, g[k], in[k]);
        }
#pragma unroll
        for (int k = 0; k < N; k++) acc[k] = __fmaf_rn(wh, in[k], acc[k]);
    }
    RsIO<T, VEC>::store(dx + (((long long)at.b * Hin + at.i) * Win + at.j) * lddx + at.c, acc);
}

// ---- the narrow 1x1 conv ------------------------------------------------------------------------------------------------------------
constexpr int N1_MAX_CIN = 256, N1_MAX_COUT = 8;
constexpr int N1_SLAB = 512;             // pixels of a slab of the weight gradient at the least
constexpr int N1_MAX_SLABS = 1024;

// the weight (Cout, Cin) as fp32 in LDS (exact)
template <typename T> __device__ __forceinline__ void n1_stage_weight(float* sw, const T* __restrict__ w, int n) {
    for (int i = threadIdx.x; i < n; i += 256) sw[i] = (float)w[i];
    __syncthreads();
}

template <typename T>
__global__ __launch_bounds__(256) void conv1x1n_kernel(const T* __restrict__ x, long long ldx, const T* __restrict__ w, const T* __restrict__ bias, T* __restrict__ y,
                                                       long long ldy, int M, int Cin, int Cout) {
    constexpr int CH = TT<T>::CH;
    __shared__ __attribute__((aligned(16))) float sw[N1_MAX_COUT * N1_MAX_CIN];
    n1_stage_weight(sw, w, Cout * Cin);
    const int l = threadIdx.x & 3, nch = Cin / CH;
    const long long m = (long long)blockIdx.x * 64 + (threadIdx.x >> 2);
    const T* px = x + (m < M ? m : (long long)M - 1) * ldx;        // a pixel past the end is clamped and not stored: every lane stays in the quad sums
    float acc[N1_MAX_COUT];
#pragma unroll
    for (int o = 0; o < N1_MAX_COUT; o++) acc[o] = 0.f;
    for (int j = l; j < nch; j += 4) {
        float v[CH];
        RsIO<T, true>::load(px + j * CH, v);
#pragma unroll
        for (int o = 0; o < N1_MAX_COUT; o++)
            if (o < Cout) {
                const float* wo = sw + o * Cin + j * CH;
#pragma unroll
                for (int e = 0; e < CH; e++) acc[o] = __fmaf_rn(v[e], wo[e], acc[o]);
            }
    }
#pragma unroll
    for (int o = 0; o < N1_MAX_COUT; o++) {
        acc[o] += dpp_quad_xor1(acc[o]);
        acc[o] += dpp_quad_xor2(acc[o]);
    }
    if (m >= M) return;
#pragma unroll
    for (int o = 0; o < N1_MAX_COUT; o++)
        if (o < Cout && (o & 3) == l) y[m * ldy + o] = (T)(acc[o] + (bias ? (float)bias[o] : 0.f));
}

template <typename T>
__global__ __launch_bounds__(256) void conv1x1n_dgrad_kernel(const T* __restrict__ dy, long long lddy, const T* __restrict__ w, T* __restrict__ dx, long long lddx,
                                                             long long total, int Cin, int Cout) {
    constexpr int CH = TT<T>::CH;
    __shared__ __attribute__((aligned(16))) float sw[N1_MAX_COUT * N1_MAX_CIN];
    n1_stage_weight(sw, w, Cout * Cin);
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    if (e >= total) return;
    const int nch = Cin / CH;
    const long long m = e / nch;
    const int c = (int)(e - m * nch) * CH;
    float v[CH];
#pragma unroll
    for (int k = 0; k < CH; k++) v[k] = 0.f;
#pragma unroll
    for (int o = 0; o < N1_MAX_COUT; o++)
        if (o < Cout) {
            const float g = (float)dy[m * lddy + o];
#pragma unroll
            for (int k = 0; k < CH; k++) v[k] = __fmaf_rn(g, sw[o * Cin + c + k], v[k]);
        }
    RsIO<T, true>::store(dx + m * lddx + c, v);
}

// part[z] = (dw (Cout, Cin), db (Cout)) of the pixels [z per, min(M, (z + 1) per)); x may be null (db alone): dw's part is then zero and not used
template <typename T>
__global__ __launch_bounds__(256) void conv1x1n_wgrad_kernel(const T* __restrict__ x, long long ldx, const T* __restrict__ dy, long long lddy, float* __restrict__ part, int M,
                                                             int Cin, int Cout, int per) {
    constexpr int CH = TT<T>::CH;
    __shared__ float red[256 * CH];       // one output channel's sums of every thread, [row lane][chunk][element]
    __shared__ float redb[256];
    const int nch = Cin / CH, R = 256 / nch;       // row lanes; the threads past R nch have no work
    const int tid = threadIdx.x, j = tid % nch, r = tid / nch;
    const long long mbeg = (long long)blockIdx.x * per, mend = M - mbeg < per ? M : mbeg + per;
    float acc[N1_MAX_COUT][CH], sb[N1_MAX_COUT];
#pragma unroll
    for (int o = 0; o < N1_MAX_COUT; o++) {
        sb[o] = 0.f;
#pragma unroll
        for (int k = 0; k < CH; k++) acc[o][k] = 0.f;
    }
    if (r < R)
        for (long long m = mbeg + r; m < mend; m += R) {
            float v[CH];
#pragma unroll
            for (int k = 0; k < CH; k++) v[k] = 0.f;
            if (x) RsIO<T, true>::load(x + m * ldx + j * CH, v);
#pragma unroll
            for (int o = 0; o < N1_MAX_COUT; o++)
                if (o < Cout) {
                    const float g = (float)dy[m * lddy + o];
                    sb[o] += g;
#pragma unroll
                    for (int k = 0; k < CH; k++) acc[o][k] = __fmaf_rn(g, v[k], acc[o][k]);
                }
        }
    float* out = part + (long long)blockIdx.x * Cout * (Cin + 1);
#pragma unroll
    for (int o = 0; o < N1_MAX_COUT; o++)
        if (o < Cout) {                   // uniform over the workgroup
            __syncthreads();
#pragma unroll
            for (int k = 0; k < CH; k++) red[tid * CH + k] = acc[o][k];
            redb[tid] = sb[o];
            __syncthreads();
            if (r == 0) {                 // tid = j: the row lanes in ascending order
#pragma unroll
                for (int k = 0; k < CH; k++) {
                    float s = red[j * CH + k];
                    for (int i = 1; i < R; i++) s += red[(i * nch + j) * CH + k];
                    out[o * Cin + j * CH + k] = s;
                }
                if (j == 0) {
                    float s = redb[0];
                    for (int i = 1; i < R; i++) s += redb[i * nch];
                    out[Cout * Cin + o] = s;
                }
            }
        }
}

// dw and db = the S slabs added in slab order, rounded once; either may be null
template <typename T>
__global__ __launch_bounds__(256) void conv1x1n_reduce_kernel(const float* __restrict__ part, T* __restrict__ dw, T* __restrict__ db, int nw, int Cout, int S) {
    const int i = blockIdx.x * 256 + threadIdx.x, n = nw + Cout;
    if (i >= n) return;
    float v = part[i];
    for (int z = 1; z < S; z++) v += part[(long long)z * n + i];
    if (i < nw) {
        if (dw) dw[i] = (T)v;
    } else if (db) {
        db[i - nw] = (T)v;
    }
}

// ---- host side ----------------------------------------------------------------------------------------------------------------------
constexpr long long MAX_PIXELS = 1LL << 30;
inline int elem_bytes(int dtype) { return dtype == MOGE_FP16 ? 2 : 4; }

// (B, n_h, n_w) pixels of a grid: the products are taken in an order that stays inside 64 bits (every factor is below 2^31)
bool too_many_pixels(int B, int n_h, int n_w) { return (long long)B * n_h > MAX_PIXELS || (long long)B * n_h * n_w > MAX_PIXELS; }

// an activation whose rows of C elements are read or written element by element: non-null, aligned to its element, pixel stride at least C
int check_scalar_pixels(const char* fn, const char* name, const char* ldname, const void* p, int64_t ld, int C, int dtype) {
    if (!p) return moge_internal_fail(MOGE_ERR_INVALID, "%s: %s is null", fn, name);
    if ((uintptr_t)p % elem_bytes(dtype)) return moge_internal_fail(MOGE_ERR_INVALID, "%s: %s is not aligned to its %d-byte elements", fn, name, elem_bytes(dtype));
    if (ld < C) return moge_internal_fail(MOGE_ERR_INVALID, "%s: %s = %lld is below the channel count %d", fn, ldname, (long long)ld, C);
    return 0;
}
int check_element_vector(const char* fn, const char* name, const void* p, bool required, int dtype) {
    if (!p && required) return moge_internal_fail(MOGE_ERR_INVALID, "%s: %s is null", fn, name);
    if ((uintptr_t)p % elem_bytes(dtype)) return moge_internal_fail(MOGE_ERR_INVALID, "%s: %s is not aligned to its %d-byte elements", fn, name, elem_bytes(dtype));
    return 0;
}

// -- resize
int rs_check_sizes(const char* fn, int dtype, int B, int Hin, int Win, int Hout, int Wout, int C) {
    if (int e = check_dtype(fn, dtype)) return e;
    if (B < 0) return moge_internal_fail(MOGE_ERR_INVALID, "%s: B < 0", fn);
    const int sizes[5] = {Hin, Win, Hout, Wout, C};
    const char* names[5] = {"Hin", "Win", "Hout", "Wout", "C"};
    for (int i = 0; i < 5; i++)
        if (sizes[i] < 1) return moge_internal_fail(MOGE_ERR_INVALID, "%s: %s = %d < 1", fn, names[i], sizes[i]);
    if (too_many_pixels(B, Hin, Win)) return moge_internal_fail(MOGE_ERR_INVALID, "%s: B Hin Win exceeds 2^30 pixels of the input grid", fn);
    if (too_many_pixels(B, Hout, Wout)) return moge_internal_fail(MOGE_ERR_INVALID, "%s: B Hout Wout exceeds 2^30 pixels of the output grid", fn);
    const long long in = (long long)B * Hin * Win, out = (long long)B * Hout * Wout;                   // at most 2^30 each, so times C < 2^31 stays inside 64 bits
    if (((in > out ? in : out) * C + 255) / 256 > 0x7fffffffLL)
        return moge_internal_fail(MOGE_ERR_INVALID, "%s: ceil(pixels C / 256) exceeds the 2^31 - 1 workgroups of a grid", fn);
    return 0;
}
int rs_check_scales(const char* fn, float sh, float sw) {
    if (!(sh > 0.f) || std::isinf(sh)) return moge_internal_fail(MOGE_ERR_INVALID, "%s: scale_h = %g is not a positive finite number", fn, (double)sh);
    if (!(sw > 0.f) || std::isinf(sw)) return moge_internal_fail(MOGE_ERR_INVALID, "%s: scale_w = %g is not a positive finite number", fn, (double)sw);
    return 0;
}
// the 16-byte form where both tensors allow it
bool rs_vector(const void* a, int64_t lda, const void* b, int64_t ldb, int C, int dtype) {
    const int ch = chunk_of(dtype);
    return C % ch == 0 && (uintptr_t)a % 16 == 0 && (uintptr_t)b % 16 == 0 && lda % ch == 0 && ldb % ch == 0;
}
struct RsWs { long long tab_h, tab_w, total; };
RsWs rs_ws(int Hin, int Win) {
    RsWs w;
    w.tab_h = 0;
    w.tab_w = align16(4LL * (Hin + 1));
    w.total = w.tab_w + align16(4LL * (Win + 1));
    return w;
}

template <typename T, bool VEC>
void rs_forward(const void* x, int64_t ldx, void* y, int64_t ldy, int B, int Hin, int Win, int Hout, int Wout, int C, float sh, float sw, hipStream_t st) {
    const long long total = (long long)B * Hout * Wout * (VEC ? C / TT<T>::CH : C);
    hipLaunchKernelGGL((resize_bilinear_kernel<T, VEC>), dim3(blocks(total, 256)), dim3(256), 0, st, (const T*)x, (long long)ldx, (T*)y, (long long)ldy, Hin, Win, Hout, Wout, C,
                       sh, sw, total);
}
template <typename T, bool VEC>
void rs_backward(const void* dy, int64_t lddy, void* dx, int64_t lddx, char* ws, int B, int Hin, int Win, int Hout, int Wout, int C, float sh, float sw, hipStream_t st) {
    const RsWs o = rs_ws(Hin, Win);
    int *tab_h = (int*)(ws + o.tab_h), *tab_w = (int*)(ws + o.tab_w);
    hipLaunchKernelGGL(resize_table_kernel, dim3(blocks((Hin > Win ? Hin : Win) + 1LL, 256), 2), dim3(256), 0, st, tab_h, tab_w, Hin, Win, Hout, Wout, sh, sw);
    const long long total = (long long)B * Hin * Win * (VEC ? C / TT<T>::CH : C);
    hipLaunchKernelGGL((resize_bilinear_grad_kernel<T, VEC>), dim3(blocks(total, 256)), dim3(256), 0, st, (const T*)dy, (long long)lddy, (T*)dx, (long long)lddx,
                       (const int*)tab_h, (const int*)tab_w, Hin, Win, Hout, Wout, C, sh, sw, total);
}

// -- narrow conv
struct N1Split { int parts; int per; };
N1Split n1_split(long long M) {
    long long s = (M + N1_SLAB - 1) / N1_SLAB;
    s = s < 1 ? 1 : (s > N1_MAX_SLABS ? N1_MAX_SLABS : s);
    const long long per = M ? (M + s - 1) / s : 1;
    return N1Split{M ? (int)((M + per - 1) / per) : 1, (int)per};
}
int n1_check_sizes(const char* fn, int dtype, int B, int H, int W, int Cin, int Cout) {
    if (int e = check_dtype(fn, dtype)) return e;
    if (B < 0) return moge_internal_fail(MOGE_ERR_INVALID, "%s: B < 0", fn);
    if (H < 1) return moge_internal_fail(MOGE_ERR_INVALID, "%s: H = %d < 1", fn, H);
    if (W < 1) return moge_internal_fail(MOGE_ERR_INVALID, "%s: W = %d < 1", fn, W);
    if (int e = check_count(fn, "Cin", Cin, dtype)) return e;
    if (Cin > N1_MAX_CIN) return moge_internal_fail(MOGE_ERR_INVALID, "%s: Cin = %d exceeds %d", fn, Cin, N1_MAX_CIN);
    if (Cout < 1 || Cout > N1_MAX_COUT) return moge_internal_fail(MOGE_ERR_INVALID, "%s: Cout = %d is not in 1 ... %d", fn, Cout, N1_MAX_COUT);
    if (too_many_pixels(B, H, W)) return moge_internal_fail(MOGE_ERR_INVALID, "%s: B H W exceeds 2^30 pixels", fn);
    return 0;
}
long long n1_backward_bytes(long long M, int Cin, int Cout) { return align16(4LL * n1_split(M).parts * Cout * (Cin + 1)); }

template <typename T>
void n1_forward(const void* x, int64_t ldx, const void* w, const void* bias, void* y, int64_t ldy, int M, int Cin, int Cout, hipStream_t st) {
    hipLaunchKernelGGL(conv1x1n_kernel<T>, dim3(blocks(M, 64)), dim3(256), 0, st, (const T*)x, (long long)ldx, (const T*)w, (const T*)bias, (T*)y, (long long)ldy, M, Cin, Cout);
}
template <typename T>
void n1_backward(const void* x, int64_t ldx, const void* w, const void* dy, int64_t lddy, void* dx, int64_t lddx, void* dw, void* db, float* part, int M, int Cin, int Cout,
                 hipStream_t st) {
    if (dx) {
        const long long total = (long long)M * (Cin / TT<T>::CH);
        hipLaunchKernelGGL(conv1x1n_dgrad_kernel<T>, dim3(blocks(total, 256)), dim3(256), 0, st, (const T*)dy, (long long)lddy, (const T*)w, (T*)dx, (long long)lddx, total, Cin,
                           Cout);
    }
    if (dw || db) {
        const N1Split sp = n1_split(M);
        hipLaunchKernelGGL(conv1x1n_wgrad_kernel<T>, dim3((unsigned)sp.parts), dim3(256), 0, st, (const T*)(dw ? x : nullptr), (long long)ldx, (const T*)dy, (long long)lddy, part,
                           M, Cin, Cout, sp.per);
        hipLaunchKernelGGL(conv1x1n_reduce_kernel<T>, dim3(blocks(Cout * (Cin + 1), 256)), dim3(256), 0, st, (const float*)part, (T*)dw, (T*)db, Cout * Cin, Cout, sp.parts);
    }
}

}  // namespace

extern "C" {

int moge_resize_bilinear_workspace(int B, int Hin, int Win, int Hout, int Wout, int C, int dtype, int64_t* forward_bytes, int64_t* backward_bytes) {
    const char* fn = "moge_resize_bilinear_workspace";
    if (!forward_bytes) return moge_internal_fail(MOGE_ERR_INVALID, "%s: forward_bytes is null", fn);
    if (!backward_bytes) return moge_internal_fail(MOGE_ERR_INVALID, "%s: backward_bytes is null", fn);
    *forward_bytes = *backward_bytes = 0;
    if (int e = rs_check_sizes(fn, dtype, B, Hin, Win, Hout, Wout, C)) return e;
    *backward_bytes = rs_ws(Hin, Win).total;
    return 0;
}

int moge_resize_bilinear_forward(int dtype, const void* x, int64_t ldx, void* y, int64_t ldy, int B, int Hin, int Win, int Hout, int Wout, int C, float scale_h, float scale_w,
                                 void* workspace, void* stream) {
    const char* fn = "moge_resize_bilinear_forward";
    (void)workspace;                     // forward_bytes is 0
    if (int e = rs_check_sizes(fn, dtype, B, Hin, Win, Hout, Wout, C)) return e;
    if (int e = rs_check_scales(fn, scale_h, scale_w)) return e;
    if (B == 0) return 0;
    if (int e = check_scalar_pixels(fn, "x", "ldx", x, ldx, C, dtype)) return e;
    if (int e = check_scalar_pixels(fn, "y", "ldy", y, ldy, C, dtype)) return e;
    const bool vec = rs_vector(x, ldx, y, ldy, C, dtype);
    hipStream_t st = (hipStream_t)stream;
    if (dtype == MOGE_FP16) (vec ? rs_forward<f16, true> : rs_forward<f16, false>)(x, ldx, y, ldy, B, Hin, Win, Hout, Wout, C, scale_h, scale_w, st);
    else (vec ? rs_forward<float, true> : rs_forward<float, false>)(x, ldx, y, ldy, B, Hin, Win, Hout, Wout, C, scale_h, scale_w, st);
    return launched("moge_resize_bilinear_forward: launch failed");
}

int moge_resize_bilinear_backward(int dtype, const void* dy, int64_t lddy, void* dx, int64_t lddx, void* workspace, int B, int Hin, int Win, int Hout, int Wout, int C,
                                  float scale_h, float scale_w, void* stream) {
    const char* fn = "moge_resize_bilinear_backward";
    if (int e = rs_check_sizes(fn, dtype, B, Hin, Win, Hout, Wout, C)) return e;
    if (int e = rs_check_scales(fn, scale_h, scale_w)) return e;
    if (B == 0) return 0;
    if (int e = check_scalar_pixels(fn, "dy", "lddy", dy, lddy, C, dtype)) return e;
    if (int e = check_scalar_pixels(fn, "dx", "lddx", dx, lddx, C, dtype)) return e;
    if (int e = check_vector(fn, "workspace", workspace, true)) return e;
    const bool vec = rs_vector(dy, lddy, dx, lddx, C, dtype);
    hipStream_t st = (hipStream_t)stream;
    char* ws = (char*)workspace;
    if (dtype == MOGE_FP16) (vec ? rs_backward<f16, true> : rs_backward<f16, false>)(dy, lddy, dx, lddx, ws, B, Hin, Win, Hout, Wout, C, scale_h, scale_w, st);
    else (vec ? rs_backward<float, true> : rs_backward<float, false>)(dy, lddy, dx, lddx, ws, B, Hin, Win, Hout, Wout, C, scale_h, scale_w, st);
    return launched("moge_resize_bilinear_backward: launch failed");
}

int moge_narrow_conv1x1_workspace(int B, int H, int W, int Cin, int Cout, int dtype, int64_t* forward_bytes, int64_t* backward_bytes) {
    const char* fn = "moge_narrow_conv1x1_workspace";
    if (!forward_bytes) return moge_internal_fail(MOGE_ERR_INVALID, "%s: forward_bytes is null", fn);
    if (!backward_bytes) return moge_internal_fail(MOGE_ERR_INVALID, "%s: backward_bytes is null", fn);
    *forward_bytes = *backward_bytes = 0;
    if (int e = n1_check_sizes(fn, dtype, B, H, W, Cin, Cout)) return e;
    *backward_bytes = n1_backward_bytes((long long)B * H * W, Cin, Cout);
    return 0;
}

int moge_narrow_conv1x1_forward(int dtype, const void* x, int64_t ldx, const void* w, const void* bias, void* y, int64_t ldy, int B, int H, int W, int Cin, int Cout,
                                void* workspace, void* stream) {
    const char* fn = "moge_narrow_conv1x1_forward";
    (void)workspace;                     // forward_bytes is 0
    if (int e = n1_check_sizes(fn, dtype, B, H, W, Cin, Cout)) return e;
    if (B == 0) return 0;
    if (int e = check_pixels(fn, "x", "ldx", x, ldx, Cin, dtype)) return e;
    if (int e = check_element_vector(fn, "w", w, true, dtype)) return e;
    if (int e = check_element_vector(fn, "bias", bias, false, dtype)) return e;
    if (int e = check_scalar_pixels(fn, "y", "ldy", y, ldy, Cout, dtype)) return e;
    if (dtype == MOGE_FP16) n1_forward<f16>(x, ldx, w, bias, y, ldy, B * H * W, Cin, Cout, (hipStream_t)stream);
    else n1_forward<float>(x, ldx, w, bias, y, ldy, B * H * W, Cin, Cout, (hipStream_t)stream);
    return launched("moge_narrow_conv1x1_forward: launch failed");
}

int moge_narrow_conv1x1_backward(int dtype, const void* x, int64_t ldx, const void* w, const void* dy, int64_t lddy, void* dx, int64_t lddx, void* dw, void* db, void* workspace,
                                 int B, int H, int W, int Cin, int Cout, void* stream) {
    const char* fn = "moge_narrow_conv1x1_backward";
    if (int e = n1_check_sizes(fn, dtype, B, H, W, Cin, Cout)) return e;
    if (B == 0 || (!dx && !dw && !db)) return 0;
    if (int e = check_scalar_pixels(fn, "dy", "lddy", dy, lddy, Cout, dtype)) return e;
    if (dx) {
        if (int e = check_element_vector(fn, "w", w, true, dtype)) return e;
        if (int e = check_pixels(fn, "dx", "lddx", dx, lddx, Cin, dtype)) return e;
    }
    if (dw) {
        if (int e = check_pixels(fn, "x", "ldx", x, ldx, Cin, dtype)) return e;
        if (int e = check_element_vector(fn, "dw", dw, true, dtype)) return e;
    }
    if (int e = check_element_vector(fn, "db", db, false, dtype)) return e;
    if (dw || db)
        if (int e = check_vector(fn, "workspace", workspace, true)) return e;
    if (dtype == MOGE_FP16) n1_backward<f16>(x, ldx, w, dy, lddy, dx, lddx, dw, db, (float*)workspace, B * H * W, Cin, Cout, (hipStream_t)stream);
    else n1_backward<float>(x, ldx, w, dy, lddy, dx, lddx, dw, db, (float*)workspace, B * H * W, Cin, Cout, (hipStream_t)stream);
    return launched("moge_narrow_conv1x1_backward: launch failed");
}

}  // extern "C"
