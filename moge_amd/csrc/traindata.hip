// Per-instance geometric warp of the training data loader (reference moge/train/dataloader.py `_process_instance`, :143-229, and
// moge/utils/data_augmentation.py `warp_perspective`; python mirror moge_amd/train_data.py).  Stateless kernels on the
// caller's stream; every pointer is device memory unless stated.  Gather-bound: no MFMA anywhere in this file.
//
//   normal map     :145-146  depth_map_to_normal_map(depth, K, mask = isfinite, edge_threshold): four faces per pixel, NaN where none counts
//   depth edge     :171-172  depth_map_edge(depth, mask = isfinite, kernel_size, ltol) -> the bilinear-eligible map isfinite & ~edge, and ~isnan
//   warp           :169-192  cv2.warpPerspective of five maps fused per target pixel: Lanczos-4 image, bilinear eligibility / disparity /
//                            normal, nearest depth, the z re-division, normal @ R^T, the flip, and the count of finite depths
//   finish         :184-186, :205-219  the empty fallback, depth_unit, the exact 1 % nanquantile clamp (quantile.h), both masks
//
// fp32 arithmetic follows the reference's numpy operation order with NO contraction (the pragma below).  Counts use integer atomics and
// nothing sums floats across threads: two runs give the same bits.
#include "common.h"
#include "quantile.h"
#include "../../include/moge_hip.h"

#pragma clang fp contract(off)

constexpr int TD_THREADS = Q_THREADS;
constexpr int TD_BLOCKS = Q_BLOCKS;

__device__ __forceinline__ bool td_finite(float d) { return fabsf(d) < __builtin_inff(); }      // false for NaN

// ------------------------------------------------------------------------------------------------------------------------
// normal map (utils3d stand-in).  p = depth_map_to_point_map: x = (u - cx) / fx * d, u = (j + 0.5) / W.  Neighbours in the order up, left,
// down, right; face k is spanned by neighbours k and k + 1 (mod 4): n_k = cross(a - p, b - p), which points at the camera (-z for a
// fronto-parallel plane).  A face counts when both neighbours are in the image and finite, the centre is finite, and the angle between n_k and
// the direction from p to the camera is below the threshold: -dot(n_k, p) / (|n_k| |p|) > cos_threshold.  normal = sum of the counted unit
// face normals (in face order), normalised; NaN x 3 without a counted face.  Norms are sqrt((x x + y y) + z z).
// ------------------------------------------------------------------------------------------------------------------------
struct TdVec { float x, y, z; };
__device__ __forceinline__ float td_norm(TdVec a) { return sqrtf((a.x * a.x + a.y * a.y) + a.z * a.z); }

__global__ __launch_bounds__(TD_THREADS) void td_normal_kernel(const float* depth, int H, int W, float fx, float fy, float cx, float cy, float cos_thr,
                                                               float* normal) {
    const long long o = (long long)blockIdx.x * TD_THREADS + threadIdx.x;
    if (o >= (long long)H * W) return;
    const int i = (int)(o / W), j = (int)(o - (long long)i * W);
    const float nanv = __builtin_nanf("");
    float* out = normal + 3 * o;
    const float d = depth[o];
    if (!td_finite(d)) { out[0] = out[1] = out[2] = nanv; return; }
    const int di[4] = {-1, 0, 1, 0}, dj[4] = {0, -1, 0, 1};
    TdVec e[4];
    bool ok[4];
    const float u = ((float)j + 0.5f) / (float)W, v = ((float)i + 0.5f) / (float)H;
    const TdVec p = {(u - cx) / fx * d, (v - cy) / fy * d, d};
    for (int k = 0; k < 4; k++) {
        const int y = i + di[k], x = j + dj[k];
        ok[k] = y >= 0 && y < H && x >= 0 && x < W;
        float dn = 0.f;
        if (ok[k]) { dn = depth[(size_t)y * W + x]; ok[k] = td_finite(dn); }
        const float un = ((float)x + 0.5f) / (float)W, vn = ((float)y + 0.5f) / (float)H;
        e[k] = {(un - cx) / fx * dn - p.x, (vn - cy) / fy * dn - p.y, dn - p.z};
    }
    const float lp = td_norm(p);
    TdVec acc = {0.f, 0.f, 0.f};
    int faces = 0;
    for (int k = 0; k < 4; k++) {
        const int k1 = (k + 1) & 3;
        if (!ok[k] || !ok[k1]) continue;
        const TdVec a = e[k], b = e[k1];
        const TdVec n = {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x};
        const float ln = td_norm(n);
        const float c = -((n.x * p.x + n.y * p.y) + n.z * p.z) / (ln * lp);
        if (!(c > cos_thr)) continue;
        acc.x = acc.x + n.x / ln; acc.y = acc.y + n.y / ln; acc.z = acc.z + n.z / ln;
        faces++;
    }
    if (!faces) { out[0] = out[1] = out[2] = nanv; return; }
    const float la = td_norm(acc);
    out[0] = acc.x / la; out[1] = acc.y / la; out[2] = acc.z / la;
}

// ------------------------------------------------------------------------------------------------------------------------
// depth edge (utils3d stand-in): over the in-image finite pixels of the k x k window, edge = log(max d) - log(min d) > ltol, never with a
// non-finite centre.  eligible = isfinite & ~edge as 0 / 1 float; known = ~isnan (the sparse mask of the nearest pre-resize).
// ------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(TD_THREADS) void td_edge_kernel(const float* depth, int H, int W, int ksize, float ltol, float* eligible, uint8_t* known) {
    const long long o = (long long)blockIdx.x * TD_THREADS + threadIdx.x;
    if (o >= (long long)H * W) return;
    const int i = (int)(o / W), j = (int)(o - (long long)i * W);
    const float d = depth[o];
    if (known) known[o] = d == d ? 1 : 0;
    if (!td_finite(d)) { eligible[o] = 0.f; return; }
    const int r = ksize / 2;
    float lo = d, hi = d;
    for (int y = max(i - r, 0); y <= min(i + r, H - 1); y++)
        for (int x = max(j - r, 0); x <= min(j + r, W - 1); x++) {
            const float t = depth[(size_t)y * W + x];
            if (!td_finite(t)) continue;
            lo = fminf(lo, t);
            hi = fmaxf(hi, t);
        }
    eligible[o] = (logf(hi) - logf(lo) > ltol) ? 0.f : 1.f;
}

// ------------------------------------------------------------------------------------------------------------------------
// warp.  Per target pixel (y, x): source coordinates (X, Y, Z) = Minv (x, y, 1) in fp32 ((m0 x + m1 y) + m2), s = (X / Z, Y / Z), once per
// source grid (image, nearest depth, raw).  Border constant 0 everywhere.
//   Lanczos-4: taps floor(s) - 3 .. floor(s) + 4 per axis; weights per axis by OpenCV's interpolateLanczos4 at the exact fraction t (float64
//     angle sums with the 45-degree table, each weight rounded to float, normalised by 1.f / their float sum; t < FLT_EPSILON is the unit tap);
//     the 64 products img * (wy[r] * wx[c]) accumulate in float in row-major order; rint, clip to uint8.
//   bilinear: (a (1 - fx) + b fx) (1 - fy) + (c (1 - fx) + d fx) fy with fx = s - floor(s); NaN and inf propagate, also through a zero weight
//     of an in-image tap.  fl(fl(1 - f) + f) == 1 for every f in [0, 1), so an all-ones source gives exactly 1.
//   nearest: rint (half to even).
// depth = eligible == 1 ? 1 / bilinear(1 / raw) : nearest, divided by (u zr0 + v zr1) + zr2 with zr = inv(transform)[2, :] and pixel-centre
// uv; normal = bilinear(normal) @ R^T.  flip: written to column OW - 1 - x with normal.x negated.  Finite depths are counted: one integer
// atomic per wave.
// ------------------------------------------------------------------------------------------------------------------------
struct TdMats { float img[9]; float nst[9]; float raw[9]; float R[9]; float zr[3]; };

__device__ __forceinline__ void td_coord(const float* m, float xf, float yf, float& sx, float& sy) {
    const float X = (m[0] * xf + m[1] * yf) + m[2];
    const float Y = (m[3] * xf + m[4] * yf) + m[5];
    const float Z = (m[6] * xf + m[7] * yf) + m[8];
    sx = X / Z;
    sy = Y / Z;
}

__device__ __forceinline__ void td_lanczos4(float t, float* w) {
    if (t < 1.1920928955078125e-7f) {
        for (int i = 0; i < 8; i++) w[i] = 0.f;
        w[3] = 1.f;
        return;
    }
    const double s45 = 0.70710678118654752440084436210485;
    const double cs[8][2] = {{1, 0}, {-s45, -s45}, {0, 1}, {s45, -s45}, {-1, 0}, {s45, s45}, {0, -1}, {-s45, s45}};
    const double y0 = -((double)t + 3) * M_PI * 0.25, s0 = sin(y0), c0 = cos(y0);
    float sum = 0.f;
    for (int i = 0; i < 8; i++) {
        const double y = -((double)t + 3 - i) * M_PI * 0.25;
        w[i] = (float)((cs[i][0] * s0 + cs[i][1] * c0) / (y * y));
        sum = sum + w[i];
    }
    sum = 1.f / sum;
    for (int i = 0; i < 8; i++) w[i] = w[i] * sum;
}

// the four taps and the two fractions of a bilinear sample at (sx, sy) of an (H, W) grid; false when no tap can be inside
struct TdTaps { int x0, y0; float fx, fy; bool in[4]; };
__device__ __forceinline__ bool td_taps(float sx, float sy, int H, int W, TdTaps& t) {
    if (!(sx > -2.f && sx < (float)W + 1.f && sy > -2.f && sy < (float)H + 1.f)) return false;
    const float flx = floorf(sx), fly = floorf(sy);
    t.x0 = (int)flx; t.y0 = (int)fly;
    t.fx = sx - flx; t.fy = sy - fly;
    for (int q = 0; q < 4; q++) {
        const int xx = t.x0 + (q & 1), yy = t.y0 + (q >> 1);
        t.in[q] = xx >= 0 && xx < W && yy >= 0 && yy < H;
    }
    return true;
}
__device__ __forceinline__ size_t td_tap_index(const TdTaps& t, int q, int W) { return (size_t)(t.y0 + (q >> 1)) * W + (t.x0 + (q & 1)); }
__device__ __forceinline__ float td_lerp(const float* v, float fx, float fy) {
    return (v[0] * (1.f - fx) + v[1] * fx) * (1.f - fy) + (v[2] * (1.f - fx) + v[3] * fx) * fy;
}

__global__ __launch_bounds__(TD_THREADS) void td_warp_kernel(const uint8_t* image, int ih, int iw, const float* nearest, int nh, int nw, const float* raw_depth,
                                                             const float* eligible, const float* normal, int H, int W, int OH, int OW, TdMats m, int flip,
                                                             uint8_t* out_u8, float* out_chw, float* out_depth, float* out_normal, uint8_t* out_bilinear, int32_t* count) {
    const long long o = (long long)blockIdx.x * TD_THREADS + threadIdx.x;
    const bool active = o < (long long)OH * OW;
    bool finite = false;
    if (active) {
        const int y = (int)(o / OW), x = (int)(o - (long long)y * OW);
        const float xf = (float)x, yf = (float)y;
        const size_t t_out = (size_t)y * OW + (flip ? OW - 1 - x : x);

        // image: Lanczos-4
        float sx, sy;
        td_coord(m.img, xf, yf, sx, sy);
        float acc[3] = {0.f, 0.f, 0.f};
        if (sx > -5.f && sx < (float)iw + 4.f && sy > -5.f && sy < (float)ih + 4.f) {
            const float flx = floorf(sx), fly = floorf(sy);
            const int x0 = (int)flx - 3, y0 = (int)fly - 3;
            float wx[8], wy[8];
            td_lanczos4(sx - flx, wx);
            td_lanczos4(sy - fly, wy);
            for (int r = 0; r < 8; r++) {
                const int yy = y0 + r;
                const bool rin = yy >= 0 && yy < ih;
                for (int c = 0; c < 8; c++) {
                    const int xx = x0 + c;
                    const float w = wy[r] * wx[c];
                    const bool in = rin && xx >= 0 && xx < iw;
                    const uint8_t* px = image + ((size_t)(in ? yy : 0) * iw + (in ? xx : 0)) * 3;
                    for (int ch = 0; ch < 3; ch++) acc[ch] = acc[ch] + (in ? (float)px[ch] : 0.f) * w;
                }
            }
        }
        for (int ch = 0; ch < 3; ch++) {
            const float r = rintf(acc[ch]);
            const uint8_t b = (uint8_t)(r < 0.f ? 0.f : (r > 255.f ? 255.f : r));
            out_u8[t_out * 3 + ch] = b;
            out_chw[(size_t)ch * OH * OW + t_out] = (float)b / 255.f;
        }

        // raw grid: eligibility, disparity, normal
        td_coord(m.raw, xf, yf, sx, sy);
        TdTaps t;
        float el = 0.f, bil = 0.f, nrm[3] = {0.f, 0.f, 0.f};
        if (td_taps(sx, sy, H, W, t)) {
            float ve[4], vd[4], vn[3][4];
            for (int q = 0; q < 4; q++) {
                const size_t s = t.in[q] ? td_tap_index(t, q, W) : 0;
                ve[q] = t.in[q] ? eligible[s] : 0.f;
                vd[q] = t.in[q] ? 1.f / raw_depth[s] : 0.f;
                for (int c = 0; c < 3; c++) vn[c][q] = t.in[q] ? normal[3 * s + c] : 0.f;
            }
            el = td_lerp(ve, t.fx, t.fy);
            bil = td_lerp(vd, t.fx, t.fy);
            for (int c = 0; c < 3; c++) nrm[c] = td_lerp(vn[c], t.fx, t.fy);
        }

        // nearest depth
        td_coord(m.nst, xf, yf, sx, sy);
        const float rx = rintf(sx), ry = rintf(sy);
        const bool inside = rx >= 0.f && rx <= (float)(nw - 1) && ry >= 0.f && ry <= (float)(nh - 1);
        const float near = inside ? nearest[(size_t)ry * nw + (size_t)rx] : 0.f;

        const float warped = el == 1.f ? 1.f / bil : near;
        const float u = (xf + 0.5f) / (float)OW, v = (yf + 0.5f) / (float)OH;
        const float d = warped / ((u * m.zr[0] + v * m.zr[1]) + m.zr[2]);
        out_depth[t_out] = d;
        if (out_bilinear) out_bilinear[t_out] = el == 1.f ? 1 : 0;
        finite = td_finite(d);

        float* on = out_normal + 3 * t_out;
        const float n0 = (nrm[0] * m.R[0] + nrm[1] * m.R[1]) + nrm[2] * m.R[2];
        on[0] = flip ? -n0 : n0;
        on[1] = (nrm[0] * m.R[3] + nrm[1] * m.R[4]) + nrm[2] * m.R[5];
        on[2] = (nrm[0] * m.R[6] + nrm[1] * m.R[7]) + nrm[2] * m.R[8];
    }
    const unsigned long long vote = __ballot(finite);
    if ((threadIdx.x & 63) == 0 && vote) atomicAdd(count, (int32_t)__popcll(vote));
}

// ------------------------------------------------------------------------------------------------------------------------
// finish.  fallback = float64(count) / float64(n) < 0.001 (the reference's `isfinite.sum() / size`): depth = 1 everywhere and *invalid = 1.
// Then depth *= unit; max_depth = nanquantile(finite depths, q) * clamp; finite depths are clipped to [0, max_depth]; mask_inf = isinf,
// mask_fin = isfinite (only_known) or ~isinf.
// ------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(TD_THREADS) void td_prepare_kernel(float* depth, int n, const int32_t* count, float unit, int has_unit, int32_t* invalid) {
    const bool fallback = (double)*count / (double)n < 0.001;
    if (blockIdx.x == 0 && threadIdx.x == 0) *invalid = fallback ? 1 : 0;
    if (!fallback && !has_unit) return;
    for (int i = blockIdx.x * TD_THREADS + threadIdx.x; i < n; i += TD_BLOCKS * TD_THREADS) {
        float d = fallback ? 1.f : depth[i];
        if (has_unit) d = d * unit;
        depth[i] = d;
    }
}

struct TdValid {
    __device__ __forceinline__ bool operator()(int, float d) const { return td_finite(d); }
};

__global__ __launch_bounds__(TD_THREADS) void td_hist_kernel(const float* depth, int n, int pass, const uint32_t* state, uint32_t* hist) {
    q_hist_body(depth, TdValid{}, n, pass, state, hist);
}

__global__ void td_select_kernel(int pass, float q, float clamp, uint32_t* state, uint32_t* hist) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    q_select_body(pass, q, clamp, state, hist);
}

__global__ __launch_bounds__(TD_THREADS) void td_clamp_kernel(float* depth, int n, const uint32_t* state, int only_known, uint8_t* mask_fin, uint8_t* mask_inf) {
    const float md = __uint_as_float(state[5]);
    for (int i = blockIdx.x * TD_THREADS + threadIdx.x; i < n; i += TD_BLOCKS * TD_THREADS) {
        float d = depth[i];
        const bool fin = td_finite(d), inf = !fin && d == d;
        if (fin) {
            d = d < 0.f ? 0.f : d;
            d = d > md ? md : d;
            depth[i] = d;
        }
        mask_inf[i] = inf ? 1 : 0;
        mask_fin[i] = (only_known ? fin : !inf) ? 1 : 0;
    }
}

static bool td_matrix_ok(const float* m) {
    for (int i = 0; i < 9; i++)
        if (!std::isfinite(m[i])) return false;
    const double det = (double)m[0] * ((double)m[4] * m[8] - (double)m[5] * m[7]) - (double)m[1] * ((double)m[3] * m[8] - (double)m[5] * m[6]) +
                       (double)m[2] * ((double)m[3] * m[7] - (double)m[4] * m[6]);
    return det != 0.0;
}

extern "C" {

int moge_train_normal_map(const float* depth, int H, int W, float fx, float fy, float cx, float cy, float edge_threshold_deg, float* normal, void* stream) {
    if (!depth || !normal) return moge_internal_fail(MOGE_ERR_INVALID, "moge_train_normal_map: null argument");
    if (H < 1 || W < 1) return moge_internal_fail(MOGE_ERR_INVALID, "moge_train_normal_map: empty map");
    if (!(fx != 0.f && fy != 0.f) || !(edge_threshold_deg > 0.f && edge_threshold_deg <= 180.f))
        return moge_internal_fail(MOGE_ERR_INVALID, "moge_train_normal_map: zero focal length or edge threshold outside (0, 180]");
    const float cos_thr = (float)cos((double)edge_threshold_deg * M_PI / 180.0);
    hipLaunchKernelGGL(td_normal_kernel, dim3(blocks((long long)H * W, TD_THREADS)), dim3(TD_THREADS), 0, (hipStream_t)stream, depth, H, W, fx, fy, cx, cy, cos_thr,
                       normal);
    return launched("moge_train_normal_map: launch failed");
}

int moge_train_depth_edge(const float* depth, int H, int W, int kernel_size, float ltol, float* eligible, uint8_t* known, void* stream) {
    if (!depth || !eligible) return moge_internal_fail(MOGE_ERR_INVALID, "moge_train_depth_edge: null argument");
    if (H < 1 || W < 1) return moge_internal_fail(MOGE_ERR_INVALID, "moge_train_depth_edge: empty map");
    if (kernel_size < 1 || kernel_size > 15 || !(kernel_size & 1)) return moge_internal_fail(MOGE_ERR_INVALID, "moge_train_depth_edge: kernel size not odd in [1, 15]");
    hipLaunchKernelGGL(td_edge_kernel, dim3(blocks((long long)H * W, TD_THREADS)), dim3(TD_THREADS), 0, (hipStream_t)stream, depth, H, W, kernel_size, ltol, eligible,
                       known);
    return launched("moge_train_depth_edge: launch failed");
}

int moge_train_warp(const uint8_t* image, int ih, int iw, const float* nearest, int nh, int nw, const float* raw_depth, const float* eligible, const float* normal,
                    int H, int W, int out_h, int out_w, const float* mats, int flip, uint8_t* out_u8, float* out_chw, float* out_depth, float* out_normal,
                    uint8_t* out_bilinear, int32_t* count, void* stream) {
    if (!image || !nearest || !raw_depth || !eligible || !normal || !mats || !out_u8 || !out_chw || !out_depth || !out_normal || !count)
        return moge_internal_fail(MOGE_ERR_INVALID, "moge_train_warp: null argument");
    if (ih < 1 || iw < 1 || nh < 1 || nw < 1 || H < 1 || W < 1 || out_h < 1 || out_w < 1) return moge_internal_fail(MOGE_ERR_INVALID, "moge_train_warp: empty map");
    if ((long long)out_h * out_w > 0x7fffffffLL) return moge_internal_fail(MOGE_ERR_INVALID, "moge_train_warp: target above 2^31 - 1 pixels");
    if (!td_matrix_ok(mats) || !td_matrix_ok(mats + 9) || !td_matrix_ok(mats + 18)) return moge_internal_fail(MOGE_ERR_INVALID, "moge_train_warp: singular or non-finite matrix");
    hipStream_t st = (hipStream_t)stream;
    TdMats m;
    for (int i = 0; i < 9; i++) { m.img[i] = mats[i]; m.nst[i] = mats[9 + i]; m.raw[i] = mats[18 + i]; m.R[i] = mats[27 + i]; }
    for (int i = 0; i < 3; i++) m.zr[i] = mats[36 + i];
    if (hipMemsetAsync(count, 0, sizeof(int32_t), st) != hipSuccess) return moge_internal_fail(MOGE_ERR_HIP, "moge_train_warp: memset failed");
    hipLaunchKernelGGL(td_warp_kernel, dim3(blocks((long long)out_h * out_w, TD_THREADS)), dim3(TD_THREADS), 0, st, image, ih, iw, nearest, nh, nw, raw_depth, eligible,
                       normal, H, W, out_h, out_w, m, flip ? 1 : 0, out_u8, out_chw, out_depth, out_normal, out_bilinear, count);
    return launched("moge_train_warp: launch failed");
}

int moge_train_finish(float* depth, int n, const int32_t* count, float depth_unit, int has_unit, float q, float clamp_max_depth, int only_known,
                      uint32_t* workspace, uint8_t* mask_fin, uint8_t* mask_inf, int32_t* invalid, void* stream) {
    if (!depth || !count || !workspace || !mask_fin || !mask_inf || !invalid || n < 1) return moge_internal_fail(MOGE_ERR_INVALID, "moge_train_finish: null argument or n < 1");
    if (!(q >= 0.f && q <= 1.f)) return moge_internal_fail(MOGE_ERR_INVALID, "moge_train_finish: q outside [0, 1]");
    hipStream_t st = (hipStream_t)stream;
    uint32_t* state = workspace;
    uint32_t* hist = workspace + 8;
    if (hipMemsetAsync(workspace, 0, MOGE_EVAL_QUANTILE_WORKSPACE * sizeof(uint32_t), st) != hipSuccess) return moge_internal_fail(MOGE_ERR_HIP, "moge_train_finish: memset failed");
    hipLaunchKernelGGL(td_prepare_kernel, dim3(TD_BLOCKS), dim3(TD_THREADS), 0, st, depth, n, count, depth_unit, has_unit, invalid);
    if (int rc = launched("moge_train_finish: prepare launch failed")) return rc;
    for (int pass = 0; pass < 4; pass++) {
        hipLaunchKernelGGL(td_hist_kernel, dim3(TD_BLOCKS), dim3(TD_THREADS), 0, st, depth, n, pass, state, hist);
        if (int rc = launched("moge_train_finish: histogram launch failed")) return rc;
        hipLaunchKernelGGL(td_select_kernel, dim3(1), dim3(64), 0, st, pass, q, clamp_max_depth, state, hist);
        if (int rc = launched("moge_train_finish: select launch failed")) return rc;
    }
    hipLaunchKernelGGL(td_clamp_kernel, dim3(TD_BLOCKS), dim3(TD_THREADS), 0, st, depth, n, state, only_known, mask_fin, mask_inf);
    return launched("moge_train_finish: clamp launch failed");
}

}  // extern "C"
