// Normal-guided depth refinement (reference moge/utils/geometry_torch.py:206-233, refine_depth_with_normal): a
// bilateral-weighted, normal-driven Jacobi relaxation of log-depth.  Stateless kernels on the caller's stream; every pointer is device memory.
//
//   prep        x0 = log(max(depth, eps)), g = the log-depth gradient the normal implies, lap = the clamped weighted sum of the g terms
//   iteration   x <- 0.1 x + 0.9 (damp x0 - lap + sum_t w_t x[p + t]) / (max(sum_t w_t, eps) + damp) on the interior, ring of width r keeps x0
//               (evaluated as x + 0.9 (damp (x0 - x) - lap + sum_t w_t (x[p + t] - x)) / (...): the same value, sums over differences)
//
// No per-tap quantity reaches HBM: the weights w_t = exp(-((x0[p+t] - x0[p]) / max(|duv_t|, eps) / 10)^2) are recomputed from an LDS tile of x0
// wherever they are used (one v_exp_f32 per tap; the per-tap factor -(1 / (10 max(|duv_t|, eps)))^2 log2(e) comes from the host in the kernel
// arguments).  Device memory: four fp32 planes per image (x0, lap, two iterates).  One launch per iteration on 32 x 32 tiles, ping-pong planes: it
// beat several iterations per launch on an LDS tile with an r * steps halo (EXPERIMENTS.md R8.2).
//
// fp32 planes and fp32 arithmetic with NO contraction (the pragma below; the two accumulations are written as fmaf, the same in the masked and
// the unmasked instantiation, so an all-true mask gives the bits of no mask).  One departure from fp32: the two end transforms, log at the start
// and exp at the end (once per pixel per call), are evaluated in double and rounded once, so x0 is the correctly rounded fp32 log and the output of
// no iterations is within 2 ulp of exp(x0) - not of depth itself: storing x0 in fp32 already costs |x0| / 2 ulp of depth.  With a mask, masked-out pixels carry a NaN in the x0 plane; a tap that sees it is skipped by a select, so nothing under
// the mask enters the arithmetic, and the output there is the input's bits.  One workgroup works on one image: a batch gives the bits of its images alone.
#include <climits>
#include <cmath>

#include "common.h"
#include "../../include/moge_hip.h"

#pragma clang fp contract(off)

constexpr int REFINE_TILE = 32;          // output tile of a workgroup (square); moge_amd/refine.py TILE mirrors it for the tests
constexpr int REFINE_THREADS = 256;
constexpr int REFINE_PX = 4;             // vertically adjacent pixels per thread: their windows share (PX + 2r) x k LDS reads
constexpr int REFINE_MAX_R = 3;

struct RefineArgs {
    const float* depth; const float* normal; const float* intrinsics; const uint8_t* mask;
    float* x0; float* lap; const float* src; float* dst; float* out;
    int H, W, last;
    float damp, eps, inv_w, inv_h;
    float c2[(REFINE_MAX_R + 1) * (REFINE_MAX_R + 1)];      // [|row offset|][|column offset|]: exp2(c2 * dx^2) is the tap's weight
};

__device__ __forceinline__ float refine_weight(float c2, float xt, float xp) {
    const float d = xt - xp;
    return __builtin_amdgcn_exp2f(c2 * (d * d));
}

__device__ __forceinline__ float refine_exp(float x) { return (float)exp((double)x); }

// ------------------------------------------------------------------------------------------------------------------------
// prep: x0 and lap planes of one tile (and the output itself when there is no iteration to run)
// ------------------------------------------------------------------------------------------------------------------------
template <int K, bool MASKED>
__global__ __launch_bounds__(REFINE_THREADS) void refine_prep_kernel(RefineArgs g, int write_out) {
    constexpr int R = K / 2, T = REFINE_TILE, S = T + 2 * R;
    __shared__ float sx[S * S], sgx[S * S], sgy[S * S];
    const int H = g.H, W = g.W, ox = blockIdx.x * T, oy = blockIdx.y * T;
    const size_t plane = (size_t)blockIdx.z * H * W;

    // inverse(K), rows 0 and 1, by the adjugate
    const float* Km = g.intrinsics + (size_t)blockIdx.z * 9;
    const float k00 = Km[0], k01 = Km[1], k02 = Km[2], k10 = Km[3], k11 = Km[4], k12 = Km[5], k20 = Km[6], k21 = Km[7], k22 = Km[8];
    const float a00 = k11 * k22 - k12 * k21, a01 = k02 * k21 - k01 * k22, a02 = k01 * k12 - k02 * k11;
    const float a10 = k12 * k20 - k10 * k22, a11 = k00 * k22 - k02 * k20, a12 = k02 * k10 - k00 * k12;
    const float a20 = k10 * k21 - k11 * k20;
    const float idet = 1.0f / (k00 * a00 + k01 * a10 + k02 * a20);
    const float i00 = a00 * idet, i01 = a01 * idet, i02 = a02 * idet, i10 = a10 * idet, i11 = a11 * idet, i12 = a12 * idet;

    for (int idx = threadIdx.x; idx < S * S; idx += REFINE_THREADS) {
        const int ly = idx / S, lx = idx - ly * S, y = oy - R + ly, x = ox - R + lx;
        float xv = 0.f, gx = 0.f, gy = 0.f;
        if (y >= 0 && y < H && x >= 0 && x < W) {
            const size_t p = plane + (size_t)y * W + x;
            const float d = g.depth[p];
            xv = (float)log((double)(d < g.eps ? g.eps : d));               // clamp_min: a NaN stays a NaN
            const float nx = g.normal[3 * p], ny = g.normal[3 * p + 1], nz = g.normal[3 * p + 2];
            const float u = ((float)x + 0.5f) * g.inv_w, v = ((float)y + 0.5f) * g.inv_h;
            const float den = nz + (nx * (i00 * u + i01 * v + i02) + ny * (i10 * u + i11 * v + i12));
            gx = -(nx * i00 + ny * i10) / den;
            gy = -(nx * i01 + ny * i11) / den;
            if (MASKED && !g.mask[p]) xv = __builtin_nanf("");
        }
        sx[idx] = xv; sgx[idx] = gx; sgy[idx] = gy;
    }
    __syncthreads();

    for (int idx = threadIdx.x; idx < T * T; idx += REFINE_THREADS) {
        const int ty = idx / T, tx = idx - ty * T, y = oy + ty, x = ox + tx;
        if (y >= H || x >= W) continue;
        const int c = (ty + R) * S + tx + R;
        const size_t p = plane + (size_t)y * W + x;
        const float xp = sx[c];
        const bool valid = !MASKED || xp == xp;
        float lap = 0.f;
        if (valid && x >= R && x <= W - 1 - R && y >= R && y <= H - 1 - R) {
            const float gxp = sgx[c], gyp = sgy[c];
#pragma unroll
            for (int a = 0; a < K; a++) {
#pragma unroll
                for (int b = 0; b < K; b++) {
                    if (a == R && b == R) continue;                         // the centre tap has duv = 0
                    const int q = c + (a - R) * S + (b - R);
                    const float xt = sx[q];
                    const float w = refine_weight(g.c2[(a > R ? a - R : R - a) * (REFINE_MAX_R + 1) + (b > R ? b - R : R - b)], xt, xp);
                    const float du = (float)(b - R) * g.inv_w, dv = (float)(a - R) * g.inv_h;
                    const float term = w * (((sgx[q] + gxp) * du + (sgy[q] + gyp) * dv) * 0.5f);
                    if (!MASKED || xt == xt) lap += term;
                }
            }
            lap = fminf(fmaxf(lap, -0.1f), 0.1f);
        }
        g.x0[p] = xp;
        g.lap[p] = lap;
        if (write_out) g.out[p] = valid ? refine_exp(xp) : g.depth[p];
    }
}

// ------------------------------------------------------------------------------------------------------------------------
// iteration: one Jacobi iteration of one tile, to the dst plane or (the last one) as exp(x) to the output.  32 columns x 8 strips of 4 rows:
// one strip per thread
// ------------------------------------------------------------------------------------------------------------------------
template <int K, bool MASKED>
__global__ __launch_bounds__(REFINE_THREADS) void refine_iter_kernel(RefineArgs g) {
    constexpr int R = K / 2, PX = REFINE_PX, T = REFINE_TILE, S = T + 2 * R;
    static_assert(T % PX == 0 && T * (T / PX) == REFINE_THREADS, "one strip of PX pixels per thread");
    __shared__ float sx0[S * S], cur[S * S];
    const int H = g.H, W = g.W, ox = blockIdx.x * T, oy = blockIdx.y * T;
    const size_t plane = (size_t)blockIdx.z * H * W;

    for (int idx = threadIdx.x; idx < S * S; idx += REFINE_THREADS) {
        const int ly = idx / S, lx = idx - ly * S, y = oy - R + ly, x = ox - R + lx;
        float a = 0.f, b = 0.f;
        if (y >= 0 && y < H && x >= 0 && x < W) {
            const size_t p = plane + (size_t)y * W + x;
            a = g.x0[p];
            b = g.src[p];
        }
        sx0[idx] = a; cur[idx] = b;
    }
    __syncthreads();

    const int tx = threadIdx.x % T, ty0 = (threadIdx.x / T) * PX, x = ox + tx, y0 = oy + ty0;
    if (x >= W) return;
    const bool col_in = x >= R && x <= W - 1 - R;
    float p0[PX + 2 * R][K], pv[PX + 2 * R][K];                    // rows ty0 - R .. ty0 + PX - 1 + R, columns tx - R .. tx + R of the tile
#pragma unroll
    for (int a = 0; a < PX + 2 * R; a++) {
#pragma unroll
        for (int b = 0; b < K; b++) {
            const int q = (ty0 + a) * S + tx + b;
            p0[a][b] = sx0[q];
            pv[a][b] = cur[q];
        }
    }
#pragma unroll
    for (int j = 0; j < PX; j++) {
        const int y = y0 + j;
        if (y >= H) continue;
        const float xp = p0[j + R][R], xc = pv[j + R][R];
        const bool valid = !MASKED || xp == xp;
        float nv = xc;
        if (valid && col_in && y >= R && y <= H - 1 - R) {
            float tot = 1.0f, acc = 0.f;                                // the centre tap: weight exp(0) = 1, difference 0
#pragma unroll
            for (int a = 0; a < K; a++) {
#pragma unroll
                for (int b = 0; b < K; b++) {
                    if (a == R && b == R) continue;
                    const float xt = p0[j + a][b];
                    const float w = refine_weight(g.c2[(a > R ? a - R : R - a) * (REFINE_MAX_R + 1) + (b > R ? b - R : R - b)], xt, xp);
                    if (!MASKED || xt == xt) {
                        tot += w;
                        acc = fmaf(w, pv[j + a][b] - xc, acc);
                    }
                }
            }
            // 0.1 x + 0.9 (damp x0 - lap + sum w x[p+t]) / (tot + damp) with sum w x[p+t] = (sum w) x + sum w (x[p+t] - x): the same
            // value, accumulated on the differences, so the rounding error scales with the update and not with |x| * sum w
            const float totc = fmaxf(tot, g.eps);
            nv = xc + 0.9f * (((fmaf(g.damp, xp - xc, acc) - g.lap[plane + (size_t)y * W + x]) + (tot - totc) * xc) / (totc + g.damp));
        }
        const size_t p = plane + (size_t)y * W + x;
        if (!g.last) g.dst[p] = nv;
        else g.out[p] = valid ? refine_exp(nv) : g.depth[p];
    }
}

// ------------------------------------------------------------------------------------------------------------------------
// host
// ------------------------------------------------------------------------------------------------------------------------
template <int K, bool MASKED>
static int refine_run(RefineArgs g, int B, int iterations, float* xa, float* xb, hipStream_t st) {
    const dim3 grid(blocks(g.W, REFINE_TILE), blocks(g.H, REFINE_TILE), (unsigned)B);
    hipLaunchKernelGGL((refine_prep_kernel<K, MASKED>), grid, dim3(REFINE_THREADS), 0, st, g, iterations == 0 ? 1 : 0);
    const float* src = g.x0;                        // x0 -> A -> B -> A ...: a plane is never updated in place; the last iteration writes `out`
    float* dst = xa;
    for (int i = 0; i < iterations; i++) {
        g.src = src; g.dst = dst; g.last = i == iterations - 1;
        hipLaunchKernelGGL((refine_iter_kernel<K, MASKED>), grid, dim3(REFINE_THREADS), 0, st, g);
        src = dst;
        dst = dst == xa ? xb : xa;
    }
    return launched("moge_refine_depth: launch failed");
}

static int refine_check(int B, int H, int W, const char* who) {
    if (B < 0 || B > 65535 || H < 1 || W < 1 || H > 65535 * REFINE_TILE || (int64_t)H * W > INT_MAX)      // grid.y, grid.z <= 65535
        return moge_internal_fail(MOGE_ERR_INVALID, "%s: need 0 <= B <= 65535, 1 <= H <= %d and H * W < 2^31, got B = %d, H = %d, W = %d", who, 65535 * REFINE_TILE, B, H, W);
    return 0;
}

extern "C" {

int moge_refine_depth_workspace(int B, int H, int W, int64_t* bytes) {
    if (!bytes) return moge_internal_fail(MOGE_ERR_INVALID, "moge_refine_depth_workspace: null argument");
    *bytes = 0;
    if (int rc = refine_check(B, H, W, "moge_refine_depth_workspace")) return rc;
    *bytes = 4 * (int64_t)B * H * W * (int64_t)sizeof(float);           // x0, lap, two iterates
    return 0;
}

int moge_refine_depth(const float* depth, const float* normal, const float* intrinsics, const uint8_t* mask, int B, int H, int W, int kernel_size,
                      int iterations, float damp, float eps, void* workspace, float* out, void* stream) {
    if (!depth || !normal || !intrinsics || !workspace || !out) return moge_internal_fail(MOGE_ERR_INVALID, "moge_refine_depth: null argument");
    if (int rc = refine_check(B, H, W, "moge_refine_depth")) return rc;
    if (kernel_size != 3 && kernel_size != 5 && kernel_size != 7) return moge_internal_fail(MOGE_ERR_INVALID, "moge_refine_depth: kernel_size must be 3, 5 or 7");
    if (H < kernel_size || W < kernel_size) return moge_internal_fail(MOGE_ERR_INVALID, "moge_refine_depth: the map is smaller than the window");
    if (iterations < 0) return moge_internal_fail(MOGE_ERR_INVALID, "moge_refine_depth: iterations < 0");
    if (B == 0) return 0;
    const size_t n = (size_t)B * H * W;
    float* ws = (float*)workspace;
    RefineArgs g{};
    g.depth = depth; g.normal = normal; g.intrinsics = intrinsics; g.mask = mask;
    g.x0 = ws; g.lap = ws + n; g.out = out;
    g.H = H; g.W = W; g.damp = damp; g.eps = eps; g.inv_w = 1.0f / (float)W; g.inv_h = 1.0f / (float)H;
    for (int i = 0; i <= REFINE_MAX_R; i++)
        for (int j = 0; j <= REFINE_MAX_R; j++) {
            double norm = std::sqrt((double)j * j / ((double)W * W) + (double)i * i / ((double)H * H));
            if (norm < (double)eps) norm = (double)eps;
            const double s = 1.0 / (norm * 10.0);
            g.c2[i * (REFINE_MAX_R + 1) + j] = (float)(-s * s * 1.4426950408889634);        // the centre's (0, 0) entry is never read
        }
    float *xa = ws + 2 * n, *xb = ws + 3 * n;
    hipStream_t st = (hipStream_t)stream;
    switch (kernel_size * 2 + (mask ? 1 : 0)) {
        case 6: return refine_run<3, false>(g, B, iterations, xa, xb, st);
        case 7: return refine_run<3, true>(g, B, iterations, xa, xb, st);
        case 10: return refine_run<5, false>(g, B, iterations, xa, xb, st);
        case 11: return refine_run<5, true>(g, B, iterations, xa, xb, st);
        case 14: return refine_run<7, false>(g, B, iterations, xa, xb, st);
        default: return refine_run<7, true>(g, B, iterations, xa, xb, st);
    }
}

}   // extern "C"
