// Panorama split and merge (the device form of moge_amd/panorama.py split_panorama_image and merge_panorama_depth; python mirror
// moge_amd/panorama_gpu.py).  Stateless kernels on the caller's stream; every pointer is device memory unless stated.
//
//   split      one thread per output pixel of a view: ray, atan2 / acos and the source pixel coordinates in fp64, the bilinear weights and the
//              blend in fp32 in the host's expression order, border = constant 0; uint8: rint (half-even) then clip
//   system     (a) per view and panorama pixel: fp64 projection, the `inside` test, the bilinear sample of log(distance) (log per tap in fp64,
//              rounded once to fp32; replicated border), the nearest mask sample -> an fp32 plane and a byte plane per view
//              (b) per panorama pixel, the views IN VIEW ORDER in fp32: the wrapped right difference, the lower difference and the 5-point
//              Laplacian, their masked means (divisor max(count, 1e-3), in fp64 as numpy's mixed-type division), the three "any" masks and seen
//   operator   A is never stored.  Row layout of u (and of b and of the row mask), M = N + (H-1) W + (H-1) + N rows for N = H W pixels:
//                [0, N)                 x rows      v[i, j] - v[i, (j+1) % W]
//                [N, N + (H-1) W)       y rows      v[i, j] - v[i+1, j]
//                [.., + (H-1))          the column-0 y rows once more (the reference enters them twice, the host keeps them)
//                [.., + N)              Laplacian   v[i-1, j] + v[i+1, j] + v[i, j-1] + v[i, j+1] - 4 v[i, j], x wraps, the top / bottom row replicated
//              Rows the mask does not select are zero rows.  A v is a gather stencil per row, A^T u a gather over the at most 11 rows that touch
//              a pixel: no scatter, no floating-point atomics.
//   LSMR       scipy.sparse.linalg.lsmr (damp = 0) in fp64, six launches per iteration:
//                1 av      u~ = (u~ / beta) (-alpha) + A (v~ / alpha) on the selected rows, partial sums of squares     (u~, v~: the unnormalised
//                2 beta    one workgroup: beta = sqrt(sum of the partials in index order)                                 vectors; 1 / beta and
//                3 atu     v~ = (v~ / alpha) (-beta) + A^T (u~ / beta), partial sums of squares                           1 / alpha are applied by
//                4 givens  one workgroup: alpha, the plane rotations, the norm estimates, the update coefficients         whoever reads them)
//                5 update  hbar, x, h; partial sums of x^2
//                6 test    one workgroup: normx, the stopping rule -> the device-side `stop` word, istop, itn
//              Every kernel returns at once when `stop` is set, so x is the iterate at which the rule first held however many launches were
//              queued behind it.  The host enqueues `poll` iterations, reads the state once, and goes on while it says so, at most maxiter
//              iterations in all.  Norms are fixed-order two-level sums (per workgroup of PANO_SPAN elements, then one workgroup over the
//              partials): two runs give the same bits and the same itn.  No workgroup waits on another; every step is a launch of its own.
#include <climits>
#include <cmath>

#include "common.h"
#include "../../include/moge_hip.h"

#pragma clang fp contract(off)

constexpr int PANO_THREADS = 256;
constexpr int PANO_ITEMS = MOGE_PANO_SPAN / PANO_THREADS;        // elements of a thread in the reducing kernels: e = block * SPAN + k * THREADS + thread
constexpr double PANO_PI = 3.141592653589793;
static_assert(PANO_ITEMS * PANO_THREADS == MOGE_PANO_SPAN, "a workgroup covers MOGE_PANO_SPAN elements");

struct PanoCams {                   // by value in the kernel arguments: rotation rows (world -> camera) and fx, fy, cx, cy, as the host's float64 copies
    double R[MOGE_PANO_MAX_VIEWS][9];
    double K[MOGE_PANO_MAX_VIEWS][4];
};

struct PanoDims { int W, H, N, oY, oE, oL, M; };     // offsets of the y rows, the extra column-0 rows and the Laplacian rows

struct PanoState {                  // the solver's scalars, in device memory (lsmr.py's names)
    double alpha, beta, inv_alpha, inv_beta, normb;
    double zetabar, alphabar, rho, rhobar, cbar, sbar;
    double betadd, betad, rhodold, tautildeold, thetatilde, zeta, d;
    double normA2, maxrbar, minrbar, normA, condA, normx, normr, normar;
    double c_hbar, c_x, c_h;        // this iteration's coefficients of the vector update
    double atol, btol, ctol;
    long long rows;                 // selected rows
    int stop, itn, istop, maxiter, beta_zero, zero_x;
};
static_assert(sizeof(PanoState) <= 8 * MOGE_PANO_STATE_DOUBLES, "the state fits its slot of the workspace");

struct PanoWs {
    double *u, *v, *h, *hbar, *part, *part_b;
    long long* part_rows;
    PanoState* state;
    float* logd;                    // [n][N]
    uint8_t* m;                     // [n][N]
    int P;
};

static PanoDims pano_dims(int width, int height) {
    PanoDims D;
    D.W = width; D.H = height; D.N = width * height;
    D.oY = D.N; D.oE = D.oY + (height - 1) * width; D.oL = D.oE + (height - 1); D.M = D.oL + D.N;
    return D;
}

static PanoWs pano_ws(void* workspace, const PanoDims& D) {
    PanoWs w;
    w.P = (int)blocks(D.M, MOGE_PANO_SPAN);
    w.u = (double*)workspace;
    w.v = w.u + D.M;
    w.h = w.v + D.N;
    w.hbar = w.h + D.N;
    w.part = w.hbar + D.N;
    w.part_b = w.part + w.P;
    w.part_rows = (long long*)(w.part_b + w.P);
    w.state = (PanoState*)(w.part_rows + w.P);
    w.logd = (float*)((double*)w.state + MOGE_PANO_STATE_DOUBLES);
    w.m = (uint8_t*)w.logd;         // + 4 n N, set by the caller that knows n
    return w;
}

// ------------------------------------------------------------------------------------------------------------------------
// sampling
// ------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ float pano_blend(float t00, float t01, float t10, float t11, float fx, float fy) {       // panorama.py _remap_bilinear
    return (t00 * (1.0f - fx) + t01 * fx) * (1.0f - fy) + (t10 * (1.0f - fx) + t11 * fx) * fy;
}

__device__ __forceinline__ int pano_clampi(long long v, int hi) { return (int)(v < 0 ? 0 : (v > hi ? hi : v)); }

__device__ __forceinline__ void pano_direction(int i, int j, int H, int W, double* d) {      // spherical_uv_to_directions(_uv_grid(H, W))[i, j]
    const double u = ((double)j + 0.5) / (double)W, v = ((double)i + 0.5) / (double)H;
    const double theta = (1.0 - u) * (2.0 * PANO_PI), phi = v * PANO_PI;
    const double s = sin(phi);
    d[0] = s * cos(theta); d[1] = s * sin(theta); d[2] = cos(phi);
}

template <typename T>
__global__ __launch_bounds__(PANO_THREADS) void pano_split_kernel(const T* img, int H, int W, PanoCams cams, int res, T* out) {
    const int p = blockIdx.x * PANO_THREADS + threadIdx.x, view = blockIdx.y;
    if (p >= res * res) return;
    const int y = p / res, x = p - y * res;
    const double* R = cams.R[view];
    const double* K = cams.K[view];
    const double u = ((double)x + 0.5) / (double)res, v = ((double)y + 0.5) / (double)res;
    const double c0 = (u - K[2]) / K[0], c1 = (v - K[3]) / K[1];
    const double r0 = c0 * R[0] + c1 * R[3] + R[6], r1 = c0 * R[1] + c1 * R[4] + R[7], r2 = c0 * R[2] + c1 * R[5] + R[8];       // cam @ R
    const double nrm = sqrt(r0 * r0 + r1 * r1 + r2 * r2);
    const double d0 = r0 / nrm, d1 = r1 / nrm, d2 = r2 / nrm;
    double md = fmod(atan2(d1, d0) / (2.0 * PANO_PI), 1.0);          // numpy's %: the sign of the divisor
    if (md < 0.0) md += 1.0;
    const double su = 1.0 - md, sv = acos(fmin(fmax(d2, -1.0), 1.0)) / PANO_PI;
    const double px = su * (double)W - 0.5, py = sv * (double)H - 0.5;
    const double fx0 = floor(px), fy0 = floor(py);
    const int x0 = (int)fx0, y0 = (int)fy0;
    const float fx = (float)(px - fx0), fy = (float)(py - fy0);
    T* o = out + ((int64_t)view * res * res + p) * 3;
    for (int c = 0; c < 3; c++) {
        auto tap = [&](int yy, int xx) -> float {
            return (xx >= 0 && xx < W && yy >= 0 && yy < H) ? (float)img[((int64_t)yy * W + xx) * 3 + c] : 0.0f;
        };
        const float r = pano_blend(tap(y0, x0), tap(y0, x0 + 1), tap(y0 + 1, x0), tap(y0 + 1, x0 + 1), fx, fy);
        if constexpr (sizeof(T) == 1) o[c] = (T)fminf(fmaxf(rintf(r), 0.0f), 255.0f);
        else o[c] = r;
    }
}

// (a) of the system: view blockIdx.y warped onto the panorama grid
__global__ __launch_bounds__(PANO_THREADS) void pano_warp_kernel(const float* dist, const uint8_t* mask, int vh, int vw, PanoCams cams, int H, int W,
                                                                 float* logd, uint8_t* m) {
    const int p = blockIdx.x * PANO_THREADS + threadIdx.x, view = blockIdx.y, N = H * W;
    if (p >= N) return;
    const int i = p / W, j = p - i * W;
    const double* R = cams.R[view];
    const double* K = cams.K[view];
    double d[3];
    pano_direction(i, j, H, W, d);
    const double cx = d[0] * R[0] + d[1] * R[1] + d[2] * R[2], cy = d[0] * R[3] + d[1] * R[4] + d[2] * R[5], z = d[0] * R[6] + d[1] * R[7] + d[2] * R[8];
    const double zs = fabs(z) > 1e-12 ? z : 1e-12;
    double pu = K[0] * cx / zs + K[2], pv = K[1] * cy / zs + K[3];
    const bool inside = z > 0.0 && pu > 0.0 && pv > 0.0 && pu < 1.0 && pv < 1.0;
    pu = fmin(fmax(pu, 0.0), 1.0); pv = fmin(fmax(pv, 0.0), 1.0);
    const double px = pu * (double)vw - 0.5, py = pv * (double)vh - 0.5;
    float val = 0.0f;
    bool mk = false;
    if (inside) {
        const float* src = dist + (int64_t)view * vh * vw;
        const double fx0 = floor(px), fy0 = floor(py);
        const long long x0 = (long long)fx0, y0 = (long long)fy0;
        const float fx = (float)(px - fx0), fy = (float)(py - fy0);
        auto tap = [&](long long yy, long long xx) -> float {
            return (float)log((double)src[(int64_t)pano_clampi(yy, vh - 1) * vw + pano_clampi(xx, vw - 1)]);
        };
        val = pano_blend(tap(y0, x0), tap(y0, x0 + 1), tap(y0 + 1, x0), tap(y0 + 1, x0 + 1), fx, fy);
        const int xi = pano_clampi((long long)rint(px), vw - 1), yi = pano_clampi((long long)rint(py), vh - 1);
        mk = mask[(int64_t)view * vh * vw + (int64_t)yi * vw + xi] != 0;
    }
    logd[(int64_t)view * N + p] = val;
    m[(int64_t)view * N + p] = mk ? 1 : 0;
}

// (b) of the system: the masked means over the views, in view order, and the row masks
__global__ __launch_bounds__(PANO_THREADS) void pano_means_kernel(const float* logd, const uint8_t* m, int n, PanoDims D, double* b, uint8_t* rows, uint8_t* seen) {
    const int p = blockIdx.x * PANO_THREADS + threadIdx.x;
    if (p >= D.N) return;
    const int W = D.W, H = D.H, i = p / W, j = p - i * W;
    const int pr = i * W + (j + 1 == W ? 0 : j + 1), pl = i * W + (j == 0 ? W - 1 : j - 1), pu = i > 0 ? p - W : p, pd = i < H - 1 ? p + W : p;
    float sx = 0.0f, sy = 0.0f, sl = 0.0f;
    int nx = 0, ny = 0, nl = 0;
    bool any = false;
    for (int v = 0; v < n; v++) {
        const float* L = logd + (int64_t)v * D.N;
        const uint8_t* K = m + (int64_t)v * D.N;
        const float c = L[p], right = L[pr], left = L[pl], up = L[pu], dn = L[pd];
        const bool mc = K[p], mr = K[pr], ml = K[pl], mu = K[pu], md = K[pd];
        any |= mc;
        if (mc && mr) { sx += c - right; nx++; }                       // (a select, not the host's multiplication by the mask: the same sum for
        if (i < H - 1 && mc && md) { sy += c - dn; ny++; }             //  finite values, and a masked-out NaN stays out)
        if (mc && mu && md && ml && mr) { sl += (((up + dn) + left) + right) - 4.0f * c; nl++; }
    }
    b[p] = (double)sx / fmax((double)nx, 1e-3);
    rows[p] = nx > 0;
    if (i < H - 1) {
        const double by = (double)sy / fmax((double)ny, 1e-3);
        b[D.oY + p] = by;
        rows[D.oY + p] = ny > 0;
        if (j == 0) { b[D.oE + i] = by; rows[D.oE + i] = ny > 0; }
    }
    b[D.oL + p] = (double)sl / fmax((double)nl, 1e-3);
    rows[D.oL + p] = nl > 0;
    seen[p] = any;
}

// ------------------------------------------------------------------------------------------------------------------------
// the operator
// ------------------------------------------------------------------------------------------------------------------------
template <typename F>
__device__ __forceinline__ double pano_row(int r, const PanoDims& D, F v) {        // (A v)[r]; v(pixel) -> value
    const int W = D.W;
    if (r < D.oY) { const int i = r / W, j = r - i * W; return v(r) - v(i * W + (j + 1 == W ? 0 : j + 1)); }
    if (r < D.oE) { const int p = r - D.oY; return v(p) - v(p + W); }
    if (r < D.oL) { const int i = r - D.oE; return v(i * W) - v((i + 1) * W); }
    const int p = r - D.oL, i = p / W, j = p - i * W;
    double acc = 0.0;
    if (i > 0) acc += v(p - W);
    if (i < D.H - 1) acc += v(p + W);
    acc += v(i * W + (j == 0 ? W - 1 : j - 1));
    acc += v(i * W + (j + 1 == W ? 0 : j + 1));
    return acc + (double)(-4 + (i == 0) + (i == D.H - 1)) * v(p);                  // a replicated row falls on the pixel itself
}

template <typename F>
__device__ __forceinline__ double pano_col(int p, const PanoDims& D, F u) {        // (A^T u)[p]; u(row) -> value (zero on unselected rows)
    const int W = D.W, H = D.H, i = p / W, j = p - i * W;
    const int pl = i * W + (j == 0 ? W - 1 : j - 1), pr = i * W + (j + 1 == W ? 0 : j + 1);
    double acc = u(p) - u(pl);
    if (i < H - 1) acc += u(D.oY + p);
    if (i > 0) acc -= u(D.oY + p - W);
    if (j == 0) {
        if (i < H - 1) acc += u(D.oE + i);
        if (i > 0) acc -= u(D.oE + i - 1);
    }
    acc += (double)(-4 + (i == 0) + (i == H - 1)) * u(D.oL + p);
    acc += u(D.oL + pl);
    acc += u(D.oL + pr);
    if (i < H - 1) acc += u(D.oL + p + W);
    if (i > 0) acc += u(D.oL + p - W);
    return acc;
}

__global__ __launch_bounds__(PANO_THREADS) void pano_apply_kernel(PanoDims D, const uint8_t* rows, int transpose, const double* in, double* out) {
    const int e = blockIdx.x * PANO_THREADS + threadIdx.x;
    if (transpose) {
        if (e < D.N) out[e] = pano_col(e, D, [&](int r) { return rows[r] ? in[r] : 0.0; });
    } else if (e < D.M) out[e] = rows[e] ? pano_row(e, D, [&](int p) { return in[p]; }) : 0.0;
}

// ------------------------------------------------------------------------------------------------------------------------
// fixed-order sums
// ------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ double pano_block_sum(double t) {        // all threads call; the total comes back to every thread
    __shared__ double wave_tot[PANO_THREADS / 64];
    __shared__ double total;
    for (int o = 32; o > 0; o >>= 1) t += __shfl_down(t, o);
    __syncthreads();                                                // (a second call in one kernel: the previous total has been read)
    if ((threadIdx.x & 63) == 0) wave_tot[threadIdx.x >> 6] = t;
    __syncthreads();
    if (threadIdx.x == 0) {
        double s = wave_tot[0];
        for (int w = 1; w < PANO_THREADS / 64; w++) s += wave_tot[w];
        total = s;
    }
    __syncthreads();
    return total;
}

__device__ __forceinline__ double pano_sum_partials(const double* part, int n) {
    double t = 0.0;
    for (int k = threadIdx.x; k < n; k += PANO_THREADS) t += part[k];
    return pano_block_sum(t);
}

// ------------------------------------------------------------------------------------------------------------------------
// LSMR (scipy/sparse/linalg/_isolve/lsmr.py, damp = 0)
// ------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ double pano_sign(double a) { return a > 0.0 ? 1.0 : (a < 0.0 ? -1.0 : 0.0); }

__device__ void pano_sym_ortho(double a, double b, double& c, double& s, double& r) {       // lsqr.py _sym_ortho
    if (b == 0.0) { c = pano_sign(a); s = 0.0; r = fabs(a); }
    else if (a == 0.0) { c = 0.0; s = pano_sign(b); r = fabs(b); }
    else if (fabs(b) > fabs(a)) { const double tau = a / b; s = pano_sign(b) / sqrt(1.0 + tau * tau); c = s * tau; r = b / s; }
    else { const double tau = b / a; c = pano_sign(a) / sqrt(1.0 + tau * tau); s = c * tau; r = a / c; }
}

// u~ = b - A x0 on the selected rows; partial sums of b^2, u~^2 and of the selected rows
__global__ __launch_bounds__(PANO_THREADS) void lsmr_init_u_kernel(PanoDims D, const double* b, const uint8_t* rows, const double* x0, double* u, double* part,
                                                                   double* part_b, long long* part_rows) {
    double su = 0.0, sb = 0.0;
    long long cnt = 0;
    for (int k = 0; k < PANO_ITEMS; k++) {
        const int r = blockIdx.x * MOGE_PANO_SPAN + k * PANO_THREADS + threadIdx.x;
        if (r >= D.M) continue;
        double val = 0.0;
        if (rows[r]) {
            val = b[r];
            sb += val * val;
            cnt++;
            if (x0) val = val - pano_row(r, D, [&](int p) { return x0[p]; });
        }
        u[r] = val;
        su += val * val;
    }
    su = pano_block_sum(su);
    sb = pano_block_sum(sb);
    const double c = pano_block_sum((double)cnt);                   // at most MOGE_PANO_SPAN: exact
    if (threadIdx.x == 0) { part[blockIdx.x] = su; part_b[blockIdx.x] = sb; part_rows[blockIdx.x] = (long long)c; }
}

__global__ __launch_bounds__(PANO_THREADS) void lsmr_init_beta_kernel(PanoState* st, const double* part, const double* part_b, const long long* part_rows, int P,
                                                                      int N, int maxiter, double atol, double btol, double conlim) {
    const double su = pano_sum_partials(part, P), sb = pano_sum_partials(part_b, P);
    long long c = 0;
    if (threadIdx.x == 0) for (int k = 0; k < P; k++) c += part_rows[k];
    if (threadIdx.x != 0) return;
    PanoState s{};
    s.normb = sqrt(sb);
    s.beta = sqrt(su);
    s.inv_beta = s.beta > 0.0 ? 1.0 / s.beta : 1.0;
    s.beta_zero = !(s.beta > 0.0);
    s.rows = c;
    s.maxiter = maxiter > 0 ? maxiter : (int)(c < N ? c : N);      // min(m, n) of the compressed system
    s.atol = atol; s.btol = btol; s.ctol = conlim > 0.0 ? 1.0 / conlim : 0.0;
    *st = s;
}

// v~ = (v~ / alpha) (-beta) + A^T (u~ / beta); FIRST: v~ = A^T (u~ / beta)
template <bool FIRST>
__global__ __launch_bounds__(PANO_THREADS) void lsmr_atu_kernel(PanoState* st, PanoDims D, const double* u, double* v, double* part) {
    if (!FIRST && (st->stop || st->beta_zero)) return;
    const double inv_beta = st->inv_beta, inv_alpha = FIRST ? 0.0 : st->inv_alpha, nbeta = -st->beta;
    const bool zero = FIRST && st->beta_zero;
    double sv = 0.0;
    for (int k = 0; k < PANO_ITEMS; k++) {
        const int p = blockIdx.x * MOGE_PANO_SPAN + k * PANO_THREADS + threadIdx.x;
        if (p >= D.N) continue;
        double val = zero ? 0.0 : pano_col(p, D, [&](int r) { return u[r] * inv_beta; });
        if (!FIRST) val = (v[p] * inv_alpha) * nbeta + val;
        v[p] = val;
        sv += val * val;
    }
    sv = pano_block_sum(sv);
    if (threadIdx.x == 0) part[blockIdx.x] = sv;
}

__global__ __launch_bounds__(PANO_THREADS) void lsmr_init_alpha_kernel(PanoState* st, const double* part, int P) {
    const double sv = pano_sum_partials(part, P);
    if (threadIdx.x != 0) return;
    PanoState s = *st;
    s.alpha = sqrt(sv);
    s.inv_alpha = s.alpha > 0.0 ? 1.0 / s.alpha : 1.0;
    s.itn = 0;
    s.zetabar = s.alpha * s.beta; s.alphabar = s.alpha; s.rho = 1.0; s.rhobar = 1.0; s.cbar = 1.0; s.sbar = 0.0;
    s.betadd = s.beta; s.betad = 0.0; s.rhodold = 1.0; s.tautildeold = 0.0; s.thetatilde = 0.0; s.zeta = 0.0; s.d = 0.0;
    s.normA2 = s.alpha * s.alpha; s.maxrbar = 0.0; s.minrbar = 1e+100; s.normA = sqrt(s.normA2); s.condA = 1.0; s.normx = 0.0;
    s.istop = 0; s.normr = s.beta; s.normar = s.alpha * s.beta;
    if (s.normar == 0.0) s.stop = 1;                                // the exact solution is x0 (or 0)
    else if (s.normb == 0.0) { s.stop = 1; s.zero_x = 1; }
    else if (s.maxiter <= 0) s.stop = 1;                            // `while itn < maxiter` never runs
    *st = s;
}

__global__ __launch_bounds__(PANO_THREADS) void lsmr_init_vec_kernel(const PanoState* st, int N, const double* v, const double* x0, double* h, double* hbar, double* x) {
    const int p = blockIdx.x * PANO_THREADS + threadIdx.x;
    if (p >= N) return;
    h[p] = v[p] * st->inv_alpha;
    hbar[p] = 0.0;
    x[p] = (x0 && !st->zero_x) ? x0[p] : 0.0;
}

// 1: u~ = (u~ / beta) (-alpha) + A (v~ / alpha)
__global__ __launch_bounds__(PANO_THREADS) void lsmr_av_kernel(const PanoState* st, PanoDims D, const uint8_t* rows, const double* v, double* u, double* part) {
    if (st->stop) return;
    const double inv_beta = st->inv_beta, inv_alpha = st->inv_alpha, nalpha = -st->alpha;
    double su = 0.0;
    for (int k = 0; k < PANO_ITEMS; k++) {
        const int r = blockIdx.x * MOGE_PANO_SPAN + k * PANO_THREADS + threadIdx.x;
        if (r >= D.M || !rows[r]) continue;                         // unselected rows were written 0 by the init and stay 0
        const double val = (u[r] * inv_beta) * nalpha + pano_row(r, D, [&](int p) { return v[p] * inv_alpha; });
        u[r] = val;
        su += val * val;
    }
    su = pano_block_sum(su);
    if (threadIdx.x == 0) part[blockIdx.x] = su;
}

// 2: beta
__global__ __launch_bounds__(PANO_THREADS) void lsmr_beta_kernel(PanoState* st, const double* part, int P) {
    if (st->stop) return;
    const double su = pano_sum_partials(part, P);
    if (threadIdx.x != 0) return;
    const double beta = sqrt(su);
    st->beta = beta;
    st->beta_zero = !(beta > 0.0);
    st->inv_beta = beta > 0.0 ? 1.0 / beta : 1.0;
}

// 4: alpha, the rotations, the estimates (lsmr.py:336-412)
__global__ __launch_bounds__(PANO_THREADS) void lsmr_givens_kernel(PanoState* st, const double* part, int P) {
    if (st->stop) return;
    const double sv = pano_sum_partials(part, P);
    if (threadIdx.x != 0) return;
    PanoState s = *st;
    s.itn += 1;
    if (!s.beta_zero) {
        s.alpha = sqrt(sv);
        s.inv_alpha = s.alpha > 0.0 ? 1.0 / s.alpha : 1.0;
    }
    const double alpha = s.alpha, beta = s.beta;
    double chat, shat, alphahat;
    pano_sym_ortho(s.alphabar, 0.0, chat, shat, alphahat);
    const double rhoold = s.rho;
    double c, sn, rho;
    pano_sym_ortho(alphahat, beta, c, sn, rho);
    s.rho = rho;
    const double thetanew = sn * alpha;
    s.alphabar = c * alpha;
    const double rhobarold = s.rhobar, zetaold = s.zeta, thetabar = s.sbar * rho, rhotemp = s.cbar * rho;
    pano_sym_ortho(s.cbar * rho, thetanew, s.cbar, s.sbar, s.rhobar);
    s.zeta = s.cbar * s.zetabar;
    s.zetabar = -s.sbar * s.zetabar;
    s.c_hbar = -(thetabar * rho / (rhoold * rhobarold));
    s.c_x = s.zeta / (rho * s.rhobar);
    s.c_h = -(thetanew / rho);
    const double betaacute = chat * s.betadd, betacheck = -shat * s.betadd;
    const double betahat = c * betaacute;
    s.betadd = -sn * betaacute;
    const double thetatildeold = s.thetatilde;
    double ctildeold, stildeold, rhotildeold;
    pano_sym_ortho(s.rhodold, thetabar, ctildeold, stildeold, rhotildeold);
    s.thetatilde = stildeold * s.rhobar;
    s.rhodold = ctildeold * s.rhobar;
    s.betad = -stildeold * s.betad + ctildeold * betahat;
    s.tautildeold = (zetaold - thetatildeold * s.tautildeold) / rhotildeold;
    const double taud = (s.zeta - s.thetatilde * s.tautildeold) / s.rhodold;
    s.d = s.d + betacheck * betacheck;
    s.normr = sqrt(s.d + (s.betad - taud) * (s.betad - taud) + s.betadd * s.betadd);
    s.normA2 = s.normA2 + beta * beta;
    s.normA = sqrt(s.normA2);
    s.normA2 = s.normA2 + alpha * alpha;
    s.maxrbar = fmax(s.maxrbar, rhobarold);
    if (s.itn > 1) s.minrbar = fmin(s.minrbar, rhobarold);
    s.condA = fmax(s.maxrbar, rhotemp) / fmin(s.minrbar, rhotemp);
    s.normar = fabs(s.zetabar);
    *st = s;
}

// 5: hbar, x, h
__global__ __launch_bounds__(PANO_THREADS) void lsmr_update_kernel(const PanoState* st, int N, const double* v, double* h, double* hbar, double* x, double* part) {
    if (st->stop) return;
    const double c_hbar = st->c_hbar, c_x = st->c_x, c_h = st->c_h, inv_alpha = st->inv_alpha;
    double sx = 0.0;
    for (int k = 0; k < PANO_ITEMS; k++) {
        const int p = blockIdx.x * MOGE_PANO_SPAN + k * PANO_THREADS + threadIdx.x;
        if (p >= N) continue;
        const double hv = h[p], hb = hbar[p] * c_hbar + hv, xv = x[p] + c_x * hb;
        hbar[p] = hb;
        x[p] = xv;
        h[p] = hv * c_h + v[p] * inv_alpha;
        sx += xv * xv;
    }
    sx = pano_block_sum(sx);
    if (threadIdx.x == 0) part[blockIdx.x] = sx;
}

// 6: normx and the stopping rule (lsmr.py:413-449)
__global__ __launch_bounds__(PANO_THREADS) void lsmr_test_kernel(PanoState* st, const double* part, int P) {
    if (st->stop) return;
    const double sx = pano_sum_partials(part, P);
    if (threadIdx.x != 0) return;
    const double normx = sqrt(sx), normr = st->normr, normA = st->normA, normb = st->normb;
    st->normx = normx;
    const double test1 = normr / normb;
    const double test2 = (normA * normr) != 0.0 ? st->normar / (normA * normr) : INFINITY;
    const double test3 = 1.0 / st->condA;
    const double t1 = test1 / (1.0 + normA * normx / normb);
    const double rtol = st->btol + st->atol * normA * normx / normb;
    int istop = 0;
    if (st->itn >= st->maxiter) istop = 7;
    if (1.0 + test3 <= 1.0) istop = 6;
    if (1.0 + test2 <= 1.0) istop = 5;
    if (1.0 + t1 <= 1.0) istop = 4;
    if (test3 <= st->ctol) istop = 3;
    if (test2 <= st->atol) istop = 2;
    if (test1 <= rtol) istop = 1;
    st->istop = istop;
    if (istop > 0) st->stop = 1;
}

// ------------------------------------------------------------------------------------------------------------------------
// the small kernels
// ------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(PANO_THREADS) void pano_resize_bilinear_kernel(const float* src, int H, int W, int oh, int ow, float* dst) {      // _resize_bilinear
    const int p = blockIdx.x * PANO_THREADS + threadIdx.x;
    if (p >= oh * ow) return;
    const int i = p / ow, j = p - i * ow;
    const double x = ((double)j + 0.5) * ((double)W / (double)ow) - 0.5, y = ((double)i + 0.5) * ((double)H / (double)oh) - 0.5;
    const double fx0 = floor(x), fy0 = floor(y);
    const long long x0 = (long long)fx0, y0 = (long long)fy0;
    const float fx = (float)(x - fx0), fy = (float)(y - fy0);
    auto tap = [&](long long yy, long long xx) { return src[(int64_t)pano_clampi(yy, H - 1) * W + pano_clampi(xx, W - 1)]; };
    dst[p] = pano_blend(tap(y0, x0), tap(y0, x0 + 1), tap(y0 + 1, x0), tap(y0 + 1, x0 + 1), fx, fy);
}

__global__ __launch_bounds__(PANO_THREADS) void pano_resize_nearest_kernel(const uint8_t* src, int H, int W, int oh, int ow, uint8_t* dst) {    // _resize_nearest
    const int p = blockIdx.x * PANO_THREADS + threadIdx.x;
    if (p >= oh * ow) return;
    const int i = p / ow, j = p - i * ow;
    const int xi = pano_clampi((long long)((double)j * ((double)W / (double)ow)), W - 1), yi = pano_clampi((long long)((double)i * ((double)H / (double)oh)), H - 1);
    dst[p] = src[(int64_t)yi * W + xi];
}

__global__ __launch_bounds__(PANO_THREADS) void pano_log_kernel(const float* src, int64_t n, double* dst) {       // np.log of a float32 map, then float64
    const int64_t p = (int64_t)blockIdx.x * PANO_THREADS + threadIdx.x;
    if (p < n) dst[p] = (double)(float)log((double)src[p]);
}

__global__ __launch_bounds__(PANO_THREADS) void pano_finish_kernel(const double* x, float* distance, int H, int W, float* points) {
    const int p = blockIdx.x * PANO_THREADS + threadIdx.x;
    if (p >= H * W) return;
    float dist;
    if (x) { dist = (float)exp(x[p]); distance[p] = dist; }
    else dist = distance[p];
    if (points) {
        const int i = p / W, j = p - i * W;
        double d[3];
        pano_direction(i, j, H, W, d);
        for (int c = 0; c < 3; c++) points[(int64_t)p * 3 + c] = dist * (float)d[c];
    }
}

// ------------------------------------------------------------------------------------------------------------------------
// host
// ------------------------------------------------------------------------------------------------------------------------
static int pano_check_map(int width, int height, const char* who) {         // M = 3 W H + ... row indices are int32
    if (width < 1 || height < 1 || (int64_t)width * height > MOGE_PANO_MAX_PIXELS)
        return moge_internal_fail(MOGE_ERR_INVALID, "%s: need width >= 1, height >= 1 and width * height <= 2^29, got width = %d, height = %d", who, width, height);
    return 0;
}

static int pano_check_image(int H, int W, const char* who) {
    if (H < 1 || W < 1 || (int64_t)H * W > MOGE_PANO_MAX_PIXELS)
        return moge_internal_fail(MOGE_ERR_INVALID, "%s: need H >= 1, W >= 1 and H * W <= 2^29, got H = %d, W = %d", who, H, W);
    return 0;
}

static void pano_cams(const float* extrinsics, const float* intrinsics, int n, PanoCams& c) {
    for (int v = 0; v < n; v++) {
        for (int r = 0; r < 3; r++)
            for (int k = 0; k < 3; k++) c.R[v][3 * r + k] = (double)extrinsics[16 * v + 4 * r + k];
        c.K[v][0] = (double)intrinsics[9 * v + 0]; c.K[v][1] = (double)intrinsics[9 * v + 4];
        c.K[v][2] = (double)intrinsics[9 * v + 2]; c.K[v][3] = (double)intrinsics[9 * v + 5];
    }
}

extern "C" {

int moge_pano_split(const void* image, int is_u8, int H, int W, const float* extrinsics, const float* intrinsics, int n, int resolution, void* out, void* stream) {
    if (int rc = pano_check_image(H, W, "moge_pano_split")) return rc;
    if (n < 1 || n > MOGE_PANO_MAX_VIEWS) return moge_internal_fail(MOGE_ERR_INVALID, "moge_pano_split: need 1 <= n <= MOGE_PANO_MAX_VIEWS views");
    if (resolution < 1 || resolution > 16384) return moge_internal_fail(MOGE_ERR_INVALID, "moge_pano_split: need 1 <= resolution <= 16384");
    if (!image || !extrinsics || !intrinsics || !out) return moge_internal_fail(MOGE_ERR_INVALID, "moge_pano_split: null argument");
    PanoCams cams;
    pano_cams(extrinsics, intrinsics, n, cams);
    const dim3 grid(blocks((int64_t)resolution * resolution, PANO_THREADS), (unsigned)n);
    hipStream_t st = (hipStream_t)stream;
    if (is_u8) hipLaunchKernelGGL(pano_split_kernel<uint8_t>, grid, dim3(PANO_THREADS), 0, st, (const uint8_t*)image, H, W, cams, resolution, (uint8_t*)out);
    else hipLaunchKernelGGL(pano_split_kernel<float>, grid, dim3(PANO_THREADS), 0, st, (const float*)image, H, W, cams, resolution, (float*)out);
    return launched("moge_pano_split: launch failed");
}

int moge_pano_merge_workspace(int width, int height, int n, int64_t* bytes) {
    if (!bytes) return moge_internal_fail(MOGE_ERR_INVALID, "moge_pano_merge_workspace: null argument");
    *bytes = 0;
    if (int rc = pano_check_map(width, height, "moge_pano_merge_workspace")) return rc;
    if (n < 0 || n > MOGE_PANO_MAX_VIEWS) return moge_internal_fail(MOGE_ERR_INVALID, "moge_pano_merge_workspace: need 0 <= n <= MOGE_PANO_MAX_VIEWS views");
    const PanoDims D = pano_dims(width, height);
    const int64_t P = blocks(D.M, MOGE_PANO_SPAN);
    *bytes = 8 * ((int64_t)D.M + 3 * (int64_t)D.N + 3 * P + MOGE_PANO_STATE_DOUBLES) + 5 * (int64_t)n * D.N;
    return 0;
}

int moge_pano_system(int width, int height, const float* distance, const uint8_t* masks, int n, int vh, int vw, const float* extrinsics, const float* intrinsics,
                     void* workspace, double* b, uint8_t* rows, uint8_t* seen, void* stream) {
    if (int rc = pano_check_map(width, height, "moge_pano_system")) return rc;
    if (n < 1 || n > MOGE_PANO_MAX_VIEWS) return moge_internal_fail(MOGE_ERR_INVALID, "moge_pano_system: need 1 <= n <= MOGE_PANO_MAX_VIEWS views");
    if (vh < 1 || vw < 1 || (int64_t)vh * vw > MOGE_PANO_MAX_PIXELS) return moge_internal_fail(MOGE_ERR_INVALID, "moge_pano_system: need view sizes >= 1 and vh * vw <= 2^29");
    if (!distance || !masks || !extrinsics || !intrinsics || !workspace || !b || !rows || !seen) return moge_internal_fail(MOGE_ERR_INVALID, "moge_pano_system: null argument");
    const PanoDims D = pano_dims(width, height);
    PanoWs w = pano_ws(workspace, D);
    w.m = (uint8_t*)(w.logd + (int64_t)n * D.N);
    PanoCams cams;
    pano_cams(extrinsics, intrinsics, n, cams);
    hipStream_t st = (hipStream_t)stream;
    const unsigned nb = blocks(D.N, PANO_THREADS);
    hipLaunchKernelGGL(pano_warp_kernel, dim3(nb, (unsigned)n), dim3(PANO_THREADS), 0, st, distance, masks, vh, vw, cams, height, width, w.logd, w.m);
    hipLaunchKernelGGL(pano_means_kernel, dim3(nb), dim3(PANO_THREADS), 0, st, w.logd, w.m, n, D, b, rows, seen);
    return launched("moge_pano_system: launch failed");
}

int moge_pano_lsmr(int width, int height, const double* b, const uint8_t* rows, const double* x0, double atol, double btol, double conlim, int maxiter, int poll,
                   void* workspace, double* x, double* info, void* stream) {
    if (int rc = pano_check_map(width, height, "moge_pano_lsmr")) return rc;
    if (poll < 1 || poll > 65536) return moge_internal_fail(MOGE_ERR_INVALID, "moge_pano_lsmr: need 1 <= poll <= 65536 iterations per read of the stop word");
    if (maxiter < 0) return moge_internal_fail(MOGE_ERR_INVALID, "moge_pano_lsmr: maxiter must be >= 0 (0: min(selected rows, pixels))");
    if (!(atol >= 0.0) || !(btol >= 0.0) || !(conlim >= 0.0)) return moge_internal_fail(MOGE_ERR_INVALID, "moge_pano_lsmr: atol, btol and conlim must be >= 0");
    if (!b || !rows || !workspace || !x || !info) return moge_internal_fail(MOGE_ERR_INVALID, "moge_pano_lsmr: null argument");
    const PanoDims D = pano_dims(width, height);
    const PanoWs w = pano_ws(workspace, D);
    hipStream_t st = (hipStream_t)stream;
    const dim3 T(PANO_THREADS);
    const unsigned gM = (unsigned)w.P, gN = blocks(D.N, MOGE_PANO_SPAN), gN1 = blocks(D.N, PANO_THREADS);
    hipLaunchKernelGGL(lsmr_init_u_kernel, dim3(gM), T, 0, st, D, b, rows, x0, w.u, w.part, w.part_b, w.part_rows);
    hipLaunchKernelGGL(lsmr_init_beta_kernel, dim3(1), T, 0, st, w.state, w.part, w.part_b, w.part_rows, w.P, D.N, maxiter, atol, btol, conlim);
    hipLaunchKernelGGL(lsmr_atu_kernel<true>, dim3(gN), T, 0, st, w.state, D, w.u, w.v, w.part);
    hipLaunchKernelGGL(lsmr_init_alpha_kernel, dim3(1), T, 0, st, w.state, w.part, (int)gN);
    hipLaunchKernelGGL(lsmr_init_vec_kernel, dim3(gN1), T, 0, st, w.state, D.N, w.v, x0, w.h, w.hbar, x);
    PanoState hs;
    auto read_state = [&]() {
        if (hipMemcpyAsync(&hs, w.state, sizeof hs, hipMemcpyDeviceToHost, st) != hipSuccess) return false;
        return hipStreamSynchronize(st) == hipSuccess;
    };
    if (!read_state()) return moge_internal_fail(MOGE_ERR_HIP, "moge_pano_lsmr: reading the solver state failed");
    int queued = 0;
    while (!hs.stop && queued < hs.maxiter) {                       // bounded by maxiter: the test kernel of iteration maxiter sets stop (istop 7)
        const int chunk = hs.maxiter - queued < poll ? hs.maxiter - queued : poll;
        for (int k = 0; k < chunk; k++) {
            hipLaunchKernelGGL(lsmr_av_kernel, dim3(gM), T, 0, st, w.state, D, rows, w.v, w.u, w.part);
            hipLaunchKernelGGL(lsmr_beta_kernel, dim3(1), T, 0, st, w.state, w.part, w.P);
            hipLaunchKernelGGL(lsmr_atu_kernel<false>, dim3(gN), T, 0, st, w.state, D, w.u, w.v, w.part);
            hipLaunchKernelGGL(lsmr_givens_kernel, dim3(1), T, 0, st, w.state, w.part, (int)gN);
            hipLaunchKernelGGL(lsmr_update_kernel, dim3(gN), T, 0, st, w.state, D.N, w.v, w.h, w.hbar, x, w.part);
            hipLaunchKernelGGL(lsmr_test_kernel, dim3(1), T, 0, st, w.state, w.part, (int)gN);
        }
        queued += chunk;
        if (int rc = launched("moge_pano_lsmr: an iteration failed")) return rc;
        if (!read_state()) return moge_internal_fail(MOGE_ERR_HIP, "moge_pano_lsmr: an iteration failed");
    }
    info[0] = hs.istop; info[1] = hs.itn; info[2] = hs.normr; info[3] = hs.normar; info[4] = hs.normA; info[5] = hs.condA; info[6] = hs.normx;
    info[7] = (double)hs.rows;
    return 0;
}

int moge_pano_resize_bilinear(const float* src, int H, int W, int out_h, int out_w, float* dst, void* stream) {
    if (int rc = pano_check_image(H, W, "moge_pano_resize_bilinear")) return rc;
    if (int rc = pano_check_image(out_h, out_w, "moge_pano_resize_bilinear")) return rc;
    if (!src || !dst) return moge_internal_fail(MOGE_ERR_INVALID, "moge_pano_resize_bilinear: null argument");
    hipLaunchKernelGGL(pano_resize_bilinear_kernel, dim3(blocks((int64_t)out_h * out_w, PANO_THREADS)), dim3(PANO_THREADS), 0, (hipStream_t)stream, src, H, W, out_h, out_w, dst);
    return launched("moge_pano_resize_bilinear: launch failed");
}

int moge_pano_resize_nearest(const uint8_t* src, int H, int W, int out_h, int out_w, uint8_t* dst, void* stream) {
    if (int rc = pano_check_image(H, W, "moge_pano_resize_nearest")) return rc;
    if (int rc = pano_check_image(out_h, out_w, "moge_pano_resize_nearest")) return rc;
    if (!src || !dst) return moge_internal_fail(MOGE_ERR_INVALID, "moge_pano_resize_nearest: null argument");
    hipLaunchKernelGGL(pano_resize_nearest_kernel, dim3(blocks((int64_t)out_h * out_w, PANO_THREADS)), dim3(PANO_THREADS), 0, (hipStream_t)stream, src, H, W, out_h, out_w, dst);
    return launched("moge_pano_resize_nearest: launch failed");
}

int moge_pano_log(const float* src, int64_t n, double* dst, void* stream) {
    if (n < 0 || n > MOGE_PANO_MAX_PIXELS) return moge_internal_fail(MOGE_ERR_INVALID, "moge_pano_log: need 0 <= n <= 2^29");
    if (!src || !dst) return moge_internal_fail(MOGE_ERR_INVALID, "moge_pano_log: null argument");
    if (n == 0) return 0;
    hipLaunchKernelGGL(pano_log_kernel, dim3(blocks(n, PANO_THREADS)), dim3(PANO_THREADS), 0, (hipStream_t)stream, src, n, dst);
    return launched("moge_pano_log: launch failed");
}

int moge_pano_finish(const double* x, float* distance, int H, int W, float* points, void* stream) {
    if (int rc = pano_check_image(H, W, "moge_pano_finish")) return rc;
    if (!distance) return moge_internal_fail(MOGE_ERR_INVALID, "moge_pano_finish: null argument");
    if (!x && !points) return moge_internal_fail(MOGE_ERR_INVALID, "moge_pano_finish: nothing to write (no x and no points)");
    hipLaunchKernelGGL(pano_finish_kernel, dim3(blocks((int64_t)H * W, PANO_THREADS)), dim3(PANO_THREADS), 0, (hipStream_t)stream, x, distance, H, W, points);
    return launched("moge_pano_finish: launch failed");
}

int moge_test_pano_apply(int width, int height, const uint8_t* rows, int transpose, const double* in, double* out, void* stream) {
    if (int rc = pano_check_map(width, height, "moge_test_pano_apply")) return rc;
    if (transpose != 0 && transpose != 1) return moge_internal_fail(MOGE_ERR_INVALID, "moge_test_pano_apply: transpose must be 0 or 1");
    if (!rows || !in || !out) return moge_internal_fail(MOGE_ERR_INVALID, "moge_test_pano_apply: null argument");
    const PanoDims D = pano_dims(width, height);
    hipLaunchKernelGGL(pano_apply_kernel, dim3(blocks(transpose ? D.N : D.M, PANO_THREADS)), dim3(PANO_THREADS), 0, (hipStream_t)stream, D, rows, transpose, in, out);
    return launched("moge_test_pano_apply: launch failed");
}

}   // extern "C"
