// Level 4 of the decoder with the 1x1 output conv folded into the resampler's WEIGHTS (fp16 throughput path, gfx950).
//
// Level 4 of a ConvStack without residual blocks is linear (modules.py:155-159, 231, 242-253):
//     out_k = Wout_k . (Conv3x3_k(Up2(x3_k)) + Win4_k . n4) + b,      n4 = Conv3x3_n(Up2(n3)) + Win4_n . uv + b_n.
// conv_pp.hip's fused output conv (DOT) still evaluates the 64 -> 4 x 32 phase conv and contracts its 128 columns with 3 + 1 rows in
// the epilogue.  A 1x1 conv commutes with everything spatial in the resampler, so here the rows D (Wout_k for a head, Wout_k . Win4_k of
// every head for the neck) are multiplied into the 4-phase weights at pack time (l4c_pack_kernel):
//     Wc[gq][4 q + e][tap * 64 + ci] = sum_m D[4 gq + e][m] . Wphase[q * 32 + m][tap * 64 + ci]       (q = py * 2 + px, one fp16 rounding)
// and the resampler is a 64 -> 16 nd conv on the low-res map: 18 v_mfma_f32_16x16x32_f16 per 16 pixels and group instead of 144, the
// 32-channel map and its fp16 rounding never exist.  Bias and the uv rank-2 term go through the same rows (fp32, added in the epilogue).
//
//   out[(((gq * B + b) * 2H + 2y + py) * 2W + 2x + px) * 4 + e] = bc[4 gq + e] + wuc[4 gq + e] u(2x + px) + wvc[4 gq + e] v(2y + py)
//                                                                + sum_{tap = (dy, dx), ci} Wc[gq][4 q + e][tap * 64 + ci] . in[b, clamp(y + dy), clamp(x + dx), ci]
//
// one (B, 2H, 2W, 4) fp32 map per group, which head_final_dot_kernel reads with a pitch of 4 (with the groups interleaved per pixel it fetched 32-byte
// pixels for 16 useful bytes: 0.32 -> 0.21 ms per head at batch 32).  A workgroup computes 16 x 16 low-res tiles: a tile's (16 + 2)^2 x 64 halo comes in
// by LDS-DMA with clamped source indices (replicate padding; conv_pp.hip's piece layout and column swizzle), the only LDS user (41 KiB: three
// workgroups per CU overlap each other's load, MFMA and store phases).  Wave (gq, rg) of the 4 nd waves keeps group gq's 16 x 576 weights in registers
// as 18 A fragments and computes tile rows 4 rg .. 4 rg + 3: the 16 A rows are 4 phases x 4 floats, so lane (pixel l15, g4) ends up
// with the four floats of high-res pixel (2y + (g4 >> 1), 2x + (g4 & 1)) - one 16-byte store, two full 512-byte row segments per wave instruction.
// The grid is what the chip holds at once and a workgroup walks tiles t, t + grid, ...: the weights are read once per workgroup, the next tile's halo
// is requested before the current tile's stores.  HBM-bound by construction: 128 B read, 64 nd B written per low-res pixel.
#include "common.h"
#include "launchers.h"

#define L4C_GPTR(p) ((const __attribute__((address_space(1))) void*)(p))
#define L4C_LPTR(p) ((__attribute__((address_space(3))) void*)(p))

namespace {

constexpr int L4C_HALO_W = 18, L4C_HALO_PX = 18 * 18, L4C_PIECES = (L4C_HALO_PX + 7) / 8, L4C_LDS = L4C_PIECES * 1024;

// waves per SIMD: nd = 1 three workgroups per CU (LDS), nd = 2 two (<= 128 registers), nd = 3 one
template <int ND, bool HAS_UV>
__global__ __launch_bounds__(256 * ND, ND == 2 ? 4 : 3) void l4c_kernel(const L4cArgs a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];          // the halo: pixel hp at hp * 128, 16-byte chunk c in slot c ^ (hx & 7)
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int gq = wave >> 2, rg = wave & 3;
    const int l15 = lane & 15, g4 = lane >> 4;
    const int H = a.H, W = a.W;
    const int tx_n = (W + 15) >> 4, ty_n = (H + 15) >> 4;
    const int ntiles = a.B * ty_n * tx_n;

    // ---- halo DMA of tile t: piece = 8 pixels x 128 B, lane = (pixel lane >> 3, chunk lane & 7); source indices clamped = replicate padding ----
    auto issue_halo = [&](int t) {
        const int tx = t % tx_n, ty = (t / tx_n) % ty_n, b = t / (tx_n * ty_n);
        const int y0 = ty * 16, x0 = tx * 16;
        const char* in_b = reinterpret_cast<const char*>(a.in) + (size_t)b * H * W * 128;
        for (int piece = wave; piece < L4C_PIECES; piece += 4 * ND) {
            int hp = piece * 8 + (lane >> 3);
            hp = hp < L4C_HALO_PX ? hp : L4C_HALO_PX - 1;                // the four padding pixels of the last piece: never read
            const int hy = hp / L4C_HALO_W, hx = hp - hy * L4C_HALO_W;
            int yy = y0 - 1 + hy, xx = x0 - 1 + hx;
            yy = yy < 0 ? 0 : (yy > H - 1 ? H - 1 : yy);
            xx = xx < 0 ? 0 : (xx > W - 1 ? W - 1 : xx);
            const unsigned off = (unsigned)((yy * W + xx) * 128 + (((lane & 7) ^ (hx & 7)) << 4));
            __builtin_amdgcn_global_load_lds(L4C_GPTR(in_b + off), L4C_LPTR(smem + piece * 1024), 16, 0, 0);
        }
    };
    int t = blockIdx.x;                                                  // (the grid never exceeds the tile count)
    issue_halo(t);
    // ---- this wave's weights, once per workgroup: A fragments, row l15 = 4 q + e of group gq, K = tap * 64 + ks * 32 + 8 g4 .. + 7 ----
    u32x4 wf[9][2];
    {
        const char* wp = reinterpret_cast<const char*>(a.wc) + ((size_t)(gq * 16 + l15) * 576 + g4 * 8) * 2;
#pragma unroll
        for (int tap = 0; tap < 9; tap++)
#pragma unroll
            for (int ks = 0; ks < 2; ks++) wf[tap][ks] = *reinterpret_cast<const u32x4*>(wp + (tap * 64 + ks * 32) * 2);
    }
    const f32x4 bv = *reinterpret_cast<const f32x4*>(a.bias + 4 * gq);
    f32x4 wu = {0.f, 0.f, 0.f, 0.f}, wv = wu;
    if constexpr (HAS_UV) {
        wu = *reinterpret_cast<const f32x4*>(a.wu + 4 * gq);
        wv = *reinterpret_cast<const f32x4*>(a.wv + 4 * gq);
    }
    const int py = g4 >> 1, px = g4 & 1;
    // A workgroup walks tiles t, t + grid, ...: the workgroups resident at one time work on neighbouring tiles (shared halo columns in L2), the
    // weights - 18 KiB per wave, more than the halo per workgroup, and the same lines for every workgroup of the chip - are read once per workgroup
    for (;;) {
    const int tx = t % tx_n, ty = (t / tx_n) % ty_n, b = t / (tx_n * ty_n);
    const int y0 = ty * 16, x0 = tx * 16;
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");                    // this tile's halo (and the previous tile's stores, issued behind its request)
    __syncthreads();

    // ---- 9 taps x 2 K-steps x 4 tile rows: B fragment = pixel (row, l15) shifted by the tap, chunk 4 ks + g4 ----
    f32x4 acc[4];
#pragma unroll
    for (int i = 0; i < 4; i++) acc[i] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int tap = 0; tap < 9; tap++) {
        const int dy = tap / 3 - 1, dx = tap % 3 - 1;
        const int hx = l15 + 1 + dx;
        const int cb = (4 * rg + 1 + dy) * (L4C_HALO_W * 128) + hx * 128 + ((g4 ^ (hx & 7)) << 4);
#pragma unroll
        for (int ks = 0; ks < 2; ks++)
#pragma unroll
            for (int i = 0; i < 4; i++) {
                const u32x4 bf = *reinterpret_cast<const u32x4*>(smem + (cb ^ (ks * 64)) + i * (L4C_HALO_W * 128));
                mma16<f16>(acc[i], wf[tap][ks], bf);
            }
    }

    // ---- every wave has read its fragments: the next tile's halo is requested in front of this tile's stores ----
    const int tn = t + (int)gridDim.x;
    __syncthreads();
    if (tn < ntiles) issue_halo(tn);
    // ---- epilogue: bias + uv at the high-res pixel of this lane's phase, one 16-byte store ----
    const int x = x0 + l15;
    float uu = 0.f;
    if constexpr (HAS_UV) uu = linspace_at(a.u0, a.u1, a.ustep, 2 * W, 2 * (x < W ? x : W - 1) + px);
#pragma unroll
    for (int i = 0; i < 4; i++) {
        const int y = y0 + 4 * rg + i;
        if (y < H && x < W) {
            f32x4 v;
#pragma unroll
            for (int e = 0; e < 4; e++) v[e] = acc[i][e] + bv[e];
            if constexpr (HAS_UV) {
                const float vq = linspace_at(a.v0, a.v1, a.vstep, 2 * H, 2 * y + py);
#pragma unroll
                for (int e = 0; e < 4; e++) v[e] += wu[e] * uu + wv[e] * vq;
            }
            const size_t o = ((((size_t)gq * a.B + b) * 2 * H + 2 * y + py) * (2 * W) + 2 * x + px) * 4;
            *reinterpret_cast<f32x4*>(a.out + o) = v;
        }
    }
    if (tn >= ntiles) break;
    t = tn;
    }
}

// Composed weights and vectors (once per model / test call).  w3: the resampler's 3x3 conv, torch layout [32][64][3][3]; d: [rows][32] fp32 (rows
// beyond `rows` up to 4 nd are zero); wc: f16 [nd][16][576]; vec: fp32 [3][12] = D . bias, D . wu, D . wv (null source -> zeros).  The phase
// combination is launch_pack_phase_conv's (elementwise.hip); every sum in double, one rounding to fp16.
__global__ void l4c_pack_kernel(const float* __restrict__ w3, const float* __restrict__ d, int rows, int nd, int nearest, const float* __restrict__ bias,
                                const float* __restrict__ wu, const float* __restrict__ wv, f16* __restrict__ wc, float* __restrict__ vec) {
    const double RB[2][3][3] = {{{.75, .25, 0.}, {.25, .75, 0.}, {0., .75, .25}}, {{.25, .75, 0.}, {0., .75, .25}, {0., .25, .75}}};
    const double RN[2][3][3] = {{{1., 0., 0.}, {0., 1., 0.}, {0., 1., 0.}}, {{0., 1., 0.}, {0., 1., 0.}, {0., 0., 1.}}};
    const double (*R)[3][3] = nearest ? RN : RB;
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx < 36) {
        const int j = idx / 12, r = idx % 12;
        const float* src = j == 0 ? bias : (j == 1 ? wu : wv);
        double s = 0.0;
        if (src && r < rows)
            for (int m = 0; m < 32; m++) s += (double)d[r * 32 + m] * (double)src[m];
        vec[idx] = (float)s;
    }
    if (idx >= nd * 16 * 576) return;
    const int k = idx % 576, r16 = (idx / 576) & 15, gq = idx / (576 * 16);
    const int tap = k >> 6, ci = k & 63, q = r16 >> 2, row = 4 * gq + (r16 & 3);
    const int py = q >> 1, px = q & 1, ta = tap / 3, tb = tap % 3;
    double s = 0.0;
    if (row < rows)
        for (int m = 0; m < 32; m++) {
            const float* ws = w3 + ((size_t)m * 64 + ci) * 9;
            double p = 0.0;
            for (int dy = 0; dy < 3; dy++)
                for (int dx = 0; dx < 3; dx++) p += (double)ws[dy * 3 + dx] * (R[py][dy][ta] * R[px][dx][tb]);
            s += (double)d[row * 32 + m] * p;
        }
    wc[idx] = (f16)(float)s;
}

template <int ND>
int launch_l4c_nd(const L4cArgs& a, hipStream_t st) {
    const long tiles = (long)a.B * ((a.H + 15) / 16) * ((a.W + 15) / 16);
    // as many workgroups as the chip holds at once (41 KiB of LDS each; nd = 2: 128 registers x 8 waves -> two per CU, nd = 3: one)
    long slots = (long)pp_device_cus() * (ND == 1 ? 3 : (ND == 2 ? 2 : 1));
    const long cap = moge_tune_get(TK_CONV_GRID);      // tests: a small grid makes small problems walk many tiles per workgroup
    if (cap > 0) slots = cap;
    const unsigned grid = (unsigned)(tiles < slots ? tiles : slots);
    if (a.wu) hipLaunchKernelGGL((l4c_kernel<ND, true>), dim3(grid), dim3(256 * ND), L4C_LDS, st, a);
    else hipLaunchKernelGGL((l4c_kernel<ND, false>), dim3(grid), dim3(256 * ND), L4C_LDS, st, a);
    return (int)hipGetLastError();
}

}  // namespace

int launch_l4c_pack(const float* w3, const float* d, int rows, int nd, int nearest, const float* bias, const float* wu, const float* wv, void* wc, float* vec,
                    hipStream_t st) {
    if (nd < 1 || nd > 3 || rows < 1 || rows > 4 * nd || !w3 || !d || !wc || !vec) return -1;
    hipLaunchKernelGGL(l4c_pack_kernel, dim3((nd * 16 * 576 + 255) / 256), dim3(256), 0, st, w3, d, rows, nd, nearest, bias, wu, wv, (f16*)wc, vec);
    return (int)hipGetLastError();
}

int launch_l4c(const L4cArgs& a, hipStream_t st) {
    if (!a.in || !a.wc || !a.bias || !a.out || a.B < 1 || a.H < 1 || a.W < 1 || (a.wu && !a.wv)) return -1;
    if ((long)a.H * a.W * 128 >= (1L << 31)) return -1;                                      // 32-bit halo offsets inside an image
    if ((long)a.B * ((a.H + 15) / 16) * ((a.W + 15) / 16) >= (1L << 31)) return -1;
    switch (a.nd) {
    case 1: return launch_l4c_nd<1>(a, st);
    case 2: return launch_l4c_nd<2>(a, st);
    case 3: return launch_l4c_nd<3>(a, st);
    default: return -1;
    }
}
