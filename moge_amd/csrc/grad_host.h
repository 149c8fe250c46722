// Host half of the trainable product family (linear_grad.hip, conv_grad.hip, convt_grad.hip): the tile and chunk arithmetic, the argument checks, the
// split rules of the weight and bias gradients, and - for the two gathered convs, whose C entries differ in a handful of constants and in the kernels
// they launch - the workspace layout, the db launch and the bodies of the three entry points, written once over a traits struct K:
//     NAME                                   entry prefix: NAME_workspace, NAME_forward, NAME_backward
//     TAPS, UP, COLS                         kernel taps; output pixels per input pixel (y and dy have UP B H W rows); columns of the widest product per Cout
//     FILL, MAX_SPLIT, MIN_KTILES            wgrad's split (grad_split)
//     DB_ROWS, DB_MAX                        db's slabs (db_split)
//     MAX_WEIGHT                             the Cin Cout limit (the pixel limit is 2^30 rows of y for both)
//     PIXELS_MSG, WEIGHT_MSG, GRID_MSG       the words of the three limits
//     forward<T>, dgrad<T>, wgrad<T>         the launches (the repack of the weight included); wgrad leaves fp32 partials [part][tap][.][.]
// Every split is a function of the sizes and the dtype only, so that the bits do not depend on the device.
#pragma once
#include <string>

#include "common.h"
#include "lds_image.h"

namespace {

inline long long tiles(long long n) { return (n + LT - 1) / LT; }
inline int chunk_of(int dtype) { return dtype == MOGE_FP16 ? 8 : 4; }
inline long long align16(long long n) { return (n + 15) / 16 * 16; }
inline long long ktiles_of(long long k, int dtype) { return (k + LCPR * chunk_of(dtype) - 1) / (LCPR * chunk_of(dtype)); }

// rows of `cols` elements (`noun`: what a row is) read or written in place: 16-byte aligned, leading dimension a multiple of 16 bytes and at least cols
int check_rows(const char* fn, const char* name, const char* ldname, const void* p, int64_t ld, int cols, int dtype, const char* noun) {
    if (!p) return moge_internal_fail(MOGE_ERR_INVALID, "%s: %s is null", fn, name);
    if ((uintptr_t)p % 16) return moge_internal_fail(MOGE_ERR_INVALID, "%s: %s is not 16-byte aligned", fn, name);
    if (ld < cols || ld % chunk_of(dtype))
        return moge_internal_fail(MOGE_ERR_INVALID, "%s: %s = %lld is not a multiple of %d elements (16-byte vector accesses) of at least the %s %d", fn, ldname,
                                  (long long)ld, chunk_of(dtype), noun, cols);
    return 0;
}
int check_dtype(const char* fn, int dtype) {
    if (dtype != MOGE_FP32 && dtype != MOGE_FP16) return moge_internal_fail(MOGE_ERR_INVALID, "%s: unknown dtype %d (MOGE_FP32 or MOGE_FP16)", fn, dtype);
    return 0;
}
// a channel or feature count
int check_count(const char* fn, const char* name, int n, int dtype) {
    if (n < 1 || n % chunk_of(dtype))
        return moge_internal_fail(MOGE_ERR_INVALID, "%s: %s = %d is not a positive multiple of %d elements (16-byte vector accesses)", fn, name, n, chunk_of(dtype));
    return 0;
}
int check_vector(const char* fn, const char* name, const void* p, bool required) {
    if (!p && required) return moge_internal_fail(MOGE_ERR_INVALID, "%s: %s is null", fn, name);
    if ((uintptr_t)p % 16) return moge_internal_fail(MOGE_ERR_INVALID, "%s: %s is not 16-byte aligned", fn, name);
    return 0;
}

// parts a weight gradient's contraction over k rows aims for, with t workgroups to a part: enough to reach `fill` workgroups, a part no shorter than
// min_ktiles K tiles, max_split at the most; 1 = no split
long long split_target(long long k, long long t, int fill, int max_split, int min_ktiles, int dtype) {
    long long s = fill / t;
    if (s > ktiles_of(k, dtype) / min_ktiles) s = ktiles_of(k, dtype) / min_ktiles;
    if (s > max_split) s = max_split;
    return s < 1 ? 1 : s;
}
// the convs' form of it: `per` K tiles to a part, `parts` parts that have work (the last one takes what is left); the workspace query and the launch both
// read this one result
struct GradSplit { int parts; long long per; };
GradSplit grad_split(long long k, long long t, int fill, int max_split, int min_ktiles, int dtype) {
    const long long ktiles = ktiles_of(k, dtype), s = split_target(k, t, fill, max_split, min_ktiles, dtype);
    const long long per = ktiles ? (ktiles + s - 1) / s : 1;
    return GradSplit{ktiles ? (int)((ktiles + per - 1) / per) : 1, per};
}
// db's slabs of at least min_rows rows
int db_split(long long rows, int min_rows, int max_slabs) {
    const long long s = (rows + min_rows - 1) / min_rows;
    return s < 1 ? 1 : (s > max_slabs ? max_slabs : (int)s);
}

// out[z][n] = the column sums of slab z of dy (M, N), S slabs of ceil(M / S) rows
template <typename T, typename TO>
void launch_colsum(const void* dy, int64_t lddy, TO* out, int M, int N, int S, hipStream_t st) {
    hipLaunchKernelGGL((lin_colsum_kernel<T, TO>), dim3(blocks(N, 8 * TT<T>::CH), (unsigned)S), dim3(256), 0, st, (const T*)dy, (long long)lddy, out, M, N, (M + S - 1) / S);
}

// ---- the gathered convs ------------------------------------------------------------------------------------------------------------
template <typename K> GradSplit conv_split(long long M, int Cin, int Cout, int dtype) {
    return grad_split(M, K::TAPS * tiles(Cout) * tiles(Cin), K::FILL, K::MAX_SPLIT, K::MIN_KTILES, dtype);
}
template <typename K> int conv_db_split(long long M) { return db_split(K::UP * M, K::DB_ROWS, K::DB_MAX); }

struct ConvWs { long long wp, part, dbpart, total; };           // byte offsets of the packed weight, the dw partials and the db partials
template <typename K> ConvWs conv_ws(long long M, int Cin, int Cout, int dtype) {
    ConvWs w;
    const long long n = (long long)Cout * Cin;
    w.wp = 0;
    w.part = align16(K::TAPS * n * (dtype == MOGE_FP16 ? 2 : 4));
    w.dbpart = w.part + 4LL * conv_split<K>(M, Cin, Cout, dtype).parts * K::TAPS * n;
    w.total = w.dbpart + align16(4LL * conv_db_split<K>(M) * Cout);
    return w;
}

template <typename K> int conv_check_sizes(const char* fn, int dtype, int B, int H, int W, int Cin, int Cout) {
    if (int e = check_dtype(fn, dtype)) return e;
    if (B < 0) return moge_internal_fail(MOGE_ERR_INVALID, "%s: B < 0", fn);
    if (H < 1) return moge_internal_fail(MOGE_ERR_INVALID, "%s: H = %d < 1", fn, H);
    if (W < 1) return moge_internal_fail(MOGE_ERR_INVALID, "%s: W = %d < 1", fn, W);
    if (int e = check_count(fn, "Cin", Cin, dtype)) return e;
    if (int e = check_count(fn, "Cout", Cout, dtype)) return e;
    constexpr long long max_pixels = (1LL << 30) / K::UP;
    if ((long long)B * H > max_pixels || (long long)B * H * W > max_pixels) return moge_internal_fail(MOGE_ERR_INVALID, "%s: %s", fn, K::PIXELS_MSG);
    if ((long long)Cin * Cout > K::MAX_WEIGHT) return moge_internal_fail(MOGE_ERR_INVALID, "%s: %s", fn, K::WEIGHT_MSG);
    const long long cols = (long long)K::COLS * Cout;
    if (tiles((long long)B * H * W) * tiles(Cin > cols ? Cin : cols) > 0x7fffffffLL) return moge_internal_fail(MOGE_ERR_INVALID, "%s: %s", fn, K::GRID_MSG);
    return 0;
}
// an activation (B, H, W, C) read or written in place on a dense pixel grid
inline int check_pixels(const char* fn, const char* name, const char* ldname, const void* p, int64_t ld, int C, int dtype) {
    return check_rows(fn, name, ldname, p, ld, C, dtype, "channel count");
}

template <typename K, typename T>
void conv_launch_backward(const void* x, int64_t ldx, const void* w, const void* dy, int64_t lddy, void* dx, int64_t lddx, void* dw, void* db, char* ws, int M, int H, int W,
                          int Cin, int Cout, int dtype, hipStream_t st) {
    const ConvWs o = conv_ws<K>(M, Cin, Cout, dtype);
    if (dx) K::template dgrad<T>(dy, lddy, w, ws + o.wp, dx, lddx, M, H, W, Cin, Cout, st);
    if (dw) {
        const GradSplit sp = conv_split<K>(M, Cin, Cout, dtype);
        float* part = (float*)(ws + o.part);
        K::template wgrad<T>(x, ldx, dy, lddy, part, M, H, W, Cin, Cout, sp.parts, (int)sp.per * LCPR * TT<T>::CH, st);      // the last argument: pixels of a part
        hipLaunchKernelGGL((lin_tap_reduce_kernel<T, K::TAPS>), dim3(blocks((int64_t)Cout * Cin, 256)), dim3(256), 0, st, (const float*)part, (T*)dw, Cout * Cin, sp.parts);
    }
    if (db) {
        const int S = conv_db_split<K>(M);
        float* part = (float*)(ws + o.dbpart);
        launch_colsum<T, float>(dy, lddy, part, K::UP * M, Cout, S, st);
        hipLaunchKernelGGL(lin_colsum_reduce_kernel<T>, dim3(blocks(Cout, 256)), dim3(256), 0, st, (const float*)part, (T*)db, Cout, S);
    }
}

template <typename K> int conv_workspace(int B, int H, int W, int Cin, int Cout, int dtype, int64_t* forward_bytes, int64_t* backward_bytes) {
    static const std::string name = std::string(K::NAME) + "_workspace";
    const char* fn = name.c_str();
    if (!forward_bytes) return moge_internal_fail(MOGE_ERR_INVALID, "%s: forward_bytes is null", fn);
    if (!backward_bytes) return moge_internal_fail(MOGE_ERR_INVALID, "%s: backward_bytes is null", fn);
    *forward_bytes = *backward_bytes = 0;
    if (int e = conv_check_sizes<K>(fn, dtype, B, H, W, Cin, Cout)) return e;
    const ConvWs o = conv_ws<K>((long long)B * H * W, Cin, Cout, dtype);
    *forward_bytes = o.part;
    *backward_bytes = o.total;
    return 0;
}

template <typename K>
int conv_forward(int dtype, const void* x, int64_t ldx, const void* w, const void* bias, void* y, int64_t ldy, int B, int H, int W, int Cin, int Cout, void* workspace,
                 void* stream) {
    static const std::string name = std::string(K::NAME) + "_forward", failed = name + ": launch failed";
    const char* fn = name.c_str();
    if (int e = conv_check_sizes<K>(fn, dtype, B, H, W, Cin, Cout)) return e;
    if (B == 0) return 0;
    if (int e = check_pixels(fn, "x", "ldx", x, ldx, Cin, dtype)) return e;
    if (int e = check_vector(fn, "w", w, true)) return e;
    if (int e = check_vector(fn, "bias", bias, false)) return e;
    if (int e = check_pixels(fn, "y", "ldy", y, ldy, Cout, dtype)) return e;
    if (int e = check_vector(fn, "workspace", workspace, true)) return e;
    if (dtype == MOGE_FP16) K::template forward<f16>(x, ldx, w, bias, y, ldy, workspace, B * H * W, H, W, Cin, Cout, (hipStream_t)stream);
    else K::template forward<float>(x, ldx, w, bias, y, ldy, workspace, B * H * W, H, W, Cin, Cout, (hipStream_t)stream);
    return launched(failed.c_str());
}

template <typename K>
int conv_backward(int dtype, const void* x, int64_t ldx, const void* w, const void* dy, int64_t lddy, void* dx, int64_t lddx, void* dw, void* db, void* workspace, int B, int H,
                  int W, int Cin, int Cout, void* stream) {
    static const std::string name = std::string(K::NAME) + "_backward", failed = name + ": launch failed";
    const char* fn = name.c_str();
    if (int e = conv_check_sizes<K>(fn, dtype, B, H, W, Cin, Cout)) return e;
    if (B == 0 || (!dx && !dw && !db)) return 0;
    if (int e = check_pixels(fn, "dy", "lddy", dy, lddy, Cout, dtype)) return e;
    if (dx) {
        if (int e = check_vector(fn, "w", w, true)) return e;
        if (int e = check_pixels(fn, "dx", "lddx", dx, lddx, Cin, dtype)) return e;
    }
    if (dw) {
        if (int e = check_pixels(fn, "x", "ldx", x, ldx, Cin, dtype)) return e;
        if (int e = check_vector(fn, "dw", dw, true)) return e;
    }
    if (int e = check_vector(fn, "db", db, false)) return e;
    if (int e = check_vector(fn, "workspace", workspace, true)) return e;
    if (dtype == MOGE_FP16) conv_launch_backward<K, f16>(x, ldx, w, dy, lddy, dx, lddx, dw, db, (char*)workspace, B * H * W, H, W, Cin, Cout, dtype, (hipStream_t)stream);
    else conv_launch_backward<K, float>(x, ldx, w, dy, lddy, dx, lddx, dw, db, (char*)workspace, B * H * W, H, W, Cin, Cout, dtype, (hipStream_t)stream);
    return launched(failed.c_str());
}

}  // namespace
