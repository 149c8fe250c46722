// The three tables of a handle and what fills them: the checkpoint's fp32 master layout, the derived fp32 vectors (aux) and the kernel-layout matrices per
// precision (packed), with the host- and device-side weight composition of the fused fp16 paths.
#include "model_internal.h"

#include <type_traits>

namespace model __attribute__((visibility("hidden"))) {

// ------------------------------------------------------------------------------------------------------------
// weight table
// ------------------------------------------------------------------------------------------------------------
static void tadd(moge_handle* h, const std::string& name, int64_t numel) {
    TInfo t{h->master_floats, numel, false};
    h->table[name] = t;
    h->master_floats += (size_t)((numel + 63) / 64 * 64);
}
static void aadd(moge_handle* h, const std::string& name, int64_t numel) {
    h->aux_off[name] = h->aux_floats;
    h->aux_floats += (size_t)((numel + 63) / 64 * 64);
}
static void padd(moge_handle* h, const std::string& name, int64_t numel) {
    h->pk_off[name] = h->pk_elems;
    h->pk_elems += (size_t)((numel + 63) / 64 * 64);
}
std::string S(const char* fmt, ...) {
    char buf[256];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    return buf;
}

// Term tables of the composed weight blocks (Ct3Slot, elementwise.hip ct3_combine_kernel).  P(k = ky * 3 + kx, s = sy * 2 + sx) = W3[:, :, ky, kx] . WT[:, :, sy, sx]^T.
// Interior, phase (py, px), tap (tdy, tdx) = low-res pixel (y + py - 1 + tdy, x + px - 1 + tdx): the 3x3 taps whose high-res row 2y + py + ky - 1 lies in that
// low-res row, with the parity it has there:   py = 0: tdy = 0 <- (ky 0, sy 1);  tdy = 1 <- (ky 1, sy 0), (ky 2, sy 1);   py = 1: tdy = 0 <- (ky 0, sy 0), (ky 1, sy 1);
// tdy = 1 <- (ky 2, sy 0) - and the same along x.
static void ct3_interior_slots(std::vector<Ct3Slot>& v) {
    auto members = [](int p, int td, int (&kk)[2], int (&ss)[2]) -> int {
        if (p == 0 && td == 0) { kk[0] = 0; ss[0] = 1; return 1; }
        if (p == 0 && td == 1) { kk[0] = 1; ss[0] = 0; kk[1] = 2; ss[1] = 1; return 2; }
        if (p == 1 && td == 0) { kk[0] = 0; ss[0] = 0; kk[1] = 1; ss[1] = 1; return 2; }
        kk[0] = 2; ss[0] = 0; return 1;
    };
    for (int py = 0; py < 2; py++) for (int px = 0; px < 2; px++) for (int tdy = 0; tdy < 2; tdy++) for (int tdx = 0; tdx < 2; tdx++) {
        Ct3Slot sl; memset(&sl, 0, sizeof(sl));
        sl.rowblk = py * 2 + px; sl.colblk = tdy * 2 + tdx;
        int ky[2], sy[2], kx[2], sx[2];
        const int ny = members(py, tdy, ky, sy), nx = members(px, tdx, kx, sx);
        for (int a = 0; a < ny; a++) for (int b2 = 0; b2 < nx; b2++) sl.term[sl.nterms++] = (ky[a] * 3 + kx[b2]) | ((sy[a] * 2 + sx[b2]) << 4);
        v.push_back(sl);
    }
}
// Border classes (conv_pp.hip ct3_border_kernel): exact (replicate-padded high-res map) minus composed (= reflecting pad), evaluated symbolically on a 4 x 4
// low-res map for one representative pixel per class; every term lands on one of the class's two cells.
static int ct3_border_slots(std::vector<Ct3Slot>& v) {
    const int H = 4, W = 4;
    struct Rep { int Y, X, cy0, cx0, cy1, cx1; };
    const Rep reps[12] = {{0, 4, 0, 1, 0, 2}, {0, 3, 0, 1, 0, 2}, {7, 4, 3, 1, 3, 2}, {7, 3, 3, 1, 3, 2},
                          {4, 0, 1, 0, 2, 0}, {3, 0, 1, 0, 2, 0}, {4, 7, 1, 3, 2, 3}, {3, 7, 1, 3, 2, 3},
                          {0, 0, 0, 0, -1, -1}, {0, 7, 0, 3, -1, -1}, {7, 0, 3, 0, -1, -1}, {7, 7, 3, 3, -1, -1}};
    for (int cls = 0; cls < 12; cls++) {
        const Rep& r = reps[cls];
        Ct3Slot sl[2]; memset(sl, 0, sizeof(sl));
        sl[0].rowblk = sl[1].rowblk = cls; sl[0].colblk = 0; sl[1].colblk = 1;
        for (int ky = 0; ky < 3; ky++) for (int kx = 0; kx < 3; kx++) {
            const int rr = r.Y + ky - 1, cc = r.X + kx - 1;
            const int r_rep = rr < 0 ? 0 : (rr > 2 * H - 1 ? 2 * H - 1 : rr), c_rep = cc < 0 ? 0 : (cc > 2 * W - 1 ? 2 * W - 1 : cc);
            const int r_ref = rr < 0 ? 1 : (rr > 2 * H - 1 ? 2 * H - 2 : rr), c_ref = cc < 0 ? 1 : (cc > 2 * W - 1 ? 2 * W - 2 : cc);
            if (r_rep == r_ref && c_rep == c_ref) continue;
            for (int side = 0; side < 2; side++) {            // + replicated, - reflected
                const int ry = side ? r_ref : r_rep, cx = side ? c_ref : c_rep;
                const int cy = ry >> 1, cxx = cx >> 1, sidx = (ry & 1) * 2 + (cx & 1);
                const int slot = (cy == r.cy0 && cxx == r.cx0) ? 0 : ((cy == r.cy1 && cxx == r.cx1) ? 1 : -1);
                if (slot < 0 || sl[slot].nterms >= 13) return -1;
                sl[slot].term[sl[slot].nterms++] = (ky * 3 + kx) | (sidx << 4) | (side ? 256 : 0);
            }
        }
        v.push_back(sl[0]); v.push_back(sl[1]);
    }
    return 0;
}

static void build_tables_v2_decoder(moge_handle* h) {
    const moge_config& c = h->cfg;
    const int D = c.embed_dim, c0 = c.dims[0];
    auto stack = [&](const std::string& name, bool neck, const int* nres, int cout) {
        const int* rs = stack_rs(c, neck);
        const int in_norm = neck ? c.neck_in_norm : c.head_in_norm, hid_norm = neck ? c.neck_hidden_norm : c.head_hidden_norm;
        for (int l = 0; l < MOGE_LEVELS; l++) {
            const int cl = c.dims[l];
            const int cin = neck ? (l == 0 ? c0 + 2 : 2) : cl;
            tadd(h, name + S(".input_blocks.%d.weight", l), (int64_t)cl * cin);
            tadd(h, name + S(".input_blocks.%d.bias", l), cl);
            if (neck) {
                aadd(h, name + S(".in%d.wu", l), cl);
                aadd(h, name + S(".in%d.wv", l), cl);
                if (l == 0) {
                    padd(h, name + ".in0.w", (int64_t)cl * c0);
                    // fp16 path: the summed output projections and this 1x1 block have no non-linearity between them (modules.py:128-131,
                    // 245): composed at pack time into ONE [c0][n_taps * D] matrix applied to the K-concatenated taps (`compose` in forward_impl)
                    padd(h, name + ".in0c.w", (int64_t)cl * c.n_taps * D);
                    aadd(h, name + ".in0c.bias", cl);
                }
                else aadd(h, name + S(".rs%d.bias2", l - 1), cl);
            } else {
                padd(h, name + S(".in%d.w", l), (int64_t)cl * cl);
            }
        }
        for (int l = 0; l < MOGE_LEVELS - 1; l++) {
            const int ci = c.dims[l], co = c.dims[l + 1];
            if (rs[l] == MOGE_RS_PIXEL_SHUFFLE) {
                // Conv2d(ci, 4 co, 3x3) -> PixelShuffle(2) -> Conv2d(co, co, 3x3)   (modules.py:146-151)
                tadd(h, name + S(".resamplers.%d.0.weight", l), (int64_t)4 * co * ci * 9);
                tadd(h, name + S(".resamplers.%d.0.bias", l), 4 * co);
                tadd(h, name + S(".resamplers.%d.2.weight", l), (int64_t)co * co * 9);
                tadd(h, name + S(".resamplers.%d.2.bias", l), co);
                padd(h, name + S(".rs%d.w3p", l), (int64_t)4 * co * 9 * ci);       // rows permuted to (dy, dx, co): the phase-conv layout
                padd(h, name + S(".rs%d.w3", l), (int64_t)co * 9 * co);
                aadd(h, name + S(".rs%d.bias4", l), 4 * co);
            } else if (rs[l] == MOGE_RS_CONV_TRANSPOSE) {
                tadd(h, name + S(".resamplers.%d.0.weight", l), (int64_t)ci * co * 4);
                tadd(h, name + S(".resamplers.%d.0.bias", l), co);
                tadd(h, name + S(".resamplers.%d.1.weight", l), (int64_t)co * co * 9);
                tadd(h, name + S(".resamplers.%d.1.bias", l), co);
                padd(h, name + S(".rs%d.wT", l), (int64_t)4 * co * ci);
                padd(h, name + S(".rs%d.w3", l), (int64_t)co * 9 * co);
                aadd(h, name + S(".rs%d.biasT", l), 4 * co);
                if (!neck) aadd(h, name + S(".rs%d.bias_in", l), co);     // resampler conv bias + next level's input-block bias (fused path)
                if (ct3_shape(ci, co)) {
                    // fp16 path (round 6): ConvTranspose2d + 3x3 composed into ONE 4-phase 2x2-tap conv on the low-res map (conv_pp.hip CT3) + its border weights
                    padd(h, name + S(".rs%d.wc", l), (int64_t)4 * co * 4 * ci);
                    padd(h, name + S(".rs%d.dw", l), (int64_t)12 * co * 2 * ci);
                    aadd(h, name + S(".rs%d.bias_ct3", l), 4 * co);
                }
                if (!neck && l == 0 && nres[0] == 0) {
                    // fp16 path: a head without level-0 residual blocks applies its ConvTranspose2d directly to its level-0 input block
                    // (modules.py:245-250): both linear, composed at pack time into one [4 co][c0] matrix on the neck's level-0 map
                    padd(h, name + ".rs0.wTc", (int64_t)4 * co * ci);
                    aadd(h, name + ".rs0.biasTc", 4 * co);
                }
            } else {
                tadd(h, name + S(".resamplers.%d.1.weight", l), (int64_t)co * ci * 9);
                tadd(h, name + S(".resamplers.%d.1.bias", l), co);
                padd(h, name + S(".rs%d.w3p", l), (int64_t)4 * co * 9 * ci);
                aadd(h, name + S(".rs%d.bias4", l), 4 * co);
            }
        }
        for (int l = 0; l < MOGE_LEVELS; l++)
            for (int j = 0; j < nres[l]; j++) {
                const int cl = c.dims[l], ch = cl * stack_mult(c, neck);          // hidden width (modules.py:222)
                // (InstanceNorm2d has no parameters: affine=False, track_running_stats=False - nothing in the state dict)
                if (in_norm && in_norm != MOGE_NORM_INSTANCE) { tadd(h, name + S(".res_blocks.%d.%d.layers.0.weight", l, j), cl); tadd(h, name + S(".res_blocks.%d.%d.layers.0.bias", l, j), cl); }
                if (hid_norm && hid_norm != MOGE_NORM_INSTANCE) { tadd(h, name + S(".res_blocks.%d.%d.layers.3.weight", l, j), ch); tadd(h, name + S(".res_blocks.%d.%d.layers.3.bias", l, j), ch); }
                for (int li = 2; li <= 5; li += 3) {
                    tadd(h, name + S(".res_blocks.%d.%d.layers.%d.weight", l, j, li), (int64_t)cl * ch * 9);
                    tadd(h, name + S(".res_blocks.%d.%d.layers.%d.bias", l, j, li), li == 2 ? ch : cl);
                    padd(h, name + S(".res%d.%d.w%d", l, j, li == 2 ? 1 : 2), (int64_t)cl * 9 * ch);
                }
            }
        if (cout > 0) {
            tadd(h, name + ".output_blocks.4.weight", (int64_t)cout * c.dims[4]);
            tadd(h, name + ".output_blocks.4.bias", cout);
            aadd(h, name + ".out4.w2", (int64_t)cout * c.dims[4]);      // output conv o level-4 input block (fp16 path, see head_final_kernel)
            aadd(h, name + ".out4.b2", cout);
            aadd(h, name + ".l4c.w", 16 * 576 / 2);                     // l4c.hip: Wout . (4-phase resampler weights), f16 [16][576]
            aadd(h, name + ".l4c.v", 3 * 12);                           // ... Wout . bias (no uv term in a head)
        }
        if (neck) {
            aadd(h, "neck.dot.w2cat", 3 * 4 * 32);                      // the heads' (Wout . Win4) rows, four per head (zero padded), head order
            aadd(h, "neck.l4c.w", 3 * 16 * 576 / 2);                    // l4c.hip: those rows . (the neck's 4-phase resampler weights), f16 [nheads][16][576]
            aadd(h, "neck.l4c.v", 3 * 12);                              // ... and . (bias, wu, wv) of level 4
        }
    };
    stack("neck", true, c.neck_res_blocks, 0);
    for (int k = 0; k < 3; k++)
        if (c.heads & HEAD_BITS[k]) stack(HEAD_NAMES[k], false, c.head_res_blocks, HEAD_COUT[k]);
    if (c.heads & MOGE_HEAD_SCALE) {
        const int hd = c.scale_hidden;
        tadd(h, "scale_head.0.weight", (int64_t)hd * D); tadd(h, "scale_head.0.bias", hd);
        tadd(h, "scale_head.2.weight", (int64_t)hd * hd); tadd(h, "scale_head.2.bias", hd);
        tadd(h, "scale_head.4.weight", hd); tadd(h, "scale_head.4.bias", 1);
    }
}

static void build_tables_v1_decoder(moge_handle* h) {
    const moge_v1_config& c = h->cfg1;
    for (int i = 0; i < c.n_up; i++) {
        const int ci = i == 0 ? c.dim_proj : c.dim_upsample[i - 1], co = c.dim_upsample[i];
        const std::string u = S("head.upsample_blocks.%d.", i);
        tadd(h, u + "0.0.weight", (int64_t)(ci + 2) * co * 4); tadd(h, u + "0.0.bias", co);
        tadd(h, u + "0.1.weight", (int64_t)co * co * 9); tadd(h, u + "0.1.bias", co);
        padd(h, S("v1.up%d.wT", i), (int64_t)4 * co * ci);
        padd(h, S("v1.up%d.w3", i), (int64_t)co * 9 * co);
        aadd(h, S("v1.up%d.wu", i), 4 * co); aadd(h, S("v1.up%d.wv", i), 4 * co); aadd(h, S("v1.up%d.biasT", i), 4 * co);
        for (int j = 0; j < c.num_res_blocks; j++) {
            const std::string r = u + S("%d.layers.", 1 + j);
            const int ch = co * v1_mult(c);                      // hidden width (v1.py:85)
            tadd(h, r + "0.weight", co); tadd(h, r + "0.bias", co);
            tadd(h, r + "2.weight", (int64_t)ch * co * 9); tadd(h, r + "2.bias", ch);
            tadd(h, r + "3.weight", ch); tadd(h, r + "3.bias", ch);
            tadd(h, r + "5.weight", (int64_t)co * ch * 9); tadd(h, r + "5.bias", co);
            padd(h, S("v1.up%d.res%d.w1", i, j), (int64_t)ch * 9 * co);
            padd(h, S("v1.up%d.res%d.w2", i, j), (int64_t)co * 9 * ch);
        }
    }
    const int cl = c.dim_upsample[c.n_up - 1], c4 = c.last_conv_channels;
    const int nl = c.last_res_blocks, ks = v1_ks(c), ch4 = c4 * v1_mult(c);
    for (int o = 0; o < 2; o++) {
        // nn.Sequential(3x3, ResidualConvBlock x last_res_blocks, ReLU, Conv2d(k = last_conv_size))   (v1.py:103-109)
        const std::string b = S("head.output_block.%d.", o);
        tadd(h, b + "0.weight", (int64_t)c4 * (cl + 2) * 9); tadd(h, b + "0.bias", c4);
        for (int j = 0; j < nl; j++) {
            const std::string r = b + S("%d.layers.", 1 + j);
            tadd(h, r + "0.weight", c4); tadd(h, r + "0.bias", c4);
            tadd(h, r + "2.weight", (int64_t)ch4 * c4 * 9); tadd(h, r + "2.bias", ch4);
            tadd(h, r + "3.weight", ch4); tadd(h, r + "3.bias", ch4);
            tadd(h, r + "5.weight", (int64_t)c4 * ch4 * 9); tadd(h, r + "5.bias", c4);
            padd(h, S("v1.out%d.res%d.w1", o, j), (int64_t)ch4 * 9 * c4);
            padd(h, S("v1.out%d.res%d.w2", o, j), (int64_t)c4 * 9 * ch4);
        }
        tadd(h, b + S("%d.weight", nl + 2), (int64_t)(o == 0 ? 3 : 1) * c4 * ks * ks); tadd(h, b + S("%d.bias", nl + 2), o == 0 ? 3 : 1);
    }
    padd(h, "v1.out.w3", (int64_t)2 * c4 * 9 * v1_cpad(cl));
    aadd(h, "v1.out.bias", 2 * c4);
}

void build_tables(moge_handle* h) {
    const moge_config& c = h->cfg;
    const int D = c.embed_dim, c0 = c.dims[0];
    const std::string bb = h->bb;
    tadd(h, bb + "cls_token", D);
    tadd(h, bb + "pos_embed", (int64_t)(1 + 37 * 37) * D);
    tadd(h, bb + "patch_embed.proj.weight", (int64_t)D * KPATCH);
    tadd(h, bb + "patch_embed.proj.bias", D);
    padd(h, "patch.w", (int64_t)D * KPATCH_PAD);
    for (int i = 0; i < c.depth; i++) {
        const std::string p = bb + S("blocks.%d.", i);
        tadd(h, p + "norm1.weight", D); tadd(h, p + "norm1.bias", D);
        tadd(h, p + "attn.qkv.weight", (int64_t)3 * D * D); tadd(h, p + "attn.qkv.bias", 3 * D);
        tadd(h, p + "attn.proj.weight", (int64_t)D * D); tadd(h, p + "attn.proj.bias", D);
        tadd(h, p + "ls1.gamma", D);
        tadd(h, p + "norm2.weight", D); tadd(h, p + "norm2.bias", D);
        tadd(h, p + "mlp.fc1.weight", (int64_t)4 * D * D); tadd(h, p + "mlp.fc1.bias", 4 * D);
        tadd(h, p + "mlp.fc2.weight", (int64_t)4 * D * D); tadd(h, p + "mlp.fc2.bias", D);
        tadd(h, p + "ls2.gamma", D);
        padd(h, S("blk%d.qkv", i), (int64_t)3 * D * D);
        padd(h, S("blk%d.proj", i), (int64_t)D * D);
        padd(h, S("blk%d.fc1", i), (int64_t)4 * D * D);
        padd(h, S("blk%d.fc2", i), (int64_t)4 * D * D);
        // LN fold (fp16 path): norm1 folded into qkv, norm2 into fc1:  W' = g (.) W,  c = row sums of W',  b' = b + W beta
        padd(h, S("blk%d.qkvf", i), (int64_t)3 * D * D);
        padd(h, S("blk%d.fc1f", i), (int64_t)4 * D * D);
        aadd(h, S("blk%d.qkv.c", i), 3 * D); aadd(h, S("blk%d.qkv.bf", i), 3 * D);
        aadd(h, S("blk%d.fc1.c", i), 4 * D); aadd(h, S("blk%d.fc1.bf", i), 4 * D);
    }
    tadd(h, bb + "norm.weight", D); tadd(h, bb + "norm.bias", D);
    for (int k = 0; k < c.n_taps; k++) {
        tadd(h, S(h->proj_fmt, k) + ".weight", (int64_t)c0 * D);
        tadd(h, S(h->proj_fmt, k) + ".bias", c0);
    }
    tadd(h, h->mean_key, 3);
    tadd(h, h->std_key, 3);
    padd(h, "outproj.w", (int64_t)c0 * c.n_taps * D);
    aadd(h, "outproj.bias", c0);
    if (h->version == 1) build_tables_v1_decoder(h);
    else build_tables_v2_decoder(h);
}

// ------------------------------------------------------------------------------------------------------------
// packing (device side, from the fp32 master)
// ------------------------------------------------------------------------------------------------------------
// Blocking copies of the host-side weight products of build_aux (load time, once per handle): n device floats into a host vector, and a vector back.
static int fetch(const float* dev, size_t n, std::vector<float>& v, hipStream_t st) {
    v.resize(n);
    HIPCHK(hipMemcpyAsync(v.data(), dev, n * sizeof(float), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    return 0;
}
static int store(float* dev, const std::vector<float>& v, hipStream_t st) {
    HIPCHK(hipMemcpyAsync(dev, v.data(), v.size() * sizeof(float), hipMemcpyHostToDevice, st));
    HIPCHK(hipStreamSynchronize(st));      // (v is pageable and may go out of scope behind the call)
    return 0;
}

static int build_aux_v1(moge_handle* h, hipStream_t st) {
    const moge_v1_config& c = h->cfg1;
    for (int i = 0; i < c.n_up; i++) {
        const int ci = i == 0 ? c.dim_proj : c.dim_upsample[i - 1], co = c.dim_upsample[i];
        const float* w = M(h, S("head.upsample_blocks.%d.0.0.weight", i));              // [ci + 2][co][2][2]; rows ci, ci + 1 = (u, v) inputs
        LCHK(launch_repack<float>(w + (size_t)ci * co * 4, A(h, S("v1.up%d.wu", i)), 4, co, 1, 1, 1, 4, 0, 0, co, 1, 0, st));
        LCHK(launch_repack<float>(w + (size_t)(ci + 1) * co * 4, A(h, S("v1.up%d.wv", i)), 4, co, 1, 1, 1, 4, 0, 0, co, 1, 0, st));
        LCHK(launch_repack<float>(M(h, S("head.upsample_blocks.%d.0.0.bias", i)), A(h, S("v1.up%d.biasT", i)), 4, 1, 1, co, 0, 0, 0, 1, co, 0, 0, st));
    }
    const int c4 = c.last_conv_channels;
    for (int o = 0; o < 2; o++)
        LCHK(launch_repack<float>(M(h, S("head.output_block.%d.0.bias", o)), A(h, "v1.out.bias") + o * c4, 1, 1, 1, c4, 0, 0, 0, 1, 0, 0, 0, st));
    return 0;
}

int build_aux(moge_handle* h, hipStream_t st) {
    if (h->aux_ready) return 0;
    const moge_config& c = h->cfg;
    if (!h->aux) HIPCHK(hipMalloc(&h->aux, h->aux_floats * sizeof(float)));
    HIPCHK(hipMemsetAsync(h->aux, 0, h->aux_floats * sizeof(float), st));
    const int c0 = c.dims[0];
    // outproj.bias = sum_k bias_k : n_taps strided adds via repack (dst += not available) -> do on host-visible path: tiny D2H/H2D
    {
        std::vector<float> acc(c0, 0.f), tmp;
        for (int k = 0; k < c.n_taps; k++) {
            CHK(fetch(M(h, S(h->proj_fmt, k) + ".bias"), c0, tmp, st));
            for (int i = 0; i < c0; i++) acc[i] += tmp[i];
        }
        CHK(store(A(h, "outproj.bias"), acc, st));
    }
    if (h->version == 1) { CHK(build_aux_v1(h, st)); h->aux_ready = true; return 0; }
    // neck uv columns + combined biases
    for (int l = 0; l < MOGE_LEVELS; l++) {
        const int cl = c.dims[l];
        const int cin = l == 0 ? c0 + 2 : 2;
        const float* w = M(h, S("neck.input_blocks.%d.weight", l));
        LCHK(launch_repack<float>(w + (cin - 2), A(h, S("neck.in%d.wu", l)), cl, 1, 1, 1, cin, 0, 0, 0, 1, 0, 0, st));
        LCHK(launch_repack<float>(w + (cin - 1), A(h, S("neck.in%d.wv", l)), cl, 1, 1, 1, cin, 0, 0, 0, 1, 0, 0, st));
        if (l > 0) {
            std::vector<float> a, b;
            CHK(fetch(M(h, S("neck.resamplers.%d.%s.bias", l - 1, rs_final_conv(c.neck_resamplers[l - 1]))), cl, a, st));
            CHK(fetch(M(h, S("neck.input_blocks.%d.bias", l)), cl, b, st));
            for (int i = 0; i < cl; i++) a[i] += b[i];
            CHK(store(A(h, S("neck.rs%d.bias2", l - 1)), a, st));
        }
    }
    auto stack = [&](const std::string& name) -> int {
        const bool neck = name == "neck";
        const int* rs = stack_rs(c, neck);
        for (int l = 0; l < MOGE_LEVELS - 1; l++) {
            const int co = c.dims[l + 1];
            if (rs[l] == MOGE_RS_CONV_TRANSPOSE) {
                LCHK(launch_repack<float>(M(h, name + S(".resamplers.%d.0.bias", l)), A(h, name + S(".rs%d.biasT", l)), 4, 1, 1, co, 0, 0, 0, 1, co, 0, 0, st));
                if (!neck) {
                    std::vector<float> a, b;
                    CHK(fetch(M(h, name + S(".resamplers.%d.1.bias", l)), co, a, st));
                    CHK(fetch(M(h, name + S(".input_blocks.%d.bias", l + 1)), co, b, st));
                    for (int i = 0; i < co; i++) a[i] += b[i];
                    CHK(store(A(h, name + S(".rs%d.bias_in", l)), a, st));
                }
                if (ct3_shape(c.dims[l], co)) {
                    // CT3: the ConvTranspose2d bias passes through all nine taps of the 3x3 (replicate padding: at the border too):
                    // bias_ct3 = (3x3 bias + next level's input-block bias) + sum_{m, k} W3[o][m][k] bT[m], once per phase
                    std::vector<float> w3, bt, base, b4((size_t)4 * co);
                    CHK(fetch(M(h, name + S(".resamplers.%d.1.weight", l)), (size_t)co * co * 9, w3, st));
                    CHK(fetch(M(h, name + S(".resamplers.%d.0.bias", l)), co, bt, st));
                    CHK(fetch(neck ? A(h, S("neck.rs%d.bias2", l)) : A(h, name + S(".rs%d.bias_in", l)), co, base, st));
                    for (int o = 0; o < co; o++) {
                        double a = base[o];
                        for (int m = 0; m < co; m++) {
                            double t = 0;
                            for (int k9 = 0; k9 < 9; k9++) t += w3[((size_t)o * co + m) * 9 + k9];
                            a += t * bt[m];
                        }
                        for (int q = 0; q < 4; q++) b4[(size_t)q * co + o] = (float)a;
                    }
                    CHK(store(A(h, name + S(".rs%d.bias_ct3", l)), b4, st));
                }
            } else if (rs_is_phase(rs[l])) {
                // up-sample x2 + 3x3 as a 4-phase conv: bias replicated per phase; the neck adds its next level's input-block bias (rs%d.bias2)
                const float* b4 = neck ? A(h, S("neck.rs%d.bias2", l)) : M(h, name + S(".resamplers.%d.1.bias", l));
                LCHK(launch_repack<float>(b4, A(h, name + S(".rs%d.bias4", l)), 4, 1, 1, co, 0, 0, 0, 1, co, 0, 0, st));
            } else {
                // pixel_shuffle: bias of the first conv, permuted from PixelShuffle's (co, dy, dx) channel order to (dy, dx, co)
                LCHK(launch_repack<float>(M(h, name + S(".resamplers.%d.0.bias", l)), A(h, name + S(".rs%d.bias4", l)), 4, 1, 1, co, 1, 0, 0, 4, co, 0, 0, st));
            }
        }
        return 0;
    };
    CHK(stack("neck"));
    const int ndot = c.dims[4] == 32 ? head_count(c) : 0;      // heads that have a group in the neck's fused-output-conv table: group = head_index
    for (int k = 0; k < 3; k++)
        if (c.heads & HEAD_BITS[k]) {
            CHK(stack(HEAD_NAMES[k]));
            // W2 = Wout . Win,  b2 = bout + Wout . bin   (level 4: out(x + in_4(n4)) = Wout x + W2 n4 + b2)
            const std::string name = HEAD_NAMES[k];
            const int c4 = c.dims[4], co = HEAD_COUT[k];
            std::vector<float> wout, win, bin, bout, w2((size_t)co * c4), b2(co);
            CHK(fetch(M(h, name + ".output_blocks.4.weight"), (size_t)co * c4, wout, st));
            CHK(fetch(M(h, name + ".output_blocks.4.bias"), co, bout, st));
            CHK(fetch(M(h, name + ".input_blocks.4.weight"), (size_t)c4 * c4, win, st));
            CHK(fetch(M(h, name + ".input_blocks.4.bias"), c4, bin, st));
            for (int o = 0; o < co; o++) {
                double bb = bout[o];
                for (int m = 0; m < c4; m++) bb += (double)wout[(size_t)o * c4 + m] * bin[m];
                b2[o] = (float)bb;
                for (int j = 0; j < c4; j++) {
                    double a = 0.0;
                    for (int m = 0; m < c4; m++) a += (double)wout[(size_t)o * c4 + m] * win[(size_t)m * c4 + j];
                    w2[(size_t)o * c4 + j] = (float)a;
                }
            }
            CHK(store(A(h, name + ".out4.w2"), w2, st));
            CHK(store(A(h, name + ".out4.b2"), b2, st));
            // level 4 of the fp16 path (l4c.hip): this head's W2 as group head_index of the neck's rows, its Wout on its own resampler
            if (ndot) {
                std::vector<float> rows4(4 * 32, 0.f);
                for (int o = 0; o < co; o++)
                    for (int j = 0; j < 32; j++) rows4[o * 32 + j] = w2[(size_t)o * c4 + j];
                CHK(store(A(h, "neck.dot.w2cat") + head_index(c, k) * 128, rows4, st));
                // ... and folded into the resampler's weights (l4c.hip, what `l4dot` of forward_impl runs): Wout . W4phase, Wout . bias
                if (c.dims[3] == 64 && rs_is_phase(c.head_resamplers[3]))
                    LCHK(launch_l4c_pack(M(h, name + ".resamplers.3.1.weight"), M(h, name + ".output_blocks.4.weight"), co, 1, c.head_resamplers[3] == MOGE_RS_NEAREST ? 1 : 0,
                                         M(h, name + ".resamplers.3.1.bias"), nullptr, nullptr, A(h, name + ".l4c.w"), A(h, name + ".l4c.v"), st));
            }
        }
    if (ndot > 0 && c.dims[3] == 64 && rs_is_phase(c.neck_resamplers[3]))      // the neck's resampler under every head's Wout . Win4 (bias: resampler + level-4 input block)
        LCHK(launch_l4c_pack(M(h, "neck.resamplers.3.1.weight"), A(h, "neck.dot.w2cat"), 4 * ndot, ndot, c.neck_resamplers[3] == MOGE_RS_NEAREST ? 1 : 0, A(h, "neck.rs3.bias2"),
                             A(h, "neck.in4.wu"), A(h, "neck.in4.wv"), A(h, "neck.l4c.w"), A(h, "neck.l4c.v"), st));
    // ---- composed linear chains (fp16 path, `compose` in forward_impl): the bias vectors, in double on the host (one-off, a few MB of D2H) ----
    {   // neck level 0: in0(sum_k proj_k(tap_k)) = (Win0 Wout) tapcat + (Win0 sum_k b_k + b_in0) + uv term
        std::vector<float> win, bo, bi, bc(c0);
        CHK(fetch(M(h, "neck.input_blocks.0.weight"), (size_t)c0 * (c0 + 2), win, st));
        CHK(fetch(A(h, "outproj.bias"), c0, bo, st));
        CHK(fetch(M(h, "neck.input_blocks.0.bias"), c0, bi, st));
        for (int o = 0; o < c0; o++) {
            double a = bi[o];
            for (int j = 0; j < c0; j++) a += (double)win[(size_t)o * (c0 + 2) + j] * bo[j];
            bc[o] = (float)a;
        }
        CHK(store(A(h, "neck.in0c.bias"), bc, st));
    }
    if (c.head_res_blocks[0] == 0 && c.head_resamplers[0] == MOGE_RS_CONV_TRANSPOSE)
        for (int k = 0; k < 3; k++)
            if (c.heads & HEAD_BITS[k]) {
                // head level 0 -> 1: convT(in0(n0)) = (WT Win0) n0 + (WT b_in0 + bT); torch ConvTranspose2d weight [ci][co][2][2]
                const std::string name = HEAD_NAMES[k];
                const int ci = c0, co = c.dims[1];
                std::vector<float> wt, bin, bt, bc((size_t)4 * co);
                CHK(fetch(M(h, name + ".resamplers.0.0.weight"), (size_t)ci * co * 4, wt, st));
                CHK(fetch(M(h, name + ".input_blocks.0.bias"), ci, bin, st));
                CHK(fetch(M(h, name + ".resamplers.0.0.bias"), co, bt, st));
                for (int q = 0; q < 4; q++)
                    for (int o = 0; o < co; o++) {
                        double a = bt[o];
                        for (int m = 0; m < ci; m++) a += (double)wt[((size_t)m * co + o) * 4 + q] * bin[m];
                        bc[(size_t)q * co + o] = (float)a;
                    }
                CHK(store(A(h, name + ".rs0.biasTc"), bc, st));
            }
    h->aux_ready = true;
    return 0;
}

// C[M][N] = A[M][K] * Bm[K][N], all fp32 row-major on the device, in exact fp32 (gemm.hip's v_mfma_f32_32x32x2_f32 path).  `scr` holds
// M * K + N * K floats (A made contiguous, Bm transposed: the GEMM kernels contract K-contiguous rows of both operands).
static int dev_matmul_f32(const float* Am, long lda, const float* Bm, long ldb, float* Cm, int Mr, int Nc, int Kc, float* scr, hipStream_t st) {
    float* Ac = scr;
    float* Bt = scr + (size_t)Mr * Kc;
    LCHK(launch_repack<float>(Am, Ac, Mr, 1, 1, Kc, lda, 0, 0, 1, Kc, 0, 0, st));
    LCHK(launch_repack<float>(Bm, Bt, Nc, 1, 1, Kc, 1, 0, 0, ldb, Kc, 0, 0, st));         // Bt[n][k] = Bm[k][n]
    GemmArgs g; memset(&g, 0, sizeof(g));
    g.a = Ac; g.lda = Kc; g.w = Bt; g.ldw = Kc; g.M = Mr; g.N = Nc; g.K = Kc; g.epi = EPI_STORE; g.out = Cm; g.ldc = Nc;
    LCHK(launch_gemm<float>(g, AMODE_LINEAR, st));
    return 0;
}

}  // namespace model

// CT3 weights of one ConvTranspose2d + 3x3 resampler (fp16 path): P = the 36 basic products in ONE exact-fp32 GEMM ([9 Cout][Cout] x [Cout][4 Cin]), then the
// interior blocks -> wc [4 Cout][4 Cin] and the border blocks -> dw [12][Cout][2 Cin] as signed sums of them, one rounding to fp16 each.
// w3 = Conv2d weight [co][co][3][3], wt = ConvTranspose2d weight [ci][co][2][2] (fp32, device).  Also the test entry's (test_api.hip): declared in launchers.h, outside the namespace.
int ct3_compose_device(const float* w3, const float* wt, int ci, int co, void* wc, void* dw, hipStream_t st) {
    std::vector<Ct3Slot> slots;
    model::ct3_interior_slots(slots);
    const int n_int = (int)slots.size();
    if (model::ct3_border_slots(slots) != 0) return -2;
    const size_t nA = (size_t)9 * co * co, nB = (size_t)4 * ci * co, nP = (size_t)9 * co * 4 * ci;
    float* arena = nullptr;
    if (hipMalloc(&arena, (nA + nB + nP) * sizeof(float) + slots.size() * sizeof(Ct3Slot)) != hipSuccess) return -3;
    float* A9 = arena; float* Bt = A9 + nA; float* P = Bt + nB;
    Ct3Slot* dsl = reinterpret_cast<Ct3Slot*>(P + nP);
    int rc = 0;
    hipError_t e = hipMemcpyAsync(dsl, slots.data(), slots.size() * sizeof(Ct3Slot), hipMemcpyHostToDevice, st);
    do {
        if (e != hipSuccess) { rc = (int)e; break; }
        // A9[(k, o)][m] = W3[o][m][k];  Bt[(s, i)][m] = WT[i][m][s]   (both K-contiguous rows: what the GEMM kernels contract)
        if ((rc = launch_repack<float>(w3, A9, 9, co, 1, co, 1, (long)co * 9, 0, 9, (long)co * co, co, 0, st))) break;
        if ((rc = launch_repack<float>(wt, Bt, 4, ci, 1, co, 1, (long)co * 4, 0, 4, (long)ci * co, co, 0, st))) break;
        GemmArgs g; memset(&g, 0, sizeof(g));
        g.a = A9; g.lda = co; g.w = Bt; g.ldw = co; g.M = 9 * co; g.N = 4 * ci; g.K = co; g.epi = EPI_STORE; g.out = P; g.ldc = 4 * ci;
        if ((rc = launch_gemm<float>(g, AMODE_LINEAR, st))) break;
        if ((rc = launch_ct3_combine(P, dsl, n_int, co, ci, wc, 4 * ci, st))) break;
        if ((rc = launch_ct3_combine(P, dsl + n_int, (int)slots.size() - n_int, co, ci, dw, 2 * ci, st))) break;
    } while (0);
    hipError_t e2 = hipStreamSynchronize(st);      // (the host-side term table must outlive its copy; pack time, not the hot path)
    hipFree(arena);
    if (rc) return rc;
    return e2 == hipSuccess ? 0 : (int)e2;
}

namespace model __attribute__((visibility("hidden"))) {

static int compose_ct3_f16(moge_handle* h, const std::string& name, int l, int ci, int co, hipStream_t st) {
    const int rc = ct3_compose_device(M(h, name + S(".resamplers.%d.1.weight", l)), M(h, name + S(".resamplers.%d.0.weight", l)), ci, co,
                                      Pm<f16>(h, name + S(".rs%d.wc", l)), Pm<f16>(h, name + S(".rs%d.dw", l)), st);
    if (rc) return moge_internal_fail(rc < 0 ? MOGE_ERR_INVALID : MOGE_ERR_HIP, "composing the ConvTranspose2d + 3x3 weights of %s level %d failed (%d)", name.c_str(), l, rc);
    return 0;
}

// Composed linear chains of the fp16 path (`compose` / `compose0` in forward_impl): products formed in fp32 from the master weights, ONE rounding to fp16.
static int compose_weights_f16(moge_handle* h, hipStream_t st) {
    const moge_config& c = h->cfg;
    const int D = c.embed_dim, c0 = c.dims[0], K4 = c.n_taps * D, co = c.dims[1];
    const size_t nscr = (size_t)c0 * c0 + (size_t)K4 * c0 + (size_t)4 * co * c0 + (size_t)c0 * c0;
    const size_t ntmp = (size_t)c0 * K4 > (size_t)4 * co * c0 ? (size_t)c0 * K4 : (size_t)4 * co * c0;
    // one temporary arena (freed on every path below): scr | tmp | wcat | wT
    float* arena = nullptr;
    HIPCHK(hipMalloc(&arena, (nscr + ntmp + (size_t)c0 * K4 + (size_t)4 * co * c0) * 4));
    float* scr = arena;
    float* tmp = scr + nscr;
    float* wcat = tmp + ntmp;
    float* wT = wcat + (size_t)c0 * K4;
    int rc = 0;
    do {
        // Wout_cat [c0][n_taps * D] (fp32), then (Win0[:, :c0]) . Wout_cat
        for (int k = 0; k < c.n_taps && !rc; k++)
            rc = launch_repack<float>(M(h, S(h->proj_fmt, k) + ".weight"), wcat + (size_t)k * D, c0, 1, 1, D, D, 0, 0, 1, K4, 0, 0, st);
        if (rc) break;
        if ((rc = dev_matmul_f32(M(h, "neck.input_blocks.0.weight"), c0 + 2, wcat, K4, tmp, c0, K4, c0, scr, st))) break;
        if ((rc = launch_convert<float, f16>(tmp, Pm<f16>(h, "neck.in0c.w"), (long)c0 * K4, st))) break;
        if (c.head_res_blocks[0] == 0 && c.head_resamplers[0] == MOGE_RS_CONV_TRANSPOSE)
            for (int k = 0; k < 3 && !rc; k++)
                if (c.heads & HEAD_BITS[k]) {
                    const std::string name = HEAD_NAMES[k];
                    // WT [(dy*2+dx)*co + o][ci] (fp32) . Win0_head [ci][ci]
                    rc = launch_repack<float>(M(h, name + ".resamplers.0.0.weight"), wT, 4, co, 1, c0, 1, 4, 0, (long)co * 4, (long)co * c0, c0, 0, st);
                    if (!rc) rc = dev_matmul_f32(wT, c0, M(h, name + ".input_blocks.0.weight"), c0, tmp, 4 * co, c0, c0, scr, st);
                    if (!rc) rc = launch_convert<float, f16>(tmp, Pm<f16>(h, name + ".rs0.wTc"), (long)4 * co * c0, st);
                }
    } while (0);
    hipError_t e = hipStreamSynchronize(st);
    hipFree(arena);
    if (rc) return moge_internal_fail(rc < 0 ? MOGE_ERR_INVALID : MOGE_ERR_HIP, "composing the level-0 linear chains failed (%d)", rc);
    HIPCHK(e);
    return 0;
}

template <typename T>
static int pack_weights_v1(moge_handle* h, hipStream_t st) {
    const moge_v1_config& c = h->cfg1;
    auto conv3 = [&](const float* w, T* dst, int co, int ci, int cip) -> int {        // torch [co][ci][3][3] -> [co][tap * cip + ci], cip >= ci zero padded
        return launch_repack<T>(w, dst, co, 9, 1, ci, (long)ci * 9, 1, 0, 9, (long)9 * cip, cip, 0, st);
    };
    for (int i = 0; i < c.n_up; i++) {
        const int ci = i == 0 ? c.dim_proj : c.dim_upsample[i - 1], co = c.dim_upsample[i];
        const std::string u = S("head.upsample_blocks.%d.", i);
        // ConvTranspose2d weight [ci + 2][co][2][2] -> [(dy*2+dx)*co + o][ci] (the two uv input rows go to the epilogue: build_aux_v1)
        LCHK(launch_repack<T>(M(h, u + "0.0.weight"), Pm<T>(h, S("v1.up%d.wT", i)), 4, co, 1, ci, 1, 4, 0, (long)co * 4, (long)co * ci, ci, 0, st));
        LCHK(conv3(M(h, u + "0.1.weight"), Pm<T>(h, S("v1.up%d.w3", i)), co, co, co));
        for (int j = 0; j < c.num_res_blocks; j++) {
            const std::string r = u + S("%d.layers.", 1 + j);
            const int ch = co * v1_mult(c);
            LCHK(conv3(M(h, r + "2.weight"), Pm<T>(h, S("v1.up%d.res%d.w1", i, j)), ch, co, co));
            LCHK(conv3(M(h, r + "5.weight"), Pm<T>(h, S("v1.up%d.res%d.w2", i, j)), co, ch, ch));
        }
    }
    const int cl = c.dim_upsample[c.n_up - 1], c4 = c.last_conv_channels, cp = v1_cpad(cl), ch4 = c4 * v1_mult(c);
    for (int o = 0; o < 2; o++) {
        LCHK(conv3(M(h, S("head.output_block.%d.0.weight", o)), Pm<T>(h, "v1.out.w3") + (size_t)o * c4 * 9 * cp, c4, cl + 2, cp));
        for (int j = 0; j < c.last_res_blocks; j++) {
            const std::string r = S("head.output_block.%d.%d.layers.", o, 1 + j);
            LCHK(conv3(M(h, r + "2.weight"), Pm<T>(h, S("v1.out%d.res%d.w1", o, j)), ch4, c4, c4));
            LCHK(conv3(M(h, r + "5.weight"), Pm<T>(h, S("v1.out%d.res%d.w2", o, j)), c4, ch4, ch4));
        }
    }
    return 0;
}

template <typename T>
static int pack_weights(moge_handle* h, hipStream_t st) {
    const int pr = TT<T>::PREC;
    if (h->pk_ready[pr]) return 0;
    const moge_config& c = h->cfg;
    const int D = c.embed_dim, c0 = c.dims[0];
    if (!h->packed[pr]) HIPCHK(hipMalloc(&h->packed[pr], h->pk_elems * sizeof(T)));
    HIPCHK(hipMemsetAsync(h->packed[pr], 0, h->pk_elems * sizeof(T), st));
    const std::string bb = h->bb;
    // patch embed [D][588] -> [D][640]
    LCHK(launch_repack<T>(M(h, bb + "patch_embed.proj.weight"), Pm<T>(h, "patch.w"), D, 1, 1, KPATCH, KPATCH, 0, 0, 1, KPATCH_PAD, 0, 0, st));
    for (int i = 0; i < c.depth; i++) {
        const std::string p = bb + S("blocks.%d.", i);
        LCHK((launch_convert<float, T>(M(h, p + "attn.proj.weight"), Pm<T>(h, S("blk%d.proj", i)), (long)D * D, st)));
        LCHK((launch_convert<float, T>(M(h, p + "mlp.fc2.weight"), Pm<T>(h, S("blk%d.fc2", i)), (long)4 * D * D, st)));
        if constexpr (!std::is_same<T, f16>::value) {
            LCHK((launch_convert<float, T>(M(h, p + "attn.qkv.weight"), Pm<T>(h, S("blk%d.qkv", i)), (long)3 * D * D, st)));
            LCHK((launch_convert<float, T>(M(h, p + "mlp.fc1.weight"), Pm<T>(h, S("blk%d.fc1", i)), (long)4 * D * D, st)));
        } else {                    // encode<f16> reads the LN-folded forms only
            LCHK(launch_fold_ln<f16>(M(h, p + "attn.qkv.weight"), M(h, p + "norm1.weight"), M(h, p + "norm1.bias"), M(h, p + "attn.qkv.bias"),
                                     Pm<T>(h, S("blk%d.qkvf", i)), A(h, S("blk%d.qkv.c", i)), A(h, S("blk%d.qkv.bf", i)), 3 * D, D, st));
            LCHK(launch_fold_ln<f16>(M(h, p + "mlp.fc1.weight"), M(h, p + "norm2.weight"), M(h, p + "norm2.bias"), M(h, p + "mlp.fc1.bias"),
                                     Pm<T>(h, S("blk%d.fc1f", i)), A(h, S("blk%d.fc1.c", i)), A(h, S("blk%d.fc1.bf", i)), 4 * D, D, st));
        }
    }
    // output projections: [c0][D] x n_taps -> [c0][n_taps*D]
    for (int k = 0; k < c.n_taps; k++)
        LCHK(launch_repack<T>(M(h, S(h->proj_fmt, k) + ".weight"), Pm<T>(h, "outproj.w") + (size_t)k * D, c0, 1, 1, D, D, 0, 0, 1,
                              (long)c.n_taps * D, 0, 0, st));
    if (h->version == 1) { CHK(pack_weights_v1<T>(h, st)); h->pk_ready[pr] = true; return 0; }
    // neck.in0: [c0][c0+2] -> [c0][c0]
    LCHK(launch_repack<T>(M(h, "neck.input_blocks.0.weight"), Pm<T>(h, "neck.in0.w"), c0, 1, 1, c0, c0 + 2, 0, 0, 1, c0, 0, 0, st));
    auto conv3 = [&](const float* w, T* dst, int co, int ci) -> int {
        // torch [co][ci][3][3] -> [co][tap*ci + ci]
        return launch_repack<T>(w, dst, co, 9, 1, ci, (long)ci * 9, 1, 0, 9, (long)9 * ci, ci, 0, st);
    };
    auto stack = [&](const std::string& name, bool neck, const int* nres) -> int {
        for (int l = 0; l < MOGE_LEVELS; l++)
            if (!neck) LCHK((launch_convert<float, T>(M(h, name + S(".input_blocks.%d.weight", l)), Pm<T>(h, name + S(".in%d.w", l)), (long)c.dims[l] * c.dims[l], st)));
        const int* rs = stack_rs(c, neck);
        for (int l = 0; l < MOGE_LEVELS - 1; l++) {
            const int ci = c.dims[l], co = c.dims[l + 1];
            if (rs[l] == MOGE_RS_CONV_TRANSPOSE) {
                // ConvTranspose2d weight [ci][co][2][2] -> [(dy*2+dx)*co + o][ci]
                LCHK(launch_repack<T>(M(h, name + S(".resamplers.%d.0.weight", l)), Pm<T>(h, name + S(".rs%d.wT", l)), 4, co, 1, ci, 1, 4, 0, (long)co * 4,
                                      (long)co * ci, ci, 0, st));
                LCHK(conv3(M(h, name + S(".resamplers.%d.1.weight", l)), Pm<T>(h, name + S(".rs%d.w3", l)), co, co));
            } else if (rs_is_phase(rs[l])) {
                LCHK(launch_pack_phase_conv<T>(M(h, name + S(".resamplers.%d.1.weight", l)), Pm<T>(h, name + S(".rs%d.w3p", l)), co, ci, st, rs[l] == MOGE_RS_NEAREST ? 1 : 0));
            } else {
                // pixel_shuffle: Conv2d weight [(o*4 + q)][ci][3][3] -> [(q*co + o)][tap*ci + c]   (q = dy*2 + dx of nn.PixelShuffle(2))
                LCHK(launch_repack<T>(M(h, name + S(".resamplers.%d.0.weight", l)), Pm<T>(h, name + S(".rs%d.w3p", l)), 4, co, 9, ci, (long)ci * 9, (long)4 * ci * 9, 1, 9,
                                      (long)co * 9 * ci, (long)9 * ci, ci, st));
                LCHK(conv3(M(h, name + S(".resamplers.%d.2.weight", l)), Pm<T>(h, name + S(".rs%d.w3", l)), co, co));
            }
        }
        for (int l = 0; l < MOGE_LEVELS; l++)
            for (int j = 0; j < nres[l]; j++) {
                const int ch = c.dims[l] * stack_mult(c, neck);
                LCHK(conv3(M(h, name + S(".res_blocks.%d.%d.layers.2.weight", l, j)), Pm<T>(h, name + S(".res%d.%d.w1", l, j)), ch, c.dims[l]));
                LCHK(conv3(M(h, name + S(".res_blocks.%d.%d.layers.5.weight", l, j)), Pm<T>(h, name + S(".res%d.%d.w2", l, j)), c.dims[l], ch));
            }
        return 0;
    };
    CHK(stack("neck", true, c.neck_res_blocks));
    for (int k = 0; k < 3; k++)
        if (c.heads & HEAD_BITS[k]) CHK(stack(HEAD_NAMES[k], false, c.head_res_blocks));
    if constexpr (std::is_same<T, f16>::value) {
        CHK(compose_weights_f16(h, st));
        for (int kk = -1; kk < 3; kk++) {                                 // neck, then the heads
            if (kk >= 0 && !(c.heads & HEAD_BITS[kk])) continue;
            const std::string name = kk < 0 ? "neck" : HEAD_NAMES[kk];
            const int* rs = stack_rs(c, kk < 0);
            for (int l = 0; l < MOGE_LEVELS - 1; l++)
                if (rs[l] == MOGE_RS_CONV_TRANSPOSE && ct3_shape(c.dims[l], c.dims[l + 1])) CHK(compose_ct3_f16(h, name, l, c.dims[l], c.dims[l + 1], st));
        }
    }
    h->pk_ready[pr] = true;
    return 0;
}

int pack_weights(moge_handle* h, int prec, hipStream_t st) { return prec == MOGE_FP16 ? pack_weights<f16>(h, st) : pack_weights<float>(h, st); }

}  // namespace model
