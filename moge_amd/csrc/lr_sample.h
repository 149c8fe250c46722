// The low-resolution sampling convention shared by csrc/metrics.hip (moge_metrics_lr_sample) and csrc/losses.hip (moge_loss_lr_sample,
// moge_loss_patch_lr_sample): utils3d.pt.masked_nearest_resize(mask=..., size=(OH, OW), return_index=True).  utils3d is not vendored, so this is an
// UNPINNED convention, restated in DESIGN.md section 10 and in tools/make_metrics_golden.py:
//   filter fh = max(1, H / OH), fw = max(1, W / OW); target centre ((j + 0.5) W / OW, (i + 0.5) H / OH); integer window ceil(fh) x ceil(fw)
//   with top-left rint(centre - (fw / 2, fh / 2)) (half to even), clipped to the image; index = the valid pixel whose centre (x + 0.5, y + 0.5)
//   is nearest the target centre, first in row-major window order on a tie.  A window without a valid pixel reports its nearest in-image
//   pixel (its value is never read through the mask).  Arithmetic in float64.
#pragma once
#include "common.h"

// cell o of the (OH, OW) grid over an (H, W) map whose valid pixels `valid(y, x)` names -> true if the window holds one; (oy, ox) = the sample
template <typename Valid>
__device__ __forceinline__ bool lr_sample_cell(int H, int W, int OH, int OW, int o, Valid valid, int& oy, int& ox) {
    const int i = o / OW, j = o - i * OW;
    const double fh = fmax(1.0, (double)H / OH), fw = fmax(1.0, (double)W / OW);
    const double cy = (i + 0.5) * H / OH, cx = (j + 0.5) * W / OW;
    const int wh = (int)ceil(fh), ww = (int)ceil(fw);
    const int y0 = (int)rint(cy - fh / 2), x0 = (int)rint(cx - fw / 2);
    double best_v = 1e300, best_a = 1e300;
    int by = -1, bx = -1, ay = min(max(y0, 0), H - 1), ax = min(max(x0, 0), W - 1);
    for (int dy = 0; dy < wh; dy++) {
        const int y = y0 + dy;
        if (y < 0 || y >= H) continue;
        const double ey = y + 0.5 - cy;
        for (int dx = 0; dx < ww; dx++) {
            const int x = x0 + dx;
            if (x < 0 || x >= W) continue;
            const double ex = x + 0.5 - cx, d = ey * ey + ex * ex;
            if (d < best_a) { best_a = d; ay = y; ax = x; }
            if (d < best_v && valid(y, x)) { best_v = d; by = y; bx = x; }
        }
    }
    oy = by >= 0 ? by : ay;
    ox = by >= 0 ? bx : ax;
    return by >= 0;
}
