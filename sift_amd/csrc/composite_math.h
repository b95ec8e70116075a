// Compositor (include/sift_hip.h, "compositor"): THE DEFINITION.  n source images under n models accumulated into one canvas.
// The HIP kernel (kernels_composite.hip) and the host loop (hostmath_capi.cpp: hostmath_composite_homography) both compile this
// header, with -ffp-contract=off; every fused operation is an explicit fmaf, every other operation is one float rounding.  It is
// built on warp_math.h: the map, the coverage test, the taps and the interpolation are warp_coords, warp_taps and warp_value as
// they are.  An extension: the reference has no counterpart.
//
// Canvas c owns the jobs j = offsets[c] .. offsets[c + 1] - 1, taken IN THAT ORDER.  For canvas pixel (x, y):
//   start      acc = +0.0f, wsum = +0.0f, cnt = 0
//   per job    covered, u, v = warp_coords(models[j], (float)(x + origin_x), (float)(y + origin_y), w, h); not covered: the job is
//              skipped; covered: val = warp_value(taps), cnt += 1 (in every blend mode) and
//     blend 0 (first)    the first covering job's val is kept; later jobs only count
//     blend 1 (mean)     acc = acc + val
//     blend 2 (feather)  wgt = fminf(fminf(u, (float)(w - 1) - u), fminf(v, (float)(h - 1) - v)) + 1.0f - the distance to the
//                        source frame's border plus one, >= 1 for a covered pixel, the same u, v for both interp values -,
//                        acc = fmaf(wgt, val, acc), wsum = wsum + wgt
//   result     cnt == 0: fill; first: the kept val; mean: acc / (float)cnt; feather: acc / wsum (correctly rounded quotients)
// With gains (sift_hip_composite_homography_gains; the overlap statistics solve them, overlap_math.h) a covering job's value is
// val = gains[j] * val, one float rounding, wherever its value is wanted at all; without, nothing changes.
// The value depends on the inputs alone: not on tiles, paths, culling or the launch.
#pragma once
#include <stdint.h>

#include "warp_math.h"

namespace sift_hip {

constexpr int kCompositeMaxJobs = 65535;   // per canvas: the count is a uint16

struct CompositeAcc {   // starts as {+0.0f, +0.0f, 0}: a plain aggregate, no constructor to call
    float acc, wsum;
    uint32_t cnt;
};

// u, v of a COVERED pixel: no NaN, so fminf is exact; a tie of -0 and +0 vanishes in the + 1.0f
SIFT_HD float composite_weight(float u, float v, int w, int hgt) {
    return __builtin_fminf(__builtin_fminf(u, (float)(w - 1) - u), __builtin_fminf(v, (float)(hgt - 1) - v)) + 1.0f;
}

// does a covering job need its value at all?  (first: only while nothing is kept)
SIFT_HD bool composite_wants_value(const CompositeAcc& a, int blend) { return blend != 0 || a.cnt == 0; }

// one covering job; val is ignored where composite_wants_value says no
SIFT_HD void composite_add(CompositeAcc& a, float val, float wgt, int blend) {
    if (blend == 0) {
        if (a.cnt == 0) a.acc = val;
    } else if (blend == 1) {
        a.acc = a.acc + val;
    } else {
        a.acc = __builtin_fmaf(wgt, val, a.acc);
        a.wsum = a.wsum + wgt;
    }
    a.cnt += 1;
}

SIFT_HD float composite_result(const CompositeAcc& a, float fill, int blend) {
    if (a.cnt == 0) return fill;
    if (blend == 0) return a.acc;
    return blend == 1 ? a.acc / (float)a.cnt : a.acc / a.wsum;
}

// one canvas pixel from the definition: jobs j0 .. j1 - 1 in order
SIFT_HD float composite_pixel(const float* imgs, int w, int hgt, const int32_t* src, const float* models, long long j0, long long j1, int x, int y, int origin_x,
                              int origin_y, float fill, int interp, int blend, uint16_t& count, const float* gains = nullptr) {
    CompositeAcc a = {0.0f, 0.0f, 0u};
    const float qx = (float)(x + origin_x), qy = (float)(y + origin_y);
    for (long long j = j0; j < j1; ++j) {
        float m[9], u, v, W;
        for (int k = 0; k < 9; ++k) m[k] = models[9 * (size_t)j + k];
        if (!warp_coords(m, qx, qy, w, hgt, u, v, W)) continue;
        float val = 0.0f;
        if (composite_wants_value(a, blend)) {
            const float* s = imgs + (size_t)(src ? src[j] : j) * (size_t)w * (size_t)hgt;
            const WarpTaps t = warp_taps(u, v, w, hgt, interp);
            val = warp_value([&](int px, int py) { return s[(size_t)py * (size_t)w + (size_t)px]; }, t, interp);
            if (gains) val = gains[j] * val;
        }
        composite_add(a, val, blend == 2 ? composite_weight(u, v, w, hgt) : 0.0f, blend);
    }
    count = (uint16_t)a.cnt;
    return composite_result(a, fill, blend);
}

}  // namespace sift_hip
