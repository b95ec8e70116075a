// Two-band compositor (include/sift_hip.h, "two-band compositor"): THE DEFINITION.  Burt and Adelson's (1983) multiresolution blend
// with K = 2 bands, as Brown and Lowe (2007, section 7) use it after gain compensation: a frame's low band is blended over the
// whole overlap, its high band is taken from ONE frame, so fine detail is not doubled where registration is a few pixels off.
// The HIP kernel (kernels_twoband.hip) and the host loop (hostmath_capi.cpp: hostmath_composite_twoband) both compile this header,
// with -ffp-contract=off; every fused operation is an explicit fmaf, every other operation is one float rounding.  It stands on
// warp_math.h and composite_math.h as they are: warp_coords, warp_taps, warp_value, composite_weight.  An extension: the reference
// has no counterpart.
//
// Canvases, jobs, offsets, src, models, origin, fill, interp, gains and count are the compositor's.  New: the radius R (0 .. 16)
// and R + 1 taps k[0 .. R], k[d] being the weight at offsets +d and -d; all finite and >= 0, k[0] >= 2^-12.
// For job j and ANY lattice point q = (X, Y), inside the canvas or not:
//   c_j(q)   the warp's coverage test
//   t_j(q)   the warp's value (times gains[j], one rounding, with gains) where covered, else +0.0f
//   m_j(q)   1.0f where covered, else 0.0f
//   row      rs_j(X, Y) = the chain acc = +0.0f; for dx = -R .. R ascending: acc = fmaf(k[|dx|], t_j(X + dx, Y), acc);
//            rn_j the same chain over m_j
//   column   ls_j(X, Y) = the same chain over dy on rs_j(X, Y + dy); ln_j the same chain over rn_j
//   bands    where c_j(q): L = ls / ln (correctly rounded; ln >= k[0]^2 > 0 there), H = t - L (one rounding).  The low band is
//            normalised by the coverage it saw: no dark rim forms at a frame's border
// Canvas pixel (x, y) is q = (x + origin_x, y + origin_y); over its covering jobs IN ORDER, from lacc = wsum = +0.0f, cnt = 0:
//   wgt = composite_weight(u, v, w, h); lacc = fmaf(wgt, L, lacc); wsum = wsum + wgt; cnt += 1;
//   the first covering job, or wgt > best (strict: the earlier job wins a tie): best = wgt, high = H
//   result   cnt == 0: fill; else lacc / wsum + high (a correctly rounded quotient, then one add)
// The low band is blended with the feather weights themselves, not with Brown and Lowe's blurred arg-max masks: the usual
// two-band simplification, one pass over the jobs instead of two.
// Consequences, bit for bit: a lattice point's value depends on the inputs alone - not on the canvas's size or origin, tiles,
// paths or culling - so a cropped canvas IS the crop of the larger one; and where a job covers every lattice point of a window,
// ln is ONE number that depends on the taps alone (twoband_full_norm), which a fast path may form once.
#pragma once
#include <stdint.h>

#include "composite_math.h"

namespace sift_hip {

constexpr int kTwobandMaxRadius = 16;
constexpr float kTwobandMinCentre = 1.0f / 4096.0f;   // k[0] >= 2^-12: ln >= 2^-24 where the job covers the pixel

struct TwobandAcc {   // starts as {+0.0f, +0.0f, +0.0f, +0.0f, 0}
    float lacc, wsum, best, high;
    uint32_t cnt;
};

SIFT_HD bool twoband_taps_ok(const float* k, int radius) {
    if (radius < 0 || radius > kTwobandMaxRadius || !(k[0] >= kTwobandMinCentre)) return false;
    for (int d = 0; d <= radius; ++d)
        if (!(k[d] >= 0.0f && k[d] < __builtin_inff())) return false;
    return true;
}

// the chain of one pass: at(d) is the pass's input at offset d
template <class At>
SIFT_HD float twoband_chain(const float* k, int radius, const At& at) {
    float acc = 0.0f;
    for (int d = -radius; d <= radius; ++d) acc = __builtin_fmaf(k[d < 0 ? -d : d], at(d), acc);
    return acc;
}

// ln where the job covers the whole (2R + 1)^2 window: the two chains over m = 1
SIFT_HD float twoband_full_norm(const float* k, int radius) {
    const float rn = twoband_chain(k, radius, [](int) { return 1.0f; });
    return twoband_chain(k, radius, [rn](int) { return rn; });
}

// c, t and the feather weight of job (s, m, gain) at the lattice point (qx, qy); gain null: none
SIFT_HD bool twoband_sample(const float* s, int w, int hgt, const float (&m)[9], float qx, float qy, int interp, const float* gain, float& t, float& wgt) {
    float u, v, W;
    t = 0.0f;
    wgt = 0.0f;
    if (!warp_coords(m, qx, qy, w, hgt, u, v, W)) return false;
    const WarpTaps taps = warp_taps(u, v, w, hgt, interp);
    t = warp_value([&](int px, int py) { return s[(size_t)py * (size_t)w + (size_t)px]; }, taps, interp);
    if (gain) t = *gain * t;
    wgt = composite_weight(u, v, w, hgt);
    return true;
}

// one covering job of a canvas pixel: its value, its two column sums and its weight
SIFT_HD void twoband_add(TwobandAcc& a, float wgt, float t, float ls, float ln) {
    const float low = ls / ln;
    const float high = t - low;
    a.lacc = __builtin_fmaf(wgt, low, a.lacc);
    a.wsum = a.wsum + wgt;
    if (a.cnt == 0 || wgt > a.best) {
        a.best = wgt;
        a.high = high;
    }
    a.cnt += 1;
}

SIFT_HD float twoband_result(const TwobandAcc& a, float fill) { return a.cnt == 0 ? fill : a.lacc / a.wsum + a.high; }

}  // namespace sift_hip
