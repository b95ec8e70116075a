// Homography warp (include/sift_hip.h, "homography warp"): THE DEFINITION.  The HIP kernel (kernels_warp.hip) and the host loop
// (hostmath_capi.cpp: hostmath_warp_homography) both compile this header, with -ffp-contract=off; every fused operation is an
// explicit fmaf, every other operation is one float rounding.  An extension: the reference has no counterpart.
//
// The model maps query to train, (tx, ty, 1) ~ H (qx, qy, 1), as everywhere else (ransac_math.h): warping the TRAIN image into
// the QUERY frame evaluates H as it comes on the query frame's pixel lattice, with no inverse.  Output pixel (x, y) of a job:
//   lattice    qx = (float)(x + origin_x), qy = (float)(y + origin_y): exact, the caller keeps |x + origin_x| < 2^24
//   map        X, Y, W: the predicate's own fmaf chains (ransac_inlier_query), u = X / W, v = Y / W - the correctly rounded quotients
//   covered    W > 0, W < +inf, 0 <= u <= (float)(w - 1), 0 <= v <= (float)(h - 1); a NaN anywhere fails one of the compares
//   uncovered  value `fill`, mask 0.  The all-zero model (iteration -1) has W = 0: every pixel is `fill`
//   bilinear   x0 = (int)floorf(u), fx = u - (float)x0, x1 = min(x0 + 1, w - 1), rows likewise;
//              top = fmaf(fx, p01 - p00, p00), bot = fmaf(fx, p11 - p10, p10), out = fmaf(fy, bot - top, top)
//   nearest    the pixel at ((int)floorf(u + 0.5f), (int)floorf(v + 0.5f))
// The value depends on (src, h, x, y, parameters) alone: not on tiles, paths or the launch.
#pragma once
#include <stdint.h>

#include "ransac_math.h"

namespace sift_hip {

// Image sizes the warp takes: (float)(w - 1) + 0.5f must not round up to w, or nearest would leave the image.
constexpr int kWarpMaxSide = 1 << 22;

struct WarpTaps {
    int x0, y0, x1, y1;   // nearest: x1 = x0, y1 = y0 (only (x0, y0) is read)
    float fx, fy;
};

// (u, v) of the lattice point (qx, qy); is the pixel covered by a w x h source?
SIFT_HD bool warp_coords(const float (&h)[9], float qx, float qy, int w, int hgt, float& u, float& v, float& W) {
    float p[4];
    ransac_inlier_query(h, qx, qy, 0.0f, p);   // X, Y, W as the predicate forms them
    W = p[2];
    u = p[0] / W;
    v = p[1] / W;
    return (W > 0.0f) & (W < __builtin_inff()) & (u >= 0.0f) & (u <= (float)(w - 1)) & (v >= 0.0f) & (v <= (float)(hgt - 1));
}

// the taps of a COVERED pixel: every index lies inside the image
SIFT_HD WarpTaps warp_taps(float u, float v, int w, int hgt, int interp) {
    WarpTaps t;
    if (interp == 0) {
        t.x0 = t.x1 = (int)__builtin_floorf(u + 0.5f);
        t.y0 = t.y1 = (int)__builtin_floorf(v + 0.5f);
        t.fx = t.fy = 0.0f;
    } else {
        t.x0 = (int)__builtin_floorf(u);
        t.y0 = (int)__builtin_floorf(v);
        t.fx = u - (float)t.x0;
        t.fy = v - (float)t.y0;
        t.x1 = t.x0 + 1 < w - 1 ? t.x0 + 1 : w - 1;
        t.y1 = t.y0 + 1 < hgt - 1 ? t.y0 + 1 : hgt - 1;
    }
    return t;
}

// px(x, y): the source pixel.  Whoever calls decides where it is read from; the arithmetic is here.
template <class Fetch>
SIFT_HD float warp_value(const Fetch& px, const WarpTaps& t, int interp) {
    if (interp == 0) return px(t.x0, t.y0);
    const float p00 = px(t.x0, t.y0), p01 = px(t.x1, t.y0), p10 = px(t.x0, t.y1), p11 = px(t.x1, t.y1);
    const float top = __builtin_fmaf(t.fx, p01 - p00, p00);
    const float bot = __builtin_fmaf(t.fx, p11 - p10, p10);
    return __builtin_fmaf(t.fy, bot - top, top);
}

// one output pixel from the definition
SIFT_HD float warp_pixel(const float* src, int w, int hgt, const float (&h)[9], int x, int y, int origin_x, int origin_y, float fill, int interp,
                         uint8_t& covered) {
    float u, v, W;
    const bool in = warp_coords(h, (float)(x + origin_x), (float)(y + origin_y), w, hgt, u, v, W);
    covered = in ? 1 : 0;
    if (!in) return fill;
    const WarpTaps t = warp_taps(u, v, w, hgt, interp);
    return warp_value([&](int a, int b) { return src[(size_t)b * (size_t)w + (size_t)a]; }, t, interp);
}

}  // namespace sift_hip
