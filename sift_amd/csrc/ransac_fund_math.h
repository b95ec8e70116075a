// RANSAC fundamental matrix over match lists (include/sift_hip.h, "epipolar verification"): THE DEFINITION.  The HIP kernels
// (kernels_ransac_fund.hip) and the host checker (hostmath_capi.cpp) both compile this header, with -ffp-contract=off; every
// fused operation is written as an explicit fma / fmaf, every division is a plain correctly rounded `/`, every other product and
// sum is one rounding.  No square root and no libm call appears anywhere (ransac_refine_math.h avoids them for the same reason:
// the device's and the host's need not round alike).  An extension: the reference has no counterpart.
//
// A correspondence is four floats (qx, qy, tx, ty); the model is F with (tx, ty, 1) F (qx, qy, 1)^T = 0, F row-major - the same
// query-to-train convention as the homography of ransac_math.h.
//   sampling   ransac_draw7: seven distinct rows of a set from the counter-based hash of ransac_math.h; its first four indices
//              are ransac_draw's
//   solve      ransac_fundamental7: the seven-point model in double, straight-line code - Gauss-Jordan with complete pivoting
//              for the two null vectors, the cubic det(l n1 + n2) = 0, its real roots by bracketed bisection; up to three models
//   predicate  ransac_fund_inlier: the Sampson distance, float, division-free
//   selection  hypothesis SLOT 3 * iteration + k is root k of sample `iteration`; the score of a slot = its inlier count over
//              ALL rows of its set, -1 when the slot is invalid; the winner is the highest score, the lowest slot among equals;
//              none (iteration -1, root -1, inliers 0, f all +0.0f, every flag 0) when no slot is valid or the set has fewer
//              than seven rows.  The flags are the predicate under the winner.
// Scores are integers: the result cannot depend on how rows or slots are tiled, split over workgroups or reduced.
// Every dynamic row / column choice is a chain of selects over compile-time indices, so that on the GPU the 7 x 9 doubles stay
// in registers.  There is no least-squares refit of F, no oriented-epipolar test and no adaptive early stop.
#pragma once
#include <stdint.h>

#include "ransac_math.h"

namespace sift_hip {

// Seven distinct indices in [0, m), m >= 7, of sample `iteration` of set `set`: ransac_draw's key and base, draw k = 0 .. 6 takes
// (uint64(hash(base + k * 0x9e3779b9)) * (m - k)) >> 32 and steps over the k indices already drawn, in ascending order.  For
// m == 7 every draw is a permutation of 0 .. 6.
SIFT_HD void ransac_draw7(uint32_t seed, uint32_t set, uint32_t iteration, uint32_t m, uint32_t (&idx)[7]) {
    const uint32_t key = ransac_hash(ransac_hash(seed ^ 0x9e3779b9u) + set * 0x85ebca6bu);
    const uint32_t base = ransac_hash(key ^ (iteration * 0xc2b2ae35u + 0x27d4eb2fu));
    uint32_t s[7] = {0, 0, 0, 0, 0, 0, 0};   // the indices drawn so far, ascending
#pragma unroll
    for (int k = 0; k < 7; ++k) {
        uint32_t v = (uint32_t)(((uint64_t)ransac_hash(base + (uint32_t)k * 0x9e3779b9u) * (uint64_t)(m - (uint32_t)k)) >> 32);
#pragma unroll
        for (int j = 0; j < k; ++j) v += v >= s[j] ? 1u : 0u;
        idx[k] = v;
        uint32_t cur = v;   // insert: s[0 .. k - 1] ascending -> s[0 .. k] ascending
#pragma unroll
        for (int j = 0; j < k; ++j) {
            const uint32_t lo = cur < s[j] ? cur : s[j], hi = cur < s[j] ? s[j] : cur;
            s[j] = lo;
            cur = hi;
        }
        s[k] = cur;
    }
}

namespace fund_detail {
SIFT_HD bool finite(double v) { return v - v == 0.0; }
// the determinant of the rows (a0 a1 a2), (b0 b1 b2), (c0 c1 c2): cofactors along the first row
SIFT_HD double det3r(double a0, double a1, double a2, double b0, double b1, double b2, double c0, double c1, double c2) {
    const double m0 = __builtin_fma(b1, c2, -(b2 * c1));
    const double m1 = __builtin_fma(b2, c0, -(b0 * c2));
    const double m2 = __builtin_fma(b0, c1, -(b1 * c0));
    return __builtin_fma(a0, m0, __builtin_fma(a1, m1, a2 * m2));
}
// det of the matrix whose row r is row r of x when bit r of `from_y` is 0, of y otherwise (x, y: 3 x 3 row-major)
template <int from_y>
SIFT_HD double det_mixed(const double (&x)[9], const double (&y)[9]) {
    const double (&r0)[9] = (from_y & 1) ? y : x;
    const double (&r1)[9] = (from_y & 2) ? y : x;
    const double (&r2)[9] = (from_y & 4) ? y : x;
    return det3r(r0[0], r0[1], r0[2], r1[3], r1[4], r1[5], r2[6], r2[7], r2[8]);
}
SIFT_HD double cubic(double A, double B, double C, double x) {
    return __builtin_fma(__builtin_fma(__builtin_fma(1.0, x, A), x, B), x, C);
}
SIFT_HD double cubic_slope(double A, double B, double x) { return __builtin_fma(__builtin_fma(3.0, x, A + A), x, B); }
// 128 fixed bisection steps between a "negative" end n and a "positive" end p; the result is p.  No early exit.
SIFT_HD double bisect_slope(double A, double B, double n, double p) {
    for (int it = 0; it < 128; ++it) {
        const double mid = 0.5 * (n + p);
        const bool neg = cubic_slope(A, B, mid) < 0.0;
        n = neg ? mid : n;
        p = neg ? p : mid;
    }
    return p;
}
SIFT_HD double bisect_cubic(double A, double B, double C, double n, double p) {
    for (int it = 0; it < 128; ++it) {
        const double mid = 0.5 * (n + p);
        const bool neg = cubic(A, B, C, mid) < 0.0;
        n = neg ? mid : n;
        p = neg ? p : mid;
    }
    return p;
}
// the root of the bracket [lo, hi], when p has opposite weak signs at its ends
SIFT_HD bool bracket_root(double A, double B, double C, double lo, double hi, double& root) {
    const double plo = cubic(A, B, C, lo), phi = cubic(A, B, C, hi);
    const bool up = (plo <= 0.0) & (phi >= 0.0), down = (plo >= 0.0) & (phi <= 0.0);
    root = bisect_cubic(A, B, C, up ? lo : hi, up ? hi : lo);
    return up | down;
}
}  // namespace fund_detail

// The fundamental matrices of seven correspondences c[k] = (qx, qy, tx, ty): f[k] = root k, nine floats row-major, all +0.0f
// when slot k is invalid.  Returns the mask of valid slots (bit k = slot k).
//   matrix     row i = [tx qx, tx qy, tx, ty qx, ty qy, ty, qx, qy, 1] in double (each product of two floats is exact), the
//              coordinates unnormalised
//   pivoting   seven steps of Gauss-Jordan elimination with complete pivoting and no swaps.  The pivot is the first entry of
//              largest magnitude in row-major order among the rows and columns not yet used; a NaN is never taken; a pivot that
//              is zero or not finite makes the sample invalid.  Every other row i, used rows included, gets mul = a[i][pc] / piv
//              and a[i][j] = fma(-mul, a[pr][j], a[i][j]) for all nine j - the multiplier form, the pivot row is not normalised:
//              two bit-identical sample rows cancel to exact zeros and the sample is rejected by its zero pivot (keypoints of one
//              location with several orientations share coordinates)
//   null       the unused columns f0 < f1; n1 has 1 at f0, 0 at f1 and -(a[i][f0] / a[i][pc_i]) at row i's pivot column; n2
//              likewise from f1
//   cubic      det(l n1 + n2) = c3 l^3 + c2 l^2 + c1 l + c0 by multilinearity: c3 = det(n1), c0 = det(n2), c2 and c1 the sums
//              (d + d) + d of the three mixed row determinants in the order of the replaced row (for c2 the row taken from n2,
//              for c1 the row taken from n1); every determinant by cofactors along the first row (fund_detail::det3r)
//   monic      A = c2 / c3, B = c1 / c3, C = c0 / c3, invalid if one is not finite; M = 1 + max(|A|, |B|, |C|) bounds the roots;
//              p(x) = fma(fma(fma(1, x, A), x, B), x, C), p'(x) = fma(fma(3, x, A + A), x, B)
//   brackets   xv = -A / 3.  If p'(xv) < 0 the critical points x1, x2 come from 128 bisection steps of p' on [-M, xv] and
//              [xv, M] (the negative end is xv), and the brackets are [-M, x1], [x1, x2], [x2, M]; otherwise the one bracket
//              is [-M, M] and roots 1 and 2 do not exist
//   roots      bracket k holds root k when p has opposite weak signs at its ends (<= 0 and >= 0, in either order; the end with
//              p <= 0 is the negative end, the lower end when both qualify); the root is the positive end after 128 bisection
//              steps of p.  No early exit, no Newton step
//   model      F[j] = fma(root, n1[j], n2[j]), all nine finite; divided by its first entry of largest magnitude (that entry
//              becomes +1, which fixes the sign); rounded to nine floats
SIFT_HD uint32_t ransac_fundamental7(const float (&c)[7][4], float (&f)[3][9]) {
    using namespace fund_detail;
#pragma unroll
    for (int k = 0; k < 3; ++k)
#pragma unroll
        for (int j = 0; j < 9; ++j) f[k][j] = 0.0f;
    double a[7][9];
#pragma unroll
    for (int i = 0; i < 7; ++i) {
        const double qx = (double)c[i][0], qy = (double)c[i][1], tx = (double)c[i][2], ty = (double)c[i][3];
        a[i][0] = tx * qx; a[i][1] = tx * qy; a[i][2] = tx;
        a[i][3] = ty * qx; a[i][4] = ty * qy; a[i][5] = ty;
        a[i][6] = qx;      a[i][7] = qy;      a[i][8] = 1.0;
    }
    uint32_t rused = 0, cused = 0;
    int pcol[7] = {0, 0, 0, 0, 0, 0, 0};   // the pivot column of every row
    bool ok = true;
#pragma unroll 1
    for (int step = 0; step < 7; ++step) {
        double best = -1.0, piv = 0.0;
        int pr = 0, pc = 0;
#pragma unroll
        for (int i = 0; i < 7; ++i)
#pragma unroll
            for (int j = 0; j < 9; ++j) {
                const double mag = __builtin_fabs(a[i][j]);
                const bool take = (((rused >> i) & 1u) == 0u) & (((cused >> j) & 1u) == 0u) & (mag > best);   // false for a NaN
                best = take ? mag : best;
                piv = take ? a[i][j] : piv;
                pr = take ? i : pr;
                pc = take ? j : pc;
            }
        ok &= finite(piv) & (piv != 0.0);
        double prow[9];
#pragma unroll
        for (int j = 0; j < 9; ++j) {
            double v = a[0][j];
#pragma unroll
            for (int i = 1; i < 7; ++i) v = pr == i ? a[i][j] : v;
            prow[j] = v;
        }
#pragma unroll
        for (int i = 0; i < 7; ++i) {
            double v = a[i][0];
#pragma unroll
            for (int j = 1; j < 9; ++j) v = pc == j ? a[i][j] : v;
            const double mul = v / piv;
            const bool other = pr != i;
#pragma unroll
            for (int j = 0; j < 9; ++j) {
                const double u = __builtin_fma(-mul, prow[j], a[i][j]);
                a[i][j] = other ? u : a[i][j];
            }
            pcol[i] = other ? pcol[i] : pc;
        }
        rused |= 1u << pr;
        cused |= 1u << pc;
    }
    if (!ok) return 0u;
    int f0 = 0, f1 = 0;   // the two unused columns, f0 < f1
    {
        int seen = 0;
#pragma unroll
        for (int j = 0; j < 9; ++j) {
            const bool is_free = ((cused >> j) & 1u) == 0u;
            f0 = (is_free & (seen == 0)) ? j : f0;
            f1 = (is_free & (seen == 1)) ? j : f1;
            seen += is_free ? 1 : 0;
        }
    }
    double n1[9], n2[9];
#pragma unroll
    for (int j = 0; j < 9; ++j) {
        n1[j] = j == f0 ? 1.0 : 0.0;
        n2[j] = j == f1 ? 1.0 : 0.0;
    }
#pragma unroll
    for (int i = 0; i < 7; ++i) {
        double v0 = a[i][0], v1 = a[i][0], vp = a[i][0];
#pragma unroll
        for (int j = 1; j < 9; ++j) {
            v0 = f0 == j ? a[i][j] : v0;
            v1 = f1 == j ? a[i][j] : v1;
            vp = pcol[i] == j ? a[i][j] : vp;
        }
        const double e1 = -(v0 / vp), e2 = -(v1 / vp);
#pragma unroll
        for (int j = 0; j < 9; ++j) {
            n1[j] = pcol[i] == j ? e1 : n1[j];
            n2[j] = pcol[i] == j ? e2 : n2[j];
        }
    }
    const double c3 = det_mixed<0>(n1, n2), c0 = det_mixed<7>(n1, n2);
    const double c2 = (det_mixed<1>(n1, n2) + det_mixed<2>(n1, n2)) + det_mixed<4>(n1, n2);
    const double c1 = (det_mixed<6>(n1, n2) + det_mixed<5>(n1, n2)) + det_mixed<3>(n1, n2);
    const double A = c2 / c3, B = c1 / c3, C = c0 / c3;
    if (!(finite(A) && finite(B) && finite(C))) return 0u;
    double mx = __builtin_fabs(A);
    mx = __builtin_fabs(B) > mx ? __builtin_fabs(B) : mx;
    mx = __builtin_fabs(C) > mx ? __builtin_fabs(C) : mx;
    const double M = 1.0 + mx;
    const double xv = -A / 3.0;
    const bool three = cubic_slope(A, B, xv) < 0.0;
    double x1 = M, x2 = M;
    if (three) {
        x1 = bisect_slope(A, B, xv, -M);
        x2 = bisect_slope(A, B, xv, M);
    }
    uint32_t valid = 0u;
#pragma unroll 1
    for (int k = 0; k < 3; ++k) {
        if (k > 0 && !three) break;
        const double lo = k == 0 ? -M : (k == 1 ? x1 : x2), hi = k == 0 ? x1 : (k == 1 ? x2 : M);
        double root;
        bool good = bracket_root(A, B, C, lo, hi, root);
        double F[9];
        double big = 0.0, mag = -1.0;
#pragma unroll
        for (int j = 0; j < 9; ++j) {
            F[j] = __builtin_fma(root, n1[j], n2[j]);
            good &= finite(F[j]);
            const double m = __builtin_fabs(F[j]);
            const bool take = m > mag;   // the first maximum stays
            big = take ? F[j] : big;
            mag = take ? m : mag;
        }
        good &= mag > 0.0;
#pragma unroll
        for (int j = 0; j < 9; ++j) {
            const float v = (float)(F[j] / big);
            // a slot index that is a loop variable: written through selects, so that f stays in registers on the GPU
            f[0][j] = (good & (k == 0)) ? v : f[0][j];
            f[1][j] = (good & (k == 1)) ? v : f[1][j];
            f[2][j] = (good & (k == 2)) ? v : f[2][j];
        }
        valid |= good ? (1u << k) : 0u;
    }
    return valid;
}

// Is the correspondence (qx, qy, tx, ty) within thr pixels of the model, by the Sampson distance?  Float, no division:
// r^2 / g <= thr^2  <=>  r^2 <= thr^2 g for g > 0, with r = t^T F q and g the squared norm of the first two entries of F q and
// of F^T t.  thr2 = thr * thr (one float product).  A NaN or an infinity anywhere makes it no inlier; so does the zero matrix.
SIFT_HD bool ransac_fund_inlier(const float (&f)[9], float qx, float qy, float tx, float ty, float thr2) {
    const float a = __builtin_fmaf(f[0], qx, __builtin_fmaf(f[1], qy, f[2]));
    const float b = __builtin_fmaf(f[3], qx, __builtin_fmaf(f[4], qy, f[5]));
    const float c = __builtin_fmaf(f[6], qx, __builtin_fmaf(f[7], qy, f[8]));
    const float r = __builtin_fmaf(tx, a, __builtin_fmaf(ty, b, c));
    const float a2 = __builtin_fmaf(f[0], tx, __builtin_fmaf(f[3], ty, f[6]));
    const float b2 = __builtin_fmaf(f[1], tx, __builtin_fmaf(f[4], ty, f[7]));
    const float g = __builtin_fmaf(a, a, __builtin_fmaf(b, b, __builtin_fmaf(a2, a2, b2 * b2)));
    const float e = r * r;
    return (e <= thr2 * g) & (g > 0.0f) & (e < __builtin_inff());
}

}  // namespace sift_hip
