// RANSAC homography over match lists (include/sift_hip.h, "geometric verification"): THE DEFINITION.  The HIP kernels
// (kernels_ransac.hip) and the host checker (hostmath_capi.cpp) both compile this header, with -ffp-contract=off; every fused
// operation is written as an explicit fma / fmaf, every other product and sum is one rounding.  An extension: the reference has
// no counterpart.
//
// A correspondence is four floats (qx, qy, tx, ty); the model maps query to train, (tx, ty, 1) ~ H (qx, qy, 1), H row-major.
//   sampling   ransac_draw: four distinct rows of a set from a counter-based integer hash of (seed, set, iteration) - no state
//              between iterations, integer arithmetic only, so exact wherever it runs
//   solve      ransac_homography4: the four-point model in double, branch-free, from 3 x 3 determinants and adjugates only
//   predicate  ransac_inlier: float, division-free
//   selection  score of a hypothesis = its inlier count over ALL rows of its set, -1 when the hypothesis is invalid; the winner is
//              the highest score, the lowest iteration among equals; none (iteration -1, inliers 0, h all +0.0f, every flag 0)
//              when no hypothesis is valid or the set has fewer than four rows.  The flags are the predicate under the winner.
// Scores are integers: the result cannot depend on how rows or hypotheses are tiled, split over workgroups or reduced.
// The H these functions select is the best MINIMAL-SAMPLE model; its least-squares refit over the inliers, with sums in a fixed
// order so that it stays bit-defined, is ransac_refine_math.h.  There is no adaptive early stop.  The other model, the
// fundamental matrix from seven-point samples, is ransac_fund_math.h; it shares the hash and the selection rule.
#pragma once
#include <stdint.h>

#include "fdlibm_atan2f.h"   // SIFT_HD

namespace sift_hip {

// the 32-bit finaliser "lowbias32" (C. Wellons, public domain): a bijection of uint32 with good avalanche
SIFT_HD uint32_t ransac_hash(uint32_t x) {
    x ^= x >> 16;
    x *= 0x7feb352du;
    x ^= x >> 15;
    x *= 0x846ca68bu;
    x ^= x >> 16;
    return x;
}

// Four distinct indices in [0, m), m >= 4, of hypothesis `iteration` of set `set`.  Draw k takes a value in [0, m - k) by
// (uint64(hash) * range) >> 32 and then steps over the k indices already drawn, in ascending order ("the v-th index that is
// still free"): distinct by construction, no retry loop.  For m == 4 every draw is a permutation of 0 .. 3.
SIFT_HD void ransac_draw(uint32_t seed, uint32_t set, uint32_t iteration, uint32_t m, uint32_t (&idx)[4]) {
    const uint32_t key = ransac_hash(ransac_hash(seed ^ 0x9e3779b9u) + set * 0x85ebca6bu);
    const uint32_t base = ransac_hash(key ^ (iteration * 0xc2b2ae35u + 0x27d4eb2fu));
    uint32_t s0 = 0, s1 = 0, s2 = 0;   // the indices drawn so far, ascending
    {
        idx[0] = (uint32_t)(((uint64_t)ransac_hash(base) * (uint64_t)m) >> 32);
        s0 = idx[0];
    }
    {
        uint32_t v = (uint32_t)(((uint64_t)ransac_hash(base + 0x9e3779b9u) * (uint64_t)(m - 1u)) >> 32);
        v += v >= s0 ? 1u : 0u;
        idx[1] = v;
        s1 = v > s0 ? v : s0;
        s0 = v > s0 ? s0 : v;
    }
    {
        uint32_t v = (uint32_t)(((uint64_t)ransac_hash(base + 2u * 0x9e3779b9u) * (uint64_t)(m - 2u)) >> 32);
        v += v >= s0 ? 1u : 0u;
        v += v >= s1 ? 1u : 0u;
        idx[2] = v;
        const uint32_t lo = v < s0 ? v : s0, mid0 = v < s0 ? s0 : v;
        s2 = mid0 > s1 ? mid0 : s1;
        s1 = mid0 > s1 ? s1 : mid0;
        s0 = lo;
    }
    {
        uint32_t v = (uint32_t)(((uint64_t)ransac_hash(base + 3u * 0x9e3779b9u) * (uint64_t)(m - 3u)) >> 32);
        v += v >= s0 ? 1u : 0u;
        v += v >= s1 ? 1u : 0u;
        v += v >= s2 ? 1u : 0u;
        idx[3] = v;
    }
}

namespace ransac_detail {
// det [a b c] of three points (x, y, 1) as columns
SIFT_HD double det3(double ax, double ay, double bx, double by, double cx, double cy) {
    const double t0 = by - cy, t1 = cy - ay, t2 = ay - by;
    return __builtin_fma(ax, t0, __builtin_fma(bx, t1, cx * t2));
}
SIFT_HD double det2(double a, double b, double c, double d) { return __builtin_fma(a, d, -(b * c)); }   // a d - b c
SIFT_HD bool finite_nonzero(double v) { return (v - v == 0.0) & (v != 0.0); }
// The projective basis of four points: columns l[k] * (x[k], y[k], 1), k = 0 .. 2, with l = adj([p0 p1 p2]) p3, i.e. l[k] = the
// determinant with column k replaced by p3 (Cramer).  M maps e_k to p_k and (1, 1, 1) to det([p0 p1 p2]) p3.  l[3] = that
// determinant.
SIFT_HD void basis(const double (&x)[4], const double (&y)[4], double (&M)[3][3], double (&l)[4]) {
    l[0] = det3(x[3], y[3], x[1], y[1], x[2], y[2]);
    l[1] = det3(x[0], y[0], x[3], y[3], x[2], y[2]);
    l[2] = det3(x[0], y[0], x[1], y[1], x[3], y[3]);
    l[3] = det3(x[0], y[0], x[1], y[1], x[2], y[2]);
    for (int k = 0; k < 3; ++k) {
        M[0][k] = l[k] * x[k];
        M[1][k] = l[k] * y[k];
        M[2][k] = l[k];
    }
}
}  // namespace ransac_detail

// The homography of four correspondences c[k] = (qx, qy, tx, ty), in double: A = basis of the query points, B = basis of the
// train points, H = B adj(A) (so H q_k ~ t_k for all four).  Returns false, and h all +0.0f, when
//   - one of the eight determinants (the l of both sides) is zero or not finite: three of the four points of a side are
//     collinear or coincide, or a coordinate is a NaN or an infinity;
//   - the four products lq[k] * lt[k] do not have the same strict sign - the orientation test.  H q_k = det(A) (lt[k] / lq[k]) t_k
//     for k = 0 .. 3 (for k = 3: det([t0 t1 t2]) / det([q0 q1 q2])), so these signs are the signs of W at the four sample points:
//     a model that puts sample points on both sides of its line at infinity (a convex quadrilateral onto a bow-tie) is not one
//     the predicate below could ever accept for all of its own sample.  The fourth product is part of the test for that reason;
//   - an entry of H is not finite.
// Otherwise H is divided by its entry of largest magnitude (the first such entry), negated if W of the first sample point is
// negative, and rounded to nine floats.
SIFT_HD bool ransac_homography4(const float (&c)[4][4], float (&h)[9]) {
    using namespace ransac_detail;
    double qx[4], qy[4], tx[4], ty[4];
    for (int k = 0; k < 4; ++k) {
        qx[k] = (double)c[k][0];
        qy[k] = (double)c[k][1];
        tx[k] = (double)c[k][2];
        ty[k] = (double)c[k][3];
    }
    double A[3][3], B[3][3], lq[4], lt[4];
    basis(qx, qy, A, lq);
    basis(tx, ty, B, lt);
    bool ok = true, pos = true, neg = true;
    for (int k = 0; k < 4; ++k) {
        ok &= finite_nonzero(lq[k]);
        ok &= finite_nonzero(lt[k]);
        const double p = lq[k] * lt[k];
        pos &= p > 0.0;
        neg &= p < 0.0;
    }
    ok &= pos | neg;
    double J[3][3];   // adj(A): J[i][j] = cofactor (j, i)
    J[0][0] = det2(A[1][1], A[1][2], A[2][1], A[2][2]);
    J[0][1] = det2(A[0][2], A[0][1], A[2][2], A[2][1]);
    J[0][2] = det2(A[0][1], A[0][2], A[1][1], A[1][2]);
    J[1][0] = det2(A[1][2], A[1][0], A[2][2], A[2][0]);
    J[1][1] = det2(A[0][0], A[0][2], A[2][0], A[2][2]);
    J[1][2] = det2(A[0][2], A[0][0], A[1][2], A[1][0]);
    J[2][0] = det2(A[1][0], A[1][1], A[2][0], A[2][1]);
    J[2][1] = det2(A[0][1], A[0][0], A[2][1], A[2][0]);
    J[2][2] = det2(A[0][0], A[0][1], A[1][0], A[1][1]);
    double H[9];
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) H[3 * i + j] = __builtin_fma(B[i][0], J[0][j], __builtin_fma(B[i][1], J[1][j], B[i][2] * J[2][j]));
    double big = H[0], mag = __builtin_fabs(H[0]);
    for (int i = 0; i < 9; ++i) {
        ok &= H[i] - H[i] == 0.0;
        const double a = __builtin_fabs(H[i]);
        const bool take = a > mag;   // the first maximum stays
        big = take ? H[i] : big;
        mag = take ? a : mag;
    }
    ok &= mag > 0.0;
    for (int i = 0; i < 9; ++i) H[i] = H[i] / big;
    const double w0 = __builtin_fma(H[6], qx[0], __builtin_fma(H[7], qy[0], H[8]));
    const bool flip = w0 < 0.0;
    for (int i = 0; i < 9; ++i) {
        const float v = (float)(flip ? -H[i] : H[i]);
        h[i] = ok ? v : 0.0f;
    }
    return ok;
}

// Is the correspondence (qx, qy, tx, ty) within thr pixels of the model?  Float, no division: the reprojection error e = |t - (X,
// Y) / W| <= thr  <=>  |t W - (X, Y)|^2 <= thr^2 W^2 for W > 0.  thr2 = thr * thr (one float product).  A NaN anywhere, an
// infinite coordinate (e2 is then an infinity or a NaN) or W <= 0 makes it no inlier.
SIFT_HD bool ransac_inlier(const float (&h)[9], float qx, float qy, float tx, float ty, float thr2) {
    const float X = __builtin_fmaf(h[0], qx, __builtin_fmaf(h[1], qy, h[2]));
    const float Y = __builtin_fmaf(h[3], qx, __builtin_fmaf(h[4], qy, h[5]));
    const float W = __builtin_fmaf(h[6], qx, __builtin_fmaf(h[7], qy, h[8]));
    const float ex = __builtin_fmaf(-tx, W, X);
    const float ey = __builtin_fmaf(-ty, W, Y);
    const float e2 = __builtin_fmaf(ex, ex, ey * ey);
    const float bound = thr2 * (W * W);
    return (W > 0.0f) & (e2 <= bound) & (e2 < __builtin_inff());
}

}  // namespace sift_hip
