// Refinement of a RANSAC homography (include/sift_hip.h, "refit"): THE DEFINITION, next to ransac_math.h and under the same
// rules.  The HIP kernel (kernels_ransac.hip: ransac_refine_kernel) and the host checker (hostmath_capi.cpp) both compile this
// header with -ffp-contract=off; every fused operation is an explicit fma, every other product, sum and quotient is one
// rounding.  An extension: the reference has no counterpart.
//
// A round re-estimates the model from its own inliers by a normalised, inhomogeneous DLT in double:
//   inliers      the rows with ransac_inlier(h, ...), n of them; n < 4 fails the round
//   moments      fixed-order sums of qx, qy, tx, ty, qx^2 + qy^2, tx^2 + ty^2 over the inliers -> refine_normalisation: centroids
//                and, per side, a power-of-two scale from the exponent of the mean squared spread (no square root)
//   normal sums  the 22 distinct fixed-order sums of A^T A and A^T b (refine_normal_terms), rows [x y 1 0 0 0 -ux -uy | u] and
//                [0 0 0 x y 1 -vx -vy | v] in normalised coordinates -> refine_system: the 8 x 9 augmented matrix
//   solve        Gaussian elimination, partial pivoting (the first entry of largest magnitude), every update one fma
//   denormalise  H = Tt^-1 Hn Tq, divided by its first entry of largest magnitude, W > 0 at the query centroid, nine floats
//   re-score     c' = the inliers of the new model among all rows; accepted when c' >= c, and the next round runs when c' > c
// A FIXED-ORDER SUM over the m rows of a set has kRefineLanes = 256 partials; partial p is the sequential sum, rows ascending,
// from +0.0, of the terms of the inlier rows i = p (mod 256); the partials are combined by the adjacent pairwise tree
// (refine_tree256): for w = 1, 2, 4 .. 128, s[p] = s[p] + s[p + w] for p = 0 (mod 2 w).  That is a strided loop of a 256-lane
// workgroup, an xor butterfly inside each wave and (W0 + W1) + (W2 + W3) over the four waves: addition commutes bit for bit, so
// a butterfly lane's s[p] + s[p ^ w] is the tree's value.
#pragma once
#include <stdint.h>

#include "ransac_math.h"

namespace sift_hip {

constexpr int kRefineLanes = 256;      // partials of a fixed-order sum
constexpr int kRefineMaxRounds = 8;    // sift_hip_ransac_params.refine is 0 .. 8
constexpr int kRefineMoments = 6;      // sums of the first pass
constexpr int kRefineSums = 22;        // sums of the second pass

struct RefineNorm {
    double cqx, cqy, sq;        // query side: centroid, scale (a power of two)
    double ctx, cty, st, ist;   // train side: centroid, scale and 1 / scale (both powers of two)
};

SIFT_HD bool refine_finite(double v) { return v - v == 0.0; }

// ---- first pass: qx, qy, tx, ty, qx^2 + qy^2, tx^2 + ty^2.  The squares of floats are exact in double; their sum rounds once.
SIFT_HD void refine_moment_terms(float qx, float qy, float tx, float ty, double (&t)[kRefineMoments]) {
    const double a = (double)qx, b = (double)qy, c = (double)tx, d = (double)ty;
    t[0] = a;
    t[1] = b;
    t[2] = c;
    t[3] = d;
    t[4] = a * a + b * b;
    t[5] = c * c + d * d;
}

// One side's centroid and scale from its sums (sx, sy, s2 = sum of x^2 + y^2) over n rows.  The mean squared spread is
// d = s2 / n - (cx^2 + cy^2); the scale is 2^-floor(e / 2) with e the unbiased exponent field of d, read from its bits (a
// subnormal d has e = -1023), so that d * scale^2 lies in [1, 4).  False when d is not finite or not > 0.
SIFT_HD bool refine_side(double sx, double sy, double s2, double dn, double& cx, double& cy, double& scale, double& inv_scale) {
    cx = sx / dn;
    cy = sy / dn;
    const double d = s2 / dn - __builtin_fma(cx, cx, cy * cy);
    const bool ok = refine_finite(d) & (d > 0.0);
    const int64_t bits = __builtin_bit_cast(int64_t, ok ? d : 1.0);
    const int64_t e = ((bits >> 52) & 0x7ff) - 1023;
    const int64_t half = e >> 1;   // floor(e / 2): -512 .. 511
    scale = __builtin_bit_cast(double, (int64_t)(1023 - half) << 52);
    inv_scale = __builtin_bit_cast(double, (int64_t)(1023 + half) << 52);
    return ok;
}

SIFT_HD bool refine_normalisation(const double (&mom)[kRefineMoments], int n, RefineNorm& nm) {
    const double dn = (double)n;
    double iq;
    const bool okq = refine_side(mom[0], mom[1], mom[4], dn, nm.cqx, nm.cqy, nm.sq, iq);
    const bool okt = refine_side(mom[2], mom[3], mom[5], dn, nm.ctx, nm.cty, nm.st, nm.ist);
    return okq & okt;
}

// ---- second pass.  x = (qx - cqx) * sq: one rounding (the difference); the scaling by a power of two is exact.
// t[0 .. 4] = xx, xy, yy, x, y;  t[5 .. 10] = u * {xx, xy, yy, x, y, 1};  t[11 .. 16] = v * {the same};
// t[17 .. 21] = (u^2 + v^2) * {xx, xy, yy, x, y}
SIFT_HD void refine_normal_terms(const RefineNorm& nm, float qx, float qy, float tx, float ty, double (&t)[kRefineSums]) {
    const double x = ((double)qx - nm.cqx) * nm.sq, y = ((double)qy - nm.cqy) * nm.sq;
    const double u = ((double)tx - nm.ctx) * nm.st, v = ((double)ty - nm.cty) * nm.st;
    const double xx = x * x, xy = x * y, yy = y * y;
    const double r = __builtin_fma(u, u, v * v);
    t[0] = xx;
    t[1] = xy;
    t[2] = yy;
    t[3] = x;
    t[4] = y;
    t[5] = u * xx;
    t[6] = u * xy;
    t[7] = u * yy;
    t[8] = u * x;
    t[9] = u * y;
    t[10] = u;
    t[11] = v * xx;
    t[12] = v * xy;
    t[13] = v * yy;
    t[14] = v * x;
    t[15] = v * y;
    t[16] = v;
    t[17] = r * xx;
    t[18] = r * xy;
    t[19] = r * yy;
    t[20] = r * x;
    t[21] = r * y;
}

// The augmented normal equations [A^T A | A^T b], row-major with 9 entries a row, for the unknowns h0 .. h7 (h8 = 1).
// Negations are exact.  M may be any memory (the kernel's is LDS).
template <typename P>
SIFT_HD void refine_system(const double (&s)[kRefineSums], int n, P M) {
    const double dn = (double)n;
    const double row[8][9] = {
        {s[0], s[1], s[3], 0.0, 0.0, 0.0, -s[5], -s[6], s[8]},
        {s[1], s[2], s[4], 0.0, 0.0, 0.0, -s[6], -s[7], s[9]},
        {s[3], s[4], dn, 0.0, 0.0, 0.0, -s[8], -s[9], s[10]},
        {0.0, 0.0, 0.0, s[0], s[1], s[3], -s[11], -s[12], s[14]},
        {0.0, 0.0, 0.0, s[1], s[2], s[4], -s[12], -s[13], s[15]},
        {0.0, 0.0, 0.0, s[3], s[4], dn, -s[14], -s[15], s[16]},
        {-s[5], -s[6], -s[8], -s[11], -s[12], -s[14], s[17], s[18], -s[20]},
        {-s[6], -s[7], -s[9], -s[12], -s[13], -s[15], s[18], s[19], -s[21]},
    };
    for (int i = 0; i < 8; ++i)
        for (int j = 0; j < 9; ++j) M[9 * i + j] = row[i][j];
}

// ---- the solve, in steps that the kernel spreads over lanes and the host runs as the loop refine_solve8.
// Step k: the pivot row p = the first row i >= k with the largest |M[i][k]|; rows k and p change places; every row i > k becomes
// M[i][j] = fma(-f, M[k][j], M[i][j]) for j > k with f = M[i][k] / M[k][k].  Entries at and below the diagonal of the finished
// columns are never read again and keep whatever they held.
template <typename P>
SIFT_HD int refine_pivot(P M, int k, bool& ok) {
    int p = k;
    double mag = __builtin_fabs(M[9 * k + k]);
    for (int i = k + 1; i < 8; ++i) {
        const double a = __builtin_fabs(M[9 * i + k]);
        const bool take = a > mag;   // the first maximum stays; a NaN is never taken, and is not replaced when it comes first
        p = take ? i : p;
        mag = take ? a : mag;
    }
    ok = refine_finite(mag) & (mag > 0.0);
    return p;
}
SIFT_HD double refine_eliminate(double f, double pivot_row_j, double mij) { return __builtin_fma(-f, pivot_row_j, mij); }

// x[i] = (M[i][8] - sum over j > i, ascending, of M[i][j] x[j]) / M[i][i], from the last row up; false when an x is not finite
template <typename P>
SIFT_HD bool refine_backsubstitute(P M, double (&x)[8]) {
    bool ok = true;
#pragma unroll
    for (int i = 7; i >= 0; --i) {
        double acc = M[9 * i + 8];
#pragma unroll
        for (int j = i + 1; j < 8; ++j) acc = __builtin_fma(-M[9 * i + j], x[j], acc);
        x[i] = acc / M[9 * i + i];
        ok &= refine_finite(x[i]);
    }
    return ok;
}

// the whole solve as one loop; M (72 doubles) is destroyed.  False when a pivot is zero or not finite or a solution is not finite.
inline bool refine_solve8(double* M, double (&x)[8]) {
    for (int k = 0; k < 8; ++k) {
        bool ok;
        const int p = refine_pivot(M, k, ok);
        if (!ok) return false;
        for (int j = 0; j < 9; ++j) {
            const double a = M[9 * k + j];
            M[9 * k + j] = M[9 * p + j];
            M[9 * p + j] = a;
        }
        for (int i = k + 1; i < 8; ++i) {
            const double f = M[9 * i + k] / M[9 * k + k];
            for (int j = k + 1; j < 9; ++j) M[9 * i + j] = refine_eliminate(f, M[9 * k + j], M[9 * i + j]);
        }
    }
    return refine_backsubstitute(M, x);
}

// ---- H = Tt^-1 Hn Tq with Hn = [x0 x1 x2; x3 x4 x5; x6 x7 1], Tq = [sq 0 -sq cqx; 0 sq -sq cqy; 0 0 1] and
// Tt^-1 = [1/st 0 ctx; 0 1/st cty; 0 0 1].  G = Hn Tq first: G[i][0] = Hn[i][0] sq, G[i][1] = Hn[i][1] sq (exact scalings),
// G[i][2] = fma(-G[i][0], cqx, fma(-G[i][1], cqy, Hn[i][2])).  Then H[0][j] = fma(ctx, G[2][j], G[0][j] / st), H[1][j] alike with
// cty, H[2][j] = G[2][j].  False (h untouched) when an entry is not finite or all are zero.  Otherwise H is divided by its first
// entry of largest magnitude, negated if W at the query centroid is negative, and rounded to nine floats.
SIFT_HD bool refine_denormalise(const double (&x)[8], const RefineNorm& nm, float (&h)[9]) {
    const double Hn[3][3] = {{x[0], x[1], x[2]}, {x[3], x[4], x[5]}, {x[6], x[7], 1.0}};
    double G[3][3];
    for (int i = 0; i < 3; ++i) {
        G[i][0] = Hn[i][0] * nm.sq;
        G[i][1] = Hn[i][1] * nm.sq;
        G[i][2] = __builtin_fma(-G[i][0], nm.cqx, __builtin_fma(-G[i][1], nm.cqy, Hn[i][2]));
    }
    double H[9];
    for (int j = 0; j < 3; ++j) {
        H[j] = __builtin_fma(nm.ctx, G[2][j], G[0][j] * nm.ist);
        H[3 + j] = __builtin_fma(nm.cty, G[2][j], G[1][j] * nm.ist);
        H[6 + j] = G[2][j];
    }
    bool ok = true;
    double big = H[0], mag = __builtin_fabs(H[0]);
    for (int i = 0; i < 9; ++i) {
        ok &= refine_finite(H[i]);
        const double a = __builtin_fabs(H[i]);
        const bool take = a > mag;   // the first maximum stays
        big = take ? H[i] : big;
        mag = take ? a : mag;
    }
    ok &= mag > 0.0;
    for (int i = 0; i < 9; ++i) H[i] = H[i] / big;
    const double w = __builtin_fma(H[6], nm.cqx, __builtin_fma(H[7], nm.cqy, H[8]));
    const bool flip = w < 0.0;
    for (int i = 0; i < 9; ++i) {
        const float v = (float)(flip ? -H[i] : H[i]);
        h[i] = ok ? v : h[i];
    }
    return ok;
}

// the combination of the 256 partials of a fixed-order sum (the host's form; the kernel's is a butterfly and LDS)
inline double refine_tree256(double (&s)[kRefineLanes]) {
    for (int w = 1; w < kRefineLanes; w *= 2)
        for (int p = 0; p < kRefineLanes; p += 2 * w) s[p] = s[p] + s[p + w];
    return s[0];
}

}  // namespace sift_hip
