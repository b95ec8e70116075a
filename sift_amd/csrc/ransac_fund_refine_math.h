// Least-squares refit of a RANSAC fundamental matrix (include/sift_hip.h, "refit of F"): THE DEFINITION, a sibling of
// ransac_refine_math.h under the same rules.  The HIP kernel (kernels_ransac.hip: ransac_fund_refine_kernel) and the host
// checker (hostmath_capi.cpp: hostmath_refine_fundamental) both compile this header with -ffp-contract=off; double arithmetic,
// every fused operation an explicit fma, every other product, sum and quotient one rounding; no square root, no libm call, no
// early exit whose outcome could differ by a step.  An extension: the reference has no counterpart.
//
// A round re-estimates the model f, whose score c is its inlier count, from its own inliers by the normalised eight-point
// method with one entry fixed (an inhomogeneous system, so that the homography refit's elimination serves) and a rank-2 step:
//   inliers      the rows with ransac_fund_inlier(f, ..., thr2), n of them; n < 8 fails the round
//   moments      the six fixed-order sums of refine_moment_terms -> refine_normalisation: centroids and power-of-two scales;
//                x, y = the normalised query coordinates, u, v = the normalised train coordinates (as refine_normal_terms)
//   moment sums  the constraint row is a = [u x, u y, u, v x, v y, v, x, y, 1]; every entry of S = sum a a^T is the sum of a
//                product P Q, P one of {1, u, v, uu, uv, vv} and Q one of {1, x, y, xx, xy, yy}: 36 sums, of which "1 1" is n
//                and the other 35 are fixed-order sums (fund_refine_terms)
//   gauge        Fn = Tt^-T f Tq^-1, the starting model in normalised coordinates (fund_refine_gauge); e = the index of its
//                first entry of largest magnitude; the refit fixes F[e] = 1
//   solve        the 8 x 8 system S[-e,-e] g = -S[-e,e] as an 8 x 9 augmented matrix (fund_refine_system), solved by
//                refine_pivot / refine_eliminate / refine_backsubstitute; a zero or non-finite pivot fails the round
//   rank 2       G = Fn'^T Fn'; the lowest root lambda of its characteristic cubic by the bracketed bisection of
//                ransac_fund_math.h; v = the cross product of the pair of rows of G - lambda I with the largest squared norm;
//                F2 = Fn' - (Fn' v) v^T / (v . v)  (fund_refine_rank2)
//   denormalise  F = Tt^T F2 Tq, divided by its first entry of largest magnitude (which becomes +1), nine floats: the normal
//                form of ransac_fundamental7 (fund_refine_denormalise)
//   re-score     c' = the inliers of the new model among all rows; accepted when c' >= c, and the next round runs when c' > c.
//                A failed round leaves the model as it was and ends the rounds.
// A FIXED-ORDER SUM is that of ransac_refine_math.h: kRefineLanes = 256 strided partials from +0.0, rows ascending, combined
// by refine_tree256's adjacent tree.
// Out of scope: Sampson-weighted or iterative (Levenberg-Marquardt) refinement - the refit minimises the algebraic error of
// the normalised rows, unweighted - and an oriented-epipolar test.
#pragma once
#include <stdint.h>

#include "ransac_fund_math.h"
#include "ransac_refine_math.h"

namespace sift_hip {

constexpr int kFundRefineSums = 35;      // fixed-order sums of the second pass
constexpr int kFundRefineMinRows = 8;    // inliers a round needs

// ---- second pass.  x, y, u, v as in refine_normal_terms: one rounding each (the difference; the scaling is exact).
// P[0 .. 5] = 1, u, v, u * u, u * v, v * v and Q[0 .. 5] = 1, x, y, x * x, x * y, y * y: one rounding each.  Sum 6 a + b holds
// P[a] * Q[b] (one more rounding when a > 0 and b > 0; P[0] * Q[b] is Q[b] and P[a] * Q[0] is P[a]); sum 0 is n and has no
// term: t[k] is the term of sum k + 1.
SIFT_HD void fund_refine_terms(const RefineNorm& nm, float qx, float qy, float tx, float ty, double (&t)[kFundRefineSums]) {
    const double x = ((double)qx - nm.cqx) * nm.sq, y = ((double)qy - nm.cqy) * nm.sq;
    const double u = ((double)tx - nm.ctx) * nm.st, v = ((double)ty - nm.cty) * nm.st;
    const double P[6] = {1.0, u, v, u * u, u * v, v * v};
    const double Q[6] = {1.0, x, y, x * x, x * y, y * y};
#pragma unroll
    for (int b = 1; b < 6; ++b) t[b - 1] = Q[b];
#pragma unroll
    for (int a = 1; a < 6; ++a) {
        t[6 * a - 1] = P[a];
#pragma unroll
        for (int b = 1; b < 6; ++b) t[6 * a + b - 1] = P[a] * Q[b];
    }
}

// Which of the 36 sums is S[i][j]: entry i of the constraint row is P[pi] Q[qi] with pi, qi in {0, 1, 2} (1, then the two
// coordinates), and the product of two such factors is index 0 .. 5 of the lists above.
SIFT_HD int fund_refine_pair(int a, int b) {
    const int lo = a < b ? a : b, hi = a < b ? b : a;
    return lo == 0 ? hi : (lo == 1 ? (hi == 1 ? 3 : 4) : 5);
}
SIFT_HD int fund_refine_sum_index(int i, int j) {
    const int pi = i < 3 ? 1 : (i < 6 ? 2 : 0), pj = j < 3 ? 1 : (j < 6 ? 2 : 0);
    const int ri = i % 3, rj = j % 3;
    const int qi = ri == 2 ? 0 : ri + 1, qj = rj == 2 ? 0 : rj + 1;
    return 6 * fund_refine_pair(pi, pj) + fund_refine_pair(qi, qj);
}

// ---- the gauge.  Fn = Tt^-T f Tq^-1 with Tq^-1 = [1/sq 0 cqx; 0 1/sq cqy; 0 0 1] and Tt^-T = [1/st 0 0; 0 1/st 0; ctx cty 1]
// (1 / sq is exact: a power of two).  A = f Tq^-1 first: A[i][0] = f[i][0] / sq, A[i][1] = f[i][1] / sq (exact scalings),
// A[i][2] = fma(f[i][0], cqx, fma(f[i][1], cqy, f[i][2])).  Then Fn[0][j] = A[0][j] / st, Fn[1][j] = A[1][j] / st,
// Fn[2][j] = fma(ctx, A[0][j], fma(cty, A[1][j], A[2][j])).  Returns e, the index of the first entry of largest magnitude (a
// NaN is never taken; 0 when none is).
SIFT_HD int fund_refine_gauge(const float (&f)[9], const RefineNorm& nm) {
    const double isq = 1.0 / nm.sq;
    double A[3][3];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const double f0 = (double)f[3 * i], f1 = (double)f[3 * i + 1], f2 = (double)f[3 * i + 2];
        A[i][0] = f0 * isq;
        A[i][1] = f1 * isq;
        A[i][2] = __builtin_fma(f0, nm.cqx, __builtin_fma(f1, nm.cqy, f2));
    }
    int e = 0;
    double mag = -1.0;
#pragma unroll
    for (int k = 0; k < 9; ++k) {
        const int i = k / 3, j = k % 3;
        const double fn = i < 2 ? A[i][j] * nm.ist : __builtin_fma(nm.ctx, A[0][j], __builtin_fma(nm.cty, A[1][j], A[2][j]));
        const double a = __builtin_fabs(fn);
        const bool take = a > mag;   // the first maximum stays
        e = take ? k : e;
        mag = take ? a : mag;
    }
    return e;
}

// Entry (r, c) of the 8 x 9 augmented matrix: with I = 0 .. 8 without e, ascending, it is S[I_r][I_c] for c < 8 and -S[I_r][e]
// for c = 8 (the negation is exact).  S36: the 36 sums, S36[0] = (double)n.  S36 may be any memory (the kernel's is LDS).
template <typename P>
SIFT_HD double fund_refine_system_entry(P S36, int e, int r, int c) {
    const int i = r + (r >= e ? 1 : 0), j = c < 8 ? c + (c >= e ? 1 : 0) : e;
    const double s = S36[fund_refine_sum_index(i, j)];
    return c < 8 ? s : -s;
}

// ---- rank 2.  F: Fn', nine doubles row-major, replaced by F2.  False (F then holds no result) when the cubic's coefficients
// are not finite, its lowest bracket holds no root, or v . v is zero or not finite.
//   G        G[i][j] = fma(F[0][i], F[0][j], fma(F[1][i], F[1][j], F[2][i] * F[2][j])) for i <= j
//   cubic    det(l I - G) = l^3 + A l^2 + B l + C: A = -((G00 + G11) + G22); B = (m01 + m02) + m12 with the principal minors
//            m_ij = fma(G_ii, G_jj, -(G_ij * G_ij)); C = -det3r(G).  G is symmetric and positive semi-definite: three real
//            roots, none negative.
//   root     M = 1 + max(|A|, |B|, |C|), xv = -A / 3; if p'(xv) < 0 the first critical point x1 = bisect_slope(A, B, xv, -M)
//            and the bracket is [-M, x1], otherwise [-M, M]; lambda = bracket_root's result there (128 fixed steps)
//   v        the rows of G - lambda I are r0 = (G00 - l, G01, G02), r1 = (G01, G11 - l, G12), r2 = (G02, G12, G22 - l); the
//            cross products r0 x r1, r0 x r2, r1 x r2, each component fma(a1, b2, -(a2 * b1)) and cyclic, have the squared norms
//            fma(c0, c0, fma(c1, c1, c2 * c2)); v = the first of the largest (a NaN is never taken)
//   F2       w[i] = fma(F[i][0], v0, fma(F[i][1], v1, F[i][2] * v2)); q[i] = w[i] / (v . v); F2[i][j] = fma(-q[i], v[j], F[i][j])
SIFT_HD bool fund_refine_rank2(double (&F)[9]) {
    using namespace fund_detail;
    const double G00 = __builtin_fma(F[0], F[0], __builtin_fma(F[3], F[3], F[6] * F[6]));
    const double G01 = __builtin_fma(F[0], F[1], __builtin_fma(F[3], F[4], F[6] * F[7]));
    const double G02 = __builtin_fma(F[0], F[2], __builtin_fma(F[3], F[5], F[6] * F[8]));
    const double G11 = __builtin_fma(F[1], F[1], __builtin_fma(F[4], F[4], F[7] * F[7]));
    const double G12 = __builtin_fma(F[1], F[2], __builtin_fma(F[4], F[5], F[7] * F[8]));
    const double G22 = __builtin_fma(F[2], F[2], __builtin_fma(F[5], F[5], F[8] * F[8]));
    const double A = -((G00 + G11) + G22);
    const double m01 = __builtin_fma(G00, G11, -(G01 * G01)), m02 = __builtin_fma(G00, G22, -(G02 * G02)),
                 m12 = __builtin_fma(G11, G22, -(G12 * G12));
    const double B = (m01 + m02) + m12;
    const double C = -det3r(G00, G01, G02, G01, G11, G12, G02, G12, G22);
    bool ok = finite(A) && finite(B) && finite(C);
    double mx = __builtin_fabs(A);
    mx = __builtin_fabs(B) > mx ? __builtin_fabs(B) : mx;
    mx = __builtin_fabs(C) > mx ? __builtin_fabs(C) : mx;
    const double M = 1.0 + mx;
    const double xv = -A / 3.0;
    const bool three = cubic_slope(A, B, xv) < 0.0;
    const double x1 = bisect_slope(A, B, xv, -M);   // used only when `three`; computed always: no branch to diverge on
    double l;
    ok &= bracket_root(A, B, C, -M, three ? x1 : M, l);
    const double r0[3] = {G00 - l, G01, G02}, r1[3] = {G01, G11 - l, G12}, r2[3] = {G02, G12, G22 - l};
    double v[3] = {0.0, 0.0, 0.0}, vv = -1.0;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const double (&a)[3] = k == 2 ? r1 : r0;
        const double (&b)[3] = k == 0 ? r1 : r2;
        const double c0 = __builtin_fma(a[1], b[2], -(a[2] * b[1]));
        const double c1 = __builtin_fma(a[2], b[0], -(a[0] * b[2]));
        const double c2 = __builtin_fma(a[0], b[1], -(a[1] * b[0]));
        const double nn = __builtin_fma(c0, c0, __builtin_fma(c1, c1, c2 * c2));
        const bool take = nn > vv;   // the first maximum stays
        v[0] = take ? c0 : v[0];
        v[1] = take ? c1 : v[1];
        v[2] = take ? c2 : v[2];
        vv = take ? nn : vv;
    }
    ok &= finite(vv) & (vv > 0.0);
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const double w = __builtin_fma(F[3 * i], v[0], __builtin_fma(F[3 * i + 1], v[1], F[3 * i + 2] * v[2]));
        const double q = w / vv;
#pragma unroll
        for (int j = 0; j < 3; ++j) F[3 * i + j] = __builtin_fma(-q, v[j], F[3 * i + j]);
    }
    return ok;
}

// ---- F = Tt^T F2 Tq with Tq = [sq 0 -sq cqx; 0 sq -sq cqy; 0 0 1] and Tt^T = [st 0 0; 0 st 0; -st ctx, -st cty, 1].
// B = F2 Tq first: B[i][0] = F2[i][0] sq, B[i][1] = F2[i][1] sq (exact scalings), B[i][2] = fma(-B[i][0], cqx, fma(-B[i][1],
// cqy, F2[i][2])).  Then D[0][j] = B[0][j] st, D[1][j] = B[1][j] st, D[2][j] = fma(-D[0][j], ctx, fma(-D[1][j], cty, B[2][j])).
// False (f untouched) when an entry is not finite or all are zero; otherwise D is divided by its first entry of largest
// magnitude and rounded to nine floats.
SIFT_HD bool fund_refine_denormalise(const double (&F2)[9], const RefineNorm& nm, float (&f)[9]) {
    double B[3][3], D[9];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        B[i][0] = F2[3 * i] * nm.sq;
        B[i][1] = F2[3 * i + 1] * nm.sq;
        B[i][2] = __builtin_fma(-B[i][0], nm.cqx, __builtin_fma(-B[i][1], nm.cqy, F2[3 * i + 2]));
    }
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        D[j] = B[0][j] * nm.st;
        D[3 + j] = B[1][j] * nm.st;
        D[6 + j] = __builtin_fma(-D[j], nm.ctx, __builtin_fma(-D[3 + j], nm.cty, B[2][j]));
    }
    bool ok = true;
    double big = D[0], mag = __builtin_fabs(D[0]);
#pragma unroll
    for (int i = 0; i < 9; ++i) {
        ok &= refine_finite(D[i]);
        const double a = __builtin_fabs(D[i]);
        const bool take = a > mag;   // the first maximum stays
        big = take ? D[i] : big;
        mag = take ? a : mag;
    }
    ok &= mag > 0.0;
#pragma unroll
    for (int i = 0; i < 9; ++i) {
        const float v = (float)(D[i] / big);
        f[i] = ok ? v : f[i];
    }
    return ok;
}

// The part of a round after the solve: the solution g of the 8 x 8 system, the gauge e -> the new model.  f: in, the model of
// the round (returned untouched when the round fails); out, the refit.
SIFT_HD bool fund_refine_finish(const double (&g)[8], int e, const RefineNorm& nm, float (&f)[9]) {
    double F[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) {
        // entry k is g[k] in front of e and g[k - 1] behind it: a chain of selects over compile-time indices
        const double below = k < 8 ? g[k < 8 ? k : 0] : 0.0, above = k > 0 ? g[k > 0 ? k - 1 : 0] : 0.0;
        F[k] = k == e ? 1.0 : (k < e ? below : above);
    }
    if (!fund_refine_rank2(F)) return false;
    return fund_refine_denormalise(F, nm, f);
}

}  // namespace sift_hip
