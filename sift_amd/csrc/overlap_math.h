// Photometric overlap statistics and gain compensation (include/sift_hip.h, "overlap statistics"): THE DEFINITION.  The HIP
// kernels (kernels_overlap.hip) and the host loop (hostmath_capi.cpp: hostmath_overlap_stats) both compile this header, with
// -ffp-contract=off; every fused operation is an explicit fmaf / fma, every other operation is one rounding.  It is built on
// warp_math.h: the map, the coverage test, the taps and the interpolation are warp_coords, warp_taps and warp_value as they are.
// An extension: the reference has no counterpart.
//
// Canvas c owns the jobs j0 .. j1 - 1, n = j1 - j0 <= kOverlapMaxJobs.  For canvas pixel (x, y) and job i of the canvas:
//   c_i   warp_coords' coverage test at ((float)(x + origin_x), (float)(y + origin_y))
//   q_i   the 8-bit intensity there: t = fmaf(val_i, scale, 0.5f) with val_i = warp_value(warp_taps(...)),
//         q = t >= 255 ? 255 : (t >= 0 ? (int)t : 0) - the quantiser of kernels_match_u8.hip; a NaN gives 0
// The statistics of the canvas are four n x n matrices of int64, each the sum over ALL canvas pixels where c_i and c_j both hold,
// for all ordered (i, j), i == j included, of
//   plane 0  N[i][j]   1            plane 2  SS[i][j]  q_i * q_i
//   plane 1  S[i][j]   q_i          plane 3  X[i][j]   q_i * q_j
// stored as stats[c][4][32][32], rows and columns >= n zero.  Integer sums: the same in every order, so the values depend on the
// inputs alone.
//
// gain_solve: Brown and Lowe's gain compensation (IJCV 2007, section 6) from N and S, the normal equations as OpenCV's
// GainCompensator forms them, in double.  alpha = 1 / sigma_n^2, beta = 1 / sigma_g^2, I_ij = (double)S[i][j] / (double)N[i][j]
// (0 where N[i][j] == 0).  Row i of [A | b], j ascending from zeros:
//   every j   b_i = fma(beta, N_ij, b_i), A_ii = fma(beta, N_ij, A_ii)
//   j != i    t = ((2 alpha) N_ij) I_ij, A_ii = fma(t, I_ij, A_ii), A_ij = fma(-t, I_ji, A_ij)
// A job with N[i][i] == 0 gets the row g_i = 1.  Gaussian elimination with partial pivoting (the first entry of largest
// magnitude), every update one fma - the refit's rules (ransac_refine_math.h) for n <= 32 -, back substitution from the last row
// up, j ascending.  Output: (float)g_i; if a pivot is zero or any value is not finite or <= 0, every gain of the canvas is 1.0f
// and its status is 1.
#pragma once
#include <stdint.h>

#include "warp_math.h"

namespace sift_hip {

constexpr int kOverlapMaxJobs = 32;                                   // per canvas: one row of the i8 matrix instruction each
constexpr int kOverlapPlanes = 4;                                     // N, S, SS, X
constexpr int kOverlapEntries = kOverlapMaxJobs * kOverlapMaxJobs;    // of one plane
constexpr int kOverlapStats = kOverlapPlanes * kOverlapEntries;       // int64 per canvas
constexpr int kGainStride = kOverlapMaxJobs + 1;                      // doubles in a row of [A | b]

SIFT_HD int overlap_quantize(float val, float scale) {
    const float t = __builtin_fmaf(val, scale, 0.5f);
    return t >= 255.0f ? 255 : (t >= 0.0f ? (int)t : 0);
}

// q of a COVERED pixel at source position (u, v) of image s
SIFT_HD int overlap_q(const float* s, int w, int hgt, float u, float v, float scale, int interp) {
    const WarpTaps t = warp_taps(u, v, w, hgt, interp);
    return overlap_quantize(warp_value([&](int px, int py) { return s[(size_t)py * (size_t)w + (size_t)px]; }, t, interp), scale);
}

// one canvas pixel from the definition, added to the canvas's statistics
SIFT_HD void overlap_pixel(const float* imgs, int w, int hgt, const int32_t* src, const float* models, long long j0, int n, int x, int y, int origin_x,
                           int origin_y, float scale, int interp, int64_t* stats) {
    bool c[kOverlapMaxJobs];
    int q[kOverlapMaxJobs];
    const float qx = (float)(x + origin_x), qy = (float)(y + origin_y);
    for (int i = 0; i < n; ++i) {
        const long long j = j0 + i;
        float m[9], u, v, W;
        for (int k = 0; k < 9; ++k) m[k] = models[9 * (size_t)j + k];
        c[i] = warp_coords(m, qx, qy, w, hgt, u, v, W);
        q[i] = c[i] ? overlap_q(imgs + (size_t)(src ? src[j] : j) * (size_t)w * (size_t)hgt, w, hgt, u, v, scale, interp) : 0;
    }
    for (int i = 0; i < n; ++i) {
        if (!c[i]) continue;
        for (int j = 0; j < n; ++j) {
            if (!c[j]) continue;
            const int e = i * kOverlapMaxJobs + j;
            stats[e] += 1;
            stats[kOverlapEntries + e] += q[i];
            stats[2 * kOverlapEntries + e] += q[i] * q[i];
            stats[3 * kOverlapEntries + e] += q[i] * q[j];
        }
    }
}

// ---- the gains, in steps that the kernel spreads over lanes and the host runs as the loop gain_solve ----
SIFT_HD double gain_weight(float sigma) { return 1.0 / ((double)sigma * (double)sigma); }

SIFT_HD double gain_mean(const int64_t* stats, int i, int j) {
    const int64_t nij = stats[i * kOverlapMaxJobs + j];
    return nij == 0 ? 0.0 : (double)stats[kOverlapEntries + i * kOverlapMaxJobs + j] / (double)nij;
}

// row i of [A | b]: n + 1 doubles
SIFT_HD void gain_row(const int64_t* stats, int n, int i, double alpha, double beta, double* row) {
    for (int j = 0; j <= n; ++j) row[j] = 0.0;
    if (stats[i * kOverlapMaxJobs + i] == 0) {
        row[i] = 1.0;
        row[n] = 1.0;
        return;
    }
    for (int j = 0; j < n; ++j) {
        const double nij = (double)stats[i * kOverlapMaxJobs + j];
        row[n] = __builtin_fma(beta, nij, row[n]);
        row[i] = __builtin_fma(beta, nij, row[i]);
        if (j == i) continue;
        const double iij = gain_mean(stats, i, j), iji = gain_mean(stats, j, i);
        const double t = ((2.0 * alpha) * nij) * iij;
        row[i] = __builtin_fma(t, iij, row[i]);
        row[j] = __builtin_fma(-t, iji, row[j]);
    }
}

// Step k on M (n rows of kGainStride doubles): the pivot row p = the first row i >= k with the largest |M[i][k]|; rows k and p
// change places; every row i > k becomes M[i][j] = fma(-f, M[k][j], M[i][j]) for j > k with f = M[i][k] / M[k][k].
SIFT_HD int gain_pivot(const double* M, int n, int k, bool& ok) {
    int p = k;
    double mag = __builtin_fabs(M[kGainStride * k + k]);
    for (int i = k + 1; i < n; ++i) {
        const double a = __builtin_fabs(M[kGainStride * i + k]);
        if (a > mag) {
            mag = a;
            p = i;
        }
    }
    ok = (mag - mag == 0.0) & (mag > 0.0);
    return p;
}

SIFT_HD void gain_eliminate_row(double* M, int n, int k, int i) {
    const double f = M[kGainStride * i + k] / M[kGainStride * k + k];
    for (int j = k + 1; j <= n; ++j) M[kGainStride * i + j] = __builtin_fma(-f, M[kGainStride * k + j], M[kGainStride * i + j]);
}

// x[i] = (M[i][n] - sum over j > i, ascending, of M[i][j] x[j]) / M[i][i], from the last row up
SIFT_HD void gain_backsubstitute(const double* M, int n, double* x) {
    for (int i = n - 1; i >= 0; --i) {
        double acc = M[kGainStride * i + n];
        for (int j = i + 1; j < n; ++j) acc = __builtin_fma(-M[kGainStride * i + j], x[j], acc);
        x[i] = acc / M[kGainStride * i + i];
    }
}

// the n floats and the status; `ok` false: a pivot failed
SIFT_HD int gain_finish(const double* x, bool ok, int n, float* gains) {
    for (int i = 0; i < n && ok; ++i) {
        const float g = (float)x[i];
        ok = (g - g == 0.0f) & (g > 0.0f);
    }
    for (int i = 0; i < n; ++i) gains[i] = ok ? (float)x[i] : 1.0f;
    return ok ? 0 : 1;
}

// the whole solve as one loop
inline int gain_solve(const int64_t* stats, int n, float sigma_n, float sigma_g, float* gains) {
    double M[kOverlapMaxJobs * kGainStride], x[kOverlapMaxJobs];
    const double alpha = gain_weight(sigma_n), beta = gain_weight(sigma_g);
    for (int i = 0; i < n; ++i) gain_row(stats, n, i, alpha, beta, M + kGainStride * i);
    bool ok = true;
    for (int k = 0; k < n && ok; ++k) {
        const int p = gain_pivot(M, n, k, ok);
        if (!ok) break;
        for (int j = 0; j <= n; ++j) {
            const double a = M[kGainStride * k + j];
            M[kGainStride * k + j] = M[kGainStride * p + j];
            M[kGainStride * p + j] = a;
        }
        for (int i = k + 1; i < n; ++i) gain_eliminate_row(M, n, k, i);
    }
    if (ok) gain_backsubstitute(M, n, x);
    return gain_finish(x, ok, n, gains);
}

}  // namespace sift_hip
