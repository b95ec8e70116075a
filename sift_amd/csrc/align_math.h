// Direct photometric refinement of a homography (include/sift_hip.h, "direct alignment"): THE DEFINITION, on top of warp_math.h
// and under its rules.  The HIP kernels (kernels_align.hip) and the host loop (hostmath_capi.cpp: hostmath_align_homography)
// both compile this header with -ffp-contract=off; every fused operation is an explicit fmaf / fma, every other operation is one
// rounding.  An extension: the reference has no counterpart.
//
// For a pair (Q, T) of w x h frames and a model H (query to train) the call minimises, by Gauss-Newton steps over the eight free
// entries of H, a gain a and a bias b (start: a = 1, b = 0),
//   E = sum over the contributing query pixels p of (Q(p) - a T(H p) - b)^2.
// PER PIXEL (x, y) of the query lattice:
//   map          u, v, W and the coverage test: warp_coords, unchanged
//   contributes  covered, u < w - 1 and v < h - 1 (the four bilinear taps are distinct), border <= x <= w - 1 - border, rows alike
//   sample       t = the warp's bilinear value; the train gradient is the derivative of the same patch, from the same four taps:
//                gx = fmaf(fy, (p11 - p10) - (p01 - p00), p01 - p00), gy = fmaf(fx, (p11 - p01) - (p10 - p00), p10 - p00)
//   normalised   the parameters are those of Hn = N H N^-1, N = the shift by the frame centre ((w - 1) / 2, (h - 1) / 2) and the
//                power-of-two scale s of align_norm (the refit's rule on the lattice's own spread): xn = (x - cx) s and
//                un = (u - cx) s - the scalings exact, the centre exact in float - and the normalised gradient is gx / s, exact.
//                Hn's third row applied to (xn, yn, 1) is W itself.
//   columns      A = ((a gx) / s) / W, B = ((a gy) / s) / W, D = -fmaf(A, un, B vn):
//                c0 .. c8 = A xn, A yn, A, B xn, B yn, B, D xn, D yn, D  (d(a T) / dHn_k, ALL nine entries: the solve picks the gauge)
//                c9 = t (gain), c10 = 1 (bias), c11 = r = Q(p) - fmaf(a, t, b)
// SUMS: the 78 entries i <= j of the 12 x 12 Gram matrix sum c_i c_j, entry e = align_entry(i, j); the pixel count travels as a
// 79th sum of ones in double (exact).  The order:
//   partial      a 64 x 64 tile of the query lattice is dealt to 256 partials: partial p holds column p & 63 of the tile and its
//                rows (p >> 6) + 4 k, k = 0 .. 15 ascending; it is the chain acc = fmaf(c_i, c_j, acc) from +0.0f over its
//                CONTRIBUTING pixels
//   tile         s = 0.0; s = s + (double)partial[p] for p = 0 .. 255 ascending
//   pair         tiles row-major; 256 chains, chain c = the sums of tiles c, c + 256, .. ascending from 0.0, then the refit's
//                adjacent pairwise tree (refine_tree256)
// so the bits depend on (images, model, gain, bias, border) and the tile size alone.
// ROUNDS (align_round, one call per pass k = 0 .. rounds): with n the count and q = E / n,
//   n < max(min_pixels, 1) -> status too_few; a sum not finite -> not_finite; both stop the pair with its last accepted model
//   k = 0 accepts the start (rms0); k > 0: q > the accepted q -> the step is undone, status rose, stop; else accepted, rounds += 1
//   k = rounds stops (the last pass only evaluates).  Otherwise the step, all in double: Hn from the nine floats; its first entry
//   of largest magnitude stays fixed, its row and column leave the system; the 10 x 10 system [J^T J | J^T r] with the diagonal
//   times (1 + damping); the refit's elimination (partial pivoting, first maximum, every update one fma; a zero or non-finite
//   pivot -> status singular, stop); Hn += x, a += x8, b += x9; H = N^-1 Hn N divided by its first entry of largest magnitude,
//   negated if W at the frame centre is negative; nine floats, two floats (not finite -> status not_finite, stop).
#pragma once
#include <stdint.h>

#include "../../include/sift_hip.h"
#include "ransac_refine_math.h"
#include "warp_math.h"

namespace sift_hip {

constexpr int kAlignTile = 64, kAlignLanes = 256, kAlignRows = kAlignTile * kAlignTile / kAlignLanes, kAlignRowStep = kAlignLanes / kAlignTile;
constexpr int kAlignCols = 12, kAlignSums = 78, kAlignRec = 80;   // a record of sums: 78 entries, the count, one zero
constexpr int kAlignUnknowns = 10, kAlignStride = kAlignUnknowns + 1, kAlignMaxRounds = 8;
static_assert(kAlignSums == kAlignCols * (kAlignCols + 1) / 2, "the upper triangle");

SIFT_HD constexpr int align_entry(int i, int j) { return i * kAlignCols - i * (i - 1) / 2 + (j - i); }   // i <= j

struct AlignNorm {
    float cx, cy, s, is;   // centre, scale and 1 / scale: all exact in float
};

// The lattice 0 .. w - 1 x 0 .. h - 1 has the mean squared spread d = ((w^2 - 1) + (h^2 - 1)) / 12; with (w^2 + h^2) / 12 in its
// place (> 0 for every size) the scale is the refit's: 2^-floor(e / 2), e the exponent of d.
SIFT_HD AlignNorm align_norm(int w, int h) {
    const double d = ((double)w * (double)w + (double)h * (double)h) / 12.0;
    const int64_t e = ((__builtin_bit_cast(int64_t, d) >> 52) & 0x7ff) - 1023, half = e >> 1;
    AlignNorm nm;
    nm.cx = (float)(w - 1) * 0.5f;
    nm.cy = (float)(h - 1) * 0.5f;
    nm.s = (float)__builtin_bit_cast(double, (int64_t)(1023 - half) << 52);
    nm.is = (float)__builtin_bit_cast(double, (int64_t)(1023 + half) << 52);
    return nm;
}

// does lattice pixel (x, y), inside the frame, contribute?  u, v, W as warp_coords leaves them
SIFT_HD bool align_contributes(const float (&h)[9], int x, int y, int w, int hgt, int border, float& u, float& v, float& W) {
    const bool in = warp_coords(h, (float)x, (float)y, w, hgt, u, v, W);
    return in & (u < (float)(w - 1)) & (v < (float)(hgt - 1)) & (x >= border) & (x <= w - 1 - border) & (y >= border) & (y <= hgt - 1 - border);
}

// the twelve columns of a contributing pixel from its four taps (p00 at (x0, y0), p01 at (x0 + 1, y0), p10 at (x0, y0 + 1))
SIFT_HD void align_columns(float p00, float p01, float p10, float p11, float fx, float fy, float q, float a, float b, const AlignNorm& nm, int x, int y,
                           float u, float v, float W, float (&c)[kAlignCols]) {
    const float top = __builtin_fmaf(fx, p01 - p00, p00), bot = __builtin_fmaf(fx, p11 - p10, p10);
    const float t = __builtin_fmaf(fy, bot - top, top);   // warp_value
    const float gx = __builtin_fmaf(fy, (p11 - p10) - (p01 - p00), p01 - p00);
    const float gy = __builtin_fmaf(fx, (p11 - p01) - (p10 - p00), p10 - p00);
    const float xn = ((float)x - nm.cx) * nm.s, yn = ((float)y - nm.cy) * nm.s;
    const float un = (u - nm.cx) * nm.s, vn = (v - nm.cy) * nm.s;
    const float iW = 1.0f / W;
    const float A = ((a * gx) * nm.is) * iW, B = ((a * gy) * nm.is) * iW;
    const float D = -__builtin_fmaf(A, un, B * vn);
    c[0] = A * xn;
    c[1] = A * yn;
    c[2] = A;
    c[3] = B * xn;
    c[4] = B * yn;
    c[5] = B;
    c[6] = D * xn;
    c[7] = D * yn;
    c[8] = D;
    c[9] = t;
    c[10] = 1.0f;
    c[11] = q - __builtin_fmaf(a, t, b);
}

// a pixel's columns read through px(x, y) -> the train pixel; the taps lie inside the frame for a contributing pixel
template <class Fetch>
SIFT_HD void align_pixel(const Fetch& px, float q, float a, float b, const AlignNorm& nm, int x, int y, float u, float v, float W, int w, int hgt,
                         float (&c)[kAlignCols]) {
    const WarpTaps t = warp_taps(u, v, w, hgt, 1);
    align_columns(px(t.x0, t.y0), px(t.x1, t.y0), px(t.x0, t.y1), px(t.x1, t.y1), t.fx, t.fy, q, a, b, nm, x, y, u, v, W, c);
}

// ---- the state of a pair between passes: the record the solve kernel keeps on the device ----
struct AlignState {
    float h[9], a, b;             // the model the next pass evaluates
    float acc_h[9], acc_a, acc_b; // the last accepted model
    double q_acc, q0;             // E / n of the accepted model and of the start
    int32_t pixels, rounds, status, active;
};

enum : int32_t {
    kAlignOk = SIFT_HIP_ALIGN_OK, kAlignNoModel = SIFT_HIP_ALIGN_NO_MODEL, kAlignTooFew = SIFT_HIP_ALIGN_TOO_FEW,
    kAlignNotFinite = SIFT_HIP_ALIGN_NOT_FINITE, kAlignSingular = SIFT_HIP_ALIGN_SINGULAR, kAlignRose = SIFT_HIP_ALIGN_ROSE
};

SIFT_HD void align_begin(const sift_hip_homography& m, AlignState& st) {
    for (int i = 0; i < 9; ++i) st.h[i] = st.acc_h[i] = m.h[i];
    st.a = st.acc_a = 1.0f;
    st.b = st.acc_b = 0.0f;
    st.q_acc = st.q0 = 0.0;
    st.pixels = st.rounds = 0;
    st.active = m.iteration >= 0 ? 1 : 0;
    st.status = st.active ? kAlignOk : kAlignNoModel;
}

SIFT_HD void align_result(const AlignState& st, sift_hip_alignment& r) {
    for (int i = 0; i < 9; ++i) r.h[i] = st.acc_h[i];
    r.gain = st.acc_a;
    r.bias = st.acc_b;
    r.rms0 = (float)__builtin_sqrt(st.q0);
    r.rms = (float)__builtin_sqrt(st.q_acc);
    r.pixels = st.pixels;
    r.rounds = st.rounds;
    r.status = st.status;
}

// Hn = N H N^-1: K = H N^-1 first, K[i][0] = H[i][0] / s, K[i][1] = H[i][1] / s (exact), K[i][2] = fma(H[i][0], cx, fma(H[i][1], cy,
// H[i][2])); then Hn[0][j] = fma(-cx, K[2][j], K[0][j]) s, Hn[1][j] alike with cy, Hn[2][j] = K[2][j]
SIFT_HD void align_normalise(const float (&h)[9], const AlignNorm& nm, double (&Hn)[9]) {
    const double cx = nm.cx, cy = nm.cy, s = nm.s, is = nm.is;
    double K[9];
    for (int i = 0; i < 3; ++i) {
        K[3 * i] = (double)h[3 * i] * is;
        K[3 * i + 1] = (double)h[3 * i + 1] * is;
        K[3 * i + 2] = __builtin_fma((double)h[3 * i], cx, __builtin_fma((double)h[3 * i + 1], cy, (double)h[3 * i + 2]));
    }
    for (int j = 0; j < 3; ++j) {
        Hn[j] = __builtin_fma(-cx, K[6 + j], K[j]) * s;
        Hn[3 + j] = __builtin_fma(-cy, K[6 + j], K[3 + j]) * s;
        Hn[6 + j] = K[6 + j];
    }
}

// H = N^-1 Hn N as refine_denormalise forms it (both sides share N), divided by its first entry of largest magnitude, negated if
// W at the frame centre is negative.  False (h untouched) when an entry is not finite or all are zero.
SIFT_HD bool align_denormalise(const double (&Hn)[9], const AlignNorm& nm, float (&h)[9]) {
    const double cx = nm.cx, cy = nm.cy, s = nm.s, is = nm.is;
    double G[9], H[9];
    for (int i = 0; i < 3; ++i) {
        G[3 * i] = Hn[3 * i] * s;
        G[3 * i + 1] = Hn[3 * i + 1] * s;
        G[3 * i + 2] = __builtin_fma(-G[3 * i], cx, __builtin_fma(-G[3 * i + 1], cy, Hn[3 * i + 2]));
    }
    for (int j = 0; j < 3; ++j) {
        H[j] = __builtin_fma(cx, G[6 + j], G[j] * is);
        H[3 + j] = __builtin_fma(cy, G[6 + j], G[3 + j] * is);
        H[6 + j] = G[6 + j];
    }
    bool ok = true;
    double big = H[0], mag = __builtin_fabs(H[0]);
    for (int i = 0; i < 9; ++i) {
        ok &= refine_finite(H[i]);
        const double m = __builtin_fabs(H[i]);
        const bool take = m > mag;   // the first maximum stays
        big = take ? H[i] : big;
        mag = take ? m : mag;
    }
    ok &= mag > 0.0;
    for (int i = 0; i < 9; ++i) H[i] = H[i] / big;
    const bool flip = __builtin_fma(H[6], cx, __builtin_fma(H[7], cy, H[8])) < 0.0;
    for (int i = 0; i < 9; ++i) {
        const float f = (float)(flip ? -H[i] : H[i]);
        h[i] = ok ? f : h[i];
    }
    return ok;
}

// The refit's elimination on the 10 x 11 augmented system M (any memory); the solution lands in M's last column.  False when a
// pivot is zero or not finite, or a solution is not finite.
template <typename P>
SIFT_HD bool align_solve10(P M) {
    constexpr int n = kAlignUnknowns, ld = kAlignStride;
    for (int k = 0; k < n; ++k) {
        int p = k;
        double mag = __builtin_fabs(M[ld * k + k]);
        for (int i = k + 1; i < n; ++i) {
            const double m = __builtin_fabs(M[ld * i + k]);
            const bool take = m > mag;   // the first maximum stays; a NaN is never taken, and is not replaced when it comes first
            p = take ? i : p;
            mag = take ? m : mag;
        }
        if (!(refine_finite(mag) & (mag > 0.0))) return false;
        for (int j = 0; j < ld; ++j) {
            const double t = M[ld * k + j];
            M[ld * k + j] = M[ld * p + j];
            M[ld * p + j] = t;
        }
        for (int i = k + 1; i < n; ++i) {
            const double f = M[ld * i + k] / M[ld * k + k];
            for (int j = k + 1; j < ld; ++j) M[ld * i + j] = refine_eliminate(f, M[ld * k + j], M[ld * i + j]);
        }
    }
    bool ok = true;
    for (int i = n - 1; i >= 0; --i) {
        double acc = M[ld * i + n];
        for (int j = i + 1; j < n; ++j) acc = __builtin_fma(-M[ld * i + j], M[ld * j + n], acc);
        acc = acc / M[ld * i + i];
        M[ld * i + n] = acc;
        ok &= refine_finite(acc);
    }
    return ok;
}

SIFT_HD void align_stop(AlignState& st, int32_t status) {
    for (int i = 0; i < 9; ++i) st.h[i] = st.acc_h[i];
    st.a = st.acc_a;
    st.b = st.acc_b;
    st.status = status;
    st.active = 0;
}

// Pass k of a pair whose sums S (kAlignRec doubles, any memory) were taken at st.h, st.a, st.b.  M: 110 doubles of work memory.
template <typename PS, typename PM>
SIFT_HD void align_round(AlignState& st, PS S, int k, int rounds, int min_pixels, double damping, const AlignNorm& nm, PM M) {
    const double dn = S[kAlignSums];
    bool finite = true;
    for (int e = 0; e < kAlignSums; ++e) finite &= refine_finite(S[e]);
    if (k == 0) st.pixels = (int32_t)dn;
    if (!(dn >= 1.0) | (dn < (double)min_pixels)) return align_stop(st, kAlignTooFew);
    if (!finite) return align_stop(st, kAlignNotFinite);
    const double q = S[kAlignSums - 1] / dn;
    if (k == 0) {
        st.q0 = q;
    } else if (q > st.q_acc) {
        return align_stop(st, kAlignRose);
    } else {
        st.rounds += 1;
    }
    for (int i = 0; i < 9; ++i) st.acc_h[i] = st.h[i];
    st.acc_a = st.a;
    st.acc_b = st.b;
    st.q_acc = q;
    st.pixels = (int32_t)dn;
    if (k >= rounds) return align_stop(st, kAlignOk);

    double Hn[9];
    align_normalise(st.h, nm, Hn);
    int fixed = 0;
    double mag = __builtin_fabs(Hn[0]);
    for (int i = 1; i < 9; ++i) {
        const double m = __builtin_fabs(Hn[i]);
        const bool take = m > mag;
        fixed = take ? i : fixed;
        mag = take ? m : mag;
    }
    // unknown i is column ci = i + (i >= fixed) of the eleven parameter columns (the nine entries, gain, bias)
    for (int i = 0; i < kAlignUnknowns; ++i) {
        const int ci = i + (i >= fixed ? 1 : 0);
        for (int j = 0; j <= kAlignUnknowns; ++j) {
            const int cj = j == kAlignUnknowns ? kAlignCols - 1 : j + (j >= fixed ? 1 : 0);
            const double g = S[ci <= cj ? align_entry(ci, cj) : align_entry(cj, ci)];
            M[kAlignStride * i + j] = i == j ? g * (1.0 + damping) : g;
        }
    }
    if (!align_solve10(M)) return align_stop(st, kAlignSingular);
    for (int j = 0; j < 9; ++j) {
        const int i = j - (j > fixed ? 1 : 0);
        const double x = M[kAlignStride * i + kAlignUnknowns];
        Hn[j] = j == fixed ? Hn[j] : Hn[j] + x;
    }
    const float a = (float)((double)st.a + M[kAlignStride * 8 + kAlignUnknowns]), b = (float)((double)st.b + M[kAlignStride * 9 + kAlignUnknowns]);
    float h[9];
    for (int i = 0; i < 9; ++i) h[i] = st.h[i];
    const bool ok = align_denormalise(Hn, nm, h) & (a - a == 0.0f) & (b - b == 0.0f);
    if (!ok) return align_stop(st, kAlignNotFinite);
    for (int i = 0; i < 9; ++i) st.h[i] = h[i];
    st.a = a;
    st.b = b;
}

// ---- the host's form of the sums (the kernel's: kernels_align.hip) ----
// sums[kAlignRec] of one pair at (h, a, b); work: 256 * kAlignRec doubles
inline void align_pair_sums(const float* Q, const float* T, int w, int hgt, const float (&h)[9], float a, float b, int border, const AlignNorm& nm,
                            double* work, double* sums) {
    const int tiles_x = (w + kAlignTile - 1) / kAlignTile, tiles_y = (hgt + kAlignTile - 1) / kAlignTile;
    for (int i = 0; i < kAlignLanes * kAlignRec; ++i) work[i] = 0.0;
    const auto px = [&](int xx, int yy) { return T[(size_t)yy * (size_t)w + (size_t)xx]; };
    for (int tile = 0; tile < tiles_x * tiles_y; ++tile) {
        double ts[kAlignRec];
        for (int e = 0; e < kAlignRec; ++e) ts[e] = 0.0;
        for (int p = 0; p < kAlignLanes; ++p) {
            float acc[kAlignSums];
            for (int e = 0; e < kAlignSums; ++e) acc[e] = 0.0f;
            int n = 0;
            const int x = (tile % tiles_x) * kAlignTile + (p & (kAlignTile - 1));
            for (int k = 0; k < kAlignRows; ++k) {
                const int y = (tile / tiles_x) * kAlignTile + p / kAlignTile + kAlignRowStep * k;
                float u, v, W, c[kAlignCols];
                if (x >= w || y >= hgt || !align_contributes(h, x, y, w, hgt, border, u, v, W)) continue;
                align_pixel(px, Q[(size_t)y * (size_t)w + (size_t)x], a, b, nm, x, y, u, v, W, w, hgt, c);
                for (int i = 0, e = 0; i < kAlignCols; ++i)
                    for (int j = i; j < kAlignCols; ++j, ++e) acc[e] = __builtin_fmaf(c[i], c[j], acc[e]);
                ++n;
            }
            for (int e = 0; e < kAlignSums; ++e) ts[e] = ts[e] + (double)acc[e];
            ts[kAlignSums] = ts[kAlignSums] + (double)n;
        }
        double* chain = work + (size_t)(tile % kAlignLanes) * kAlignRec;
        for (int e = 0; e < kAlignRec; ++e) chain[e] = chain[e] + ts[e];
    }
    for (int e = 0; e < kAlignRec; ++e) {
        double s[kRefineLanes];
        for (int c = 0; c < kRefineLanes; ++c) s[c] = work[(size_t)c * kAlignRec + e];
        sums[e] = refine_tree256(s);
    }
}

}  // namespace sift_hip
