// CPU build of the product's scalar math headers (the same code the HIP kernels inline), so the
// `-m "not gpu"` tests can check them against libm and against the oracle without a GPU.
// Not part of libsift_hip.so and never used by the product path.
#include <math.h>
#include <stdint.h>

#include "fdlibm_atan2f.h"
#include "grad_math.h"
#include "hist_bins.h"
#include "linalg3.h"
#include "ransac_fund_math.h"
#include "ransac_math.h"
#include "ransac_refine_math.h"
#include "../../include/sift_hip.h"   // sift_hip_homography, sift_hip_fundamental

extern "C" {
float hostmath_atan2f(float y, float x) { return sift_hip::fdlibm_atan2f(y, x); }
void hostmath_atan2f_array(const float* y, const float* x, int n, float* out) {
    for (int i = 0; i < n; ++i) out[i] = sift_hip::fdlibm_atan2f(y[i], x[i]);
}
// the GPU's branch-free common path + fallback; also reports how many inputs took the common path
int hostmath_atan2f_sel_array(const float* y, const float* x, int n, float* out) {
    int common = 0;
    for (int i = 0; i < n; ++i) {
        float r;
        common += sift_hip::fdlibm_atan2f_common(y[i], x[i], r) ? 1 : 0;
        out[i] = sift_hip::fdlibm_atan2f_sel(y[i], x[i]);
    }
    return common;
}
// alg::gradientMagnitude as the gradient kernels compute it (grad_math.h); returns how many inputs took the exact routine
long long hostmath_magnitude_array(const float* dx, const float* dy, long long n, float* out) {
    long long slow = 0;
    for (long long i = 0; i < n; ++i) {
        out[i] = sift_hip::gradient_magnitude(dx[i], dy[i]);
    }
    return slow;
}
// a / b as the atan2f restatement divides (fdlibm_atan2f.h: div_in_range); mismatches against the compiler's division
long long hostmath_div_mismatches(const float* a, const float* b, long long n) {
    long long bad = 0;
    for (long long i = 0; i < n; ++i) {
        const float q = sift_hip::div_in_range(a[i], b[i]), w = a[i] / b[i];
        bad += sift_hip::f2i(q) != sift_hip::f2i(w) ? 1 : 0;
    }
    return bad;
}
// matrices row-fastest like vigra::Matrix: a[i + 3*j] = A(i, j)
int hostmath_inverse3(const float* a, float* res) {
    float A[3][3], R[3][3] = {};
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) A[i][j] = a[i + 3 * j];
    const bool ok = sift_hip::inverse3(A, R);
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) res[i + 3 * j] = R[i][j];
    return ok ? 1 : 0;
}
int hostmath_solve3(const float* a, const float* b, float* res) {
    float A[3][3], B[3] = {b[0], b[1], b[2]}, R[3] = {0, 0, 0};
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) A[i][j] = a[i + 3 * j];
    const bool ok = sift_hip::solve3<true>(A, B, R);
    res[0] = R[0]; res[1] = R[1]; res[2] = R[2];
    return ok ? 1 : 0;
}
// inputs with bit patterns first .. first + count - 1 whose fast bin differs from the division's; *example = one of them
long long hostmath_hist8_bin_mismatches(unsigned long long first, unsigned long long count, unsigned* example) {
    long long bad = 0;
    for (unsigned long long i = first; i < first + count; ++i) {
        const float v = sift_hip::i2f((int32_t)(uint32_t)i);
        if (sift_hip::hist8_bin(v) != sift_hip::hist8_bin_div(v)) {
            ++bad;
            if (example) *example = (uint32_t)i;
        }
    }
    return bad;
}
float hostmath_vertex_parabola(uint16_t lnx, float lny, uint16_t px, float py, uint16_t rnx, float rny) {
    return sift_hip::vertex_parabola(lnx, lny, px, py, rnx, rny);
}
// Descriptor matching as include/sift_hip.h defines it, in plain loops: what the GPU matcher must reproduce bit for bit.
// q: nq x 128, t: nt x 128, q_valid / t_valid: one byte per row or NULL (all valid); idx: nq x 2, dist2: nq x 2.
static float match_dot(const float* a, const float* b) {
    float acc = 0.0f;
    for (int k = 0; k < 128; ++k) acc = fmaf(a[k], b[k], acc);
    return acc;
}
void hostmath_match_knn2(const float* q, const uint8_t* q_valid, long long nq, const float* t, const uint8_t* t_valid, long long nt,
                         int32_t* idx, float* dist2) {
    float* tn = new float[nt > 0 ? nt : 1];
    for (long long j = 0; j < nt; ++j) tn[j] = match_dot(t + j * 128, t + j * 128);
    for (long long i = 0; i < nq; ++i) {
        float d1 = INFINITY, d2 = INFINITY;
        int32_t i1 = -1, i2 = -1;
        if (!q_valid || q_valid[i]) {
            const float na = match_dot(q + i * 128, q + i * 128);
            for (long long j = 0; j < nt; ++j) {   // j ascending: a later row replaces an earlier one only when strictly nearer
                if (t_valid && !t_valid[j]) continue;
                const float s = na + tn[j];
                const float v = s - 2.0f * match_dot(q + i * 128, t + j * 128);
                const float d = (v < 0.0f) ? 0.0f : v;
                if (d != d) continue;
                if (i1 < 0 || d < d1) {
                    d2 = d1; i2 = i1; d1 = d; i1 = (int32_t)j;
                } else if (i2 < 0 || d < d2) {
                    d2 = d; i2 = (int32_t)j;
                }
            }
        }
        idx[2 * i] = i1; idx[2 * i + 1] = i2;
        dist2[2 * i] = d1; dist2[2 * i + 1] = d2;
    }
    delete[] tn;
}
// Guided matching as include/sift_hip.h defines it, in plain loops: hostmath_match_knn2 with one more condition on a candidate,
// the verification's predicate under the model m (nine floats; model 0: ransac_inlier, 1: ransac_fund_inlier) between the query
// row's point and the train row's.  q_xy / t_xy: two floats per row.  reverse 0: idx / dist2 are nq x 2, the top-2 train rows of
// every query row.  reverse 1: they are nt x 2, the top-2 QUERY rows of every train row under the same predicate with the same
// arguments - the cross-check's reverse best.
void hostmath_match_knn2_guided(const float* q, const uint8_t* q_valid, const float* q_xy, long long nq, const float* t, const uint8_t* t_valid,
                                const float* t_xy, long long nt, int model, const float* m, float threshold, int reverse, int32_t* idx,
                                float* dist2) {
    float mm[9];
    for (int k = 0; k < 9; ++k) mm[k] = m[k];
    const float thr2 = threshold * threshold;
    const float* own = reverse ? t : q;                 // the rows that get an entry, and the rows they choose among
    const float* other = reverse ? q : t;
    const uint8_t* own_valid = reverse ? t_valid : q_valid;
    const uint8_t* other_valid = reverse ? q_valid : t_valid;
    const long long n_own = reverse ? nt : nq, n_other = reverse ? nq : nt;
    float* on = new float[n_other > 0 ? n_other : 1];
    for (long long j = 0; j < n_other; ++j) on[j] = match_dot(other + j * 128, other + j * 128);
    for (long long i = 0; i < n_own; ++i) {
        float d1 = INFINITY, d2 = INFINITY;
        int32_t i1 = -1, i2 = -1;
        if (!own_valid || own_valid[i]) {
            const float na = match_dot(own + i * 128, own + i * 128);
            for (long long j = 0; j < n_other; ++j) {
                if (other_valid && !other_valid[j]) continue;
                const long long qi = reverse ? j : i, tj = reverse ? i : j;
                const bool adm = model == 1 ? sift_hip::ransac_fund_inlier(mm, q_xy[2 * qi], q_xy[2 * qi + 1], t_xy[2 * tj], t_xy[2 * tj + 1], thr2)
                                            : sift_hip::ransac_inlier(mm, q_xy[2 * qi], q_xy[2 * qi + 1], t_xy[2 * tj], t_xy[2 * tj + 1], thr2);
                if (!adm) continue;
                const float s = na + on[j];
                const float v = s - 2.0f * match_dot(own + i * 128, other + j * 128);
                const float d = (v < 0.0f) ? 0.0f : v;
                if (d != d) continue;
                if (i1 < 0 || d < d1) {
                    d2 = d1; i2 = i1; d1 = d; i1 = (int32_t)j;
                } else if (i2 < 0 || d < d2) {
                    d2 = d; i2 = (int32_t)j;
                }
            }
        }
        idx[2 * i] = i1; idx[2 * i + 1] = i2;
        dist2[2 * i] = d1; dist2[2 * i + 1] = d2;
    }
    delete[] on;
}
// 8-bit descriptors as include/sift_hip.h defines them ("8-bit descriptors and integer matching"): the quantiser, and
// hostmath_match_knn2 over byte rows - d2 = sum (a[k] - b[k])^2 in int32, the same order rule, (float)d2 out.
void hostmath_quantize(const float* desc, long long rows, uint8_t* out) {
    for (long long i = 0; i < rows * 128; ++i) {
        const float t = fmaf(desc[i], 255.0f, 0.5f);
        out[i] = t >= 255.0f ? (uint8_t)255 : (t >= 0.0f ? (uint8_t)(int)t : (uint8_t)0);
    }
}
void hostmath_match_knn2_u8(const uint8_t* q, const uint8_t* q_valid, long long nq, const uint8_t* t, const uint8_t* t_valid, long long nt,
                            int32_t* idx, float* dist2) {
    for (long long i = 0; i < nq; ++i) {
        int32_t d1 = 0, d2 = 0, i1 = -1, i2 = -1;
        if (!q_valid || q_valid[i]) {
            for (long long j = 0; j < nt; ++j) {   // j ascending: a later row replaces an earlier one only when strictly nearer
                if (t_valid && !t_valid[j]) continue;
                int32_t d = 0;
                for (int k = 0; k < 128; ++k) {
                    const int32_t e = (int32_t)q[i * 128 + k] - (int32_t)t[j * 128 + k];
                    d += e * e;
                }
                if (i1 < 0 || d < d1) {
                    d2 = d1; i2 = i1; d1 = d; i1 = (int32_t)j;
                } else if (i2 < 0 || d < d2) {
                    d2 = d; i2 = (int32_t)j;
                }
            }
        }
        idx[2 * i] = i1; idx[2 * i + 1] = i2;
        dist2[2 * i] = i1 < 0 ? INFINITY : (float)d1;
        dist2[2 * i + 1] = i2 < 0 ? INFINITY : (float)d2;
    }
}
// RANSAC homography as ransac_math.h defines it, in plain loops: what sift_hip_ransac_homography must reproduce bit for bit.
void hostmath_ransac_draw(uint32_t seed, uint32_t set, uint32_t iteration, uint32_t m, uint32_t* idx) {
    uint32_t d[4];
    sift_hip::ransac_draw(seed, set, iteration, m, d);
    for (int k = 0; k < 4; ++k) idx[k] = d[k];
}
// c: four rows (qx, qy, tx, ty); h: nine floats; returns 1 when the sample gives a model
int hostmath_homography4(const float* c, float* h) {
    float cc[4][4], hh[9];
    for (int k = 0; k < 16; ++k) cc[k / 4][k % 4] = c[k];
    const bool ok = sift_hip::ransac_homography4(cc, hh);
    for (int k = 0; k < 9; ++k) h[k] = hh[k];
    return ok ? 1 : 0;
}
int hostmath_ransac_inlier(const float* h, const float* row, float thr) {
    float hh[9];
    for (int k = 0; k < 9; ++k) hh[k] = h[k];
    return sift_hip::ransac_inlier(hh, row[0], row[1], row[2], row[3], thr * thr) ? 1 : 0;
}
// pts: rows of four floats, set s = rows offsets[s] .. offsets[s+1] - 1; inlier (one byte per row) and scores (n_sets x
// iterations) may be NULL
void hostmath_ransac_homography(const float* pts, int n_sets, const int64_t* offsets, uint32_t iterations, uint32_t seed, float thr,
                                sift_hip_homography* models, uint8_t* inlier, int32_t* scores) {
    const float thr2 = thr * thr;
    if (inlier && n_sets > 0)
        for (int64_t i = 0; i < offsets[0]; ++i) inlier[i] = 0;   // rows in front of the first set belong to none
    for (int s = 0; s < n_sets; ++s) {
        const float* p = pts + 4 * offsets[s];
        const int64_t m = offsets[s + 1] - offsets[s];
        sift_hip_homography best{};
        best.iteration = -1;
        int32_t best_score = -1;
        for (uint32_t it = 0; it < iterations; ++it) {
            int32_t score = -1;
            float h[9] = {};
            if (m >= 4) {
                uint32_t d[4];
                float c[4][4];
                sift_hip::ransac_draw(seed, (uint32_t)s, it, (uint32_t)m, d);
                for (int k = 0; k < 4; ++k)
                    for (int e = 0; e < 4; ++e) c[k][e] = p[4 * (int64_t)d[k] + e];
                if (sift_hip::ransac_homography4(c, h)) {
                    score = 0;
                    for (int64_t i = 0; i < m; ++i) score += sift_hip::ransac_inlier(h, p[4 * i], p[4 * i + 1], p[4 * i + 2], p[4 * i + 3], thr2) ? 1 : 0;
                }
            }
            if (scores) scores[(int64_t)s * iterations + it] = score;
            if (score > best_score) {   // strictly: the lowest iteration keeps a tie
                best_score = score;
                for (int k = 0; k < 9; ++k) best.h[k] = h[k];
                best.inliers = score;
                best.iteration = (int32_t)it;
            }
        }
        models[s] = best;
        if (inlier)
            for (int64_t i = 0; i < m; ++i)
                inlier[offsets[s] + i] = best.iteration >= 0 && sift_hip::ransac_inlier(best.h, p[4 * i], p[4 * i + 1], p[4 * i + 2], p[4 * i + 3], thr2) ? 1 : 0;
    }
}

}  // extern "C"

// ---- the refinement as ransac_refine_math.h defines it, in plain loops: what ransac_refine_kernel must reproduce bit for bit.
namespace {
using namespace sift_hip;
int refine_count(const float* p, int64_t m, const float (&h)[9], float thr2) {
    int c = 0;
    for (int64_t i = 0; i < m; ++i) c += ransac_inlier(h, p[4 * i], p[4 * i + 1], p[4 * i + 2], p[4 * i + 3], thr2) ? 1 : 0;
    return c;
}
// K fixed-order sums over the inliers of h: 256 strided partials from +0.0, rows ascending, then the adjacent tree
template <int K, typename Terms>
int refine_fixed_sums(const float* p, int64_t m, const float (&h)[9], float thr2, Terms terms, double (&out)[K]) {
    double s[K][kRefineLanes];
    for (int k = 0; k < K; ++k)
        for (int l = 0; l < kRefineLanes; ++l) s[k][l] = 0.0;
    int n = 0;
    for (int64_t i = 0; i < m; ++i) {
        if (!ransac_inlier(h, p[4 * i], p[4 * i + 1], p[4 * i + 2], p[4 * i + 3], thr2)) continue;
        double t[K];
        terms(p[4 * i], p[4 * i + 1], p[4 * i + 2], p[4 * i + 3], t);
        for (int k = 0; k < K; ++k) s[k][i % kRefineLanes] = s[k][i % kRefineLanes] + t[k];
        ++n;
    }
    for (int k = 0; k < K; ++k) out[k] = refine_tree256(s[k]);
    return n;
}
int refine_moments(const float* p, int64_t m, const float (&h)[9], float thr2, double (&mom)[kRefineMoments]) {
    return refine_fixed_sums<kRefineMoments>(
        p, m, h, thr2, [](float a, float b, float c, float d, double (&t)[kRefineMoments]) { refine_moment_terms(a, b, c, d, t); }, mom);
}
void refine_normal_sums(const float* p, int64_t m, const float (&h)[9], float thr2, const RefineNorm& nm, double (&s)[kRefineSums]) {
    refine_fixed_sums<kRefineSums>(
        p, m, h, thr2, [&nm](float a, float b, float c, float d, double (&t)[kRefineSums]) { refine_normal_terms(nm, a, b, c, d, t); }, s);
}
// one round: h -> h2; false when the round fails.  n = the inliers of h (its score).
bool refine_round(const float* p, int64_t m, const float (&h)[9], float thr2, float (&h2)[9], int& n) {
    double mom[kRefineMoments], s[kRefineSums], M[72], x[8];
    RefineNorm nm;
    n = refine_moments(p, m, h, thr2, mom);
    if (n < 4 || !refine_normalisation(mom, n, nm)) return false;
    refine_normal_sums(p, m, h, thr2, nm, s);
    refine_system(s, n, M);
    if (!refine_solve8(M, x)) return false;
    for (int k = 0; k < 9; ++k) h2[k] = h[k];
    return refine_denormalise(x, nm, h2);
}
// all rounds of one set: the model in place, its inlier count and the rounds accepted
void refine_set(const float* p, int64_t m, float thr2, int rounds, float (&h)[9], int32_t& inliers, int32_t& refined) {
    refined = 0;
    int c = refine_count(p, m, h, thr2);
    for (int r = 0; r < rounds; ++r) {
        float h2[9];
        int n;
        if (!refine_round(p, m, h, thr2, h2, n)) break;   // n == c: the score is the inlier count
        const int c2 = refine_count(p, m, h2, thr2);
        if (c2 < c) break;
        for (int k = 0; k < 9; ++k) h[k] = h2[k];
        ++refined;
        if (c2 == c) break;
        c = c2;
    }
    inliers = c;
}
void refine_models(const float* pts, int n_sets, const int64_t* offsets, float thr, int rounds, sift_hip_homography* models, uint8_t* inlier) {
    const float thr2 = thr * thr;
    if (inlier && n_sets > 0)
        for (int64_t i = 0; i < offsets[0]; ++i) inlier[i] = 0;
    for (int s = 0; s < n_sets; ++s) {
        const float* p = pts + 4 * offsets[s];
        const int64_t m = offsets[s + 1] - offsets[s];
        sift_hip_homography& mdl = models[s];
        if (mdl.iteration >= 0) refine_set(p, m, thr2, rounds, mdl.h, mdl.inliers, mdl.refined);   // a model that is none is left alone
        if (inlier)
            for (int64_t i = 0; i < m; ++i)
                inlier[offsets[s] + i] = mdl.iteration >= 0 && ransac_inlier(mdl.h, p[4 * i], p[4 * i + 1], p[4 * i + 2], p[4 * i + 3], thr2) ? 1 : 0;
    }
}
}  // namespace

extern "C" {
// models: in-out; rounds 0 .. 8 (0 only counts the inliers of the given models)
void hostmath_refine_homography(const float* pts, int n_sets, const int64_t* offsets, float thr, int rounds, sift_hip_homography* models,
                                uint8_t* inlier) {
    refine_models(pts, n_sets, offsets, thr, rounds, models, inlier);
}
// hostmath_ransac_homography followed by `refine` rounds on every winner; refine 0 is hostmath_ransac_homography itself
void hostmath_ransac_homography_refined(const float* pts, int n_sets, const int64_t* offsets, uint32_t iterations, uint32_t seed, float thr,
                                        sift_hip_homography* models, uint8_t* inlier, int32_t* scores, int refine) {
    hostmath_ransac_homography(pts, n_sets, offsets, iterations, seed, thr, models, inlier, scores);
    if (refine > 0) refine_models(pts, n_sets, offsets, thr, refine, models, inlier);
}
// The sums of one round over m rows under h: out[0 .. 5] the moments, out[6 .. 27] the normal sums.  Returns n, the number of
// inliers, or -1 - n when n < 4 or the normalisation fails (out[6 ..] is then untouched).
int hostmath_refine_sums(const float* pts, long long m, const float* h, float thr, double* out) {
    float hh[9];
    for (int k = 0; k < 9; ++k) hh[k] = h[k];
    double mom[kRefineMoments], s[kRefineSums];
    RefineNorm nm;
    const int n = refine_moments(pts, m, hh, thr * thr, mom);
    for (int k = 0; k < kRefineMoments; ++k) out[k] = mom[k];
    if (n < 4 || !refine_normalisation(mom, n, nm)) return -1 - n;
    refine_normal_sums(pts, m, hh, thr * thr, nm, s);
    for (int k = 0; k < kRefineSums; ++k) out[kRefineMoments + k] = s[k];
    return n;
}
// the centroids and scales of hostmath_refine_sums' normalisation: cqx, cqy, sq, ctx, cty, st; returns 1 when it exists
int hostmath_refine_normalisation(const double* mom, int n, double* out) {
    double mm[kRefineMoments];
    for (int k = 0; k < kRefineMoments; ++k) mm[k] = mom[k];
    RefineNorm nm;
    const bool ok = refine_normalisation(mm, n, nm);
    out[0] = nm.cqx; out[1] = nm.cqy; out[2] = nm.sq; out[3] = nm.ctx; out[4] = nm.cty; out[5] = nm.st;
    return ok ? 1 : 0;
}
// a: 8 x 8 row-major, b: 8 -> x: 8; returns 1 when the elimination finds eight pivots and a finite solution
int hostmath_solve8(const double* a, const double* b, double* x) {
    double M[72], xx[8] = {};
    for (int i = 0; i < 8; ++i) {
        for (int j = 0; j < 8; ++j) M[9 * i + j] = a[8 * i + j];
        M[9 * i + 8] = b[i];
    }
    const bool ok = refine_solve8(M, xx);
    for (int i = 0; i < 8; ++i) x[i] = xx[i];
    return ok ? 1 : 0;
}
}

// ---- RANSAC fundamental matrix as ransac_fund_math.h defines it, in plain loops: what sift_hip_ransac_fundamental must
// reproduce bit for bit.
extern "C" {
void hostmath_ransac_draw7(uint32_t seed, uint32_t set, uint32_t iteration, uint32_t m, uint32_t* idx) {
    uint32_t d[7];
    sift_hip::ransac_draw7(seed, set, iteration, m, d);
    for (int k = 0; k < 7; ++k) idx[k] = d[k];
}
// c: seven rows (qx, qy, tx, ty); f: 3 x 9 floats; returns the mask of valid slots
int hostmath_fundamental7(const float* c, float* f) {
    float cc[7][4], ff[3][9];
    for (int k = 0; k < 28; ++k) cc[k / 4][k % 4] = c[k];
    const uint32_t mask = sift_hip::ransac_fundamental7(cc, ff);
    for (int k = 0; k < 27; ++k) f[k] = ff[k / 9][k % 9];
    return (int)mask;
}
int hostmath_fund_inlier(const float* f, const float* row, float thr) {
    float ff[9];
    for (int k = 0; k < 9; ++k) ff[k] = f[k];
    return sift_hip::ransac_fund_inlier(ff, row[0], row[1], row[2], row[3], thr * thr) ? 1 : 0;
}
// pts, offsets, inlier as for hostmath_ransac_homography; scores (may be NULL): n_sets x 3 * iterations
void hostmath_ransac_fundamental(const float* pts, int n_sets, const int64_t* offsets, uint32_t iterations, uint32_t seed, float thr,
                                 sift_hip_fundamental* models, uint8_t* inlier, int32_t* scores) {
    const float thr2 = thr * thr;
    if (inlier && n_sets > 0)
        for (int64_t i = 0; i < offsets[0]; ++i) inlier[i] = 0;   // rows in front of the first set belong to none
    for (int s = 0; s < n_sets; ++s) {
        const float* p = pts + 4 * offsets[s];
        const int64_t m = offsets[s + 1] - offsets[s];
        sift_hip_fundamental best{};
        best.iteration = -1;
        best.root = -1;
        int32_t best_score = -1;
        for (uint32_t it = 0; it < iterations; ++it) {
            float f[3][9] = {};
            uint32_t mask = 0;
            if (m >= 7) {
                uint32_t d[7];
                float c[7][4];
                sift_hip::ransac_draw7(seed, (uint32_t)s, it, (uint32_t)m, d);
                for (int k = 0; k < 7; ++k)
                    for (int e = 0; e < 4; ++e) c[k][e] = p[4 * (int64_t)d[k] + e];
                mask = sift_hip::ransac_fundamental7(c, f);
            }
            for (int k = 0; k < 3; ++k) {
                int32_t score = -1;
                if ((mask >> k) & 1u) {
                    score = 0;
                    for (int64_t i = 0; i < m; ++i)
                        score += sift_hip::ransac_fund_inlier(f[k], p[4 * i], p[4 * i + 1], p[4 * i + 2], p[4 * i + 3], thr2) ? 1 : 0;
                }
                if (scores) scores[((int64_t)s * iterations + it) * 3 + k] = score;
                if (score > best_score) {   // strictly: the lowest slot keeps a tie
                    best_score = score;
                    for (int j = 0; j < 9; ++j) best.f[j] = f[k][j];
                    best.inliers = score;
                    best.iteration = (int32_t)it;
                    best.root = k;
                }
            }
        }
        models[s] = best;
        if (inlier)
            for (int64_t i = 0; i < m; ++i)
                inlier[offsets[s] + i] =
                    best.iteration >= 0 && sift_hip::ransac_fund_inlier(best.f, p[4 * i], p[4 * i + 1], p[4 * i + 2], p[4 * i + 3], thr2) ? 1 : 0;
    }
}
}
