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
#include "ransac_fund_refine_math.h"
#include "localize_math.h"
#include "warp_math.h"
#include "composite_math.h"
#include "overlap_math.h"
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
// Guided matching over byte rows (include/sift_hip.h, "guided matching on 8-bit descriptors"): hostmath_match_knn2_u8 with the
// condition of hostmath_match_knn2_guided - the int32 distance, the UNSPLIT predicates, the same arguments and `reverse`.
void hostmath_match_knn2_guided_u8(const uint8_t* q, const uint8_t* q_valid, const float* q_xy, long long nq, const uint8_t* t,
                                   const uint8_t* t_valid, const float* t_xy, long long nt, int model, const float* m, float threshold, int reverse,
                                   int32_t* idx, float* dist2) {
    float mm[9];
    for (int k = 0; k < 9; ++k) mm[k] = m[k];
    const float thr2 = threshold * threshold;
    const uint8_t* own = reverse ? t : q;
    const uint8_t* other = reverse ? q : t;
    const uint8_t* own_valid = reverse ? t_valid : q_valid;
    const uint8_t* other_valid = reverse ? q_valid : t_valid;
    const long long n_own = reverse ? nt : nq, n_other = reverse ? nq : nt;
    for (long long i = 0; i < n_own; ++i) {
        int32_t d1 = 0, d2 = 0, i1 = -1, i2 = -1;
        if (!own_valid || own_valid[i]) {
            for (long long j = 0; j < n_other; ++j) {
                if (other_valid && !other_valid[j]) continue;
                const long long qi = reverse ? j : i, tj = reverse ? i : j;
                const bool adm = model == 1 ? sift_hip::ransac_fund_inlier(mm, q_xy[2 * qi], q_xy[2 * qi + 1], t_xy[2 * tj], t_xy[2 * tj + 1], thr2)
                                            : sift_hip::ransac_inlier(mm, q_xy[2 * qi], q_xy[2 * qi + 1], t_xy[2 * tj], t_xy[2 * tj + 1], thr2);
                if (!adm) continue;
                int32_t d = 0;
                for (int k = 0; k < 128; ++k) {
                    const int32_t e = (int32_t)own[i * 128 + k] - (int32_t)other[j * 128 + k];
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
// The nq x nt admissibility matrix through the predicates' split parts, composed as the guided 8-bit tile kernel composes them:
// the part of the row that owns the loop once, the parts of the other side's rows once each, the tail per element.  reverse 0:
// the query rows own the loop (a forward tile); reverse 1: the train rows do (a tile of the cross-check).  out[i * nt + j] either way.
void hostmath_guided_admissible_split(int model, const float* m, float threshold, const float* q_xy, long long nq, const float* t_xy,
                                      long long nt, int reverse, uint8_t* out) {
    float mm[9];
    for (int k = 0; k < 9; ++k) mm[k] = m[k];
    const float thr2 = threshold * threshold;
    auto query_part = [&](long long i, float (&p)[4]) {
        if (model == 1) sift_hip::ransac_fund_inlier_query(mm, q_xy[2 * i], q_xy[2 * i + 1], thr2, p);
        else sift_hip::ransac_inlier_query(mm, q_xy[2 * i], q_xy[2 * i + 1], thr2, p);
    };
    auto train_part = [&](long long j, float (&p)[4]) {
        if (model == 1) sift_hip::ransac_fund_inlier_train(mm, t_xy[2 * j], t_xy[2 * j + 1], p);
        else sift_hip::ransac_inlier_train(mm, t_xy[2 * j], t_xy[2 * j + 1], p);
    };
    const long long n_own = reverse ? nt : nq, n_other = reverse ? nq : nt;
    float (*stage)[4] = new float[n_other > 0 ? n_other : 1][4];
    for (long long j = 0; j < n_other; ++j) reverse ? query_part(j, stage[j]) : train_part(j, stage[j]);
    for (long long i = 0; i < n_own; ++i) {
        float mine[4];
        reverse ? train_part(i, mine) : query_part(i, mine);
        for (long long j = 0; j < n_other; ++j) {
            const float (&qp)[4] = reverse ? stage[j] : mine;
            const float (&tp)[4] = reverse ? mine : stage[j];
            const bool ok = model == 1 ? sift_hip::ransac_fund_inlier_tail(qp, tp, thr2) : sift_hip::ransac_inlier_tail(qp, tp, thr2);
            out[reverse ? j * nt + i : i * nt + j] = ok ? 1 : 0;
        }
    }
    delete[] stage;
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

// ---- the refit of F as ransac_fund_refine_math.h defines it, in plain loops: what ransac_fund_refine_kernel must reproduce
// bit for bit.
namespace {
int fund_refine_count(const float* p, int64_t m, const float (&f)[9], float thr2) {
    int c = 0;
    for (int64_t i = 0; i < m; ++i) c += ransac_fund_inlier(f, p[4 * i], p[4 * i + 1], p[4 * i + 2], p[4 * i + 3], thr2) ? 1 : 0;
    return c;
}
// K fixed-order sums over the inliers of f (refine_fixed_sums with the epipolar predicate)
template <int K, typename Terms>
int fund_refine_fixed_sums(const float* p, int64_t m, const float (&f)[9], float thr2, Terms terms, double (&out)[K]) {
    double s[K][kRefineLanes];
    for (int k = 0; k < K; ++k)
        for (int l = 0; l < kRefineLanes; ++l) s[k][l] = 0.0;
    int n = 0;
    for (int64_t i = 0; i < m; ++i) {
        if (!ransac_fund_inlier(f, p[4 * i], p[4 * i + 1], p[4 * i + 2], p[4 * i + 3], thr2)) continue;
        double t[K];
        terms(p[4 * i], p[4 * i + 1], p[4 * i + 2], p[4 * i + 3], t);
        for (int k = 0; k < K; ++k) s[k][i % kRefineLanes] = s[k][i % kRefineLanes] + t[k];
        ++n;
    }
    for (int k = 0; k < K; ++k) out[k] = refine_tree256(s[k]);
    return n;
}
// the first two passes of a round: n, the normalisation and the 36 sums (S36[0] = n); false when the round fails there
bool fund_refine_sums36(const float* p, int64_t m, const float (&f)[9], float thr2, int& n, RefineNorm& nm, double (&S36)[36]) {
    double mom[kRefineMoments], s[kFundRefineSums];
    n = fund_refine_fixed_sums<kRefineMoments>(
        p, m, f, thr2, [](float a, float b, float c, float d, double (&t)[kRefineMoments]) { refine_moment_terms(a, b, c, d, t); }, mom);
    if (n < kFundRefineMinRows || !refine_normalisation(mom, n, nm)) return false;
    fund_refine_fixed_sums<kFundRefineSums>(
        p, m, f, thr2, [&nm](float a, float b, float c, float d, double (&t)[kFundRefineSums]) { fund_refine_terms(nm, a, b, c, d, t); }, s);
    S36[0] = (double)n;
    for (int k = 0; k < kFundRefineSums; ++k) S36[k + 1] = s[k];
    return true;
}
// one round: f -> f2; false when the round fails
bool fund_refine_round(const float* p, int64_t m, const float (&f)[9], float thr2, float (&f2)[9]) {
    double S36[36], M[72], g[8];
    RefineNorm nm;
    int n;
    if (!fund_refine_sums36(p, m, f, thr2, n, nm, S36)) return false;
    const int e = fund_refine_gauge(f, nm);
    for (int r = 0; r < 8; ++r)
        for (int c = 0; c < 9; ++c) M[9 * r + c] = fund_refine_system_entry(S36, e, r, c);
    if (!refine_solve8(M, g)) return false;
    for (int k = 0; k < 9; ++k) f2[k] = f[k];
    return fund_refine_finish(g, e, nm, f2);
}
}  // namespace

extern "C" {
// models: in-out; rounds 0 .. 8 (0 only counts the inliers of the given models); refined (may be NULL): the rounds accepted
void hostmath_refine_fundamental(const float* pts, int n_sets, const int64_t* offsets, float thr, int rounds, sift_hip_fundamental* models,
                                 int32_t* refined, uint8_t* inlier) {
    const float thr2 = thr * thr;
    if (inlier && n_sets > 0)
        for (int64_t i = 0; i < offsets[0]; ++i) inlier[i] = 0;
    for (int s = 0; s < n_sets; ++s) {
        const float* p = pts + 4 * offsets[s];
        const int64_t m = offsets[s + 1] - offsets[s];
        sift_hip_fundamental& mdl = models[s];
        int accepted = 0;
        if (mdl.iteration >= 0) {   // a model that is none is left alone
            int c = fund_refine_count(p, m, mdl.f, thr2);
            for (int r = 0; r < rounds; ++r) {
                float f2[9];
                if (!fund_refine_round(p, m, mdl.f, thr2, f2)) break;
                const int c2 = fund_refine_count(p, m, f2, thr2);
                if (c2 < c) break;
                for (int k = 0; k < 9; ++k) mdl.f[k] = f2[k];
                ++accepted;
                if (c2 == c) break;
                c = c2;
            }
            mdl.inliers = c;
        }
        if (refined) refined[s] = accepted;
        if (inlier)
            for (int64_t i = 0; i < m; ++i)
                inlier[offsets[s] + i] =
                    mdl.iteration >= 0 && ransac_fund_inlier(mdl.f, p[4 * i], p[4 * i + 1], p[4 * i + 2], p[4 * i + 3], thr2) ? 1 : 0;
    }
}
// The sums of one round over m rows under f: out[0] = n, out[1 .. 35] the 35 fixed-order sums (P-major: 6 a + b holds P[a] Q[b]);
// norm[0 .. 5] = cqx, cqy, sq, ctx, cty, st.  Returns n, or -1 - n when n < 8 or the normalisation fails (out is then untouched).
int hostmath_fund_refine_sums(const float* pts, long long m, const float* f, float thr, double* out, double* norm) {
    float ff[9];
    for (int k = 0; k < 9; ++k) ff[k] = f[k];
    double S36[36];
    RefineNorm nm;
    int n;
    if (!fund_refine_sums36(pts, m, ff, thr * thr, n, nm, S36)) return -1 - n;
    for (int k = 0; k < 36; ++k) out[k] = S36[k];
    norm[0] = nm.cqx; norm[1] = nm.cqy; norm[2] = nm.sq; norm[3] = nm.ctx; norm[4] = nm.cty; norm[5] = nm.st;
    return n;
}
}

// ---- sub-pixel localisation (localize_math.h): the plain loop ---------------------------------------------------
extern "C" {
// m points of one stack of L levels back to back (w x h each), every point inside the interior; octave and coord_scale as the
// batch call passes them (0 and 1.0f for sift_hip_localize_points)
void hostmath_localize(const float* dogs, int L, int w, int h, const uint16_t* xs, const uint16_t* ys, const uint16_t* is, int m, int max_moves,
                       int octave, float coord_scale, sift_hip_localized* out) {
    using namespace sift_hip;
    const size_t px = (size_t)w * (size_t)h;
    const auto fetch = [&](int x, int y, int i, float (&s)[27]) {
        for (int c = -1; c <= 1; ++c)
            for (int b = -1; b <= 1; ++b)
                for (int a = -1; a <= 1; ++a) s[9 * (c + 1) + 3 * (b + 1) + (a + 1)] = dogs[(size_t)(i + c) * px + (size_t)(y + b) * (size_t)w + (size_t)(x + a)];
    };
    for (int k = 0; k < m; ++k) out[k] = localize_point(fetch, w, h, L, xs[k], ys[k], is[k], max_moves, octave, coord_scale);
}
}

// ---- homography warp (warp_math.h): the plain loop ---------------------------------------------------------------
extern "C" {
// job j: image src[j] (src null: image j) of imgs (w x h each) under models[9 j ..] -> out[j] (out_h x out_w) and, unless null, mask[j]
void hostmath_warp_homography(const float* imgs, int w, int h, int n_jobs, const int32_t* src, const float* models, const sift_hip_warp_params* p,
                              float* out, uint8_t* mask) {
    using namespace sift_hip;
    const size_t px = (size_t)p->out_w * (size_t)p->out_h;
    for (int j = 0; j < n_jobs; ++j) {
        const float* s = imgs + (size_t)(src ? src[j] : j) * (size_t)w * (size_t)h;
        float m[9];
        for (int k = 0; k < 9; ++k) m[k] = models[9 * (size_t)j + k];
        for (int y = 0; y < p->out_h; ++y)
            for (int x = 0; x < p->out_w; ++x) {
                uint8_t covered;
                const size_t o = (size_t)j * px + (size_t)y * (size_t)p->out_w + (size_t)x;
                out[o] = warp_pixel(s, w, h, m, x, y, p->origin_x, p->origin_y, p->fill, p->interp, covered);
                if (mask) mask[o] = covered;
            }
    }
}
}

// ---- compositor (composite_math.h): the plain loop ---------------------------------------------------------------
extern "C" {
// canvas c: jobs offsets[c] .. offsets[c + 1] - 1 in order (job j reads image src[j]; src null: image j) -> out[c] (out_h x out_w)
// and, unless null, count[c]
void hostmath_composite_homography(const float* imgs, int w, int h, int n_canvases, const int64_t* offsets, const int32_t* src, const float* models,
                                   const sift_hip_composite_params* p, float* out, uint16_t* count) {
    using namespace sift_hip;
    const size_t px = (size_t)p->out_w * (size_t)p->out_h;
    for (int c = 0; c < n_canvases; ++c)
        for (int y = 0; y < p->out_h; ++y)
            for (int x = 0; x < p->out_w; ++x) {
                uint16_t cnt;
                const size_t o = (size_t)c * px + (size_t)y * (size_t)p->out_w + (size_t)x;
                out[o] = composite_pixel(imgs, w, h, src, models, offsets[c], offsets[c + 1], x, y, p->origin_x, p->origin_y, p->fill, p->interp, p->blend, cnt);
                if (count) count[o] = cnt;
            }
}
}

// ---- compositor with gains, overlap statistics and gains (composite_math.h, overlap_math.h): the plain loops ------------
extern "C" {
void hostmath_composite_homography_gains(const float* imgs, int w, int h, int n_canvases, const int64_t* offsets, const int32_t* src, const float* models,
                                         const sift_hip_composite_params* p, const float* gains, float* out, uint16_t* count) {
    using namespace sift_hip;
    const size_t px = (size_t)p->out_w * (size_t)p->out_h;
    for (int c = 0; c < n_canvases; ++c)
        for (int y = 0; y < p->out_h; ++y)
            for (int x = 0; x < p->out_w; ++x) {
                uint16_t cnt;
                const size_t o = (size_t)c * px + (size_t)y * (size_t)p->out_w + (size_t)x;
                out[o] = composite_pixel(imgs, w, h, src, models, offsets[c], offsets[c + 1], x, y, p->origin_x, p->origin_y, p->fill, p->interp, p->blend, cnt, gains);
                if (count) count[o] = cnt;
            }
}

// canvas c: the statistics of jobs offsets[c] .. offsets[c + 1] - 1 (at most 32) -> stats[c] (4 x 32 x 32) and, unless null,
// gains[offsets[c] ..] and status[c]
void hostmath_overlap_stats(const float* imgs, int w, int h, int n_canvases, const int64_t* offsets, const int32_t* src, const float* models,
                            const sift_hip_overlap_params* p, int64_t* stats, float* gains, uint8_t* status) {
    using namespace sift_hip;
    for (int c = 0; c < n_canvases; ++c) {
        int64_t* st = stats + (size_t)c * kOverlapStats;
        const int n = (int)(offsets[c + 1] - offsets[c]);
        for (int k = 0; k < kOverlapStats; ++k) st[k] = 0;
        for (int y = 0; y < p->out_h; ++y)
            for (int x = 0; x < p->out_w; ++x) overlap_pixel(imgs, w, h, src, models, offsets[c], n, x, y, p->origin_x, p->origin_y, p->scale, p->interp, st);
        if (gains) {
            const int bad = gain_solve(st, n, p->sigma_n, p->sigma_g, gains + offsets[c]);
            if (status) status[c] = (uint8_t)bad;
        }
    }
}
}

// ---- two-band compositor (twoband_math.h): the plain loop ----------------------------------------------------------
#include <vector>

#include "twoband_math.h"

extern "C" {
// canvas c: jobs offsets[c] .. offsets[c + 1] - 1 in order -> out[c] (out_h x out_w) and, unless null, count[c].  Job after job:
// t and m on the canvas widened by R on every side, rs and rn on the canvas widened by R above and below, then every canvas
// pixel's bands into its accumulator.  The caller keeps the header's conditions on radius and taps.
void hostmath_composite_twoband(const float* imgs, int w, int h, int n_canvases, const int64_t* offsets, const int32_t* src, const float* models,
                                const sift_hip_twoband_params* p, const float* taps, const float* gains, float* out, uint16_t* count) {
    using namespace sift_hip;
    const int R = p->radius, ow = p->out_w, oh = p->out_h, pw = ow + 2 * R, ph = oh + 2 * R;
    const size_t px = (size_t)ow * (size_t)oh;
    std::vector<float> t((size_t)pw * ph), m((size_t)pw * ph), rs((size_t)ow * ph), rn((size_t)ow * ph), wgt(px);
    std::vector<TwobandAcc> acc(px);
    for (int c = 0; c < n_canvases; ++c) {
        for (size_t o = 0; o < px; ++o) acc[o] = TwobandAcc{0.0f, 0.0f, 0.0f, 0.0f, 0u};
        for (int64_t j = offsets[c]; j < offsets[c + 1]; ++j) {
            float mdl[9];
            for (int k = 0; k < 9; ++k) mdl[k] = models[9 * (size_t)j + k];
            const float* s = imgs + (size_t)(src ? src[j] : j) * (size_t)w * (size_t)h;
            for (int y = 0; y < ph; ++y)
                for (int x = 0; x < pw; ++x) {   // the lattice point (x - R + origin_x, y - R + origin_y)
                    float val, wg;
                    const bool cov = twoband_sample(s, w, h, mdl, (float)(x - R + p->origin_x), (float)(y - R + p->origin_y), p->interp, gains ? gains + j : nullptr, val, wg);
                    t[(size_t)y * pw + x] = val;
                    m[(size_t)y * pw + x] = cov ? 1.0f : 0.0f;
                    if (x >= R && x < R + ow && y >= R && y < R + oh) wgt[(size_t)(y - R) * ow + (x - R)] = wg;
                }
            for (int y = 0; y < ph; ++y)
                for (int x = 0; x < ow; ++x) {
                    const size_t at = (size_t)y * pw + (x + R);
                    rs[(size_t)y * ow + x] = twoband_chain(taps, R, [&](int d) { return t[at + d]; });
                    rn[(size_t)y * ow + x] = twoband_chain(taps, R, [&](int d) { return m[at + d]; });
                }
            for (int y = 0; y < oh; ++y)
                for (int x = 0; x < ow; ++x) {
                    const size_t q = (size_t)(y + R) * pw + (x + R);
                    if (m[q] == 0.0f) continue;
                    const size_t at = (size_t)(y + R) * ow + x;
                    const float ls = twoband_chain(taps, R, [&](int d) { return rs[at + (ptrdiff_t)d * ow]; });
                    const float ln = twoband_chain(taps, R, [&](int d) { return rn[at + (ptrdiff_t)d * ow]; });
                    twoband_add(acc[(size_t)y * ow + x], wgt[(size_t)y * ow + x], t[q], ls, ln);
                }
        }
        for (size_t o = 0; o < px; ++o) {
            out[(size_t)c * px + o] = twoband_result(acc[o], p->fill);
            if (count) count[(size_t)c * px + o] = (uint16_t)acc[o].cnt;
        }
    }
}
}

// ---- direct alignment (align_math.h): the plain loop ---------------------------------------------------------------
#include "align_math.h"

extern "C" {
// the 80 sums of one pair (q, t) of imgs at (h, gain, bias): align_pair_sums
void hostmath_align_sums(const float* imgs, int w, int h, int q, int t, const float* model, float gain, float bias, int border, double* sums) {
    using namespace sift_hip;
    const size_t frame = (size_t)w * (size_t)h;
    std::vector<double> work((size_t)kAlignLanes * kAlignRec);
    float m[9];
    for (int k = 0; k < 9; ++k) m[k] = model[k];
    align_pair_sums(imgs + (size_t)q * frame, imgs + (size_t)t * frame, w, h, m, gain, bias, border, align_norm(w, h), work.data(), sums);
}

// sift_hip_align_homography on the host: models in and out, out and sums (may be null: n_pairs x 80 doubles of each pair's last pass)
void hostmath_align_homography(const float* imgs, int w, int h, int n_pairs, const int32_t* pair_q, const int32_t* pair_t, const sift_hip_align_params* p,
                               sift_hip_homography* models, sift_hip_alignment* out, double* sums) {
    using namespace sift_hip;
    const size_t frame = (size_t)w * (size_t)h;
    const AlignNorm nm = align_norm(w, h);
    std::vector<double> work((size_t)kAlignLanes * kAlignRec);
    for (int pair = 0; pair < n_pairs; ++pair) {
        AlignState st;
        align_begin(models[pair], st);
        double S[kAlignRec] = {0.0}, M[kAlignUnknowns * kAlignStride];
        for (int k = 0; k <= p->rounds && st.active; ++k) {
            align_pair_sums(imgs + (size_t)pair_q[pair] * frame, imgs + (size_t)pair_t[pair] * frame, w, h, st.h, st.a, st.b, p->border, nm, work.data(), S);
            align_round(st, S, k, p->rounds, p->min_pixels, (double)p->damping, nm, M);
        }
        align_result(st, out[pair]);
        for (int i = 0; i < 9; ++i) models[pair].h[i] = st.acc_h[i];
        if (sums)
            for (int e = 0; e < kAlignRec; ++e) sums[(size_t)pair * kAlignRec + e] = S[e];
    }
}
}
