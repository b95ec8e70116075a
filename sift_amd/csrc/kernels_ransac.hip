// RANSAC homography over match lists (include/sift_hip.h, "geometric verification").  The arithmetic is ransac_math.h, compiled
// here and by the host checker alike; the kernels only decide who computes what.  No MFMA, no atomics with a return value, and
// every count is an integer, so no launch shape or tiling can show in the result.
//
// Scoring is the hot loop: n_sets x iterations x m predicates of 14 float operations.  Lane = hypothesis: a workgroup holds 256
// models in nine VGPRs a lane and up to kRansacRows rows of its set in LDS as 16-byte rows; all lanes read the same row (one
// ds_read_b128 whose 64 addresses are equal: a broadcast, no bank conflict), the count stays in a register and leaves the lane
// once, as an integer add to the hypothesis' score.  The other layout (lane = row, the model wave-uniform, ballot + popcount per
// 64 rows) issues the same vector operations per predicate but pays a cross-lane step per hypothesis and wastes lanes on the
// short lists (a few hundred rows) that a ratio test leaves; this one wastes lanes only below 256 iterations.
#include "ransac_kernels.h"
#include "ransac_fund_math.h"
#include "ransac_math.h"
#include "ransac_refine_math.h"

namespace sift_hip {

namespace {
typedef float f4v __attribute__((ext_vector_type(4)));

// the set of a row: the first s with off[s + 1] > row (sets may be empty); row >= off[0] and row < off[n_sets]
__device__ __forceinline__ int set_of_row(const int64_t* __restrict__ off, int n_sets, long long row) {
    int lo = 0, hi = n_sets - 1;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (off[mid + 1] <= row) lo = mid + 1; else hi = mid;
    }
    return lo;
}
}  // namespace

// What the scoring, selection and flag kernels need to know of a model: its record, its predicate, and how many hypothesis
// slots a sample yields.  The nine floats mean nothing to those kernels.
struct HomographyModel {
    typedef sift_hip_homography Rec;
    static constexpr int kSlots = 1;
    static __device__ __forceinline__ const float* coef(const Rec* r) { return r->h; }
    static __device__ __forceinline__ float* coef(Rec* r) { return r->h; }
    static __device__ __forceinline__ bool inlier(const float (&h)[9], float qx, float qy, float tx, float ty, float thr2) {
        return ransac_inlier(h, qx, qy, tx, ty, thr2);
    }
    // the record's last field: refinement rounds
    static __device__ __forceinline__ void finish(Rec* r, bool any, int win) { r->iteration = any ? win : -1; r->refined = 0; }
};
struct FundamentalModel {
    typedef sift_hip_fundamental Rec;
    static constexpr int kSlots = 3;
    static __device__ __forceinline__ const float* coef(const Rec* r) { return r->f; }
    static __device__ __forceinline__ float* coef(Rec* r) { return r->f; }
    static __device__ __forceinline__ bool inlier(const float (&f)[9], float qx, float qy, float tx, float ty, float thr2) {
        return ransac_fund_inlier(f, qx, qy, tx, ty, thr2);
    }
    // slot 3 * iteration + root
    static __device__ __forceinline__ void finish(Rec* r, bool any, int win) { r->iteration = any ? win / 3 : -1; r->root = any ? win % 3 : -1; }
};

// one lane per (set, iteration): draw, gather four rows, solve in double
__global__ __launch_bounds__(256) void ransac_hypothesis_kernel(const float* __restrict__ pts, const int64_t* __restrict__ off, int n_sets,
                                                                uint32_t iterations, uint32_t seed, RansacHyp* __restrict__ hyp) {
    const long long gid = (long long)blockIdx.x * 256 + threadIdx.x;
    if (gid >= (long long)n_sets * iterations) return;
    const int set = (int)(gid / iterations);
    const uint32_t it = (uint32_t)(gid % iterations);
    const int64_t row0 = off[set], m = off[set + 1] - row0;
    RansacHyp out;
    for (int k = 0; k < 9; ++k) out.h[k] = 0.0f;
    out.valid = 0;
    if (m >= 4) {
        uint32_t d[4];
        float c[4][4];
        ransac_draw(seed, (uint32_t)set, it, (uint32_t)m, d);
        for (int k = 0; k < 4; ++k) {
            const f4v r = *reinterpret_cast<const f4v*>(pts + 4 * (row0 + (int64_t)d[k]));
            c[k][0] = r.x; c[k][1] = r.y; c[k][2] = r.z; c[k][3] = r.w;
        }
        out.valid = ransac_homography4(c, out.h) ? 1 : 0;
    }
    hyp[gid] = out;
}

// One lane per (set, sample): draw, gather seven rows, solve in double, three records (slot 3 * sample + root).  The 7 x 9
// doubles of the elimination live in registers (ransac_fund_math.h indexes them by select chains), which is what the launch
// bound is sized for.
__global__ __launch_bounds__(kFundLanes) void ransac_fund_hypothesis_kernel(const float* __restrict__ pts, const int64_t* __restrict__ off, int n_sets,
                                                                            uint32_t iterations, uint32_t seed, RansacHyp* __restrict__ hyp) {
    const long long gid = (long long)blockIdx.x * kFundLanes + threadIdx.x;
    if (gid >= (long long)n_sets * iterations) return;
    const int set = (int)(gid / iterations);
    const uint32_t it = (uint32_t)(gid % iterations);
    const int64_t row0 = off[set], m = off[set + 1] - row0;
    float f[3][9];
    uint32_t mask = 0;
#pragma unroll
    for (int k = 0; k < 3; ++k)
#pragma unroll
        for (int j = 0; j < 9; ++j) f[k][j] = 0.0f;
    if (m >= 7) {
        uint32_t d[7];
        float c[7][4];
        ransac_draw7(seed, (uint32_t)set, it, (uint32_t)m, d);
#pragma unroll
        for (int k = 0; k < 7; ++k) {
            const f4v r = *reinterpret_cast<const f4v*>(pts + 4 * (row0 + (int64_t)d[k]));
            c[k][0] = r.x; c[k][1] = r.y; c[k][2] = r.z; c[k][3] = r.w;
        }
        mask = ransac_fundamental7(c, f);
    }
    RansacHyp* out = hyp + 3 * (size_t)gid;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
#pragma unroll
        for (int j = 0; j < 9; ++j) out[k].h[j] = f[k][j];
        out[k].valid = (int32_t)((mask >> k) & 1u);
    }
}

// `slots`: hypothesis slots per set (iterations x the model's slots per sample)
template <typename Model>
__global__ __launch_bounds__(kRansacHyps) void ransac_score_kernel(const float* __restrict__ pts, const RansacHyp* __restrict__ hyp,
                                                                   const RansacTile* __restrict__ tiles, uint32_t slots, float thr2,
                                                                   int32_t* __restrict__ scores) {
    __shared__ __attribute__((aligned(16))) f4v rows[kRansacRows];
    const RansacTile t = tiles[blockIdx.x];
    const int n = t.row_hi - t.row_lo;   // <= kRansacRows
    for (int i = threadIdx.x; i < n; i += kRansacHyps) rows[i] = *reinterpret_cast<const f4v*>(pts + 4 * ((size_t)t.row_lo + i));
    __syncthreads();
    const uint32_t it = (uint32_t)t.hyp0 + threadIdx.x;
    if (it >= slots) return;
    const size_t slot = (size_t)t.set * slots + it;
    const RansacHyp me = hyp[slot];
    if (!me.valid) return;
    int count = 0;
#pragma unroll 8
    for (int i = 0; i < n; ++i) {
        const f4v r = rows[i];
        count += Model::inlier(me.h, r.x, r.y, r.z, r.w, thr2) ? 1 : 0;
    }
    if (count) atomicAdd(&scores[slot], count);   // the result is not used: an add without return
}

// one workgroup per set: -1 into the scores of invalid hypotheses, the argmax under (score descending, slot ascending)
template <typename Model>
__global__ __launch_bounds__(256) void ransac_select_kernel(const RansacHyp* __restrict__ hyp, uint32_t iterations, int32_t* __restrict__ scores,
                                                            typename Model::Rec* __restrict__ models) {
    __shared__ int s_score[256];
    __shared__ int s_iter[256];
    const int tid = threadIdx.x;
    const size_t base = (size_t)blockIdx.x * iterations;
    int best = -1, best_it = 0x7fffffff;
    for (uint32_t i = tid; i < iterations; i += 256) {   // ascending: a later iteration replaces only when strictly better
        const int s = hyp[base + i].valid ? scores[base + i] : -1;
        scores[base + i] = s;
        if (s > best) { best = s; best_it = (int)i; }
    }
    s_score[tid] = best;
    s_iter[tid] = best_it;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if (tid < w) {
            const int os = s_score[tid + w], oi = s_iter[tid + w];
            if (os > s_score[tid] || (os == s_score[tid] && oi < s_iter[tid])) { s_score[tid] = os; s_iter[tid] = oi; }
        }
        __syncthreads();
    }
    const bool any = s_score[0] >= 0;
    const int win = s_iter[0];
    typename Model::Rec* out = models + blockIdx.x;
    if (tid < 9) Model::coef(out)[tid] = any ? hyp[base + win].h[tid] : 0.0f;
    if (tid == 9) out->inliers = any ? s_score[0] : 0;
    if (tid == 10) Model::finish(out, any, win);
}

namespace {
// The wave's part of a fixed-order sum: the xor butterfly w = 1 .. 32.  Lane p holds s[p] + s[p ^ w], which is bit for bit the
// adjacent tree's s[p & ~w] + s[p | w]; after the last step every lane of the wave holds the sum of the wave's 64 partials.
__device__ __forceinline__ double refine_wave_sum(double v) {
#pragma unroll
    for (int w = 1; w < 64; w <<= 1) v = v + __shfl_xor(v, w, 64);
    return v;
}
__device__ __forceinline__ int refine_wave_count(int v) {
#pragma unroll
    for (int w = 1; w < 64; w <<= 1) v += __shfl_xor(v, w, 64);
    return v;
}
}  // namespace

// One workgroup of kRefineLanes lanes per set, every round of the set in this one launch (ransac_refine_math.h).  Lane p owns
// partial p of every fixed-order sum, in registers; the four waves' sums meet in LDS as (W0 + W1) + (W2 + W3).  Whatever
// decides how a round ends (n, the normalisation, the pivots, the solution, c') is computed by EVERY lane from the same LDS
// values, so the decision is uniform by construction: all lanes leave the loop together, and none before the last barrier it
// shares.  The 8 x 9 system lives in LDS: lane 9 i + j (< 72) updates entry (i, j) of an elimination step.
// The score c of the model a round starts from is the n of its first pass, so the caller's models (sift_hip_refine_homography)
// need none; rounds == 0 only counts.
__global__ __launch_bounds__(kRefineLanes) void ransac_refine_kernel(const float* __restrict__ pts, const int64_t* __restrict__ off, int rounds,
                                                                     float thr2, sift_hip_homography* __restrict__ models) {
    __shared__ double s_part[kRefineSums * 4];   // the waves' sums of a pass
    __shared__ double s_M[72];                   // the augmented normal equations
    __shared__ int s_cnt[4];
    const int tid = threadIdx.x, wave = tid >> 6;
    sift_hip_homography* mdl = models + blockIdx.x;
    if (mdl->iteration < 0) return;   // none: left alone.  The whole workgroup, before any barrier.
    const int64_t row0 = off[blockIdx.x];
    const int m = (int)(off[blockIdx.x + 1] - row0);
    const f4v* __restrict__ rows = reinterpret_cast<const f4v*>(pts + 4 * row0);
    float h[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) h[k] = mdl->h[k];
    int c = 0, refined = 0;
    for (int round = 0; round < (rounds > 0 ? rounds : 1); ++round) {
        __syncthreads();   // the LDS of the previous round is read
        // ---- pass 1: the inliers of h and their moments ----
        int n = 0;
        double mom[kRefineMoments];
#pragma unroll
        for (int k = 0; k < kRefineMoments; ++k) mom[k] = 0.0;
        for (int i = tid; i < m; i += kRefineLanes) {
            const f4v r = rows[i];
            const bool in = ransac_inlier(h, r.x, r.y, r.z, r.w, thr2);
            double t[kRefineMoments];
            refine_moment_terms(r.x, r.y, r.z, r.w, t);
            n += in ? 1 : 0;
#pragma unroll
            for (int k = 0; k < kRefineMoments; ++k) mom[k] = in ? mom[k] + t[k] : mom[k];
        }
        n = refine_wave_count(n);
#pragma unroll
        for (int k = 0; k < kRefineMoments; ++k) mom[k] = refine_wave_sum(mom[k]);
        if ((tid & 63) == 0) {
            s_cnt[wave] = n;
#pragma unroll
            for (int k = 0; k < kRefineMoments; ++k) s_part[4 * k + wave] = mom[k];
        }
        __syncthreads();
        n = (s_cnt[0] + s_cnt[1]) + (s_cnt[2] + s_cnt[3]);
#pragma unroll
        for (int k = 0; k < kRefineMoments; ++k) mom[k] = (s_part[4 * k] + s_part[4 * k + 1]) + (s_part[4 * k + 2] + s_part[4 * k + 3]);
        c = n;   // the score of h is its inlier count
        if (rounds == 0) break;
        RefineNorm nm;
        if (n < 4 || !refine_normalisation(mom, n, nm)) break;
        __syncthreads();   // s_part is read
        // ---- pass 2: the normal sums ----
        {
            double acc[kRefineSums];
#pragma unroll
            for (int k = 0; k < kRefineSums; ++k) acc[k] = 0.0;
            for (int i = tid; i < m; i += kRefineLanes) {
                const f4v r = rows[i];
                const bool in = ransac_inlier(h, r.x, r.y, r.z, r.w, thr2);
                double t[kRefineSums];
                refine_normal_terms(nm, r.x, r.y, r.z, r.w, t);
#pragma unroll
                for (int k = 0; k < kRefineSums; ++k) acc[k] = in ? acc[k] + t[k] : acc[k];
            }
#pragma unroll
            for (int k = 0; k < kRefineSums; ++k) acc[k] = refine_wave_sum(acc[k]);
            if ((tid & 63) == 0) {
#pragma unroll
                for (int k = 0; k < kRefineSums; ++k) s_part[4 * k + wave] = acc[k];
            }
            __syncthreads();
            if (tid == 0) {
#pragma unroll
                for (int k = 0; k < kRefineSums; ++k) acc[k] = (s_part[4 * k] + s_part[4 * k + 1]) + (s_part[4 * k + 2] + s_part[4 * k + 3]);
                refine_system(acc, n, s_M);
            }
            __syncthreads();
        }
        // ---- the solve: step k reads its inputs, a barrier, writes, a barrier ----
        bool ok = true;
        const int ei = tid / 9, ej = tid - 9 * ei;   // this lane's entry, for tid < 72
        for (int k = 0; k < 8; ++k) {
            bool piv_ok;
            const int p = refine_pivot(s_M, k, piv_ok);
            ok &= piv_ok;
            double val = 0.0, pj = 0.0, f = 0.0;
            const bool mine = tid < 72 && ei >= k;
            int src = ei;
            if (mine) {
                src = ei == k ? p : (ei == p ? k : ei);   // rows k and p change places
                val = s_M[9 * src + ej];
                pj = s_M[9 * p + ej];
                f = s_M[9 * src + k] / s_M[9 * p + k];
            }
            __syncthreads();
            if (mine) s_M[9 * ei + ej] = (ei > k && ej > k) ? refine_eliminate(f, pj, val) : val;
            __syncthreads();
        }
        double x[8];
        ok &= refine_backsubstitute(s_M, x);
        float h2[9];
#pragma unroll
        for (int k = 0; k < 9; ++k) h2[k] = h[k];
        ok = ok && refine_denormalise(x, nm, h2);
        if (!ok) break;
        // ---- pass 3: the score of the new model ----
        int c2 = 0;
        for (int i = tid; i < m; i += kRefineLanes) {
            const f4v r = rows[i];
            c2 += ransac_inlier(h2, r.x, r.y, r.z, r.w, thr2) ? 1 : 0;
        }
        c2 = refine_wave_count(c2);
        if ((tid & 63) == 0) s_cnt[wave] = c2;
        __syncthreads();
        c2 = (s_cnt[0] + s_cnt[1]) + (s_cnt[2] + s_cnt[3]);
        if (c2 < c) break;
#pragma unroll
        for (int k = 0; k < 9; ++k) h[k] = h2[k];
        ++refined;
        c = c2;
        if (c2 == n) break;
    }
    if (tid == 0) {
#pragma unroll
        for (int k = 0; k < 9; ++k) mdl->h[k] = h[k];
        mdl->inliers = c;
        mdl->refined = refined;
    }
}

// one lane per row: the predicate under the winner of the row's set
template <typename Model>
__global__ __launch_bounds__(256) void ransac_flags_kernel(const float* __restrict__ pts, const int64_t* __restrict__ off, int n_sets, long long rows,
                                                           const typename Model::Rec* __restrict__ models, float thr2, uint8_t* __restrict__ inlier) {
    const long long row = (long long)blockIdx.x * 256 + threadIdx.x;
    if (row >= rows) return;
    bool in = false;
    if (row >= off[0]) {
        const typename Model::Rec* mdl = models + set_of_row(off, n_sets, row);
        if (mdl->iteration >= 0) {
            float h[9];
            for (int k = 0; k < 9; ++k) h[k] = Model::coef(mdl)[k];
            const f4v r = *reinterpret_cast<const f4v*>(pts + 4 * (size_t)row);
            in = Model::inlier(h, r.x, r.y, r.z, r.w, thr2);
        }
    }
    inlier[row] = in ? 1 : 0;
}

// one lane per record of the dense match list: the keypoints' image coordinates, (float)(x << octave) * coord_scale
__global__ __launch_bounds__(256) void ransac_gather_kernel(const sift_hip_match_rec* __restrict__ recs, const int64_t* __restrict__ off, int n_pairs,
                                                            long long rows, const sift_hip_keypoint* __restrict__ kp, const int* __restrict__ kp_row0,
                                                            float coord_scale, float* __restrict__ pts) {
    const long long row = (long long)blockIdx.x * 256 + threadIdx.x;
    if (row >= rows) return;
    const int p = set_of_row(off, n_pairs, row);
    const sift_hip_match_rec rec = recs[row];
    const sift_hip_keypoint q = kp[(size_t)kp_row0[2 * p] + (size_t)rec.query], t = kp[(size_t)kp_row0[2 * p + 1] + (size_t)rec.train];
    f4v o;
    o.x = (float)((uint32_t)q.x << q.octave) * coord_scale;
    o.y = (float)((uint32_t)q.y << q.octave) * coord_scale;
    o.z = (float)((uint32_t)t.x << t.octave) * coord_scale;
    o.w = (float)((uint32_t)t.y << t.octave) * coord_scale;
    *reinterpret_cast<f4v*>(pts + 4 * (size_t)row) = o;
}

void launch_ransac_hypotheses(hipStream_t s, const float* d_pts, const int64_t* d_off, int n_sets, uint32_t iterations, uint32_t seed,
                              RansacHyp* d_hyp) {
    const long long n = (long long)n_sets * iterations;
    if (n <= 0) return;
    hipLaunchKernelGGL(ransac_hypothesis_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, d_pts, d_off, n_sets, iterations, seed, d_hyp);
}
void launch_ransac_score(hipStream_t s, const float* d_pts, const RansacHyp* d_hyp, const RansacTile* d_tiles, int n_tiles, uint32_t iterations,
                         float thr2, int32_t* d_scores) {
    if (n_tiles <= 0) return;
    hipLaunchKernelGGL(ransac_score_kernel<HomographyModel>, dim3((unsigned)n_tiles), dim3(kRansacHyps), 0, s, d_pts, d_hyp, d_tiles, iterations, thr2, d_scores);
}
void launch_ransac_select(hipStream_t s, const RansacHyp* d_hyp, int n_sets, uint32_t iterations, int32_t* d_scores, sift_hip_homography* d_models) {
    if (n_sets <= 0) return;
    hipLaunchKernelGGL(ransac_select_kernel<HomographyModel>, dim3((unsigned)n_sets), dim3(256), 0, s, d_hyp, iterations, d_scores, d_models);
}
void launch_ransac_refine(hipStream_t s, const float* d_pts, const int64_t* d_off, int n_sets, int rounds, float thr2, sift_hip_homography* d_models) {
    if (n_sets <= 0) return;
    hipLaunchKernelGGL(ransac_refine_kernel, dim3((unsigned)n_sets), dim3(kRefineLanes), 0, s, d_pts, d_off, rounds, thr2, d_models);
}
void launch_ransac_flags(hipStream_t s, const float* d_pts, const int64_t* d_off, int n_sets, long long rows, const sift_hip_homography* d_models,
                         float thr2, uint8_t* d_inlier) {
    if (rows <= 0 || n_sets <= 0) return;
    hipLaunchKernelGGL(ransac_flags_kernel<HomographyModel>, dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, s, d_pts, d_off, n_sets, rows, d_models, thr2, d_inlier);
}
void launch_fund_hypotheses(hipStream_t s, const float* d_pts, const int64_t* d_off, int n_sets, uint32_t iterations, uint32_t seed, RansacHyp* d_hyp) {
    const long long n = (long long)n_sets * iterations;
    if (n <= 0) return;
    hipLaunchKernelGGL(ransac_fund_hypothesis_kernel, dim3((unsigned)((n + kFundLanes - 1) / kFundLanes)), dim3(kFundLanes), 0, s, d_pts, d_off, n_sets,
                       iterations, seed, d_hyp);
}
void launch_fund_score(hipStream_t s, const float* d_pts, const RansacHyp* d_hyp, const RansacTile* d_tiles, int n_tiles, uint32_t slots, float thr2,
                       int32_t* d_scores) {
    if (n_tiles <= 0) return;
    hipLaunchKernelGGL(ransac_score_kernel<FundamentalModel>, dim3((unsigned)n_tiles), dim3(kRansacHyps), 0, s, d_pts, d_hyp, d_tiles, slots, thr2, d_scores);
}
void launch_fund_select(hipStream_t s, const RansacHyp* d_hyp, int n_sets, uint32_t slots, int32_t* d_scores, sift_hip_fundamental* d_models) {
    if (n_sets <= 0) return;
    hipLaunchKernelGGL(ransac_select_kernel<FundamentalModel>, dim3((unsigned)n_sets), dim3(256), 0, s, d_hyp, slots, d_scores, d_models);
}
void launch_fund_flags(hipStream_t s, const float* d_pts, const int64_t* d_off, int n_sets, long long rows, const sift_hip_fundamental* d_models,
                       float thr2, uint8_t* d_inlier) {
    if (rows <= 0 || n_sets <= 0) return;
    hipLaunchKernelGGL(ransac_flags_kernel<FundamentalModel>, dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, s, d_pts, d_off, n_sets, rows, d_models, thr2,
                       d_inlier);
}
void launch_ransac_gather(hipStream_t s, const sift_hip_match_rec* d_recs, const int64_t* d_off, int n_pairs, long long rows,
                          const sift_hip_keypoint* d_kp, const int* d_kp_row0, float coord_scale, float* d_pts) {
    if (rows <= 0 || n_pairs <= 0) return;
    hipLaunchKernelGGL(ransac_gather_kernel, dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, s, d_recs, d_off, n_pairs, rows, d_kp, d_kp_row0,
                       coord_scale, d_pts);
}

}  // namespace sift_hip
