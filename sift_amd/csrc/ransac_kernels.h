// RANSAC homography: the records the host (ransac.cpp) hands to the kernels (kernels_ransac.hip), their launchers, and what
// ransac.cpp needs from a context and from the matcher.  The definition of the result is ransac_math.h and ransac_refine_math.h.
#pragma once
#include <stdint.h>

#include "common.h"
#include "match_kernels.h"

namespace sift_hip {

constexpr int kRansacHyps = 256;     // hypotheses a workgroup of the scoring kernel scores: one per lane
constexpr int kRansacRows = 1024;    // rows of a set a workgroup stages in LDS (16 KB); a longer set is split over workgroups

// one hypothesis: the model and whether the sample gave one (h all +0.0f otherwise)
struct RansacHyp { float h[9]; int32_t valid; };
// one workgroup of the scoring kernel: hypotheses [hyp0, hyp0 + kRansacHyps) of a set against rows [row_lo, row_hi) of `pts`
struct RansacTile { int set, hyp0, row_lo, row_hi; };
static_assert(sizeof(RansacHyp) == 40 && sizeof(RansacTile) == 16 && sizeof(sift_hip_homography) == 48 && sizeof(sift_hip_ransac_params) == 16,
              "ransac record packing");

// d_off: n_sets + 1 row offsets.  Every launcher is one launch for all sets.
void launch_ransac_hypotheses(hipStream_t s, const float* d_pts, const int64_t* d_off, int n_sets, uint32_t iterations, uint32_t seed,
                              RansacHyp* d_hyp);
// d_scores (n_sets x iterations) must be zero: partial counts of the row ranges are added to it
void launch_ransac_score(hipStream_t s, const float* d_pts, const RansacHyp* d_hyp, const RansacTile* d_tiles, int n_tiles, uint32_t iterations,
                         float thr2, int32_t* d_scores);
// invalid hypotheses' scores become -1; the winner of every set -> d_models
void launch_ransac_select(hipStream_t s, const RansacHyp* d_hyp, int n_sets, uint32_t iterations, int32_t* d_scores, sift_hip_homography* d_models);
// `rounds` refinement rounds (ransac_refine_math.h) on every model with iteration >= 0, in place: h, inliers, refined
void launch_ransac_refine(hipStream_t s, const float* d_pts, const int64_t* d_off, int n_sets, int rounds, float thr2, sift_hip_homography* d_models);
void launch_ransac_flags(hipStream_t s, const float* d_pts, const int64_t* d_off, int n_sets, long long rows, const sift_hip_homography* d_models,
                         float thr2, uint8_t* d_inlier);
// ---- the fundamental matrix (ransac_fund_math.h): the same scoring, selection and flag kernels, instantiated with its
// predicate, over 3 * iterations hypothesis slots per set (slot 3 * sample + root); RansacHyp's h holds f ----
constexpr int kFundLanes = 256;      // lanes of a workgroup of the seven-point solver: one per (set, sample)
constexpr int kFundMinRows = 7, kHomographyMinRows = 4;
static_assert(sizeof(sift_hip_fundamental) == 48, "ransac record packing");
// d_hyp: n_sets x 3 * iterations records
void launch_fund_hypotheses(hipStream_t s, const float* d_pts, const int64_t* d_off, int n_sets, uint32_t iterations, uint32_t seed, RansacHyp* d_hyp);
// the tiles' hyp0 counts slots; d_scores (n_sets x slots) must be zero
void launch_fund_score(hipStream_t s, const float* d_pts, const RansacHyp* d_hyp, const RansacTile* d_tiles, int n_tiles, uint32_t slots, float thr2,
                       int32_t* d_scores);
void launch_fund_select(hipStream_t s, const RansacHyp* d_hyp, int n_sets, uint32_t slots, int32_t* d_scores, sift_hip_fundamental* d_models);
void launch_fund_flags(hipStream_t s, const float* d_pts, const int64_t* d_off, int n_sets, long long rows, const sift_hip_fundamental* d_models,
                       float thr2, uint8_t* d_inlier);
// rows of sift_hip_result_verify: record i of pair p (d_off: the pairs' record offsets) -> (qx, qy, tx, ty); d_kp_row0: for
// every pair the first keypoint row of its query image and of its train image (2 ints per pair)
void launch_ransac_gather(hipStream_t s, const sift_hip_match_rec* d_recs, const int64_t* d_off, int n_pairs, long long rows,
                          const sift_hip_keypoint* d_kp, const int* d_kp_row0, float coord_scale, float* d_pts);

// ---- the context as ransac.cpp sees it (context.cpp); uploads, downloads and errors go through the match_* accessors ----
struct RansacState;                        // scratch, owned by the context once the first call made it
void ransac_state_free(RansacState* st);   // ransac.cpp; sift_hip_destroy calls it
RansacState** ransac_ctx_state(sift_hip_ctx* c);
bool ransac_ctx_subpixel(sift_hip_ctx* c);   // did the last batch run with subpixel (coordinates of the doubled image)?

// ---- the matcher as ransac.cpp sees it (match.cpp) ----
// sift_hip_result_match that also leaves its list on the device: *d_recs = the dense records (device memory: the matcher's
// scratch, or `recs` itself when that is device memory), valid until the context's next match call; host_counts: n_pairs
// entries (always filled, unlike `counts`, which may be NULL).
int match_result_on_device(sift_hip_ctx* c, const char* who, int n_pairs, const int32_t* pair_q, const int32_t* pair_t,
                           const sift_hip_match_params* params, sift_hip_match_rec* recs, int32_t* counts, int64_t* total,
                           const sift_hip_match_rec** d_recs, int32_t* host_counts, char* err, int errlen);

}  // namespace sift_hip
