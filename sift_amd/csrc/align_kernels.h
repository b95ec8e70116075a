// Direct alignment: what the host (align.cpp) hands to the kernels (kernels_align.hip), the launchers, and what align.cpp needs
// from a context.  The definition of the result is align_math.h.
#pragma once
#include <stdint.h>

#include "align_math.h"
#include "common.h"
#include "match_kernels.h"

namespace sift_hip {

// the tile sum's LDS: [entry][lane] floats, a row of 256 lanes padded to an odd pitch, half of the 78 entries at a time
constexpr int kAlignHalf = kAlignSums / 2, kAlignPitch = kAlignLanes + 1, kAlignLdsFloats = kAlignHalf * kAlignPitch;
// the pair sum: 16 of a record's 80 doubles at a time over 256 chains
constexpr int kAlignBatch = 16;
static_assert(kAlignRec % kAlignBatch == 0 && 2 * kAlignHalf == kAlignSums, "batches");
static_assert(sizeof(sift_hip_align_params) == 20 && sizeof(sift_hip_alignment) == 64, "alignment record packing");

struct AlignArgs {
    int w, h, n_pairs, tiles_x, tiles_y;
    int rounds, border, min_pixels, path;
    float damping;
    AlignNorm nm;
};

// one thread per pair: d_state[p] from d_models[p], d_out[p], zeros in d_sums[p]
void launch_align_begin(hipStream_t s, const sift_hip_homography* d_models, int n_pairs, AlignState* d_state, sift_hip_alignment* d_out, double* d_sums);
// pass k: every (pair, tile) in one launch -> d_partials[pair][tile][80]; the tiles of a pair that has stopped leave at once
void launch_align_accumulate(hipStream_t s, const float* d_imgs, const int* d_pair_q, const int* d_pair_t, const AlignState* d_state, const AlignArgs& a,
                             double* d_partials);
// pass k: one workgroup per pair: the tile tree, align_round; writes d_state[p], d_out[p], d_models[p].h and d_sums[p]
void launch_align_solve(hipStream_t s, const double* d_partials, const AlignArgs& a, int k, AlignState* d_state, sift_hip_homography* d_models,
                        sift_hip_alignment* d_out, double* d_sums);
void tu_touch_align(hipStream_t s);

// ---- the context as align.cpp sees it (context.cpp) ----
struct AlignScratch;                        // scratch, owned by the context once the first call made it
void align_state_free(AlignScratch* st);    // align.cpp; sift_hip_destroy calls it
AlignScratch** align_ctx_state(sift_hip_ctx* c);

}  // namespace sift_hip
