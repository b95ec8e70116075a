// Compositor: what the host (composite.cpp) hands to the kernel (kernels_composite.hip), the launcher, and what composite.cpp
// needs from a context.  The definition of the result is composite_math.h.
#pragma once
#include <stdint.h>

#include "common.h"
#include "match_kernels.h"

namespace sift_hip {

constexpr int kCompLanes = 256;               // a workgroup: a 64 x 16 CANVAS tile, four consecutive rows of one column per lane
constexpr int kCompTileW = 64, kCompTileH = 16, kCompRowsPerLane = 4, kCompWaves = kCompLanes / 64;
// two staged boxes used alternately (kernels_composite.hip) and two sets of per-wave coverage flags: 32 KB to the byte
constexpr int kCompBoxFloats = 4096 - kCompWaves;
static_assert(kCompTileW * kCompTileH == kCompLanes * kCompRowsPerLane, "a lane per column of four rows");
static_assert(2 * (kCompBoxFloats + kCompWaves) * 4 == 32768, "the LDS budget");
static_assert(sizeof(sift_hip_composite_params) == 24, "composite record packing");

struct CompositeArgs {
    int out_w, out_h, origin_x, origin_y;
    float fill;
    int interp;   // 0 nearest, 1 bilinear
    int blend;    // 0 first, 1 mean, 2 feather
    int path;     // 1: every tap comes from global memory
    int vec;      // the images' rows are 16-byte aligned: boxes are staged by 16-byte loads
};

// every canvas in one launch: canvas c accumulates jobs d_offsets[c] .. d_offsets[c + 1] - 1 (job j reads image d_src[j]; d_src
// null: image j) into d_out[c] and, unless null, d_count[c]; d_tiles (three counters, zeroed by the caller: (tile, job) visits
// staged, direct, skipped) may be null; d_gains (one float per job) may be null: no gains
void launch_composite(hipStream_t s, const float* d_imgs, int w, int h, const int* d_src, const float* d_models, const long long* d_offsets, int n_canvases,
                      const CompositeArgs& a, float* d_out, uint16_t* d_count, unsigned long long* d_tiles, const float* d_gains);
void tu_touch_composite(hipStream_t s);

// ---- the context as composite.cpp sees it (context.cpp); uploads, downloads and errors go through the match_* accessors ----
struct CompositeState;                           // scratch, owned by the context once the first call made it
void composite_state_free(CompositeState* st);   // composite.cpp; sift_hip_destroy calls it
CompositeState** composite_ctx_state(sift_hip_ctx* c);

}  // namespace sift_hip
