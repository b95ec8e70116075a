// Homography warp: what the host (warp.cpp) hands to the kernel (kernels_warp.hip), the launcher, and what warp.cpp needs from a
// context.  The definition of the result is warp_math.h.
#pragma once
#include <stdint.h>

#include "common.h"
#include "match_kernels.h"

namespace sift_hip {

constexpr int kWarpLanes = 256;                // a workgroup: a 64 x 16 output tile, four consecutive rows of one column per lane
constexpr int kWarpTileW = 64, kWarpTileH = 16, kWarpRowsPerLane = 4;
constexpr int kWarpLdsFloats = 8192;           // the staged box: 32 KB, five workgroups in a CU's 160 KB (kernels_warp.hip)
static_assert(kWarpTileW * kWarpTileH == kWarpLanes * kWarpRowsPerLane, "a lane per column of four rows");
static_assert(sizeof(sift_hip_warp_params) == 24, "warp record packing");

struct WarpArgs {
    int out_w, out_h, origin_x, origin_y;
    float fill;
    int interp;   // 0 nearest, 1 bilinear
    int path;     // 1: every tile reads its taps from global memory
    int vec;      // the images' rows are 16-byte aligned: boxes are staged by 16-byte loads
};

// every job in one launch: job j warps image d_src[j] (d_src null: image j) under d_models[9 j ..] into d_out[j]; d_mask and
// d_tiles (two counters, zeroed by the caller: tiles staged, tiles direct) may be null
void launch_warp(hipStream_t s, const float* d_imgs, int w, int h, const int* d_src, const float* d_models, int n_jobs, const WarpArgs& a, float* d_out,
                 uint8_t* d_mask, unsigned long long* d_tiles);
void tu_touch_warp(hipStream_t s);

// ---- the context as warp.cpp sees it (context.cpp); uploads, downloads and errors go through the match_* accessors ----
struct WarpState;                      // scratch, owned by the context once the first call made it
void warp_state_free(WarpState* st);   // warp.cpp; sift_hip_destroy calls it
WarpState** warp_ctx_state(sift_hip_ctx* c);

}  // namespace sift_hip
