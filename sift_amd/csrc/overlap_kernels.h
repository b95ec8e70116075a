// Overlap statistics: what the host (overlap.cpp) hands to the kernels (kernels_overlap.hip), the launchers, and what
// overlap.cpp needs from a context.  The definition of the result is overlap_math.h.
#pragma once
#include <stdint.h>

#include "common.h"
#include "match_kernels.h"

namespace sift_hip {

constexpr int kOvlLanes = 256, kOvlWaves = kOvlLanes / 64;
// a workgroup owns a 64 x 64 REGION of one canvas: 16 chunks of 64 x 4 = 256 pixels, the k dimension of one round of products
constexpr int kOvlRegionW = 64, kOvlRegionH = 64, kOvlChunkH = 4, kOvlChunkPx = kOvlRegionW * kOvlChunkH, kOvlChunks = kOvlRegionH / kOvlChunkH;
// LDS: [plane][job][pixel] int8, a row of 256 pixels padded to an odd number of 16-byte slots (the operands are read 16 bytes a lane)
constexpr int kOvlRowBytes = kOvlChunkPx + 16, kOvlPlaneBytes = 32 * kOvlRowBytes, kOvlLdsBytes = 4 * kOvlPlaneBytes;
// |term| <= 128 * 128 = 2^14 and a chunk has 2^8 pixels: 511 chunks stay below 2^31 in one int32 accumulator
constexpr int kOvlMaxChunksPerFlush = 511;
static_assert(kOvlChunks <= kOvlMaxChunksPerFlush, "the int32 bound");
static_assert(kOvlChunkPx == 4 * 64, "a wave's 64 lanes own the chunk's 64 quads of four x-adjacent pixels");
static_assert(5 * 1024 * 4 <= kOvlLdsBytes, "the flush sums the waves' five accumulators in the planes' memory");
static_assert(sizeof(sift_hip_overlap_params) == 32, "overlap record packing");

struct OverlapArgs {
    int out_w, out_h, origin_x, origin_y;
    float scale;
    int interp;   // 0 nearest, 1 bilinear
    int path;     // 1: every chunk is flushed by itself
};

// every canvas in one launch: canvas c adds the statistics of jobs d_offsets[c] .. d_offsets[c + 1] - 1 (at most 32; job j reads
// image d_src[j]; d_src null: image j) to d_stats[c] (4 x 32 x 32 int64, ZEROED by the caller on the same stream)
void launch_overlap_stats(hipStream_t s, const float* d_imgs, int w, int h, const int* d_src, const float* d_models, const long long* d_offsets,
                          int n_canvases, const OverlapArgs& a, long long* d_stats);
// one workgroup per canvas: d_gains[d_offsets[c] ..] and d_status[c] from d_stats[c] (overlap_math.h: gain_solve)
void launch_overlap_gains(hipStream_t s, const long long* d_stats, const long long* d_offsets, int n_canvases, float sigma_n, float sigma_g,
                          float* d_gains, uint8_t* d_status);
void tu_touch_overlap(hipStream_t s);

// ---- the context as overlap.cpp sees it (context.cpp) ----
struct OverlapState;                         // scratch, owned by the context once the first call made it
void overlap_state_free(OverlapState* st);   // overlap.cpp; sift_hip_destroy calls it
OverlapState** overlap_ctx_state(sift_hip_ctx* c);

}  // namespace sift_hip
