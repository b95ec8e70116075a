// Two-band compositor: what the host (twoband.cpp) hands to the kernel (kernels_twoband.hip), the launcher, and what twoband.cpp
// needs from a context.  The definition of the result is twoband_math.h.
#pragma once
#include <stdint.h>

#include "common.h"
#include "match_kernels.h"

namespace sift_hip {

constexpr int kTwobandLanes = 256;            // a workgroup: a 64 x 32 CANVAS tile, eight consecutive rows of one column per lane
constexpr int kTwobandTileW = 64, kTwobandTileH = 32, kTwobandRowsPerLane = 8, kTwobandWaves = kTwobandLanes / 64;
constexpr int kTwobandRun = 8;                // the row pass: a lane forms runs of eight consecutive outputs of one row
constexpr int kTwobandTaps = 17;              // kTwobandMaxRadius + 1 (twoband_math.h)
static_assert(kTwobandTileW * kTwobandTileH == kTwobandLanes * kTwobandRowsPerLane, "a lane per column of eight rows");
static_assert(kTwobandTileW % kTwobandRun == 0, "whole runs in a row");
static_assert(sizeof(sift_hip_twoband_params) == 24, "two-band record packing");

// The planes of one job over the tile and its halo of `radius`, in LDS: t as floats and m as bytes over (TW + 2R) x (TH + 2R)
// in rows of an odd pitch, then rs and rn as floats over TW x (TH + 2R) in rows of TW + 1.  R = 16: 24832 + 6208 + 2 x 16640 =
// 64320 bytes, R = 6: 9 KB + 2 KB + 2 x 11 KB; the kernel's flags and taps (132 bytes) come on top.
constexpr int twoband_pitch(int radius) { return (kTwobandTileW + 2 * radius) | 1; }
constexpr int twoband_rows(int radius) { return kTwobandTileH + 2 * radius; }
constexpr int twoband_m_bytes(int radius) { return (twoband_pitch(radius) * twoband_rows(radius) + 3) & ~3; }
constexpr size_t twoband_lds_bytes(int radius) {
    return (size_t)twoband_pitch(radius) * twoband_rows(radius) * 4 + twoband_m_bytes(radius) + 2 * (size_t)(kTwobandTileW + 1) * twoband_rows(radius) * 4;
}
static_assert(twoband_lds_bytes(16) == 64320, "the LDS budget at the largest radius");
static_assert(twoband_lds_bytes(16) + 132 <= 65536, "planes, flags and taps within 64 KB");

struct TwobandArgs {
    int out_w, out_h, origin_x, origin_y;
    float fill;
    int interp;   // 0 nearest, 1 bilinear
    int path;     // 1: every visit takes the general path (rn and ln formed from m)
    int radius;
    float full_norm;            // twoband_full_norm(taps, radius)
    float taps[kTwobandTaps];   // k[0 .. radius]
};

// every canvas in one launch, as launch_composite; d_tiles (three counters, zeroed by the caller): (tile, job) visits on the
// general path, on the constant-norm path, skipped
void launch_twoband(hipStream_t s, const float* d_imgs, int w, int h, const int* d_src, const float* d_models, const long long* d_offsets, int n_canvases,
                    const TwobandArgs& a, float* d_out, uint16_t* d_count, unsigned long long* d_tiles, const float* d_gains);
void tu_touch_twoband(hipStream_t s);

// ---- the context as twoband.cpp sees it (context.cpp) ----
struct TwobandState;                         // scratch, owned by the context once the first call made it
void twoband_state_free(TwobandState* st);   // twoband.cpp; sift_hip_destroy calls it
TwobandState** twoband_ctx_state(sift_hip_ctx* c);

}  // namespace sift_hip
