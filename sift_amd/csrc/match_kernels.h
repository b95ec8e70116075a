// Descriptor matching: the records the host (match.cpp) hands to the kernels (kernels_match.hip), their launchers, and what
// match.cpp needs from a context (accessors defined in context.cpp).  The definition of the result is in include/sift_hip.h.
#pragma once
#include <stdint.h>

#include "common.h"

namespace sift_hip {

constexpr int kMatchQ = 128;          // query rows a workgroup of the tile kernel keeps in LDS
constexpr int kMatchT = 64;           // train rows per LDS stage
constexpr int kMatchSplitRows = 256;  // a split of a train set is a multiple of this many rows (host-side choice, never visible)
constexpr int kMatchNone = 0x7fffffff;   // index of a missing entry inside the kernels (sorts after every row); -1 on the way out

// one workgroup of the tile kernel: a block of query rows against a range of its train set
struct MatchTile {
    int q_row0, q_rows;   // first query row (row of the descriptor array), rows of the block (<= kMatchQ)
    int t_set0;           // first row of the train set
    int t_lo, t_hi;       // train rows [t_lo, t_hi) of the set, t_lo a multiple of kMatchT
    int pair_dir;         // guided matching: 2 * pair + direction (1: a tile of the cross-check, roles swapped); else 0
};
// what the guided instantiations of the tile kernel read besides: (x, y) of every descriptor row, nine floats per pair, threshold^2
struct MatchGuideArgs {
    const float* xy = nullptr;
    const float* models = nullptr;
    float thr2 = 0.0f;
};
// one block of query rows of one pair: its partial top-2s (tiles first_tile .. + n_tiles) become rows of the result
struct MatchBlock {
    int q_row0, q_rows;
    int out_row0;         // row of the idx / dist2 arrays
    int first_tile, n_tiles;
    int pad;
};
struct MatchTop2 { float d1, d2; int i1, i2; };   // partial result of one query row in one tile
static_assert(sizeof(sift_hip_match_rec) == 16 && sizeof(sift_hip_match_params) == 8 && sizeof(MatchTop2) == 16, "match record packing");
// one pair of the filter: its rows of the top-2 arrays, the rows of the reverse best (cross-check; -1 none)
struct MatchPair {
    int row0, rows;
    int rev_row0;
    int pad;
};

void launch_match_norms(hipStream_t s, const float* d_desc, const sift_hip_keypoint* d_kp, long long rows, float* d_norm, uint8_t* d_valid);
void launch_match_tiles(hipStream_t s, const float* d_desc, const float* d_norm, const uint8_t* d_valid, const MatchTile* d_tiles,
                        int n_tiles, MatchTop2* d_part);
// model: SIFT_HIP_GUIDE_HOMOGRAPHY or SIFT_HIP_GUIDE_FUNDAMENTAL
void launch_match_tiles_guided(hipStream_t s, const float* d_desc, const float* d_norm, const uint8_t* d_valid, const MatchTile* d_tiles,
                               int n_tiles, MatchTop2* d_part, int model, const MatchGuideArgs& ga);
// (float)(x << octave) * coord_scale, (float)(y << octave) * coord_scale of every keypoint record -> two floats per row
void launch_match_coords(hipStream_t s, const sift_hip_keypoint* d_kp, long long rows, float coord_scale, float* d_xy);
void launch_match_merge(hipStream_t s, const MatchTop2* d_part, const uint8_t* d_valid, const MatchBlock* d_blocks, int n_blocks,
                        int32_t* d_idx, float* d_dist);
// records of every pair at the pair's own rows of d_seg (query order), per-pair counts; then the dense list in pair order
void launch_match_filter(hipStream_t s, const int32_t* d_idx, const float* d_dist, const MatchPair* d_pairs, int n_pairs, int use_ratio,
                         float ratio2, int cross_check, sift_hip_match_rec* d_seg, int32_t* d_counts);
void launch_match_pack(hipStream_t s, const sift_hip_match_rec* d_seg, const MatchPair* d_pairs, const int32_t* d_counts, int n_pairs,
                       sift_hip_match_rec* d_out);
void tu_touch_match(hipStream_t s);

// ---- 8-bit rows (kernels_match_u8.hip; include/sift_hip.h, "8-bit descriptors and integer matching") ----------
// the quantiser alone: rows x 128 floats -> rows x 128 bytes (both 16-byte aligned)
void launch_match_quantize(hipStream_t s, const float* d_desc, long long rows, uint8_t* d_out);
// n'(a) = sum (a[k] - 128)^2 and the valid flag of every byte row
void launch_match_norms_u8(hipStream_t s, const uint8_t* d_desc8, const sift_hip_keypoint* d_kp, long long rows, int32_t* d_norm, uint8_t* d_valid);
// both in one pass over float rows: d_desc8 receives the bytes
void launch_match_quantize_norms(hipStream_t s, const float* d_desc, const sift_hip_keypoint* d_kp, long long rows, uint8_t* d_desc8,
                                 int32_t* d_norm, uint8_t* d_valid);
// the tile kernel on the i8 matrix instruction: the tables and the partials of launch_match_tiles, distances as (float)d2
void launch_match_tiles_u8(hipStream_t s, const uint8_t* d_desc8, const int32_t* d_norm, const uint8_t* d_valid, const MatchTile* d_tiles,
                           int n_tiles, MatchTop2* d_part);

// scratch of the matcher and of the geometric verification (ransac.cpp): device memory that only grows, kept with the context
struct ScratchBuf {
    void* p = nullptr;
    size_t cap = 0;
    void ensure(size_t bytes) {
        if (bytes <= cap) return;
        ApiGuard api;
        if (p) SIFT_HIP_CHECK(hipFree(p));
        p = nullptr;
        cap = 0;
        SIFT_HIP_CHECK(hipMalloc(&p, bytes + bytes / 4));
        cap = bytes + bytes / 4;
    }
    void release() {
        ApiGuard api;
        if (p) (void)hipFree(p);
        p = nullptr;
        cap = 0;
    }
    template <class T>
    T* as() const { return reinterpret_cast<T*>(p); }
};

// ---- the context as match.cpp sees it (context.cpp) ---------------------------------------------------------
struct MatchState;                       // scratch of the matcher, owned by the context once the first match call made it
void match_state_free(MatchState* st);   // match.cpp; sift_hip_destroy calls it
struct MatchCtxView {
    int device;
    hipStream_t stream;
    bool have_result;
    const sift_hip_keypoint* d_kp;       // results of the last batch (sift_hip_result_device)
    const float* d_desc;
    const int32_t* counts;
    int n_images;
    MatchState** state;
};
MatchCtxView match_ctx_view(sift_hip_ctx* c);
bool match_ptr_on_device(const void* p);                                              // as sift_hip_result_copy tells its targets apart
void match_upload(sift_hip_ctx* c, void* dev, const void* host, size_t bytes);        // queued on the context's stream
void match_download(sift_hip_ctx* c, void* dst, const void* dev, size_t bytes);       // complete on return
void match_wait(sift_hip_ctx* c);
int match_guarded(char* err, int errlen, int (*fn)(void*), void* arg);                // HIP failures -> SIFT_HIP_EHIP + text
void match_set_err(char* err, int errlen, const char* msg);

}  // namespace sift_hip
