// Direct alignment (include/sift_hip.h, "direct alignment"; the definition: align_math.h).
//
// A pass over all pairs is two launches, and the passes of a call follow each other on the stream with no host synchronisation:
// whether a pair still runs is a flag in its device record (AlignState), which the solve kernel writes and both kernels read.
//
// align_accumulate_kernel: grid (tiles, pairs).  A workgroup of 256 lanes owns a 64 x 64 tile of the query lattice; lane l keeps
//   column l & 63 and the 16 rows (l >> 6) + 4 k, so a wave reads one query row of 64 floats at a time and a lane IS one of the
//   definition's 256 partials.  The pair's model, gain and bias are the same in every lane: scalar loads from the record.  Per
//   pixel: the map and the contribution test; one ballot per wave and row skips the rest when no lane contributes; the four train
//   taps come straight from global memory (near-registered models: the rows a wave touches are the rows its neighbours touch); the
//   twelve columns and the 78 fmaf accumulators live in registers.
//   Tile sum: the lanes store their partials to LDS as [entry][lane] floats with a pitch of 257 (consecutive lanes, consecutive
//   banks; the readers, one lane per entry, are 257 floats apart: different banks), 39 entries at a time and then 39 and the pixel
//   count - 41 KB, so several workgroups share a CU - and lane e adds entry e over lanes 0 .. 255 in double, ascending: the
//   definition's order, no shuffles, no atomics.  80 doubles per tile go to partials[pair][tile] with plain vector stores.
// align_solve_kernel: one workgroup per pair.  Lane c runs chain c (tiles c, c + 256, ..) of 16 entries at a time, the adjacent
//   pairwise tree runs in LDS, and lane 0 then runs align_round - the same function the host loop runs - on the 80 sums and a
//   10 x 11 system in LDS, and writes the record, the result and the model.
#include "align_kernels.h"
#include "common.h"

namespace sift_hip {

template <int PATH>
__global__ __launch_bounds__(kAlignLanes) void align_accumulate_kernel(const float* __restrict__ imgs, const int* __restrict__ pair_q,
                                                                       const int* __restrict__ pair_t, const AlignState* __restrict__ state, AlignArgs a,
                                                                       double* __restrict__ partials) {
    __shared__ float part[(kAlignHalf + 1) * kAlignPitch];
    const int tid = threadIdx.x, pair = blockIdx.y, tile = blockIdx.x;
    const AlignState& st = state[pair];
    if (!st.active) return;   // the same in every lane of the workgroup
    float m[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) m[k] = st.h[k];
    const float gain = st.a, bias = st.b;
    const int w = a.w, h = a.h;
    const size_t frame = (size_t)w * (size_t)h;
    const float* __restrict__ Q = imgs + (size_t)pair_q[pair] * frame;
    const float* __restrict__ T = imgs + (size_t)pair_t[pair] * frame;
    const int x = (tile % a.tiles_x) * kAlignTile + (tid & (kAlignTile - 1)), y0 = (tile / a.tiles_x) * kAlignTile + tid / kAlignTile;
    const auto px = [&](int xx, int yy) { return T[(size_t)yy * (size_t)w + (size_t)xx]; };

    float acc[kAlignSums];
#pragma unroll
    for (int e = 0; e < kAlignSums; ++e) acc[e] = 0.0f;
    int n = 0;
    for (int k = 0; k < kAlignRows; ++k) {
        const int y = y0 + kAlignRowStep * k;
        float u, v, W, c[kAlignCols];
        const bool on = align_contributes(m, x, y, w, h, a.border, u, v, W) & (x < w) & (y < h);
        if (PATH == 0) {
            if (__builtin_amdgcn_ballot_w64(on) == 0) continue;
            if (on) {
                align_pixel(px, Q[(size_t)y * (size_t)w + (size_t)x], gain, bias, a.nm, x, y, u, v, W, w, h, c);
#pragma unroll
                for (int i = 0, e = 0; i < kAlignCols; ++i)
#pragma unroll
                    for (int j = i; j < kAlignCols; ++j, ++e) acc[e] = __builtin_fmaf(c[i], c[j], acc[e]);
                ++n;
            }
        } else {
            // every lane computes; one that does not contribute maps to train pixel (0, 0) and reads a query pixel of the frame
            const int xc = x < w ? x : w - 1, yc = y < h ? y : h - 1;
            align_pixel(px, Q[(size_t)yc * (size_t)w + (size_t)xc], gain, bias, a.nm, x, y, on ? u : 0.0f, on ? v : 0.0f, on ? W : 1.0f, w, h, c);
#pragma unroll
            for (int i = 0, e = 0; i < kAlignCols; ++i)
#pragma unroll
                for (int j = i; j < kAlignCols; ++j, ++e) {
                    const float s = __builtin_fmaf(c[i], c[j], acc[e]);
                    acc[e] = on ? s : acc[e];
                }
            n += on ? 1 : 0;
        }
    }

    // ---- tile sum: entries 0 .. 38, then 39 .. 77 and the count ----
    double* out = partials + ((size_t)pair * (size_t)(a.tiles_x * a.tiles_y) + (size_t)tile) * kAlignRec;
#pragma unroll
    for (int half = 0; half < 2; ++half) {
        if (half) __syncthreads();
#pragma unroll
        for (int e = 0; e < kAlignHalf; ++e) part[e * kAlignPitch + tid] = acc[kAlignHalf * half + e];
        if (half) part[kAlignHalf * kAlignPitch + tid] = (float)n;   // at most 16: exact
        __syncthreads();
        if (tid < kAlignHalf + half) {
            double s = 0.0;
            for (int p = 0; p < kAlignLanes; ++p) s = s + (double)part[tid * kAlignPitch + p];
            out[kAlignHalf * half + tid] = s;
        }
    }
    if (tid == 0) out[kAlignRec - 1] = 0.0;
}

__global__ __launch_bounds__(kAlignLanes) void align_solve_kernel(const double* __restrict__ partials, AlignArgs a, int k, AlignState* __restrict__ state,
                                                                  sift_hip_homography* __restrict__ models, sift_hip_alignment* __restrict__ out,
                                                                  double* __restrict__ sums) {
    __shared__ double red[kAlignBatch * kAlignLanes];
    __shared__ double S[kAlignRec];
    __shared__ double M[kAlignUnknowns * kAlignStride];
    const int tid = threadIdx.x, pair = blockIdx.x, n_tiles = a.tiles_x * a.tiles_y;
    if (!state[pair].active) return;   // the same in every lane: lane 0 writes the record after the last barrier
    const double* __restrict__ mine = partials + (size_t)pair * (size_t)n_tiles * kAlignRec;
    for (int batch = 0; batch < kAlignRec / kAlignBatch; ++batch) {
#pragma unroll
        for (int e = 0; e < kAlignBatch; ++e) {
            double s = 0.0;
            for (int t = tid; t < n_tiles; t += kAlignLanes) s = s + mine[(size_t)t * kAlignRec + kAlignBatch * batch + e];
            red[e * kAlignLanes + tid] = s;
        }
        __syncthreads();
        for (int wd = 1; wd < kAlignLanes; wd *= 2) {   // refine_tree256 on 16 rows at once
            const int per_row = kAlignLanes / (2 * wd);
            for (int i = tid; i < kAlignBatch * per_row; i += kAlignLanes) {
                const int idx = (i / per_row) * kAlignLanes + (i % per_row) * 2 * wd;
                red[idx] = red[idx] + red[idx + wd];
            }
            __syncthreads();
        }
        if (tid < kAlignBatch) S[kAlignBatch * batch + tid] = red[tid * kAlignLanes];
        __syncthreads();
    }
    if (tid < kAlignRec) sums[(size_t)pair * kAlignRec + tid] = S[tid];
    if (tid != 0) return;
    AlignState st = state[pair];
    align_round(st, S, k, a.rounds, a.min_pixels, (double)a.damping, a.nm, M);
    state[pair] = st;
    sift_hip_alignment r;
    align_result(st, r);
    out[pair] = r;
#pragma unroll
    for (int i = 0; i < 9; ++i) models[pair].h[i] = st.acc_h[i];
}

__global__ void align_begin_kernel(const sift_hip_homography* __restrict__ models, int n_pairs, AlignState* __restrict__ state,
                                   sift_hip_alignment* __restrict__ out, double* __restrict__ sums) {
    const int pair = blockIdx.x * blockDim.x + threadIdx.x;
    if (pair >= n_pairs) return;
    AlignState st;
    align_begin(models[pair], st);
    state[pair] = st;
    sift_hip_alignment r;
    align_result(st, r);
    out[pair] = r;
    for (int e = 0; e < kAlignRec; ++e) sums[(size_t)pair * kAlignRec + e] = 0.0;
}

__global__ void tu_probe_align_kernel() {}

void launch_align_begin(hipStream_t s, const sift_hip_homography* d_models, int n_pairs, AlignState* d_state, sift_hip_alignment* d_out, double* d_sums) {
    if (n_pairs <= 0) return;
    hipLaunchKernelGGL(align_begin_kernel, dim3((unsigned)((n_pairs + 63) / 64)), dim3(64), 0, s, d_models, n_pairs, d_state, d_out, d_sums);
}

void launch_align_accumulate(hipStream_t s, const float* d_imgs, const int* d_pair_q, const int* d_pair_t, const AlignState* d_state, const AlignArgs& a,
                             double* d_partials) {
    if (a.n_pairs <= 0) return;
    const dim3 grid((unsigned)(a.tiles_x * a.tiles_y), (unsigned)a.n_pairs);
    if (a.path == 0)
        hipLaunchKernelGGL(align_accumulate_kernel<0>, grid, dim3(kAlignLanes), 0, s, d_imgs, d_pair_q, d_pair_t, d_state, a, d_partials);
    else
        hipLaunchKernelGGL(align_accumulate_kernel<1>, grid, dim3(kAlignLanes), 0, s, d_imgs, d_pair_q, d_pair_t, d_state, a, d_partials);
}

void launch_align_solve(hipStream_t s, const double* d_partials, const AlignArgs& a, int k, AlignState* d_state, sift_hip_homography* d_models,
                        sift_hip_alignment* d_out, double* d_sums) {
    if (a.n_pairs <= 0) return;
    hipLaunchKernelGGL(align_solve_kernel, dim3((unsigned)a.n_pairs), dim3(kAlignLanes), 0, s, d_partials, a, k, d_state, d_models, d_out, d_sums);
}

void tu_touch_align(hipStream_t s) { hipLaunchKernelGGL(tu_probe_align_kernel, dim3(1), dim3(1), 0, s); }

}  // namespace sift_hip
