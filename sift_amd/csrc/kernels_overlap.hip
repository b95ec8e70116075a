// Overlap statistics and gains (include/sift_hip.h, "overlap statistics"; the definition: overlap_math.h).
//
// With c_i(p) "job i covers canvas pixel p" and q_i(p) its 8-bit intensity there, the statistics are Gram matrices over the pixels:
// N = C^T C, S = Q^T C, SS = (Q.Q)^T C, X = Q^T Q with Q_i = c_i q_i - products of 8-bit numbers summed in integers, the work of
// v_mfma_i32_32x32x32_i8 with the canvas's (at most 32) jobs as the rows and columns and the PIXELS as the k dimension.
//
// One launch covers every canvas.  A workgroup of 256 lanes owns a 64 x 64 region of one canvas and walks it in 16 chunks of
// 64 x 4 = 256 pixels.  Per chunk:
//   map       wave v takes the jobs i = v, v + 4, ... of the canvas; its 64 lanes own the chunk's 64 quads of four x-adjacent
//             pixels, so a job's model is the same in every lane of the wave and ONE ballot says whether the job covers any pixel
//             of the chunk: if not, zeros are stored and no tap is read.  A covered pixel's taps come from global memory through
//             the definition's own functions.  The lane packs its four pixels into one dword per plane and stores four dwords
//             into LDS, [plane][job][pixel] int8:  c,  c (q - 128),  c ((q q >> 8) - 128),  c ((q q & 255) - 128)
//             (the instruction is signed x signed: the matcher's - 128).  Rows of 256 pixels are 272 bytes apart, an odd number
//             of 16-byte slots, so the 32 jobs' 16-byte operand reads fall into different banks.
//   barrier
//   products  the chunk's 8 k-steps of 32 pixels are dealt over the waves, two each.  A lane (c, h) reads bytes 32 s + 16 h ..
//             + 15 of job c of each plane - both operands of every product by the same rule, so any k order would do - and
//             the wave runs  C^T C,  A^T C,  Hi^T C,  Lo^T C,  A^T A  into five 32 x 32 int32 accumulators, 80 registers a lane,
//             kept ACROSS all chunks of the region
//   barrier   (the planes are overwritten by the next chunk)
// |term| <= 2^14 and a chunk has 2^8 pixels, so 511 chunks fit an int32; a region has 16.
// Flush, at the region's end (path = 1: after every chunk, the same sums): the four waves add their accumulators into
// one 5 x 1024 int32 array in LDS (integer adds: no order), 256 lanes undo the offsets for four entries each,
//   S = A^T C + 128 N,  X_ij = (A^T A)_ij + 128 (S_ij + S_ji) - 16384 N_ij,  SS = 256 (Hi^T C + 128 N) + (Lo^T C + 128 N),
// and add the entries with N_ij != 0 to stats[canvas] by 64-bit atomicAdd.  Integer addition commutes: the result does not depend
// on the launch.  Rows and columns >= n stay zero because their LDS rows are zeroed and never written.
//
// overlap_gains_kernel: one wave per canvas, lane r owns row r of [A | b] in LDS and runs the definition's steps.
#include "common.h"
#include "overlap_kernels.h"
#include "overlap_math.h"

namespace sift_hip {

namespace {

typedef int i16v __attribute__((ext_vector_type(16)));
typedef int i4v __attribute__((ext_vector_type(4)));

constexpr int kRedInts = 5 * kOverlapEntries;   // the flush's array

}  // namespace

__global__ __launch_bounds__(kOvlLanes) void overlap_stats_kernel(const float* __restrict__ imgs, int w, int h, const int* __restrict__ src,
                                                                  const float* __restrict__ models, const long long* __restrict__ offsets, OverlapArgs a,
                                                                  unsigned long long* __restrict__ stats) {
    __shared__ __attribute__((aligned(16))) unsigned char planes[kOvlLdsBytes];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, canvas = blockIdx.z;
    const int j0 = (int)offsets[canvas], n = min((int)offsets[canvas + 1] - j0, kOverlapMaxJobs);   // the host refuses more
    if (n <= 0) return;   // the same in every lane of the workgroup
    const int ry0 = blockIdx.y * kOvlRegionH;
    const int n_chunks = min(kOvlChunks, (a.out_h - ry0 + kOvlChunkH - 1) / kOvlChunkH);
    const int x = blockIdx.x * kOvlRegionW + 4 * (lane & 15), yq = lane >> 4;   // the lane's quad within a chunk
    const int c = lane & 31, hh = lane >> 5;                                    // the lane's place in an operand
    unsigned* words = reinterpret_cast<unsigned*>(planes);
    int* red = reinterpret_cast<int*>(planes);
    unsigned long long* out = stats + (size_t)canvas * kOverlapStats;

    for (int i = tid; i < kOvlLdsBytes / 4; i += kOvlLanes) words[i] = 0u;
    __syncthreads();

    i16v acc[5];
#pragma unroll
    for (int k = 0; k < 5; ++k)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[k][r] = 0;

    for (int ch = 0; ch < n_chunks; ++ch) {
        // ---- map ----
        const int y = ry0 + kOvlChunkH * ch + yq;
        const float qy = (float)(y + a.origin_y);
        for (int i = wave; i < n; i += kOvlWaves) {
            const int j = j0 + i;
            float m[9], u[4], v[4];
#pragma unroll
            for (int k = 0; k < 9; ++k) m[k] = models[9 * (size_t)j + k];
            unsigned cov = 0u;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                float W;
                const bool in = warp_coords(m, (float)(x + e + a.origin_x), qy, w, h, u[e], v[e], W) & (x + e < a.out_w) & (y < a.out_h);
                cov |= (in ? 1u : 0u) << e;
            }
            unsigned d0 = 0u, d1 = 0u, d2 = 0u, d3 = 0u;
            if (__builtin_amdgcn_ballot_w64(cov != 0u) != 0) {   // else: zeros, and the job's image is not touched
                const float* __restrict__ s = imgs + (size_t)(src ? src[j] : j) * (size_t)w * (size_t)h;
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    if (!((cov >> e) & 1u)) continue;
                    const int q = overlap_q(s, w, h, u[e], v[e], a.scale, a.interp), qq = q * q;
                    d0 |= 1u << (8 * e);
                    d1 |= (unsigned)((q - 128) & 255) << (8 * e);
                    d2 |= (unsigned)(((qq >> 8) - 128) & 255) << (8 * e);
                    d3 |= (unsigned)(((qq & 255) - 128) & 255) << (8 * e);
                }
            }
            unsigned* row = words + (i * kOvlRowBytes) / 4 + lane;
            row[0] = d0;
            row[kOvlPlaneBytes / 4] = d1;
            row[2 * kOvlPlaneBytes / 4] = d2;
            row[3 * kOvlPlaneBytes / 4] = d3;
        }
        __syncthreads();

        // ---- products: k-steps wave and wave + 4 ----
#pragma unroll
        for (int s = 0; s < kOvlChunkPx / 32 / kOvlWaves; ++s) {
            const unsigned char* p = planes + c * kOvlRowBytes + 32 * (wave + kOvlWaves * s) + 16 * hh;
            const i4v C = *reinterpret_cast<const i4v*>(p), A = *reinterpret_cast<const i4v*>(p + kOvlPlaneBytes);
            const i4v Hi = *reinterpret_cast<const i4v*>(p + 2 * kOvlPlaneBytes), Lo = *reinterpret_cast<const i4v*>(p + 3 * kOvlPlaneBytes);
            acc[0] = __builtin_amdgcn_mfma_i32_32x32x32_i8(C, C, acc[0], 0, 0, 0);
            acc[1] = __builtin_amdgcn_mfma_i32_32x32x32_i8(A, C, acc[1], 0, 0, 0);
            acc[2] = __builtin_amdgcn_mfma_i32_32x32x32_i8(Hi, C, acc[2], 0, 0, 0);
            acc[3] = __builtin_amdgcn_mfma_i32_32x32x32_i8(Lo, C, acc[3], 0, 0, 0);
            acc[4] = __builtin_amdgcn_mfma_i32_32x32x32_i8(A, A, acc[4], 0, 0, 0);
        }
        __syncthreads();

        // ---- flush ----
        const bool last = ch == n_chunks - 1;
        if (!last && a.path == 0) continue;
        for (int i = tid; i < kRedInts; i += kOvlLanes) red[i] = 0;
        __syncthreads();
#pragma unroll
        for (int k = 0; k < 5; ++k)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                // element r of lane (c, hh): row (r & 3) + 8 (r >> 2) + 4 hh (the first operand's job), column c (the second's)
                const int e = ((r & 3) + 8 * (r >> 2) + 4 * hh) * kOverlapMaxJobs + c;
                if (acc[k][r] != 0) atomicAdd(&red[k * kOverlapEntries + e], acc[k][r]);
                acc[k][r] = 0;
            }
        __syncthreads();
        for (int e = tid; e < kOverlapEntries; e += kOvlLanes) {
            const long long N = red[e];
            if (N == 0) continue;   // then every plane's entry is zero
            const int et = (e & 31) * kOverlapMaxJobs + (e >> 5);
            const long long S = (long long)red[kOverlapEntries + e] + 128 * N, St = (long long)red[kOverlapEntries + et] + 128 * N;
            const long long SS = 256 * ((long long)red[2 * kOverlapEntries + e] + 128 * N) + ((long long)red[3 * kOverlapEntries + e] + 128 * N);
            const long long X = (long long)red[4 * kOverlapEntries + e] + 128 * (S + St) - 16384 * N;
            atomicAdd(&out[e], (unsigned long long)N);
            if (S) atomicAdd(&out[kOverlapEntries + e], (unsigned long long)S);
            if (SS) atomicAdd(&out[2 * kOverlapEntries + e], (unsigned long long)SS);
            if (X) atomicAdd(&out[3 * kOverlapEntries + e], (unsigned long long)X);
        }
        if (last) break;
        __syncthreads();
        for (int i = tid; i < kRedInts; i += kOvlLanes) red[i] = 0;   // the rows >= n among them: zero again
        __syncthreads();
    }
}

// One wave per canvas.  Lane r < n forms and owns row r; the pivot search reads one column and is done by every lane alike; the
// exchange of rows k and p is dealt over the lanes by column.
__global__ __launch_bounds__(64) void overlap_gains_kernel(const long long* __restrict__ stats, const long long* __restrict__ offsets, float sigma_n,
                                                           float sigma_g, float* __restrict__ gains, uint8_t* __restrict__ status) {
    __shared__ double M[kOverlapMaxJobs * kGainStride];
    __shared__ double xs[kOverlapMaxJobs];
    const int lane = threadIdx.x, canvas = blockIdx.x;
    const long long j0 = offsets[canvas];
    const int n = min((int)(offsets[canvas + 1] - j0), kOverlapMaxJobs);
    const int64_t* st = reinterpret_cast<const int64_t*>(stats) + (size_t)canvas * kOverlapStats;
    if (lane < n) gain_row(st, n, lane, gain_weight(sigma_n), gain_weight(sigma_g), M + kGainStride * lane);
    __syncthreads();
    bool ok = true;
    for (int k = 0; k < n; ++k) {
        const int p = gain_pivot(M, n, k, ok);
        if (!ok) break;   // the same in every lane
        __syncthreads();
        if (lane <= n && p != k) {
            const double t = M[kGainStride * k + lane];
            M[kGainStride * k + lane] = M[kGainStride * p + lane];
            M[kGainStride * p + lane] = t;
        }
        __syncthreads();
        if (lane > k && lane < n) gain_eliminate_row(M, n, k, lane);
        __syncthreads();
    }
    if (lane != 0) return;
    if (ok) gain_backsubstitute(M, n, xs);
    const int bad = gain_finish(xs, ok, n, gains + j0);
    if (status) status[canvas] = (uint8_t)bad;
}

__global__ void tu_probe_overlap_kernel() {}

void launch_overlap_stats(hipStream_t s, const float* d_imgs, int w, int h, const int* d_src, const float* d_models, const long long* d_offsets,
                          int n_canvases, const OverlapArgs& a, long long* d_stats) {
    if (n_canvases <= 0) return;
    const dim3 grid((unsigned)((a.out_w + kOvlRegionW - 1) / kOvlRegionW), (unsigned)((a.out_h + kOvlRegionH - 1) / kOvlRegionH), (unsigned)n_canvases);
    hipLaunchKernelGGL(overlap_stats_kernel, grid, dim3(kOvlLanes), 0, s, d_imgs, w, h, d_src, d_models, d_offsets, a,
                       reinterpret_cast<unsigned long long*>(d_stats));
}

void launch_overlap_gains(hipStream_t s, const long long* d_stats, const long long* d_offsets, int n_canvases, float sigma_n, float sigma_g,
                          float* d_gains, uint8_t* d_status) {
    if (n_canvases <= 0) return;
    hipLaunchKernelGGL(overlap_gains_kernel, dim3((unsigned)n_canvases), dim3(64), 0, s, d_stats, d_offsets, sigma_n, sigma_g, d_gains, d_status);
}

void tu_touch_overlap(hipStream_t s) { hipLaunchKernelGGL(tu_probe_overlap_kernel, dim3(1), dim3(1), 0, s); }

}  // namespace sift_hip
