// Descriptor matching (include/sift_hip.h, "descriptor matching"): squared distances of 128-float rows on the f32 matrix
// instruction, top-2 per query row, ratio test, cross-check, ordered compaction.  The one place of this library that uses MFMA.
//
// The result is DEFINED, bit for bit: dot(a, b) is the k-ascending fmaf chain from +0.0f, d2 = max0(n(a) + n(b) - 2 dot(a, b)),
// candidates ordered by (d2, index).  v_mfma_f32_32x32x2_f32 is that chain: D = fma(a[k+1], b[k+1], fma(a[k], b[k], C)), one
// rounding per product, no wider accumulator - so 64 of them into ONE accumulator, k ascending, give the chain's value, and a
// ten-line host loop (hostmath_match_knn2) checks every bit.  -ffp-contract=off as everywhere: the epilogue's n(a) + n(b) and
// s - 2 * dot are one rounding each (2 * dot is exact).
//
// Tile kernel: 256 threads, 4 waves.  LDS: 128 query rows + 2 stages of 64 train rows, 132 floats a row = 67 584 + 67 584 bytes
// (+ the stages' norms and valid flags) of the CU's 160 KB.  A row is stored with its even k first and its odd k second: lane
// (c = lane & 31, h = lane >> 5) of the instruction holds element k = 2 s + h of row c in step s, so four steps are one
// 16-byte read of floats 64 h + 4 m .. + 3 of the row.  Row stride 132 floats = 4 banks on: 16 lanes of such a read cover the
// 64 banks once.  Wave w owns query rows 32 w .. 32 w + 31 as the B operand (the result's column, i.e. the lane) and both
// 32-row halves of the train stage as A operands: two independent accumulator tiles.  A lane then holds ONE query row and 16
// train rows per tile in its registers, so the running top-2 is four registers per lane and needs no cross-lane step until
// the end, where the two lanes of a query row (h = 0, 1) merge through one shuffle.
#include <algorithm>

#include "match_kernels.h"
#include "ransac_fund_math.h"   // ransac_inlier, ransac_fund_inlier: the guided instantiations' admissibility test

namespace sift_hip {

namespace {

typedef float f16v __attribute__((ext_vector_type(16)));
typedef float f4v __attribute__((ext_vector_type(4)));
typedef float f2v __attribute__((ext_vector_type(2)));

constexpr int kRowStride = 132;   // floats of an LDS row
constexpr float kInf = __builtin_inff();

// (v, j) into the running first two of the order (d2, index) when `take`; j differs from i1 and i2.  Selects, no branches.
__device__ __forceinline__ void top2_insert(bool take, float v, int j, float& d1, int& i1, float& d2, int& i2) {
    const bool lt1 = take & ((v < d1) | ((v == d1) & (j < i1)));
    const bool lt2 = take & ((v < d2) | ((v == d2) & (j < i2)));
    const float nd2 = lt1 ? d1 : (lt2 ? v : d2);
    const int ni2 = lt1 ? i1 : (lt2 ? j : i2);
    d1 = lt1 ? v : d1;
    i1 = lt1 ? j : i1;
    d2 = nd2;
    i2 = ni2;
}

// 4 floats k .. k+3 of a row -> the row's LDS image (even k at k / 2, odd k at 64 + k / 2)
__device__ __forceinline__ void store_row4(float* row, int c4, f4v v) {
    f2v e = {v.x, v.z}, o = {v.y, v.w};
    *reinterpret_cast<f2v*>(row + 2 * c4) = e;
    *reinterpret_cast<f2v*>(row + 64 + 2 * c4) = o;
}

// The guide of a tile kernel instantiation (include/sift_hip.h, "guided matching"): none, or one of the two verification
// predicates, called with the arguments the RANSAC kernels give them.
struct NoGuide {
    static constexpr bool kOn = false;
    static __device__ __forceinline__ bool admissible(const float (&)[9], float, float, float, float, float) { return true; }
};
struct HomographyGuide {
    static constexpr bool kOn = true;
    static __device__ __forceinline__ bool admissible(const float (&m)[9], float qx, float qy, float tx, float ty, float thr2) {
        return ransac_inlier(m, qx, qy, tx, ty, thr2);
    }
};
struct FundamentalGuide {
    static constexpr bool kOn = true;
    static __device__ __forceinline__ bool admissible(const float (&m)[9], float qx, float qy, float tx, float ty, float thr2) {
        return ransac_fund_inlier(m, qx, qy, tx, ty, thr2);
    }
};

}  // namespace

// n(a) = dot(a, a) as the chain, and the row's valid flag.  64 rows per workgroup: fetched coalesced into LDS (129 floats a row:
// the 64 chains then read 64 different banks), one thread per row runs the chain.
__global__ __launch_bounds__(256) void match_norm_kernel(const float* __restrict__ desc, const sift_hip_keypoint* __restrict__ kp, long long rows,
                                                         float* __restrict__ norm, uint8_t* __restrict__ valid) {
    __shared__ float s[64 * 129];
    const long long row0 = (long long)blockIdx.x * 64;
    const int n = (int)min((long long)64, rows - row0);
    for (int f = threadIdx.x; f < n * 128; f += 256) s[(f >> 7) * 129 + (f & 127)] = desc[(size_t)row0 * 128 + f];
    __syncthreads();
    const int r = threadIdx.x;
    if (r < n) {
        float acc = 0.0f;
#pragma unroll 16
        for (int k = 0; k < 128; ++k) acc = __fmaf_rn(s[r * 129 + k], s[r * 129 + k], acc);
        norm[row0 + r] = acc;
        valid[row0 + r] = kp ? (kp[row0 + r].has_descriptor != 0 ? 1 : 0) : 1;
    }
}

// Guide::kOn: a candidate also has to be admissible under its pair's model.  The stage's train coordinates travel with its norms
// and flags; the lane's own point stays in two registers, the tile's model and direction are wave-uniform.  In a tile of the
// cross-check (direction 1) the lane holds a train row and the stage's rows are query rows: the predicate's arguments keep their
// meaning, so the two points change places, not the model.  Admissibility does not depend on the products: a lane forms the 32
// bits of its stage rows two at a time behind each group of eight matrix instructions, and the epilogue's ballot asks for an
// admissible candidate - under a narrow band nearly every element is skipped although the lane's second best is still +inf.
// (Little of that arithmetic runs under the products yet: DESIGN.md 3d has the cost and what was tried.)
template <class Guide>
__global__ __launch_bounds__(256) void match_tile_kernel(const float* __restrict__ desc, const float* __restrict__ norm,
                                                         const uint8_t* __restrict__ valid, const MatchTile* __restrict__ tiles,
                                                         MatchTop2* __restrict__ part, MatchGuideArgs ga) {
    __shared__ __attribute__((aligned(16))) float sq[kMatchQ * kRowStride];
    __shared__ __attribute__((aligned(16))) float st[2][kMatchT * kRowStride];
    __shared__ __attribute__((aligned(16))) float stn[2][kMatchT];
    __shared__ __attribute__((aligned(16))) unsigned char stv[2][kMatchT];
    __shared__ __attribute__((aligned(16))) float stxy[2][Guide::kOn ? 2 * kMatchT : 4];   // (x, y) of the stage's rows

    struct { int q_row0, q_rows, t_set0, t_lo, t_hi; } tl;   // wave-uniform: scalar registers
    tl.q_row0 = tiles[blockIdx.x].q_row0; tl.q_rows = tiles[blockIdx.x].q_rows; tl.t_set0 = tiles[blockIdx.x].t_set0;
    tl.t_lo = tiles[blockIdx.x].t_lo; tl.t_hi = tiles[blockIdx.x].t_hi;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, c = lane & 31, h = lane >> 5;
    const f4v zero4 = {0.0f, 0.0f, 0.0f, 0.0f};

    // the query block: rows past the block's end are zeros, and never read out (their results are not written)
    for (int f = tid; f < kMatchQ * 32; f += 256) {
        const int r = f >> 5, c4 = f & 31;
        f4v v = zero4;
        if (r < tl.q_rows) v = *reinterpret_cast<const f4v*>(desc + ((size_t)(tl.q_row0 + r) * 128 + 4 * c4));
        store_row4(sq + r * kRowStride, c4, v);
    }
    const int my_q = w * 32 + c;
    const float nq = my_q < tl.q_rows ? norm[tl.q_row0 + my_q] : 0.0f;
    float gm[9] = {};        // the tile's model (scalar registers)
    bool swapped = false;    // a tile of the cross-check: the lane's row is the train row of the predicate
    float lx = 0.0f, ly = 0.0f;
    if constexpr (Guide::kOn) {
        const int pd = tiles[blockIdx.x].pair_dir;
        swapped = (pd & 1) != 0;
#pragma unroll
        for (int k = 0; k < 9; ++k) gm[k] = ga.models[9 * (size_t)(pd >> 1) + k];
        if (my_q < tl.q_rows) {
            lx = ga.xy[2 * (size_t)(tl.q_row0 + my_q)];
            ly = ga.xy[2 * (size_t)(tl.q_row0 + my_q) + 1];
        }
    }

    const int n_stages = (tl.t_hi - tl.t_lo + kMatchT - 1) / kMatchT;
    f4v pre[8];            // the next stage's rows on their way from memory: fetched before this stage's products, stored after
    float pre_n = 0.0f;
    int pre_v = 0;
    f2v pre_xy = {0.0f, 0.0f};
    auto fetch = [&](int stage) {
        const int t0 = tl.t_lo + stage * kMatchT;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int f = tid + 256 * i, r = f >> 5, c4 = f & 31;
            pre[i] = zero4;
            if (t0 + r < tl.t_hi) pre[i] = *reinterpret_cast<const f4v*>(desc + ((size_t)(tl.t_set0 + t0 + r) * 128 + 4 * c4));
        }
        if (tid < kMatchT) {
            const bool in = t0 + tid < tl.t_hi;      // rows past the range are masked by index, like invalid ones
            pre_n = in ? norm[tl.t_set0 + t0 + tid] : 0.0f;
            pre_v = in ? (int)valid[tl.t_set0 + t0 + tid] : 0;
            if constexpr (Guide::kOn) {
                pre_xy.x = in ? ga.xy[2 * (size_t)(tl.t_set0 + t0 + tid)] : 0.0f;
                pre_xy.y = in ? ga.xy[2 * (size_t)(tl.t_set0 + t0 + tid) + 1] : 0.0f;
            }
        }
    };
    auto stash = [&](int buf) {
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int f = tid + 256 * i, r = f >> 5, c4 = f & 31;
            store_row4(st[buf] + r * kRowStride, c4, pre[i]);
        }
        if (tid < kMatchT) {
            stn[buf][tid] = pre_n;
            stv[buf][tid] = (unsigned char)pre_v;
            if constexpr (Guide::kOn) *reinterpret_cast<f2v*>(&stxy[buf][2 * tid]) = pre_xy;
        }
    };

    float d1 = kInf, d2 = kInf;
    int i1 = kMatchNone, i2 = kMatchNone;

    if (n_stages > 0) {
        fetch(0);
        stash(0);
    }
    __syncthreads();

    const float* qrow = sq + my_q * kRowStride + 64 * h;
    for (int stage = 0; stage < n_stages; ++stage) {
        const int buf = stage & 1;
        if (stage + 1 < n_stages) fetch(stage + 1);

        const float* t0row = st[buf] + c * kRowStride + 64 * h;
        const float* t1row = t0row + 32 * kRowStride;
        // the norms and valid flags of this lane's 32 train rows (4 consecutive rows per read), on their way during the products
        f4v tn[8];
        unsigned tv[8];
#pragma unroll
        for (int g = 0; g < 8; ++g) {
            const int tr0 = (g >> 2) * 32 + 8 * (g & 3) + 4 * h;
            tn[g] = *reinterpret_cast<const f4v*>(&stn[buf][tr0]);
            tv[g] = *reinterpret_cast<const unsigned*>(&stv[buf][tr0]);
        }
        // guided: the coordinates of the same rows, two consecutive rows per read - result elements 2 m and 2 m + 1 of the 32
        f4v cxy[Guide::kOn ? 16 : 1];
        unsigned adm = 0u;   // bit 16 half + r: the row of result element r of that half is admissible
        if constexpr (Guide::kOn) {
#pragma unroll
            for (int m = 0; m < 16; ++m) {
                const int r = 2 * (m & 7), tr0 = (m >> 3) * 32 + (r & 3) + 8 * (r >> 2) + 4 * h;
                cxy[m] = *reinterpret_cast<const f4v*>(&stxy[buf][2 * tr0]);
            }
        }
        f16v acc0, acc1;
#pragma unroll
        for (int r = 0; r < 16; ++r) { acc0[r] = 0.0f; acc1[r] = 0.0f; }
        // 16 groups of 4 steps: k = 8 m + 2 e + h, e = 0 .. 3, ascending into the same accumulators.  Group m + 1's operands
        // are read from LDS before group m's products are issued, so the reads' latency runs under 8 instructions of 64 cycles.
        f4v b[2], a0[2], a1[2];
        b[0] = *reinterpret_cast<const f4v*>(qrow);
        a0[0] = *reinterpret_cast<const f4v*>(t0row);
        a1[0] = *reinterpret_cast<const f4v*>(t1row);
#pragma unroll
        for (int m = 0; m < 16; ++m) {
            const int cur = m & 1, nxt = cur ^ 1;
            if (m + 1 < 16) {
                b[nxt] = *reinterpret_cast<const f4v*>(qrow + 4 * (m + 1));
                a0[nxt] = *reinterpret_cast<const f4v*>(t0row + 4 * (m + 1));
                a1[nxt] = *reinterpret_cast<const f4v*>(t1row + 4 * (m + 1));
            }
            __builtin_amdgcn_sched_barrier(0);   // the next group's reads are issued in front of this group's products ...
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a0[cur][e], b[cur][e], acc0, 0, 0, 0);
                acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a1[cur][e], b[cur][e], acc1, 0, 0, 0);
            }
            if constexpr (Guide::kOn) {
#pragma unroll
                for (int u = 0; u < 2; ++u) {
                    const float ex = u ? cxy[m].z : cxy[m].x, ey = u ? cxy[m].w : cxy[m].y;
                    // the direction is wave-uniform: a branch, and in each arm the predicate has its arguments in their places,
                    // so what depends on the lane's own point alone is one computation for all calls - the same roundings
                    const bool ok = swapped ? Guide::admissible(gm, ex, ey, lx, ly, ga.thr2) : Guide::admissible(gm, lx, ly, ex, ey, ga.thr2);
                    adm |= ok ? (1u << (2 * m + u)) : 0u;
                }
                asm volatile("" : "+v"(adm));   // the two bits are formed here, behind this group's products, not in the epilogue
            }
            __builtin_amdgcn_sched_barrier(0);   // ... and are not moved behind them
        }
        // result element r of lane (c, h): train row (r & 3) + 8 (r >> 2) + 4 h of the half, query row c of the wave's 32.
        // Once a few hundred rows have been seen nearly every candidate is farther than the lane's second best: the wave
        // forms s - 2 dot and leaves the rest (clamp, masks, the order) to the few elements where some lane is not beyond it
        // (a NaN and a negative value fail the test and take the full path).
        const int jbase = tl.t_lo + stage * kMatchT;
#pragma unroll
        for (int half = 0; half < 2; ++half) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int tr = half * 32 + (r & 3) + 8 * (r >> 2) + 4 * h;
                const float dot = half ? acc1[r] : acc0[r];
                const float sum = nq + tn[half * 4 + (r >> 2)][r & 3];
                float v = sum - 2.0f * dot;
                bool cand = !(v > d2);
                if constexpr (Guide::kOn) cand &= ((adm >> (16 * half + r)) & 1u) != 0;
                if (__builtin_amdgcn_ballot_w64(cand) != 0) {
                    v = (v < 0.0f) ? 0.0f : v;
                    bool row_ok = ((tv[half * 4 + (r >> 2)] >> (8 * (r & 3))) & 0xffu) != 0;
                    if constexpr (Guide::kOn) row_ok &= ((adm >> (16 * half + r)) & 1u) != 0;
                    top2_insert(row_ok & (v == v), v, jbase + tr, d1, i1, d2, i2);
                }
            }
        }
        if (stage + 1 < n_stages) stash(buf ^ 1);   // last read in stage - 1, behind that stage's barrier
        __syncthreads();
    }

    // the two lanes of a query row hold disjoint train rows: each takes the other's two entries
    const float od1 = __shfl_xor(d1, 32), od2 = __shfl_xor(d2, 32);
    const int oi1 = __shfl_xor(i1, 32), oi2 = __shfl_xor(i2, 32);
    top2_insert(oi1 != kMatchNone, od1, oi1, d1, i1, d2, i2);
    top2_insert(oi2 != kMatchNone, od2, oi2, d1, i1, d2, i2);
    if (h == 0 && my_q < tl.q_rows) {
        MatchTop2 o;
        o.d1 = d1; o.d2 = d2; o.i1 = i1; o.i2 = i2;
        part[(size_t)blockIdx.x * kMatchQ + my_q] = o;
    }
}

// the image coordinates of every keypoint record, as sift_hip_result_verify gathers them per match: (float)(x << octave) * scale
__global__ __launch_bounds__(256) void match_coords_kernel(const sift_hip_keypoint* __restrict__ kp, long long rows, float coord_scale,
                                                           float* __restrict__ xy) {
    const long long row = (long long)blockIdx.x * 256 + threadIdx.x;
    if (row >= rows) return;
    const sift_hip_keypoint k = kp[row];
    f2v o;
    o.x = (float)((uint32_t)k.x << k.octave) * coord_scale;
    o.y = (float)((uint32_t)k.y << k.octave) * coord_scale;
    *reinterpret_cast<f2v*>(xy + 2 * (size_t)row) = o;
}

// the partial top-2s of a block's tiles -> its rows of the result, by the same order; an invalid query row has no entry
__global__ __launch_bounds__(kMatchQ) void match_merge_kernel(const MatchTop2* __restrict__ part, const uint8_t* __restrict__ valid,
                                                              const MatchBlock* __restrict__ blocks, int32_t* __restrict__ idx,
                                                              float* __restrict__ dist) {
    const MatchBlock b = blocks[blockIdx.x];
    const int r = threadIdx.x;
    if (r >= b.q_rows) return;
    float d1 = kInf, d2 = kInf;
    int i1 = kMatchNone, i2 = kMatchNone;
    if (valid[b.q_row0 + r] != 0) {
        for (int t = 0; t < b.n_tiles; ++t) {
            const MatchTop2 p = part[(size_t)(b.first_tile + t) * kMatchQ + r];
            top2_insert(p.i1 != kMatchNone, p.d1, p.i1, d1, i1, d2, i2);
            top2_insert(p.i2 != kMatchNone, p.d2, p.i2, d1, i1, d2, i2);
        }
    }
    const size_t o = (size_t)(b.out_row0 + r) * 2;
    idx[o] = i1 == kMatchNone ? -1 : i1;
    idx[o + 1] = i2 == kMatchNone ? -1 : i2;
    dist[o] = i1 == kMatchNone ? kInf : d1;
    dist[o + 1] = i2 == kMatchNone ? kInf : d2;
}

// One workgroup per pair walks the pair's query rows 256 at a time: ratio test, cross-check, and the kept rows' records in
// query order at the pair's own segment (ballot + popcount inside a wave, the waves' totals through LDS).  No atomics.
__global__ __launch_bounds__(256) void match_filter_kernel(const int32_t* __restrict__ idx, const float* __restrict__ dist,
                                                           const MatchPair* __restrict__ pairs, int use_ratio, float ratio2, int cross_check,
                                                           sift_hip_match_rec* __restrict__ seg, int32_t* __restrict__ counts) {
    __shared__ int wave_total[4];
    const MatchPair p = pairs[blockIdx.x];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    int kept = 0;   // records of this pair so far (the same in every thread)
    for (int base = 0; base < p.rows; base += 256) {
        const int i = base + tid;
        bool keep = false;
        sift_hip_match_rec rec;
        rec.query = i; rec.train = -1; rec.dist2 = kInf; rec.second2 = kInf;
        if (i < p.rows) {
            const size_t o = (size_t)(p.row0 + i) * 2;
            rec.train = idx[o];
            rec.dist2 = dist[o];
            rec.second2 = dist[o + 1];
            keep = rec.train >= 0;
            if (keep && use_ratio) keep = rec.dist2 < ratio2 * rec.second2;
            if (keep && cross_check) keep = idx[(size_t)(p.rev_row0 + rec.train) * 2] == i;
        }
        const unsigned long long m = __ballot(keep);
        const int before = __popcll(m & ((1ull << lane) - 1ull));
        if (lane == 0) wave_total[w] = __popcll(m);
        __syncthreads();
        int off = kept;
        for (int k = 0; k < w; ++k) off += wave_total[k];
        if (keep) seg[(size_t)p.row0 + off + before] = rec;
        kept += wave_total[0] + wave_total[1] + wave_total[2] + wave_total[3];
        __syncthreads();
    }
    if (tid == 0) counts[blockIdx.x] = kept;
}

// the pairs' segments -> one dense list in pair order (a pair's place is the sum of the counts before it)
__global__ __launch_bounds__(256) void match_pack_kernel(const sift_hip_match_rec* __restrict__ seg, const MatchPair* __restrict__ pairs,
                                                         const int32_t* __restrict__ counts, sift_hip_match_rec* __restrict__ out) {
    __shared__ long long partial[256];
    const int tid = threadIdx.x;
    long long sum = 0;
    for (int k = tid; k < (int)blockIdx.x; k += 256) sum += counts[k];
    partial[tid] = sum;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (tid < s) partial[tid] += partial[tid + s];
        __syncthreads();
    }
    const long long base = partial[0];
    const MatchPair p = pairs[blockIdx.x];
    const int n = counts[blockIdx.x];
    for (int i = tid; i < n; i += 256) out[base + i] = seg[(size_t)p.row0 + i];
}

void launch_match_norms(hipStream_t s, const float* d_desc, const sift_hip_keypoint* d_kp, long long rows, float* d_norm, uint8_t* d_valid) {
    if (rows <= 0) return;
    hipLaunchKernelGGL(match_norm_kernel, dim3((unsigned)((rows + 63) / 64)), dim3(256), 0, s, d_desc, d_kp, rows, d_norm, d_valid);
}
void launch_match_tiles(hipStream_t s, const float* d_desc, const float* d_norm, const uint8_t* d_valid, const MatchTile* d_tiles,
                        int n_tiles, MatchTop2* d_part) {
    if (n_tiles <= 0) return;
    hipLaunchKernelGGL(match_tile_kernel<NoGuide>, dim3((unsigned)n_tiles), dim3(256), 0, s, d_desc, d_norm, d_valid, d_tiles, d_part, MatchGuideArgs{});
}
void launch_match_tiles_guided(hipStream_t s, const float* d_desc, const float* d_norm, const uint8_t* d_valid, const MatchTile* d_tiles,
                               int n_tiles, MatchTop2* d_part, int model, const MatchGuideArgs& ga) {
    if (n_tiles <= 0) return;
    if (model == SIFT_HIP_GUIDE_FUNDAMENTAL)
        hipLaunchKernelGGL(match_tile_kernel<FundamentalGuide>, dim3((unsigned)n_tiles), dim3(256), 0, s, d_desc, d_norm, d_valid, d_tiles, d_part, ga);
    else
        hipLaunchKernelGGL(match_tile_kernel<HomographyGuide>, dim3((unsigned)n_tiles), dim3(256), 0, s, d_desc, d_norm, d_valid, d_tiles, d_part, ga);
}
void launch_match_coords(hipStream_t s, const sift_hip_keypoint* d_kp, long long rows, float coord_scale, float* d_xy) {
    if (rows <= 0) return;
    hipLaunchKernelGGL(match_coords_kernel, dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, s, d_kp, rows, coord_scale, d_xy);
}
void launch_match_merge(hipStream_t s, const MatchTop2* d_part, const uint8_t* d_valid, const MatchBlock* d_blocks, int n_blocks,
                        int32_t* d_idx, float* d_dist) {
    if (n_blocks <= 0) return;
    hipLaunchKernelGGL(match_merge_kernel, dim3((unsigned)n_blocks), dim3(kMatchQ), 0, s, d_part, d_valid, d_blocks, d_idx, d_dist);
}
void launch_match_filter(hipStream_t s, const int32_t* d_idx, const float* d_dist, const MatchPair* d_pairs, int n_pairs, int use_ratio,
                         float ratio2, int cross_check, sift_hip_match_rec* d_seg, int32_t* d_counts) {
    if (n_pairs <= 0) return;
    hipLaunchKernelGGL(match_filter_kernel, dim3((unsigned)n_pairs), dim3(256), 0, s, d_idx, d_dist, d_pairs, use_ratio, ratio2, cross_check,
                       d_seg, d_counts);
}
void launch_match_pack(hipStream_t s, const sift_hip_match_rec* d_seg, const MatchPair* d_pairs, const int32_t* d_counts, int n_pairs,
                       sift_hip_match_rec* d_out) {
    if (n_pairs <= 0) return;
    hipLaunchKernelGGL(match_pack_kernel, dim3((unsigned)n_pairs), dim3(256), 0, s, d_seg, d_pairs, d_counts, d_out);
}

__global__ void tu_probe_match_kernel() {}
void tu_touch_match(hipStream_t s) { hipLaunchKernelGGL(tu_probe_match_kernel, dim3(1), dim3(1), 0, s); }

}  // namespace sift_hip
