// 8-bit descriptor matching (include/sift_hip.h, "8-bit descriptors and integer matching"): the quantiser, the integer norms,
// and the tile kernel on the i8 matrix instruction.  Rows are 128 bytes; d2(a, b) = sum (a[k] - b[k])^2 is an exact integer
// <= 128 * 255^2 < 2^24, the same number in every summation order, so nothing here depends on a k order, a tile or a split.
//
// v_mfma_i32_32x32x32_i8 is signed x signed: a row travels as a' = a - 128 (byte ^ 0x80, an int8).  The difference a - b is
// unchanged, so d2 = n'(a) + n'(b) - 2 dot'(a, b) with n'(a) = sum (a[k] - 128)^2 <= 2^21 and |dot'| <= 2^21: exact in int32.
//
// Tile kernel: 256 threads, 4 waves, the partition of the f32 kernel (MatchTile, kMatchQ = 128 query rows a workgroup, stages
// of kMatchT = 64 train rows), so the tables, the merge, the filter and the pack are shared.  Wave w owns query rows 32 w ..
// 32 w + 31 as the B operand: lane (c = lane & 31, h = lane >> 5) holds bytes 32 s + 16 h .. + 15 of row c for step s = 0 .. 3 -
// 16 registers that are loaded from memory once and stay for the whole tile; the query block needs no LDS.  The train stage
// lies in LDS, two buffers, a row of 128 bytes at a stride of 144: the A operand of step s is one 16-byte read at the same
// byte offset of the train row, so A and B agree on which k a lane's bytes are, whatever the instruction's own k-to-lane map.
// Stride 144 bytes = 9 slots of 16 bytes: a ds_read_b128 is served in four groups of 16 lanes, each group holding every residue
// of c mod 16 once (lanes 0-3, 12-15, 20-27 / 4-11, 16-19, 28-31 of a half), and 9 c mod 16 is a bijection on those residues (9 is
// odd) - 16 lanes, 16 different slots, the 64 banks once.  LDS: 2 * 64 * 144 + 2 * 64 * 4 + 2 * 64 = 19 072 bytes.
#include "match_kernels.h"

namespace sift_hip {

namespace {

typedef int i16v __attribute__((ext_vector_type(16)));
typedef int i4v __attribute__((ext_vector_type(4)));
typedef float f4v __attribute__((ext_vector_type(4)));

constexpr int kRowStrideU8 = 144;            // bytes of an LDS row: an odd number of 16-byte slots
constexpr int kNoDist = 0x7fffffff;          // "no entry yet" inside the tile kernel (every d2 is < 2^24)
constexpr float kInf = __builtin_inff();
constexpr int kSignFlip = (int)0x80808080u;  // byte ^ 0x80 = (a - 128) as int8, four at a time

// include/sift_hip.h, "Quantiser"
__device__ __forceinline__ unsigned quantize1(float v) {
    const float t = __fmaf_rn(v, 255.0f, 0.5f);
    return t >= 255.0f ? 255u : (t >= 0.0f ? (unsigned)(int)t : 0u);
}
__device__ __forceinline__ int quantize4(f4v v) {
    return (int)(quantize1(v.x) | (quantize1(v.y) << 8) | (quantize1(v.z) << 16) | (quantize1(v.w) << 24));
}
// sum (a[k] - 128)^2 over the 16 bytes of q
__device__ __forceinline__ int norm16(i4v q) {
    int acc = 0;
#pragma unroll
    for (int w = 0; w < 4; ++w) {
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            const int a = (int)(((unsigned)q[w] >> (8 * b)) & 0xffu) - 128;
            acc += a * a;
        }
    }
    return acc;
}

// (v, j) into the running first two of the order (d2, index) when `take`; j differs from i1 and i2.  Selects, no branches.
__device__ __forceinline__ void top2_insert_i(bool take, int v, int j, int& d1, int& i1, int& d2, int& i2) {
    const bool lt1 = take & ((v < d1) | ((v == d1) & (j < i1)));
    const bool lt2 = take & ((v < d2) | ((v == d2) & (j < i2)));
    const int nd2 = lt1 ? d1 : (lt2 ? v : d2);
    const int ni2 = lt1 ? i1 : (lt2 ? j : i2);
    d1 = lt1 ? v : d1;
    i1 = lt1 ? j : i1;
    d2 = nd2;
    i2 = ni2;
}

}  // namespace

// Streaming: 16 floats in, 16 bytes out per thread.
__global__ __launch_bounds__(256) void match_quantize_kernel(const float* __restrict__ desc, long long n16, uint8_t* __restrict__ out) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n16) return;
    const f4v* src = reinterpret_cast<const f4v*>(desc) + 4 * i;
    i4v q;
#pragma unroll
    for (int w = 0; w < 4; ++w) q[w] = quantize4(src[w]);
    reinterpret_cast<i4v*>(out)[i] = q;
}

// n'(a) and the valid flag of every row; eight threads a row, 16 bytes each, their sums meet through three shuffles.  kQuantize:
// the rows arrive as floats and leave as bytes on the way (the quantiser and the norms in one pass over the descriptors).
template <bool kQuantize>
__global__ __launch_bounds__(256) void match_norm_u8_kernel(const float* __restrict__ desc, const uint8_t* __restrict__ desc8_in,
                                                            uint8_t* __restrict__ desc8_out, const sift_hip_keypoint* __restrict__ kp,
                                                            long long rows, int32_t* __restrict__ norm, uint8_t* __restrict__ valid) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;   // the 16-byte piece; rows * 8 of them
    const long long row = i >> 3;
    int acc = 0;
    if (row < rows) {
        i4v q;
        if constexpr (kQuantize) {
            const f4v* src = reinterpret_cast<const f4v*>(desc) + 4 * i;
#pragma unroll
            for (int w = 0; w < 4; ++w) q[w] = quantize4(src[w]);
            reinterpret_cast<i4v*>(desc8_out)[i] = q;
        } else {
            q = reinterpret_cast<const i4v*>(desc8_in)[i];
        }
        acc = norm16(q);
    }
    acc += __shfl_xor(acc, 1);
    acc += __shfl_xor(acc, 2);
    acc += __shfl_xor(acc, 4);
    if (row < rows && (threadIdx.x & 7) == 0) {
        norm[row] = acc;
        valid[row] = kp ? (kp[row].has_descriptor != 0 ? 1 : 0) : 1;
    }
}

__global__ __launch_bounds__(256) void match_tile_u8_kernel(const uint8_t* __restrict__ desc, const int32_t* __restrict__ norm,
                                                            const uint8_t* __restrict__ valid, const MatchTile* __restrict__ tiles,
                                                            MatchTop2* __restrict__ part) {
    __shared__ __attribute__((aligned(16))) unsigned char st[2][kMatchT * kRowStrideU8];
    __shared__ __attribute__((aligned(16))) int stn[2][kMatchT];
    __shared__ __attribute__((aligned(16))) unsigned char stv[2][kMatchT];

    struct { int q_row0, q_rows, t_set0, t_lo, t_hi; } tl;   // wave-uniform: scalar registers
    tl.q_row0 = tiles[blockIdx.x].q_row0; tl.q_rows = tiles[blockIdx.x].q_rows; tl.t_set0 = tiles[blockIdx.x].t_set0;
    tl.t_lo = tiles[blockIdx.x].t_lo; tl.t_hi = tiles[blockIdx.x].t_hi;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, c = lane & 31, h = lane >> 5;
    const i4v zero4 = {0, 0, 0, 0};

    // the lane's query row: rows past the block's end are zeros, and never read out (their results are not written)
    const int my_q = w * 32 + c;
    i4v b[4];
    int nq = 0;
#pragma unroll
    for (int s = 0; s < 4; ++s) b[s] = zero4;
    if (my_q < tl.q_rows) {
        const i4v* qrow = reinterpret_cast<const i4v*>(desc + (size_t)(tl.q_row0 + my_q) * 128);
#pragma unroll
        for (int s = 0; s < 4; ++s) b[s] = qrow[2 * s + h] ^ kSignFlip;
        nq = norm[tl.q_row0 + my_q];
    }

    const int n_stages = (tl.t_hi - tl.t_lo + kMatchT - 1) / kMatchT;
    i4v pre[2];            // the next stage's rows on their way from memory: fetched before this stage's products, stored after
    int pre_n = 0, pre_v = 0;
    auto fetch = [&](int stage) {
        const int t0 = tl.t_lo + stage * kMatchT;
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int f = tid + 256 * i, r = f >> 3, c16 = f & 7;
            pre[i] = zero4;
            if (t0 + r < tl.t_hi) pre[i] = *reinterpret_cast<const i4v*>(desc + ((size_t)(tl.t_set0 + t0 + r) * 128 + 16 * c16)) ^ kSignFlip;
        }
        if (tid < kMatchT) {
            const bool in = t0 + tid < tl.t_hi;      // rows past the range are masked by index, like invalid ones
            pre_n = in ? norm[tl.t_set0 + t0 + tid] : 0;
            pre_v = in ? (int)valid[tl.t_set0 + t0 + tid] : 0;
        }
    };
    auto stash = [&](int buf) {
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int f = tid + 256 * i, r = f >> 3, c16 = f & 7;
            *reinterpret_cast<i4v*>(&st[buf][r * kRowStrideU8 + 16 * c16]) = pre[i];
        }
        if (tid < kMatchT) {
            stn[buf][tid] = pre_n;
            stv[buf][tid] = (unsigned char)pre_v;
        }
    };

    int d1 = kNoDist, d2 = kNoDist;
    int i1 = kMatchNone, i2 = kMatchNone;
    int thr = kNoDist - nq;   // d2 - nq: a candidate has n'(b) - 2 dot' <= thr, which is d2(a, b) <= d2

    if (n_stages > 0) {
        fetch(0);
        stash(0);
    }
    __syncthreads();

    for (int stage = 0; stage < n_stages; ++stage) {
        const int buf = stage & 1;
        if (stage + 1 < n_stages) fetch(stage + 1);

        const unsigned char* t0row = &st[buf][c * kRowStrideU8 + 16 * h];
        const unsigned char* t1row = t0row + 32 * kRowStrideU8;
        i4v a0[4], a1[4];
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            a0[s] = *reinterpret_cast<const i4v*>(t0row + 32 * s);
            a1[s] = *reinterpret_cast<const i4v*>(t1row + 32 * s);
        }
        // the norms and valid flags of this lane's 32 train rows (4 consecutive rows per read), on their way during the products
        i4v tn[8];
        unsigned tv[8];
#pragma unroll
        for (int g = 0; g < 8; ++g) {
            const int tr0 = (g >> 2) * 32 + 8 * (g & 3) + 4 * h;
            tn[g] = *reinterpret_cast<const i4v*>(&stn[buf][tr0]);
            tv[g] = *reinterpret_cast<const unsigned*>(&stv[buf][tr0]);
        }
        i16v acc0, acc1;
#pragma unroll
        for (int r = 0; r < 16; ++r) { acc0[r] = 0; acc1[r] = 0; }
#pragma unroll
        for (int s = 0; s < 4; ++s) {   // k = 32 s .. 32 s + 31 into the same accumulators
            acc0 = __builtin_amdgcn_mfma_i32_32x32x32_i8(a0[s], b[s], acc0, 0, 0, 0);
            acc1 = __builtin_amdgcn_mfma_i32_32x32x32_i8(a1[s], b[s], acc1, 0, 0, 0);
        }
        // result element r of lane (c, h): train row (r & 3) + 8 (r >> 2) + 4 h of the half, query row c of the wave's 32.
        // Once a few hundred rows have been seen nearly every candidate is farther than the lane's second best: the wave
        // forms n'(b) - 2 dot' and leaves the rest (masks, the order) to the few elements where some lane is not beyond it.
        const int jbase = tl.t_lo + stage * kMatchT;
#pragma unroll
        for (int half = 0; half < 2; ++half) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int tr = half * 32 + (r & 3) + 8 * (r >> 2) + 4 * h;
                const int dot = half ? acc1[r] : acc0[r];
                const int u = tn[half * 4 + (r >> 2)][r & 3] - 2 * dot;
                if (__builtin_amdgcn_ballot_w64(u <= thr) != 0) {
                    const bool row_ok = ((tv[half * 4 + (r >> 2)] >> (8 * (r & 3))) & 0xffu) != 0;
                    top2_insert_i(row_ok, nq + u, jbase + tr, d1, i1, d2, i2);
                    thr = d2 - nq;
                }
            }
        }
        if (stage + 1 < n_stages) stash(buf ^ 1);   // last read in stage - 1, behind that stage's barrier
        __syncthreads();
    }

    // the two lanes of a query row hold disjoint train rows: each takes the other's two entries
    const int od1 = __shfl_xor(d1, 32), od2 = __shfl_xor(d2, 32);
    const int oi1 = __shfl_xor(i1, 32), oi2 = __shfl_xor(i2, 32);
    top2_insert_i(oi1 != kMatchNone, od1, oi1, d1, i1, d2, i2);
    top2_insert_i(oi2 != kMatchNone, od2, oi2, d1, i1, d2, i2);
    if (h == 0 && my_q < tl.q_rows) {
        MatchTop2 o;
        o.d1 = i1 == kMatchNone ? kInf : (float)d1;   // exact: d2 < 2^24
        o.d2 = i2 == kMatchNone ? kInf : (float)d2;
        o.i1 = i1; o.i2 = i2;
        part[(size_t)blockIdx.x * kMatchQ + my_q] = o;
    }
}

void launch_match_quantize(hipStream_t s, const float* d_desc, long long rows, uint8_t* d_out) {
    if (rows <= 0) return;
    const long long n16 = rows * 8;
    hipLaunchKernelGGL(match_quantize_kernel, dim3((unsigned)((n16 + 255) / 256)), dim3(256), 0, s, d_desc, n16, d_out);
}
void launch_match_norms_u8(hipStream_t s, const uint8_t* d_desc8, const sift_hip_keypoint* d_kp, long long rows, int32_t* d_norm, uint8_t* d_valid) {
    if (rows <= 0) return;
    hipLaunchKernelGGL(match_norm_u8_kernel<false>, dim3((unsigned)((rows * 8 + 255) / 256)), dim3(256), 0, s, nullptr, d_desc8, nullptr, d_kp,
                       rows, d_norm, d_valid);
}
void launch_match_quantize_norms(hipStream_t s, const float* d_desc, const sift_hip_keypoint* d_kp, long long rows, uint8_t* d_desc8,
                                 int32_t* d_norm, uint8_t* d_valid) {
    if (rows <= 0) return;
    hipLaunchKernelGGL(match_norm_u8_kernel<true>, dim3((unsigned)((rows * 8 + 255) / 256)), dim3(256), 0, s, d_desc, nullptr, d_desc8, d_kp, rows,
                       d_norm, d_valid);
}
void launch_match_tiles_u8(hipStream_t s, const uint8_t* d_desc8, const int32_t* d_norm, const uint8_t* d_valid, const MatchTile* d_tiles,
                           int n_tiles, MatchTop2* d_part) {
    if (n_tiles <= 0) return;
    hipLaunchKernelGGL(match_tile_u8_kernel, dim3((unsigned)n_tiles), dim3(256), 0, s, d_desc8, d_norm, d_valid, d_tiles, d_part);
}

}  // namespace sift_hip
