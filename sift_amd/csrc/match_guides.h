// The guide of a tile kernel instantiation (include/sift_hip.h, "guided matching"): none, or one of the two verification
// predicates.  The f32 tile kernel (kernels_match.hip) calls admissible(), the predicate with the arguments the RANSAC kernels
// give it; the 8-bit tile kernel (kernels_match_u8.hip) composes the same bit from the predicate's parts (ransac_math.h,
// ransac_fund_math.h): kQueryN / kTrainN of a part's four floats are in use.
#pragma once
#include <hip/hip_runtime.h>

#include "ransac_fund_math.h"  // ransac_inlier, ransac_fund_inlier and their parts

namespace sift_hip {

struct NoGuide {
    static constexpr bool kOn = false;
    static constexpr int kQueryN = 0, kTrainN = 0;
    static __device__ __forceinline__ bool admissible(const float (&)[9], float, float, float, float, float) { return true; }
    static __device__ __forceinline__ void query_part(const float (&)[9], float, float, float, float (&)[4]) {}
    static __device__ __forceinline__ void train_part(const float (&)[9], float, float, float (&)[4]) {}
    static __device__ __forceinline__ bool tail(const float (&)[4], const float (&)[4], float) { return true; }
};
struct HomographyGuide {
    static constexpr bool kOn = true;
    static constexpr int kQueryN = 4, kTrainN = 2;
    static __device__ __forceinline__ bool admissible(const float (&m)[9], float qx, float qy, float tx, float ty, float thr2) {
        return ransac_inlier(m, qx, qy, tx, ty, thr2);
    }
    static __device__ __forceinline__ void query_part(const float (&m)[9], float qx, float qy, float thr2, float (&p)[4]) {
        ransac_inlier_query(m, qx, qy, thr2, p);
    }
    static __device__ __forceinline__ void train_part(const float (&m)[9], float tx, float ty, float (&p)[4]) { ransac_inlier_train(m, tx, ty, p); }
    static __device__ __forceinline__ bool tail(const float (&q)[4], const float (&t)[4], float thr2) { return ransac_inlier_tail(q, t, thr2); }
};
struct FundamentalGuide {
    static constexpr bool kOn = true;
    static constexpr int kQueryN = 3, kTrainN = 3;
    static __device__ __forceinline__ bool admissible(const float (&m)[9], float qx, float qy, float tx, float ty, float thr2) {
        return ransac_fund_inlier(m, qx, qy, tx, ty, thr2);
    }
    static __device__ __forceinline__ void query_part(const float (&m)[9], float qx, float qy, float thr2, float (&p)[4]) {
        ransac_fund_inlier_query(m, qx, qy, thr2, p);
    }
    static __device__ __forceinline__ void train_part(const float (&m)[9], float tx, float ty, float (&p)[4]) {
        ransac_fund_inlier_train(m, tx, ty, p);
    }
    static __device__ __forceinline__ bool tail(const float (&q)[4], const float (&t)[4], float thr2) { return ransac_fund_inlier_tail(q, t, thr2); }
};

}  // namespace sift_hip
