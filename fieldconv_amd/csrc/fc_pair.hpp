// The pair distance of the feature-matching kernels (fc_loss.hip: pair lists, dense counts; fc_match.hip: nearest rows) and the
// geometry of the dense tile they share.  ONE definition: every kernel that includes this gives the same bits for the same pair.
//   d2(a,b) = ((t0*t0 + t1*t1) + t2*t2) + ... with t_c = xT[a,c] - xS[b,c], c ascending, every operation rounded on its own
// (no contraction), so that numpy in the same dtype restates it exactly.
#pragma once
#include "fc_common.hpp"

namespace fc {

constexpr int kDenseThreads = 256;          // 16 x 16 lanes, each owning 4 x 4 pairs of a 64 x 64 tile
constexpr int kDenseTile = 64;
constexpr int kDenseChunk = 16;             // channels staged per pass
constexpr int kDensePitch = kDenseTile + 4; // row pitch of the transposed LDS tiles (keeps 16-byte alignment, spreads the banks)

// acc + t*t with t = a - b; a distance starts from acc = 0 (0 + t*t == t*t exactly).
template <typename T>
__device__ __forceinline__ T d2_step(T acc, T a, T b) {
#pragma clang fp contract(off)          // (plain operators: __fmul_rn / __fadd_rn are header functions that hipcc contracts)
    const T t = a - b;
    return acc + t * t;
}

template <typename T>
__device__ __forceinline__ T pair_d2(const T* __restrict__ a, const T* __restrict__ b, int C) {
    T acc = 0;
    for (int c = 0; c < C; ++c) acc = d2_step(acc, a[c], b[c]);
    return acc;
}

template <typename T>
__device__ __forceinline__ T quiet_nan() {
    return static_cast<T>(__int_as_float(0x7fc00000));
}

constexpr int64_t kMaxPairRows = (int64_t)1 << 24;          // rows_fit_32bit's row limit (fc_api.hip)

// What every entry point over two feature matrices checks first: rows within N < 2^24 and N*C*8 < 4 GiB, dtype 0 or 1.
inline bool features_ok(const void* xS, int32_t nS, const void* xT, int32_t nT, int32_t C, int32_t dtype) {
    return xS && xT && nS >= 1 && nT >= 1 && nS < kMaxPairRows && nT < kMaxPairRows && C >= 1 && (dtype == 0 || dtype == 1) &&
           (uint64_t)(nS > nT ? nS : nT) * (uint64_t)C * 8u < ((uint64_t)1 << 32);
}

}  // namespace fc
