// Philox4x32-10 (Salmon, Moraes, Dror, Shaw: "Parallel random numbers: as easy as 1, 2, 3", SC'11; the Random123 constants), as
// device functions.  A counter-based generator: a block of four 32-bit words is a pure function of a 128-bit counter and a 64-bit
// key, so there is no state to synchronise, a draw can sit inside a stream capture, and numpy restates it bit for bit
// (tests/_philox_ref.py).
//
//   round    from (c0, c1, c2, c3) and (k0, k1):  p0 = M0 * c0, p1 = M1 * c2 as 64-bit products,
//            c = (hi(p1) ^ c1 ^ k0, lo(p1), hi(p0) ^ c3 ^ k1, lo(p0)); then k0 += W0, k1 += W1.  Ten rounds.
//
// The package's convention (philox_draw):
//   key      (lo32(seed), hi32(seed))
//   counter  (lo32(q), hi32(q), lo32(step), stream): q the 64-bit block number, step the draw number, stream the user --
//            0 element dropout, 1 channel dropout, 2 augmentation
//   entry e  of a draw is word e & 3 of block e >> 2; a uniform is u = (word >> 8) * 2^-24, exact in float32, in [0, 1)
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace fc {

constexpr uint32_t kPhiloxM0 = 0xD2511F53u, kPhiloxM1 = 0xCD9E8D57u;
constexpr uint32_t kPhiloxW0 = 0x9E3779B9u, kPhiloxW1 = 0xBB67AE85u;

enum PhiloxStream : uint32_t { kStreamElementDropout = 0, kStreamChannelDropout = 1, kStreamAugment = 2 };

struct PhiloxBlock { uint32_t w[4]; };

__device__ __forceinline__ PhiloxBlock philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1) {
#pragma unroll
    for (int round = 0; round < 10; ++round) {
        const uint32_t hi0 = __umulhi(kPhiloxM0, c0), lo0 = kPhiloxM0 * c0;
        const uint32_t hi1 = __umulhi(kPhiloxM1, c2), lo1 = kPhiloxM1 * c2;
        c0 = hi1 ^ c1 ^ k0;
        c1 = lo1;
        c2 = hi0 ^ c3 ^ k1;
        c3 = lo0;
        k0 += kPhiloxW0;
        k1 += kPhiloxW1;
    }
    return {{c0, c1, c2, c3}};
}

// block q of draw `step` of user `stream` under `seed`
__device__ __forceinline__ PhiloxBlock philox_draw(uint64_t seed, uint64_t q, uint32_t step, uint32_t stream) {
    return philox4x32_10((uint32_t)q, (uint32_t)(q >> 32), step, stream, (uint32_t)seed, (uint32_t)(seed >> 32));
}

// word k of a block for a k known only at run time (selects: an indexed array would live in scratch)
__device__ __forceinline__ uint32_t philox_word(const PhiloxBlock& r, uint32_t k) {
    return k == 0 ? r.w[0] : (k == 1 ? r.w[1] : (k == 2 ? r.w[2] : r.w[3]));
}

// the 24 bits a decision or a uniform is made of
__device__ __forceinline__ uint32_t philox_bits24(uint32_t word) { return word >> 8; }
__device__ __forceinline__ float philox_uniform(uint32_t word) { return (float)(word >> 8) * 5.9604644775390625e-08f; }       // 2^-24

// the draw number: the caller's value, or the one a device tensor holds now (a graph replay reads the current one)
__device__ __forceinline__ uint32_t philox_step(int64_t step, const int64_t* __restrict__ step_ptr) {
    return (uint32_t)(step_ptr != nullptr ? *step_ptr : step);
}

}  // namespace fc
