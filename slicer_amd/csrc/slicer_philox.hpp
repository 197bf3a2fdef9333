// slicer_philox.hpp -- internal: Philox4x32-10 (Salmon, Moraes, Dror, Shaw 2011), the counter-based generator of the
// shape noise, one body for the host (slicer_noise_words) and the device (slicer_noise.hip).
// Integers only, so both give the same bits.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace slicer {

constexpr uint32_t kPhiloxM0 = 0xD2511F53u, kPhiloxM1 = 0xCD9E8D57u;  // the round's multipliers
constexpr uint32_t kPhiloxW0 = 0x9E3779B9u, kPhiloxW1 = 0xBB67AE85u;  // the Weyl increments of the key

// c[0 .. 3] <- ten rounds of (c0, c1, c2, c3) -> (hi(M1 c2) ^ c1 ^ k0, lo(M1 c2), hi(M0 c0) ^ c3 ^ k1, lo(M0 c0)), the key
// bumped between rounds
__host__ __device__ inline void philox4x32_10(uint32_t (&c)[4], uint32_t k0, uint32_t k1)
{
#pragma unroll
    for (int round = 0; round < 10; round++) {
        const uint64_t p0 = (uint64_t)kPhiloxM0 * c[0], p1 = (uint64_t)kPhiloxM1 * c[2];
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c[1] ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c[3] ^ k1;
        c[0] = n0;
        c[1] = (uint32_t)p1;
        c[2] = n2;
        c[3] = (uint32_t)p0;
        k0 += kPhiloxW0;
        k1 += kPhiloxW1;
    }
}

// the four words of block b of (seed, stream, realisation): counter (lo b, hi b, realisation, stream), key (lo seed, hi seed)
__host__ __device__ inline void noise_block_words(uint64_t seed, uint32_t stream, uint32_t realisation, uint64_t b,
                                                  uint32_t (&w)[4])
{
    w[0] = (uint32_t)b;
    w[1] = (uint32_t)(b >> 32);
    w[2] = realisation;
    w[3] = stream;
    philox4x32_10(w, (uint32_t)seed, (uint32_t)(seed >> 32));
}

}  // namespace slicer
