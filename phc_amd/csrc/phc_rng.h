// phc_rng.h -- the counter-based random draws of the device code: no generator state, a draw is a hash of (stream key, index).  Shared by the reset
// launch (phc_kernels.hip: start times) and the push schedule (phc_push.h).  PHC_HD: the host builds of the tests run the same integer arithmetic.
#pragma once
#include "phc_math.h"

namespace phc {

// counter-based uniform in [0,1): the host folds (seed, counter) into one 64-bit stream key (splitmix64); per env a 32-bit
// avalanche hash (murmur3 finaliser rounds) of the env id under that key, top 24 bits -> float like torch.rand
PHC_HD float hash_u01(uint64_t key, uint32_t env) {
    uint32_t x = env * 0x9E3779B1u ^ (uint32_t)key;
    x ^= x >> 16; x *= 0x85EBCA6Bu; x ^= x >> 13; x *= 0xC2B2AE35u; x ^= x >> 16;
    x += (uint32_t)(key >> 32);
    x ^= x >> 15; x *= 0x2C1B3C6Du; x ^= x >> 12; x *= 0x297A2D39u; x ^= x >> 15;
    return (float)(x >> 8) * (1.0f / 16777216.0f);
}
PHC_HD uint64_t splitmix64(uint64_t z) {
    z += 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

}  // namespace phc
