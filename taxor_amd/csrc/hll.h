// hll.h -- the HyperLogLog sketch of `taxor search --coverage-file` ("Distinct-hash coverage"): the ONE slot
// function, for host and device, and the host's estimator.  A sketch of precision P has m = 2^P byte registers.
#pragma once
#include "ixf_arith.h"

#include <cmath>

namespace taxor {

constexpr uint32_t HLL_MIN_PRECISION = 4, HLL_MAX_PRECISION = 16, HLL_DEFAULT_PRECISION = 12;

struct hll_slot_t {
    uint32_t index;   // register, below 2^P
    uint32_t rho;     // 1 .. 64 - P + 1
};

// The index's hashes are wyhash values already, and under FracMinHash scaling the selected ones have a small wyhash(h): the xor
// takes h off that orbit before it is mixed again.
TAXOR_HD hll_slot_t hll_slot(uint64_t hash, uint32_t precision)
{
    const uint64_t w = wyhash_u64(hash ^ 0x9E3779B97F4A7C15ull);
    const uint64_t rest = w << precision;
    hll_slot_t s;
    s.index = (uint32_t)(w >> (64u - precision));
#if defined(__HIP_DEVICE_COMPILE__)
    s.rho = rest ? (uint32_t)__clzll((long long)rest) + 1u : 64u - precision + 1u;
#else
    s.rho = rest ? (uint32_t)__builtin_clzll(rest) + 1u : 64u - precision + 1u;
#endif
    return s;
}

// The raw estimate with the small-range correction (linear counting); no large-range correction: the hashes are 64-bit.  Doubles,
// summed in index order.
inline double hll_estimate(const uint8_t *registers, uint32_t precision)
{
    const uint64_t m = 1ull << precision;
    const double md = (double)m;
    const double alpha = m == 16 ? 0.673 : m == 32 ? 0.697 : m == 64 ? 0.709 : 0.7213 / (1.0 + 1.079 / md);
    double sum = 0.0;
    uint64_t zeros = 0;
    for (uint64_t j = 0; j < m; ++j) {
        sum += std::ldexp(1.0, -(int)registers[j]);
        zeros += registers[j] == 0;
    }
    double e = alpha * md * md / sum;
    if (e <= 2.5 * md && zeros > 0) e = md * std::log(md / (double)zeros);
    return e;
}

} // namespace taxor
