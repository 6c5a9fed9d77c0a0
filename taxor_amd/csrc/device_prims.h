// device_prims.h -- the device primitives every kernel file shares (device code only): lane / wave / block scans, and the
// sequence functions that pin bit-exactness against the reference -- the dna4 mapping, base extraction from the 2-bit
// packing, reverse complement, canonical form.  `taxor build` (genome_keys.hip) and `taxor search` (kernels.hip) hash with
// the SAME definitions: an index built with one rule is never queried with another.  Wave = 64 lanes.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace taxor {

// ---- lane and wave -----------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t lane_id() { return threadIdx.x & 63u; }

template <class T> __device__ __forceinline__ T wave_incl_add(T v)
{
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const T t = __shfl_up(v, d);
        if ((int)lane_id() >= d) v += t;
    }
    return v;
}

__device__ __forceinline__ int wave_incl_max(int v)
{
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int t = __shfl_up(v, d);
        if ((int)lane_id() >= d) v = max(v, t);
    }
    return v;
}

// maximum over the wave, the same in every lane (xor butterfly); T = uint32_t, long long, double
template <class T> __device__ __forceinline__ T wave_max(T v)
{
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) {
        const T t = __shfl_xor(v, d);
        v = t > v ? t : v;
    }
    return v;
}

// append one record per participating lane with a single atomic per wave (ballot + popcount).
// Returns the slot for lanes with pred, undefined otherwise.
__device__ __forceinline__ uint32_t wave_append(bool pred, uint32_t *counter)
{
    const unsigned long long m = __ballot(pred);
    if (m == 0ull) return 0;
    const int leader = __ffsll((long long)m) - 1;
    uint32_t base = 0;
    if ((int)lane_id() == leader) base = atomicAdd(counter, (uint32_t)__popcll(m));
    base = __shfl(base, leader);
    return base + (uint32_t)__popcll(m & ((1ull << lane_id()) - 1ull));
}

// ---- block (WAVES = threads per block / 64, a compile-time constant: the loops over the wave sums stay unrolled) ---------------------
// exclusive prefix sum over the block; *total = block sum.  scratch: >= WAVES values in LDS, the caller's
template <int WAVES, class T> __device__ __forceinline__ T block_excl_add(T v, T *scratch, T *total)
{
    const T incl = wave_incl_add(v);
    const uint32_t w = threadIdx.x >> 6;
    __syncthreads();                                   // a previous call's readers are done with the scratch
    if (lane_id() == 63) scratch[w] = incl;
    __syncthreads();
    T off = 0, tot = 0;
#pragma unroll
    for (uint32_t i = 0; i < (uint32_t)WAVES; ++i) {
        const T x = scratch[i];
        if (i < w) off += x;
        tot += x;
    }
    *total = tot;
    return off + incl - v;
}

// exclusive prefix max over the block (identity -1).  scratch: >= WAVES words in LDS
template <int WAVES> __device__ __forceinline__ int block_excl_max(int v, int *scratch)
{
    const int incl = wave_incl_max(v);
    const uint32_t w = threadIdx.x >> 6;
    __syncthreads();
    if (lane_id() == 63) scratch[w] = incl;
    __syncthreads();
    int off = -1;
#pragma unroll
    for (uint32_t i = 0; i < (uint32_t)WAVES; ++i)
        if (i < w) off = max(off, scratch[i]);
    int prev = __shfl_up(incl, 1);
    if (lane_id() == 0) prev = -1;
    return max(off, prev);
}

// ---- sequence ----------------------------------------------------------------------------------------------------------------------
// seqan3 dna4 char_to_rank (dna4_traits.hpp:15-18): IUPAC codes -> first base, U -> T, N -> A; both cases.  0xFF = not dna15.
__device__ __forceinline__ uint32_t dna4_code(uint8_t c)
{
    if ((uint8_t)((c | 0x20) - 'a') >= 26u) return 0xFFu;
    switch (c | 0x20) {
    case 'a': case 'r': case 'w': case 'm': case 'd': case 'h': case 'v': case 'n': return 0;
    case 'c': case 'y': case 's': case 'b': return 1;
    case 'g': case 'k': return 2;
    case 't': case 'u': return 3;
    default: return 0xFFu;
    }
}

__device__ __forceinline__ uint32_t revcomp32(uint32_t x, int nb)
{
    x = __brev(~x);
    x = ((x >> 1) & 0x55555555u) | ((x & 0x55555555u) << 1);
    return x >> (32 - 2 * nb);
}

__device__ __forceinline__ uint64_t revcomp64(uint64_t x, int nb)
{
    x = __brevll(~x);
    x = ((x >> 1) & 0x5555555555555555ull) | ((x & 0x5555555555555555ull) << 1);
    return x >> (64 - 2 * nb);
}

// n-base value (n <= 32) starting at base o (0..15) of word a, read from a and the two words after it (first base in the top bits)
__device__ __forceinline__ uint64_t bases3(uint32_t a, uint32_t b, uint32_t c, uint32_t o, int n)
{
    const uint64_t hi = ((uint64_t)a << 32) | b;
    const int end = 2 * (int)o + 2 * n;
    const uint64_t mask = (n < 32) ? ((1ull << (2 * n)) - 1ull) : ~0ull;
    if (end <= 64) return (hi >> (64 - end)) & mask;
    const int sh = end - 64;                          // 1..30
    return ((hi << sh) | (uint64_t)(c >> (32 - sh))) & mask;
}

// ... from a staged word array (LDS): W[word + 2] must be readable
__device__ __forceinline__ uint64_t lds_bases(const uint32_t *W, uint32_t word, uint32_t o, int n)
{
    return bases3(W[word], W[word + 1], W[word + 2], o, n);
}

// ... from a record's packed words in global memory, base position pos; words past the record read as zero
__device__ __forceinline__ uint64_t global_bases(const uint32_t *pk, uint32_t nwords, uint32_t pos, int n)
{
    const uint32_t wi = pos >> 4;
    return bases3(pk[wi], wi + 1 < nwords ? pk[wi + 1] : 0u, wi + 2 < nwords ? pk[wi + 2] : 0u, pos & 15u, n);
}

// the smaller of an n-base value and its reverse complement
__device__ __forceinline__ uint64_t canon(uint64_t f, int n)
{
    const uint64_t rc = revcomp64(f, n);
    return f < rc ? f : rc;
}

} // namespace taxor
