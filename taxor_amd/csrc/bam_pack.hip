// bam_pack.hip -- k_pack_nibbles: the 4-bit SEQ fields of BAM records (bam.h) -> k_pack_dna4's 2-bit layout (kernels.hip): 16 bases
// per word, the first base in the top bits, the words of a read padded with zeros to a multiple of four.  Everything behind the
// packed words -- syncmers, minimisers, the query, the finalize -- is the same as for ASCII input.
//
// A nibble is an IUPAC code of the alphabet "=ACMGRSVTWYHKDBN"; its 2-bit value is dna4_code (device_prims.h) of that letter:
// sixteen 2-bit values, one 32-bit constant, no table in LDS.  A read stored reverse-complemented (flag 0x10) is restored here:
// output base i is the complement of input base len-1-i, the complement taken on the IUPAC code -- the four bits reversed -- BEFORE
// the dna4 mapping, as `samtools fastq` followed by the reference's reader does (R -> Y -> C; mapping first would give R -> A -> T).
// So the reverse table is the forward table indexed by the bit-reversed nibble, and a reversed word walks its source backwards.
#include "kernels.h"
#include "device_prims.h"

namespace taxor {

static constexpr int BLK = 256;

// dna4_code of the letter of every nibble, 2 bits each (nibble 0, '=', is not dna15: it is flagged where it is met); rev: of the
// complement's letter
__device__ __forceinline__ uint32_t nibble_table(bool rev)
{
    const char letters[17] = "=ACMGRSVTWYHKDBN";
    uint32_t t = 0;
#pragma unroll
    for (uint32_t n = 1; n < 16; ++n) {
        const uint32_t src = rev ? (((n & 1u) << 3) | ((n & 2u) << 1) | ((n & 4u) >> 1) | ((n & 8u) >> 3)) : n;
        t |= (dna4_code((uint8_t)letters[src]) & 3u) << (2u * n);
    }
    return t;
}

// y: sixteen source nibbles, nibble k at bits 4k.  Forward: nibble k is base b0 + k of the read; reversed: base b0 + 15 - k.
// Bases at or past len stay zero (the spare low nibble of an odd-length read's last byte never gets here).
template <bool REV> __device__ __forceinline__ uint32_t word_of_nibbles(uint64_t y, uint32_t b0, uint32_t len, uint32_t table, bool &bad)
{
    uint32_t word = 0;
#pragma unroll
    for (uint32_t k = 0; k < 16; ++k) {
        const uint32_t i = REV ? 15u - k : k;
        if (b0 + i < len) {
            const uint32_t nib = (uint32_t)(y >> (4u * k)) & 15u;
            bad = bad || nib == 0u;
            word |= ((table >> (2u * nib)) & 3u) << (30u - 2u * i);
        }
    }
    return word;
}

// high and low nibble of every byte exchanged: base m of a byte string then sits at bits 4m
__device__ __forceinline__ uint64_t swap_nibbles(uint64_t x)
{
    return ((x & 0x0F0F0F0F0F0F0F0Full) << 4) | ((x >> 4) & 0x0F0F0F0F0F0F0F0Full);
}

// one block per read (grid-stride), one thread per 16-base word: sixteen nibbles are 8 bytes at any byte alignment (9 for a reversed
// word, whose window may begin at an odd base), read as three aligned dwords and funnel-shifted by the misalignment.  The source
// buffer has slack past its end, so the third dword is always readable; no load lies before the buffer's first byte.
__global__ __launch_bounds__(BLK) void k_pack_nibbles(const uint8_t *__restrict__ seq4, const uint64_t *__restrict__ boff,
                                                      const uint32_t *__restrict__ rlen, const uint8_t *__restrict__ rev,
                                                      const uint64_t *__restrict__ poff, uint32_t *__restrict__ packed,
                                                      uint32_t n_reads, Counters *ctr)
{
    const uint32_t t_fwd = nibble_table(false), t_rev = nibble_table(true);
    for (uint32_t r = blockIdx.x; r < n_reads; r += gridDim.x) {
        const uint64_t a0 = boff[r];
        const uint32_t len = rlen[r];
        const bool reverse = rev != nullptr && rev[r] != 0;
        const uint32_t nw = (len + 15u) >> 4;
        const uint32_t nw_pad = (nw + 3u) & ~3u;
        uint32_t *dst = packed + poff[r];
        bool bad = false;
        for (uint32_t w = threadIdx.x; w < nw_pad; w += BLK) {
            uint32_t word = 0;
            if (w < nw) {
                const uint32_t b0 = w << 4;
                // first source byte of the word's window: forward, base b0; reversed, base max(len - 16 - b0, 0)
                const uint32_t jhi = len - 1u - b0;                       // reversed: the source base of output base b0
                const uint32_t jlo = jhi >= 15u ? jhi - 15u : 0u;
                const uint64_t A = a0 + (reverse ? (uint64_t)(jlo >> 1) : (uint64_t)(b0 >> 1));
                const uint32_t *src = reinterpret_cast<const uint32_t *>(seq4 + (A & ~3ull));
                const uint32_t sh = (uint32_t)(A & 3ull) * 8u;
                const uint32_t q0 = src[0], q1 = src[1], q2 = src[2];
                const uint32_t x0 = sh ? ((q0 >> sh) | (q1 << (32u - sh))) : q0;
                const uint32_t x1 = sh ? ((q1 >> sh) | (q2 << (32u - sh))) : q1;
                const uint64_t xs = swap_nibbles(((uint64_t)x1 << 32) | x0);   // base m of the window at bits 4m
                if (!reverse) {
                    word = word_of_nibbles<false>(xs, b0, len, t_fwd, bad);
                } else {
                    // the window's base m is source base 2*(jlo >> 1) + m; nibble k of y must be source base jhi - 15 + k
                    const int t = (int)(jhi - 2u * (jlo >> 1)) - 15;       // -15 .. 1
                    uint64_t y;
                    if (t == 1) y = (xs >> 4) | ((uint64_t)(((q2 >> sh) >> 4) & 15u) << 60);   // base 16: the high nibble of the ninth byte
                    else if (t == 0) y = xs;
                    else y = xs << (4u * (uint32_t)(-t));
                    word = word_of_nibbles<true>(y, b0, len, t_rev, bad);
                }
            }
            dst[w] = word;
        }
        if (__any(bad) && lane_id() == 0) atomicOr(&ctr->flags, FLAG_ALPHABET);
    }
}

void launch_pack_nibbles(const uint8_t *seq4, const uint64_t *boff, const uint32_t *rlen, const uint8_t *rev, const uint64_t *poff,
                         uint32_t *packed, uint32_t n_reads, Counters *ctr, hipStream_t st, int max_grid)
{
    if (!n_reads) return;
    int grid = (int)(n_reads < 8192u ? n_reads : 8192u);
    if (max_grid > 0 && grid > max_grid) grid = max_grid;
    hipLaunchKernelGGL(k_pack_nibbles, dim3(grid), dim3(BLK), 0, st, seq4, boff, rlen, rev, poff, packed, n_reads, ctr);
}

} // namespace taxor
