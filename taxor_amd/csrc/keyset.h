// keyset.h -- duplicate-free copy of a device array of 64-bit keys (hierarchical build, see keyset.hip)
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace taxor {

// The set's slot rule and insertion, shared by KeyUnion's kernels and the genome keyer's per-bin sets (genome_keys.hip): an
// open-addressing table of 64-bit keys with linear probing, all bytes 0xFF = empty.  The empty marker itself is never inserted;
// callers keep it aside.
constexpr uint64_t KEYSET_EMPTY = ~0ull;

__device__ __forceinline__ uint64_t keyset_slot_hash(uint64_t k)
{
    k ^= k >> 32;
    k *= 0xD6E8FEB86659FD93ull;
    k ^= k >> 32;
    return k;
}

// 1 for the one caller that took the key's slot, 0 when the key was there already, -1 when every slot of the table (mask + 1)
// holds another key (callers size their tables so that this cannot happen, and raise a flag if it does)
__device__ __forceinline__ int keyset_insert(uint64_t *tab, uint64_t mask, uint64_t key)
{
    uint64_t s = keyset_slot_hash(key) & mask;
    for (uint64_t probes = 0; probes <= mask; ++probes) {
        const uint64_t old = atomicCAS((unsigned long long *)&tab[s], (unsigned long long)KEYSET_EMPTY, (unsigned long long)key);
        if (old == KEYSET_EMPTY) return 1;
        if (old == key) return 0;
        s = (s + 1) & mask;
    }
    return -1;
}

// number of distinct keys of d_in[0, n) (the empty marker included when present); waits for `st`
hipError_t keyset_count_distinct(const uint64_t *d_in, uint64_t n, uint64_t *n_out, hipStream_t st);

// Scratch of the union step, kept from one IXF to the next (a hipMalloc / hipFree pair per IXF costs more than the union of a small one).
struct KeyUnion {
    uint64_t *table = nullptr;             // open-addressing set, 1.5 .. 3 slots per input key
    uint64_t table_entries = 0;
    unsigned long long *d_ctl = nullptr;   // [0] keys written, [1] the input held the empty marker itself
    unsigned long long *h_ctl = nullptr;   // page-locked
    ~KeyUnion() { release(); }
    void release();
    // d_out (room for n keys) receives the distinct keys of d_in[0, n) in no particular order, *n_out their number.  Waits for `st`.
    hipError_t unique(const uint64_t *d_in, uint64_t n, uint64_t *d_out, uint64_t *n_out, hipStream_t st);
    // nothing is copied: d_keep[i] = 1 for one occurrence of every distinct key of d_in[0, n), 0 for its duplicates; *n_kept = the ones.
    hipError_t mark(const uint64_t *d_in, uint64_t n, uint8_t *d_keep, uint64_t *n_kept, hipStream_t st);
private:
    hipError_t prepare(uint64_t n, uint64_t *entries, hipStream_t st);
public:
};

}
