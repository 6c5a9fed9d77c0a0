// read_probe.h -- what the per-read analyses share on the device (coverage, lca, confidence, hitmap, breakpoint, segments, exclusive;
// DESIGN.md section 10.10): the output filter, a wave minimum, the byte-register maximum, the piece a host cuts, the lookup of one hash
// among a user bin's leaf bins, the candidate walk and the probe that turns a piece into match words.  Device code only; the kernels
// are static templates: a file that launches one instantiates its own copy under its own compile flags, the others emit nothing.
#pragma once
#include "device_prims.h"
#include "ixf_arith.h"
#include "kernels.h"

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace taxor {

constexpr int READ_BLOCK = 256;                   // threads per block
constexpr int READ_WAVES = READ_BLOCK / 64;       // reads / pieces per block pass (one wave each)
constexpr uint32_t READ_SPLIT = 2048;             // hashes of one read per piece: a multiple of 64, so a piece's rounds are the read's
constexpr int HLL_CAS_ROUNDS = 256;               // a swap fails only when a byte of the word rose: 4 bytes x at most 61 values

// taxor_search.cpp:285, evaluated as written: the search's output filter
__device__ __forceinline__ bool keeps(uint32_t c, uint32_t mx) { return !((double)c < (double)mx * 0.8); }

// minimum over the wave, the same in every lane (xor butterfly, like wave_max)
template <class T> __device__ __forceinline__ T wave_min(T v)
{
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) {
        const T t = __shfl_xor(v, d);
        v = t < v ? t : v;
    }
    return v;
}

// byte `lane4` of *word = max(that byte, rho): the load in front of the swap ends the update where the register is high enough already.
// false: the update did not complete in HLL_CAS_ROUNDS
__device__ __forceinline__ bool hll_register_max(uint32_t *word, uint32_t lane4, uint32_t rho)
{
    const uint32_t shift = lane4 * 8u;
    uint32_t cur = __atomic_load_n(word, __ATOMIC_RELAXED);
    for (int it = 0; it < HLL_CAS_ROUNDS; ++it) {
        if (((cur >> shift) & 0xFFu) >= rho) return true;
        const uint32_t want = (cur & ~(0xFFu << shift)) | (rho << shift);
        const uint32_t seen = atomicCAS(word, cur, want);
        if (seen == cur) return true;
        cur = seen;
    }
    return false;
}

// at most READ_SPLIT consecutive hashes of one read: the unit of work of one wave
struct Piece {
    uint32_t read;       // index in the batch
    uint32_t first;      // offset of the piece's first hash in the staging buffer
    uint32_t n;          // hashes, at most READ_SPLIT
    uint32_t rank0;      // rank of the piece's first hash in the read's list: a multiple of READ_SPLIT, 0 for the read's first piece
};

// Hash h among the leaf technical bins leaf[l0 .. l1) of one user bin: the probe (three rows, fingerprint) once per IXF -- a split user
// bin's parts stand side by side in one IXF -- and three one-byte gathers per leaf bin at data[row * stride + bin].  Only lanes with
// `need` look anything up; every lane walks the same leaf bins.  STOP_AT_FIRST: a lane that has matched makes no further lookup, so
// `lookups` grows by the index of the first matching leaf bin plus one; otherwise by l1 - l0.
template <bool STOP_AT_FIRST, class Counter>
__device__ __forceinline__ bool leaf_lookup(const IxfDesc *__restrict__ ixf, const uint2 *__restrict__ leaf, uint64_t l0, uint64_t l1, uint64_t h, bool need,
                                            Counter &lookups)
{
    bool matched = false;
    uint32_t cur_ixf = 0xFFFFFFFFu;
    IxfDesc d{};
    ixf_probe p{};
    for (uint64_t l = l0; l < l1; ++l) {
        const uint2 lf = leaf[l];                             // the same in every lane
        if (lf.x != cur_ixf) {
            cur_ixf = lf.x;
            d = ixf[lf.x];
            p = ixf_probe_key_arith(h, d.seed, d.seg_len, d.arith);
        }
        if (need && !(STOP_AT_FIRST && matched)) {
            const uint8_t f = d.data[(uint64_t)p.row[0] * d.stride + lf.y] ^ d.data[(uint64_t)p.row[1] * d.stride + lf.y] ^
                              d.data[(uint64_t)p.row[2] * d.stride + lf.y];
            matched |= f == (uint8_t)(p.fp4 & 0xFFu);
            ++lookups;
        }
    }
    return matched;
}

// one atomic per wave for a per-lane counter
__device__ __forceinline__ void wave_add_to(unsigned long long *dst, unsigned long long mine)
{
    const unsigned long long sum = wave_incl_add(mine);
    if (lane_id() == 63 && sum) atomicAdd(dst, sum);
}

// ---- the candidate walk (breakpoint, segments, exclusive) ----------------------------------------------------------------------------
// The CANDIDATES of a read are its tuples with count > 0, in CSR order.  The CSR's tuples are indexed from t0 (off[0] == t0).
enum : uint32_t { CAND_BAD_BIN = 1u, CAND_MISCOUNT = 2u };      // err flags; a file's own flags start at 4

struct LeafRange {
    uint64_t l0, l1;     // the candidate's user bin's leaf technical bins are leaf[l0 .. l1)
};

// a tuple is a candidate when its count is above 0; one that names a user bin outside the index is reported through err
__device__ __forceinline__ bool is_candidate(const int64_t *__restrict__ ub, const uint32_t *__restrict__ count, uint64_t i, uint64_t hi, uint64_t t0,
                                             uint64_t n_bins, bool *bad)
{
    if (i >= hi || count[i - t0] == 0) return false;
    const int64_t b = ub[i - t0];
    if (b < 0 || (uint64_t)b >= n_bins) {
        *bad = true;
        return false;
    }
    return true;
}

// one wave per read, tuples 64 at a time: M, the read's candidates, as a Count.  A read without a hash leaves at once
template <class Count>
static __global__ __launch_bounds__(READ_BLOCK) void k_cand_count(const uint64_t *__restrict__ off, const int64_t *__restrict__ ub, const uint32_t *__restrict__ count,
                                                                  uint64_t t0, const uint32_t *__restrict__ nh, uint64_t n_reads, uint64_t n_bins,
                                                                  Count *__restrict__ n_cand, uint32_t *__restrict__ err)
{
    bool bad = false;
    for (uint64_t r = (uint64_t)blockIdx.x * READ_WAVES + (threadIdx.x >> 6); r < n_reads; r += (uint64_t)gridDim.x * READ_WAVES) {
        uint32_t m = 0;
        if (nh[r] != 0) {
            const uint64_t lo = off[r], hi = off[r + 1];
            for (uint64_t base = lo; base < hi; base += 64) m += (uint32_t)__popcll(__ballot(is_candidate(ub, count, base + lane_id(), hi, t0, n_bins, &bad)));
        }
        if (lane_id() == 0) n_cand[r] = (Count)m;
    }
    if (bad) atomicOr(err, CAND_BAD_BIN);
}

// The same walk over the EXAMINED reads: cand_off is the host's sum of their counts, read r's candidates go to [cand_off[r],
// cand_off[r + 1]) in CSR order (a ballot ranks the candidates of each 64).  WITH_LEAF: the range of the user bin's leaf bins as well
template <bool WITH_LEAF>
static __global__ __launch_bounds__(READ_BLOCK) void k_cand_fill(const uint64_t *__restrict__ off, const int64_t *__restrict__ ub, const uint32_t *__restrict__ count,
                                                                 uint64_t t0, uint64_t n_reads, uint64_t n_bins, const uint64_t *__restrict__ leaf_off,
                                                                 const uint64_t *__restrict__ cand_off, uint64_t *__restrict__ o_tuple, int64_t *__restrict__ o_ub,
                                                                 LeafRange *__restrict__ o_leaf, uint32_t *__restrict__ err)
{
    bool bad = false, miscount = false;
    for (uint64_t r = (uint64_t)blockIdx.x * READ_WAVES + (threadIdx.x >> 6); r < n_reads; r += (uint64_t)gridDim.x * READ_WAVES) {
        const uint64_t dst0 = cand_off[r], room = cand_off[r + 1] - dst0;
        if (room == 0) continue;
        const uint64_t lo = off[r], hi = off[r + 1];
        uint64_t written = 0;
        for (uint64_t base = lo; base < hi; base += 64) {
            const uint64_t i = base + lane_id();
            const bool k = is_candidate(ub, count, i, hi, t0, n_bins, &bad);
            const uint64_t m = __ballot(k);
            const uint64_t at = written + (uint64_t)__popcll(m & ((1ull << lane_id()) - 1ull));
            if (k && at < room) {                         // never past the read's room: a walk that disagrees with the count is reported below
                const int64_t b = ub[i - t0];             // inside the index: is_candidate said so
                o_tuple[dst0 + at] = i;
                o_ub[dst0 + at] = b;
                if (WITH_LEAF) o_leaf[dst0 + at] = LeafRange{leaf_off[b], leaf_off[b + 1]};
            }
            written += (uint64_t)__popcll(m);
        }
        miscount = miscount || written != room;
    }
    if (bad) atomicOr(err, CAND_BAD_BIN);
    if (miscount) atomicOr(err, CAND_MISCOUNT);
}

// ---- the match matrix (breakpoint, segments) -----------------------------------------------------------------------------------------
// the examined reads' candidates and where a read's match words lie within its group's scratch
struct MaskLayout {
    const uint64_t *cand_off;     // [n_reads + 1]; an empty range: the read is not examined
    const int64_t *cand_ub;       // [n_cand] checked against n_bins by the count's walk
    const uint64_t *mask_off;     // [n_reads] first mask word of the read: mask[mask_off[r] + c * rounds + k]
    const uint32_t *nh;           // [n_reads] rounds = ceil(nh / 64)
    uint64_t *mask;
};

struct MaskProbeArgs {
    const IxfDesc *ixf;
    const uint64_t *leaf_off;     // [n_bins + 1] user bin b's leaf technical bins are leaf[leaf_off[b] .. leaf_off[b + 1])
    const uint2 *leaf;            // (IXF, bin)
    MaskLayout l;
    const Piece *pieces;
    const uint64_t *hashes;       // the staged part of the saved lists
    uint32_t n_pieces;
    unsigned long long *lookups;
};

// One wave per piece, 64 hashes per round, one per lane; for each candidate in turn the lookup and the ballot of the lanes that matched,
// stored as ONE 64-bit word mask[c][round] by one lane: the whole match matrix at 8 bytes per (candidate, 64 hashes).  Every word is
// written exactly once, by one wave: nothing is zeroed and nothing is added.  STOP_AT_FIRST is leaf_lookup's; both callers stop.
template <bool STOP_AT_FIRST>
static __global__ __launch_bounds__(READ_BLOCK) void k_probe_mask(MaskProbeArgs a)
{
    unsigned long long lookups = 0;
    const uint32_t lane = lane_id();
    for (uint64_t pi = (uint64_t)blockIdx.x * READ_WAVES + (threadIdx.x >> 6); pi < a.n_pieces; pi += (uint64_t)gridDim.x * READ_WAVES) {
        const Piece pc = a.pieces[pi];
        const uint64_t c0 = a.l.cand_off[pc.read], c1 = a.l.cand_off[pc.read + 1];
        const uint64_t rounds = ((uint64_t)a.l.nh[pc.read] + 63) >> 6;
        uint64_t *mask = a.l.mask + a.l.mask_off[pc.read];
        for (uint32_t h0 = 0; h0 < pc.n; h0 += 64) {
            const uint32_t j = h0 + lane;
            const bool active = j < pc.n;
            const uint64_t h = active ? a.hashes[(uint64_t)pc.first + j] : 0;
            const uint64_t round = ((uint64_t)pc.rank0 + h0) >> 6;    // < rounds: rank0 + h0 < the read's hashes
            for (uint64_t c = c0; c < c1; ++c) {
                const uint64_t b = (uint64_t)a.l.cand_ub[c];          // the same in every lane
                const uint64_t m = __ballot(leaf_lookup<STOP_AT_FIRST>(a.ixf, a.leaf, a.leaf_off[b], a.leaf_off[b + 1], h, active, lookups));
                if (lane == 0) mask[(c - c0) * rounds + round] = m;
            }
        }
    }
    wave_add_to(a.lookups, lookups);
}

} // namespace taxor
