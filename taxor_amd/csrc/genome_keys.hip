// genome_keys.hip -- the key sets of `taxor build`, on the device: whole reference genomes -> the DISTINCT keys of every user bin,
// FracMinHash-filtered, sorted ascending.  The reference does this on the CPU, one genome file per thread (src/main/
// compute_hashes.cpp:50-142: seq_to_syncmers / minimiser_hash per record, union over the file's records, wyhash filter).
//
//   k_gk_pack        ASCII -> dna4 (dna4_traits.hpp:15-18, the mapping of kernels.hip's k_pack_dna4) -> 2 bits, one thread per
//                    16-base word over the whole call (records of any length share the grid)
//   k_gk_syncmers    one TILE of GT consecutive windows of one record per block iteration: canonical s-mer values, leftmost /
//                    rightmost argmin per window, the chain walk of kernels.hip's k_syncmers from the
//                    tile's own anchors, wyhash of the selected canonical k-mers, insertion into the user bin's set.  No
//                    per-read dedup in LDS and no read-long state: the block takes the next tile after one pass
//   k_gk_fixup       the windows of a tile BEFORE its first anchor: their tracked position is history (a run of tied windows
//                    -- a homopolymer, (AT)n, TTAGGG -- crossing the tile edge).  One thread per tile whose predecessor has an
//                    anchor walks the chain on from that tile's carried position, through any following anchor-less tiles
//   k_gk_minimisers  minimiser mode: the VALUE set of seqan3's minimiser_hash is {minimum of each window} -- which of several
//                    equal minima the view keeps moves positions, not values -- so tiles overlap by window - 1 k-mers and
//                    carry no state
//   k_cc_*           order-preserving compaction (occupied slots of the per-bin tables, or flagged keys) with new range bounds
//
// Sets: one open-addressing table per user bin of a call (keyset.h's insertion: the slot rule of KeyUnion), sized from its
// records' selection bound.  A call's sets are compacted into one bin-grouped array; a user bin whose records span calls has one
// such segment per call.  _finish gathers the segments per bin, sorts every bin (rocPRIM segmented radix sort), and drops the
// duplicates of bins with several segments.
#include "../../include/taxor_gpu_tools.h"
#include "device_prims.h"
#include "hip_host.h"
#include "ixf_arith.h"
#include "keyset.h"

#include <hip/hip_runtime.h>
#include <rocprim/device/device_segmented_radix_sort.hpp>

#include <algorithm>
#include <cstring>
#include <map>
#include <string>
#include <vector>

namespace {

using namespace taxor;

constexpr int GB = 256;                              // threads per block
constexpr int GC = 8;                                // consecutive windows per thread in the resolve pass
constexpr int GT = GB * GC;                          // windows per tile
constexpr int GMAX_W = 512;                          // k-mers per minimiser window, at most (index_create's limit)
constexpr int GWORDS = (GT + GMAX_W + 64) / 16 + 4;  // packed words staged per tile
constexpr uint64_t CC_BLOCK = 4096;                  // elements per block of the ordered compaction
constexpr uint64_t REGION_MIN = 4096;                // slots of the smallest per-bin table

enum : uint32_t { GK_ALPHABET = 1u, GK_TABLE_FULL = 2u };

struct GkArgs {
    const uint32_t *packed;
    const uint64_t *poff;      // first packed word of record r (records start on 4-word boundaries)
    const uint32_t *rlen;      // bases of record r
    const uint32_t *rreg;      // set (table region) of record r's user bin in this call
    const uint2 *tiles;        // (record, first window); the tiles of one record are consecutive, in window order
    uint32_t n_tiles;
    uint64_t *tab;             // every region's slots, region after region
    const uint64_t *reg_base;  // first slot of region g
    const uint64_t *reg_mask;  // slots of region g - 1 (a power of two minus one)
    uint32_t *reg_marker;      // 1 = the key equal to the empty marker was met (it cannot sit in a table)
    int *carry;                // syncmers: tracked s-mer position after the tile's last window, record coordinates (-1: none)
    uint32_t *pend;            // syncmers: windows before the tile's first anchor (k_gk_fixup resolves them)
    uint32_t *flags;
    int k, s, t;
    int wm;                    // minimiser mode: window length in k-mers (window_size - k + 1)
    uint64_t seed;             // minimiser mode: hixf::adjust_seed(k)
    double scaling_limit;      // > 0: keep a key only if (double)wyhash(key) <= limit (compute_hashes.cpp, FracMinHash)
};

__device__ __forceinline__ void gk_emit(const GkArgs &a, uint32_t reg, uint64_t h)
{
    if (a.scaling_limit > 0.0 && !((double)wyhash_u64(h) <= a.scaling_limit)) return;
    if (h == KEYSET_EMPTY) { a.reg_marker[reg] = 1u; return; }
    if (keyset_insert(a.tab + a.reg_base[reg], a.reg_mask[reg], h) < 0) atomicOr(a.flags, GK_TABLE_FULL);
}

__global__ __launch_bounds__(GB) void k_gk_pack(const uint8_t *__restrict__ ascii, const uint64_t *__restrict__ aoff,
                                                const uint64_t *__restrict__ poff, uint32_t n_rec, uint64_t total_words,
                                                uint32_t *__restrict__ packed, uint32_t *flags)
{
    bool bad = false;
    for (uint64_t gw = (uint64_t)blockIdx.x * GB + threadIdx.x; gw < total_words; gw += (uint64_t)gridDim.x * GB) {
        uint32_t lo = 0, hi = n_rec;                  // poff[lo] <= gw < poff[hi], the last such record (empty ones are skipped)
        while (hi - lo > 1) {
            const uint32_t mid = (lo + hi) >> 1;
            if (poff[mid] <= gw) lo = mid;
            else hi = mid;
        }
        const uint64_t a0 = aoff[lo], len = aoff[lo + 1] - a0;
        const uint64_t b0 = (gw - poff[lo]) << 4;
        uint32_t word = 0;
#pragma unroll
        for (int c = 0; c < 16; ++c) {
            if (b0 + (uint64_t)c < len) {
                uint32_t code = dna4_code(ascii[a0 + b0 + (uint64_t)c]);
                if (code > 3u) { bad = true; code = 0; }
                word |= code << (30 - 2 * c);
            }
        }
        packed[gw] = word;
    }
    if (bad) atomicOr(flags, GK_ALPHABET);
}

__global__ __launch_bounds__(GB) void k_gk_syncmers(const GkArgs a)
{
    __shared__ uint32_t sW[GWORDS];
    __shared__ uint64_t sV[GT + 32];
    __shared__ uint8_t sLm[GT], sRm[GT];
    __shared__ int sScr[8];
    __shared__ int sFirst;
    const int k = a.k, s = a.s, t = a.t, w = k - s + 1;
    const int tid = (int)threadIdx.x;
    for (uint32_t ti = blockIdx.x; ti < a.n_tiles; ti += gridDim.x) {
        const uint2 td = a.tiles[ti];
        const uint32_t r = td.x;
        const int x0 = (int)td.y;
        const uint32_t L = a.rlen[r];
        const uint32_t *__restrict__ pk = a.packed + a.poff[r];
        const uint32_t nwords = (((L + 15u) >> 4) + 3u) & ~3u;
        const int nw_tile = min(GT, (int)L - k + 1 - x0);
        const uint32_t reg = a.rreg[r];
        const uint32_t wbase = (uint32_t)x0 >> 4;
        __syncthreads();                                           // the previous tile is done with the LDS
        for (int i = tid; i < GWORDS; i += GB) {
            const uint32_t wi = wbase + (uint32_t)i;
            sW[i] = wi < nwords ? pk[wi] : 0u;
        }
        if (tid == 0) sFirst = GT;
        __syncthreads();
        // canonical s-mer values (syncmer.cpp:103-110; the s-mer "hash" is the raw 2-bit value)
        for (int i = tid; i < nw_tile + w - 1; i += GB) {
            const uint32_t pos = (uint32_t)(x0 + i);
            sV[i] = canon(lds_bases(sW, (pos >> 4) - wbase, pos & 15u, s), s);
        }
        __syncthreads();
        // leftmost / rightmost argmin per window (interleaved: conflict-free LDS)
        for (int xl = tid; xl < nw_tile; xl += GB) {
            uint64_t m = sV[xl];
            int lm = 0, rm = 0;
            for (int j = 1; j < w; ++j) {
                const uint64_t v = sV[xl + j];
                if (v < m) { m = v; lm = j; rm = j; }
                else if (v == m) rm = j;
            }
            sLm[xl] = (uint8_t)lm;
            sRm[xl] = (uint8_t)rm;
        }
        __syncthreads();
        // anchors: a unique minimum fixes the tracked position whatever the history; window 0 of a record takes Lm
        const int xs = tid * GC;
        int last_anchor = -1, first_anchor = GT;
#pragma unroll
        for (int c = 0; c < GC; ++c) {
            const int xl = xs + c;
            if (xl < nw_tile && (sLm[xl] == sRm[xl] || x0 + xl == 0)) {
                last_anchor = xl;
                first_anchor = min(first_anchor, xl);
            }
        }
        if (first_anchor < GT) atomicMin(&sFirst, first_anchor);
        const int anchor = block_excl_max<GB / 64>(last_anchor, sScr);   // (its barriers also publish sFirst)
        bool known = anchor >= 0;
        int p = -1;
        if (known && xs < nw_tile) {
            p = anchor + (int)sLm[anchor];
            while (p < xs) p = (p + 1) + (int)sRm[p + 1];           // the chain q -> Rm(q + 1) through tied windows
        }
#pragma unroll
        for (int c = 0; c < GC; ++c) {
            const int xl = xs + c;
            if (xl < nw_tile) {
                const int lm = sLm[xl], rm = sRm[xl];
                if (lm == rm || x0 + xl == 0) { p = xl + lm; known = true; }
                else if (known && p < xl) p = xl + rm;
                if (known && p == xl + t - 1) {                    // an open syncmer (syncmer.cpp:142-145)
                    const uint32_t pos = (uint32_t)(x0 + xl);
                    gk_emit(a, reg, wyhash_u64(canon(lds_bases(sW, (pos >> 4) - wbase, pos & 15u, k), k)));
                }
            }
        }
        if (xs < nw_tile && xs + GC >= nw_tile) a.carry[ti] = known ? x0 + p : -1;   // owner of the tile's last window
        if (tid == 0) a.pend[ti] = (uint32_t)min(sFirst, nw_tile);
    }
}

// rightmost argmin of the canonical s-mer values of window x, from global memory
__device__ int gk_rm_global(const uint32_t *pk, uint32_t nwords, int x, int s, int w)
{
    uint64_t m = ~0ull;
    int rm = 0;
    for (int j = 0; j < w; ++j) {
        const uint64_t v = canon(global_bases(pk, nwords, (uint32_t)(x + j), s), s);
        if (v <= m) { m = v; rm = j; }
    }
    return rm;
}

__global__ __launch_bounds__(GB) void k_gk_fixup(const GkArgs a)
{
    const int k = a.k, s = a.s, t = a.t, w = k - s + 1;
    for (uint32_t ti = blockIdx.x * GB + threadIdx.x; ti < a.n_tiles; ti += gridDim.x * GB) {
        const uint2 td = a.tiles[ti];
        if (td.y == 0 || a.pend[ti] == 0) continue;                 // the tile resolved itself from its first window
        if (a.pend[ti - 1] >= (uint32_t)GT) continue;              // predecessor without an anchor: an earlier walk reaches this tile
        const uint32_t r = td.x;
        const uint32_t L = a.rlen[r];
        const uint32_t *__restrict__ pk = a.packed + a.poff[r];
        const uint32_t nwords = (((L + 15u) >> 4) + 3u) & ~3u;
        const int nwin = (int)L - k + 1;
        const uint32_t reg = a.rreg[r];
        int p = a.carry[ti - 1];
        for (uint32_t tj = ti;; ++tj) {
            const int x0 = (int)a.tiles[tj].y;
            const int nw_tile = min(GT, nwin - x0);
            const int pe = (int)a.pend[tj];
            for (int x = x0; x < x0 + pe; ++x) {                   // windows without a unique minimum: only the chain moves p
                if (p < x) p = x + gk_rm_global(pk, nwords, x, s, w);
                if (p == x + t - 1) gk_emit(a, reg, wyhash_u64(canon(global_bases(pk, nwords, (uint32_t)x, k), k)));
            }
            if (pe < nw_tile) break;                               // the tile has an anchor: k_gk_syncmers did the rest
            a.carry[tj] = p;
            if (tj + 1 >= a.n_tiles || a.tiles[tj + 1].x != r) break;
        }
    }
}

__global__ __launch_bounds__(GB) void k_gk_minimisers(const GkArgs a)
{
    __shared__ uint32_t sW[GWORDS];
    __shared__ uint64_t sV[GT + GMAX_W];
    const int k = a.k;
    const int tid = (int)threadIdx.x;
    for (uint32_t ti = blockIdx.x; ti < a.n_tiles; ti += gridDim.x) {
        const uint2 td = a.tiles[ti];
        const uint32_t r = td.x;
        const int x0 = (int)td.y;
        const uint32_t L = a.rlen[r];
        const uint32_t *__restrict__ pk = a.packed + a.poff[r];
        const uint32_t nwords = (((L + 15u) >> 4) + 3u) & ~3u;
        const int nk = (int)L - k + 1;
        const int W = min(a.wm, nk);                               // the view shrinks the window to the text
        const int nw_tile = min(GT, nk - W + 1 - x0);
        const uint32_t reg = a.rreg[r];
        const uint32_t wbase = (uint32_t)x0 >> 4;
        __syncthreads();
        for (int i = tid; i < GWORDS; i += GB) {
            const uint32_t wi = wbase + (uint32_t)i;
            sW[i] = wi < nwords ? pk[wi] : 0u;
        }
        __syncthreads();
        for (int i = tid; i < nw_tile + W - 1; i += GB) {
            const uint32_t pos = (uint32_t)(x0 + i);
            const uint64_t f = lds_bases(sW, (pos >> 4) - wbase, pos & 15u, k);
            const uint64_t rc = revcomp64(f, k);
            sV[i] = min(f ^ a.seed, rc ^ a.seed);
        }
        __syncthreads();
        const int xs = tid * GC;
        uint64_t prev = 0;
        for (int c = 0; c < GC; ++c) {
            const int xl = xs + c;
            if (xl >= nw_tile) break;
            uint64_t m = sV[xl];
            for (int j = 1; j < W; ++j) m = min(m, sV[xl + j]);
            if (c == 0 || m != prev) gk_emit(a, reg, m);           // (neighbouring windows mostly share their minimum)
            prev = m;
        }
    }
}

// ---- order-preserving compaction: keep(i) = flag ? flag[i] != 0 : in[i] != EMPTY
__device__ __forceinline__ bool cc_keep(const uint64_t *in, const uint8_t *flag, uint64_t i)
{
    return flag ? flag[i] != 0 : in[i] != KEYSET_EMPTY;
}

__global__ __launch_bounds__(GB) void k_cc_count(const uint64_t *__restrict__ in, const uint8_t *__restrict__ flag, uint64_t n, uint64_t *cnt)
{
    __shared__ uint32_t sN;
    if (threadIdx.x == 0) sN = 0;
    __syncthreads();
    const uint64_t i0 = (uint64_t)blockIdx.x * CC_BLOCK, i1 = min(n, i0 + CC_BLOCK);
    uint32_t c = 0;
    for (uint64_t i = i0 + threadIdx.x; i < i1; i += GB) c += cc_keep(in, flag, i) ? 1u : 0u;
    if (c) atomicAdd(&sN, c);
    __syncthreads();
    if (threadIdx.x == 0) cnt[blockIdx.x] = sN;
}

__global__ __launch_bounds__(GB) void k_cc_scatter(const uint64_t *__restrict__ in, const uint8_t *__restrict__ flag, uint64_t n,
                                                   const uint64_t *__restrict__ base, uint64_t *__restrict__ out)
{
    __shared__ uint32_t sScr[8];
    const uint64_t i0 = (uint64_t)blockIdx.x * CC_BLOCK, i1 = min(n, i0 + CC_BLOCK);
    uint64_t at = base[blockIdx.x];
    for (uint64_t j = i0; j < i1; j += GB) {                      // (uniform trip count: the scan is a block operation)
        const uint64_t i = j + threadIdx.x;
        const bool keep = i < i1 && cc_keep(in, flag, i);
        uint32_t tot;
        const uint32_t rank = block_excl_add<GB / 64>(keep ? 1u : 0u, sScr, &tot);
        if (keep) out[at + rank] = in[i];
        at += tot;
    }
}

// new_bounds[j] = elements kept before position bounds[j]
__global__ __launch_bounds__(GB) void k_cc_bounds(const uint64_t *__restrict__ in, const uint8_t *__restrict__ flag, uint64_t n,
                                                  const uint64_t *__restrict__ base, const uint64_t *__restrict__ bounds, uint64_t nb,
                                                  uint64_t *__restrict__ new_bounds)
{
    for (uint64_t j = (uint64_t)blockIdx.x * GB + threadIdx.x; j < nb; j += (uint64_t)gridDim.x * GB) {
        const uint64_t pos = min(bounds[j], n), b = pos / CC_BLOCK;
        uint64_t v = base[b];
        for (uint64_t i = b * CC_BLOCK; i < pos; ++i) v += cc_keep(in, flag, i) ? 1u : 0u;
        new_bounds[j] = v;
    }
}

__global__ __launch_bounds__(GB) void k_gk_starts(const uint64_t *__restrict__ off, uint64_t n_bins, uint8_t *__restrict__ start)
{
    for (uint64_t b = (uint64_t)blockIdx.x * GB + threadIdx.x; b < n_bins; b += (uint64_t)gridDim.x * GB)
        if (off[b + 1] > off[b]) start[off[b]] = 1;
}

// after the sort: keep the first key of every run of equal keys within a bin
__global__ __launch_bounds__(GB) void k_gk_dup_flags(const uint64_t *__restrict__ a, const uint8_t *__restrict__ start, uint64_t n,
                                                     uint8_t *__restrict__ keep)
{
    for (uint64_t i = (uint64_t)blockIdx.x * GB + threadIdx.x; i < n; i += (uint64_t)gridDim.x * GB)
        keep[i] = (i == 0 || start[i] || a[i] != a[i - 1]) ? 1 : 0;
}

#define GK_TRY(expr) TAXOR_HIP_TRY_PREFIX("keyer", expr, #expr)

// scratch grows to what a call needs, never below 16 elements
template <class T> hipError_t want(DeviceBuf<T> &b, uint64_t n) { return b.reserve(n, std::max<uint64_t>(n, 16)); }

// order-preserving compaction of d_in[0, n) (kept: d_flag[i] != 0, or the slots that are not empty when d_flag is null) into a new
// device array *d_out of exactly the kept size (nullptr when nothing is kept); new_bounds[j] = elements kept before bounds[j]
int ordered_compact(const uint64_t *d_in, const uint8_t *d_flag, uint64_t n, const std::vector<uint64_t> &bounds, uint64_t **d_out,
                    std::vector<uint64_t> &new_bounds, uint64_t *total, hipStream_t st)
{
    *d_out = nullptr;
    *total = 0;
    const uint64_t nblk = (n + CC_BLOCK - 1) / CC_BLOCK;
    DeviceBuf<uint64_t> cnt, base, bnd, nbnd;
    std::vector<uint64_t> h(nblk + 1, 0);
    if (nblk) {
        GK_TRY(want(cnt, nblk));
        hipLaunchKernelGGL(k_cc_count, dim3((uint32_t)nblk), dim3(GB), 0, st, d_in, d_flag, n, cnt.p);
        GK_TRY(hipGetLastError());
        GK_TRY(hipMemcpyAsync(h.data(), cnt.p, nblk * sizeof(uint64_t), hipMemcpyDeviceToHost, st));
        GK_TRY(hipStreamSynchronize(st));
    }
    uint64_t run = 0;
    for (uint64_t b = 0; b < nblk; ++b) {
        const uint64_t c = h[b];
        h[b] = run;
        run += c;
    }
    h[nblk] = run;
    *total = run;
    GK_TRY(want(base, nblk + 1));
    GK_TRY(hipMemcpyAsync(base.p, h.data(), (nblk + 1) * sizeof(uint64_t), hipMemcpyHostToDevice, st));
    if (run) {
        GK_TRY(hipMalloc((void **)d_out, run * sizeof(uint64_t)));
        hipLaunchKernelGGL(k_cc_scatter, dim3((uint32_t)nblk), dim3(GB), 0, st, d_in, d_flag, n, base.p, *d_out);
        GK_TRY(hipGetLastError());
    }
    const uint64_t nb = bounds.size();
    new_bounds.assign(nb, 0);
    if (nb) {
        GK_TRY(want(bnd, nb));
        GK_TRY(want(nbnd, nb));
        GK_TRY(hipMemcpyAsync(bnd.p, bounds.data(), nb * sizeof(uint64_t), hipMemcpyHostToDevice, st));
        hipLaunchKernelGGL(k_cc_bounds, dim3(grid_for(nb, GB, 4096)), dim3(GB), 0, st, d_in, d_flag, n, base.p, bnd.p, nb, nbnd.p);
        GK_TRY(hipGetLastError());
        GK_TRY(hipMemcpyAsync(new_bounds.data(), nbnd.p, nb * sizeof(uint64_t), hipMemcpyDeviceToHost, st));
    }
    GK_TRY(hipStreamSynchronize(st));
    return TAXOR_OK;
}

} // namespace

struct taxor_gpu_keyer {
    int device = 0;
    hipStream_t st = nullptr;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    taxor_keyer_params p{};
    int wm = 0;
    double limit = 0.0;
    int grid = 2048;
    // scratch of one call (grows, never shrinks until _finish)
    DeviceBuf<uint8_t> ascii;
    DeviceBuf<uint64_t> aoff, poff, tab, reg_base, reg_mask;
    DeviceBuf<uint32_t> packed, rlen, rreg, pend, reg_marker, flags;
    DeviceBuf<uint2> tiles;
    DeviceBuf<int> carry;
    // what the calls left: per call one bin-grouped array, per (user bin, call) one segment of it
    struct Seg { uint64_t bin, chunk, off, n; };
    std::vector<uint64_t *> chunks;
    std::vector<Seg> segs;
    std::vector<uint8_t> marker;
    // result
    bool finished = false;
    std::vector<uint64_t> bin_off, h_keys;
    bool have_h_keys = false;
    uint64_t *d_keys = nullptr;
    uint64_t *d_arranged = nullptr;
    taxor_keyer_stats stats{};
    void release_scratch()
    {
        ascii.release(); aoff.release(); poff.release(); tab.release(); reg_base.release(); reg_mask.release();
        packed.release(); rlen.release(); rreg.release(); pend.release(); reg_marker.release(); flags.release();
        tiles.release(); carry.release();
    }
    ~taxor_gpu_keyer()
    {
        (void)hipSetDevice(device);
        release_scratch();
        for (uint64_t *c : chunks) (void)hipFree(c);
        if (d_keys) (void)hipFree(d_keys);
        if (d_arranged) (void)hipFree(d_arranged);
        if (ev0) (void)hipEventDestroy(ev0);
        if (ev1) (void)hipEventDestroy(ev1);
        if (st) (void)hipStreamDestroy(st);
    }
};

extern "C" {

int taxor_gpu_keyer_create(int device, const taxor_keyer_params *prm, taxor_gpu_keyer **out)
{
    if (!prm || !out) return fail(TAXOR_E_ARG, "keyer_create: null argument");
    *out = nullptr;
    const taxor_keyer_params &p = *prm;
    if (p.n_bins == 0 || p.n_bins >= (1ull << 32)) return fail(TAXOR_E_ARG, "keyer_create: n_bins must be in [1, 2^32)");
    if (p.use_syncmer) {
        const int k = (int)p.kmer_size, s = (int)p.syncmer_size, t = (int)p.t_syncmer;
        if (k < 2 || k > 32 || s < 1 || s >= k || k - s + 1 > 32 || t < 1 || t > k - s + 1)
            return fail(TAXOR_E_ARG, "keyer_create: unsupported k=" + std::to_string(k) + " s=" + std::to_string(s) + " t=" + std::to_string(t) +
                                      " (need k <= 32, 1 <= s < k, k - s < 32, 1 <= t <= k - s + 1)");
    } else {
        if (p.kmer_size < 1 || p.kmer_size > 32) return fail(TAXOR_E_ARG, "keyer_create: k-mer size outside [1,32]");
        if (p.window_size < p.kmer_size || p.window_size - p.kmer_size + 1 > (uint64_t)GMAX_W)
            return fail(TAXOR_E_ARG, "keyer_create: window size must be in [k, k+511]");
    }
    if (hipSetDevice(device) != hipSuccess) return fail(TAXOR_E_HIP, "keyer_create: no device " + std::to_string(device));
    auto kr = new taxor_gpu_keyer();
    kr->device = device;
    kr->p = p;
    kr->wm = p.use_syncmer ? 0 : (int)(p.window_size - p.kmer_size + 1);
    kr->limit = p.scaling > 1 ? (double)UINT64_MAX / (double)p.scaling : 0.0;   // compute_hashes.cpp: double(v) <= double(UINT64_MAX) / scaling
    kr->marker.assign(p.n_bins, 0);
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) == hipSuccess) kr->grid = prop.multiProcessorCount * 8;
    if (hipStreamCreateWithFlags(&kr->st, hipStreamNonBlocking) != hipSuccess || hipEventCreate(&kr->ev0) != hipSuccess ||
        hipEventCreate(&kr->ev1) != hipSuccess) {
        delete kr;
        return fail(TAXOR_E_HIP, "keyer_create: stream / event creation failed");
    }
    *out = kr;
    return TAXOR_OK;
}

void taxor_gpu_keyer_destroy(taxor_gpu_keyer *kr) { delete kr; }

int taxor_gpu_keyer_add(taxor_gpu_keyer *kr, const char *bases, const uint64_t *rec_off, const uint32_t *rec_bin, uint64_t n_records)
{
    if (!kr || (n_records && (!bases || !rec_off || !rec_bin))) return fail(TAXOR_E_ARG, "keyer_add: null argument");
    if (kr->finished) return fail(TAXOR_E_ARG, "keyer_add: the keyer is finished");
    if (n_records == 0) return TAXOR_OK;
    if (n_records >= (1ull << 31)) return fail(TAXOR_E_ARG, "keyer_add: too many records in one call");
    const double t0 = now_s();
    GK_TRY(hipSetDevice(kr->device));
    const taxor_keyer_params &p = kr->p;
    const int k = (int)p.kmer_size, s = (int)p.syncmer_size, t = (int)p.t_syncmer, w = k - s + 1;
    // ---- host plan: packed offsets, tiles, one set per user bin of the call sized from its records' selection bound
    const uint64_t a_first = rec_off[0];
    std::vector<uint64_t> aoff(n_records + 1), poff(n_records + 1);
    std::vector<uint32_t> rlen(n_records), rreg(n_records);
    std::vector<uint2> tiles;
    std::map<uint64_t, uint32_t> reg_of;
    std::vector<uint64_t> reg_bin, reg_bound;
    uint64_t words = 0;
    for (uint64_t r = 0; r < n_records; ++r) {
        if (rec_off[r + 1] < rec_off[r]) return fail(TAXOR_E_ARG, "keyer_add: record offsets decrease");
        const uint64_t L = rec_off[r + 1] - rec_off[r];
        if (L >= (1ull << 31)) return fail(TAXOR_E_ARG, "keyer_add: record " + std::to_string(r) + " is longer than 2^31 - 1 bases");
        if (rec_bin[r] >= p.n_bins)
            return fail(TAXOR_E_ARG, "keyer_add: record " + std::to_string(r) + " names user bin " + std::to_string(rec_bin[r]) + " of " +
                                          std::to_string(p.n_bins));
        aoff[r] = rec_off[r] - a_first;
        poff[r] = words;
        rlen[r] = (uint32_t)L;
        words += (((L + 15) >> 4) + 3) & ~3ull;
        auto it = reg_of.find(rec_bin[r]);
        if (it == reg_of.end()) {
            it = reg_of.emplace(rec_bin[r], (uint32_t)reg_bin.size()).first;
            reg_bin.push_back(rec_bin[r]);
            reg_bound.push_back(0);
        }
        rreg[r] = it->second;
        const int64_t nk = (int64_t)L - k + 1;
        int64_t nwin = 0, bound = 0;
        if (p.use_syncmer) {
            nwin = nk;
            if (nwin > 0) bound = nwin / std::max(1, std::min(t, w - t + 1)) + 2;   // open syncmers lie at least min(t, w-t+1) apart
        } else if (nk > 0) {
            nwin = nk - std::min<int64_t>(kr->wm, nk) + 1;
            bound = nwin;
        }
        reg_bound[it->second] += (uint64_t)std::max<int64_t>(bound, 0);
        for (int64_t x0 = 0; x0 < nwin; x0 += GT) tiles.push_back(make_uint2((uint32_t)r, (uint32_t)x0));
    }
    const uint64_t a_total = rec_off[n_records] - a_first;
    aoff[n_records] = a_total;
    poff[n_records] = words;
    if (tiles.size() >= (1ull << 32)) return fail(TAXOR_E_ARG, "keyer_add: too many tiles in one call");
    const uint64_t n_reg = reg_bin.size();
    std::vector<uint64_t> reg_base(n_reg + 1), reg_mask(n_reg);
    uint64_t slots = 0;
    for (uint64_t g = 0; g < n_reg; ++g) {
        uint64_t e = REGION_MIN;
        while (e < reg_bound[g] + reg_bound[g] / 2 + 1) e <<= 1;                   // load <= 2/3 at the bound
        reg_base[g] = slots;
        reg_mask[g] = e - 1;
        slots += e;
    }
    reg_base[n_reg] = slots;
    // ---- device
    hipStream_t st = kr->st;
    GK_TRY(want(kr->ascii, a_total + 64));
    GK_TRY(want(kr->aoff, n_records + 1));
    GK_TRY(want(kr->poff, n_records + 1));
    GK_TRY(want(kr->rlen, n_records));
    GK_TRY(want(kr->rreg, n_records));
    GK_TRY(want(kr->packed, words + 4));
    GK_TRY(want(kr->tiles, tiles.size()));
    GK_TRY(want(kr->carry, tiles.size()));
    GK_TRY(want(kr->pend, tiles.size()));
    GK_TRY(want(kr->tab, slots));
    GK_TRY(want(kr->reg_base, n_reg + 1));
    GK_TRY(want(kr->reg_mask, n_reg));
    GK_TRY(want(kr->reg_marker, n_reg));
    GK_TRY(want(kr->flags, 1));
    if (a_total) GK_TRY(hipMemcpyAsync(kr->ascii.p, bases + a_first, a_total, hipMemcpyHostToDevice, st));
    GK_TRY(hipMemcpyAsync(kr->aoff.p, aoff.data(), aoff.size() * sizeof(uint64_t), hipMemcpyHostToDevice, st));
    GK_TRY(hipMemcpyAsync(kr->poff.p, poff.data(), poff.size() * sizeof(uint64_t), hipMemcpyHostToDevice, st));
    GK_TRY(hipMemcpyAsync(kr->rlen.p, rlen.data(), rlen.size() * sizeof(uint32_t), hipMemcpyHostToDevice, st));
    GK_TRY(hipMemcpyAsync(kr->rreg.p, rreg.data(), rreg.size() * sizeof(uint32_t), hipMemcpyHostToDevice, st));
    if (!tiles.empty()) GK_TRY(hipMemcpyAsync(kr->tiles.p, tiles.data(), tiles.size() * sizeof(uint2), hipMemcpyHostToDevice, st));
    GK_TRY(hipMemcpyAsync(kr->reg_base.p, reg_base.data(), (n_reg + 1) * sizeof(uint64_t), hipMemcpyHostToDevice, st));
    GK_TRY(hipMemcpyAsync(kr->reg_mask.p, reg_mask.data(), n_reg * sizeof(uint64_t), hipMemcpyHostToDevice, st));
    GK_TRY(hipMemsetAsync(kr->tab.p, 0xFF, slots * sizeof(uint64_t), st));
    GK_TRY(hipMemsetAsync(kr->reg_marker.p, 0, n_reg * sizeof(uint32_t), st));
    GK_TRY(hipMemsetAsync(kr->flags.p, 0, sizeof(uint32_t), st));
    GkArgs a{};
    a.packed = kr->packed.p;
    a.poff = kr->poff.p;
    a.rlen = kr->rlen.p;
    a.rreg = kr->rreg.p;
    a.tiles = kr->tiles.p;
    a.n_tiles = (uint32_t)tiles.size();
    a.tab = kr->tab.p;
    a.reg_base = kr->reg_base.p;
    a.reg_mask = kr->reg_mask.p;
    a.reg_marker = kr->reg_marker.p;
    a.carry = kr->carry.p;
    a.pend = kr->pend.p;
    a.flags = kr->flags.p;
    a.k = k;
    a.s = s;
    a.t = t;
    a.wm = kr->wm;
    a.seed = 0x8F3F73B5CF1C9ADEull >> (64 - 2 * k);                               // hixf::adjust_seed, adjust_seed.hpp:40-44
    a.scaling_limit = kr->limit;
    GK_TRY(hipEventRecord(kr->ev0, st));
    if (words)
        hipLaunchKernelGGL(k_gk_pack, dim3(grid_for(words, GB, 16384)), dim3(GB), 0, st, kr->ascii.p, kr->aoff.p, kr->poff.p,
                           (uint32_t)n_records, words, kr->packed.p, kr->flags.p);
    if (!tiles.empty()) {
        const int g = (int)std::min<uint64_t>(tiles.size(), (uint64_t)kr->grid);
        if (p.use_syncmer) {
            hipLaunchKernelGGL(k_gk_syncmers, dim3(g), dim3(GB), 0, st, a);
            hipLaunchKernelGGL(k_gk_fixup, dim3(grid_for(tiles.size(), GB, 4096)), dim3(GB), 0, st, a);
        } else {
            hipLaunchKernelGGL(k_gk_minimisers, dim3(g), dim3(GB), 0, st, a);
        }
    }
    GK_TRY(hipGetLastError());
    GK_TRY(hipEventRecord(kr->ev1, st));
    uint32_t flags = 0;
    std::vector<uint32_t> mk(n_reg);
    GK_TRY(hipMemcpyAsync(&flags, kr->flags.p, sizeof flags, hipMemcpyDeviceToHost, st));
    GK_TRY(hipMemcpyAsync(mk.data(), kr->reg_marker.p, n_reg * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    GK_TRY(hipStreamSynchronize(st));
    float ms = 0.f;
    GK_TRY(hipEventElapsedTime(&ms, kr->ev0, kr->ev1));
    if (flags & GK_ALPHABET) return fail(TAXOR_E_ALPHABET, "keyer_add: character outside the dna15 alphabet in the input");
    if (flags & GK_TABLE_FULL) return fail(TAXOR_E_INTERNAL, "keyer_add: a user bin's set outgrew its selection bound");
    // ---- the call's sets -> one bin-grouped array; one segment per user bin
    std::vector<uint64_t> nb;
    uint64_t *chunk = nullptr, total = 0;
    if (int rc = ordered_compact(kr->tab.p, nullptr, slots, reg_base, &chunk, nb, &total, st)) return rc;
    if (chunk) kr->chunks.push_back(chunk);
    for (uint64_t g = 0; g < n_reg; ++g) {
        if (mk[g]) kr->marker[reg_bin[g]] = 1;
        const uint64_t n = nb[g + 1] - nb[g];
        if (n) kr->segs.push_back({reg_bin[g], (uint64_t)kr->chunks.size() - 1, nb[g], n});
    }
    kr->stats.calls += 1;
    kr->stats.records += n_records;
    kr->stats.bases += a_total;
    kr->stats.tiles += tiles.size();
    kr->stats.call_keys += total;
    kr->stats.seconds_device += ms * 1e-3;
    kr->stats.seconds_add += now_s() - t0;
    return TAXOR_OK;
}

int taxor_gpu_keyer_finish(taxor_gpu_keyer *kr, const uint64_t **bin_off, const uint64_t **keys, const uint64_t **d_keys)
{
    if (!kr) return fail(TAXOR_E_ARG, "keyer_finish: null keyer");
    GK_TRY(hipSetDevice(kr->device));
    hipStream_t st = kr->st;
    if (!kr->finished) {
        const double t0 = now_s();
        kr->release_scratch();
        const uint64_t nbin = kr->p.n_bins;
        std::vector<uint64_t> cnt(nbin, 0), nseg(nbin, 0);
        for (const auto &sg : kr->segs) { cnt[sg.bin] += sg.n; ++nseg[sg.bin]; }
        bool multi = false;
        for (uint64_t b = 0; b < nbin; ++b) {
            if (kr->marker[b]) ++cnt[b];
            multi = multi || nseg[b] > 1;
        }
        std::vector<uint64_t> off(nbin + 1, 0);
        for (uint64_t b = 0; b < nbin; ++b) off[b + 1] = off[b] + cnt[b];
        const uint64_t N = off[nbin];
        if (N >= (1ull << 32)) return fail(TAXOR_E_ARG, "keyer_finish: more than 2^32 - 1 keys (the segmented sort's limit)");
        uint64_t *A = nullptr, *B = nullptr;
        GK_TRY(hipMalloc((void **)&A, (N + 1) * sizeof(uint64_t)));
        GK_TRY(hipMalloc((void **)&B, (N + 1) * sizeof(uint64_t)));
        std::vector<uint64_t> fill(off.begin(), off.end() - 1);
        for (const auto &sg : kr->segs) {
            GK_TRY(hipMemcpyAsync(A + fill[sg.bin], kr->chunks[sg.chunk] + sg.off, sg.n * sizeof(uint64_t), hipMemcpyDeviceToDevice, st));
            fill[sg.bin] += sg.n;
        }
        static const uint64_t marker = KEYSET_EMPTY;
        for (uint64_t b = 0; b < nbin; ++b)
            if (kr->marker[b]) GK_TRY(hipMemcpyAsync(A + fill[b], &marker, sizeof marker, hipMemcpyHostToDevice, st));
        GK_TRY(hipStreamSynchronize(st));
        for (uint64_t *c : kr->chunks) (void)hipFree(c);
        kr->chunks.clear();
        kr->segs.clear();
        // every bin ascending: the builder's output is a function of its key lists, so sorted keys make builds repeatable
        if (N) {
            std::vector<uint32_t> beg(nbin), end(nbin);
            for (uint64_t b = 0; b < nbin; ++b) { beg[b] = (uint32_t)off[b]; end[b] = (uint32_t)off[b + 1]; }
            DeviceBuf<uint32_t> d_beg, d_end;
            GK_TRY(want(d_beg, nbin));
            GK_TRY(want(d_end, nbin));
            GK_TRY(hipMemcpyAsync(d_beg.p, beg.data(), nbin * sizeof(uint32_t), hipMemcpyHostToDevice, st));
            GK_TRY(hipMemcpyAsync(d_end.p, end.data(), nbin * sizeof(uint32_t), hipMemcpyHostToDevice, st));
            size_t tmp_bytes = 0;
            GK_TRY(rocprim::segmented_radix_sort_keys(nullptr, tmp_bytes, A, B, (unsigned)N, (unsigned)nbin, d_beg.p, d_end.p, 0, 64, st));
            DeviceBuf<uint8_t> tmp;
            GK_TRY(want(tmp, tmp_bytes));
            GK_TRY(rocprim::segmented_radix_sort_keys((void *)tmp.p, tmp_bytes, A, B, (unsigned)N, (unsigned)nbin, d_beg.p, d_end.p, 0, 64, st));
            GK_TRY(hipStreamSynchronize(st));
        }
        (void)hipFree(A);
        if (multi && N) {
            // a bin whose records came in several calls holds a key once per call that met it: keep the first of each run
            DeviceBuf<uint8_t> start, keep;
            DeviceBuf<uint64_t> d_off;
            GK_TRY(want(start, N));
            GK_TRY(want(keep, N));
            GK_TRY(want(d_off, nbin + 1));
            GK_TRY(hipMemsetAsync(start.p, 0, N, st));
            GK_TRY(hipMemcpyAsync(d_off.p, off.data(), (nbin + 1) * sizeof(uint64_t), hipMemcpyHostToDevice, st));
            hipLaunchKernelGGL(k_gk_starts, dim3(grid_for(nbin, GB, 4096)), dim3(GB), 0, st, d_off.p, nbin, start.p);
            hipLaunchKernelGGL(k_gk_dup_flags, dim3(grid_for(N, GB, 16384)), dim3(GB), 0, st, B, start.p, N, keep.p);
            GK_TRY(hipGetLastError());
            uint64_t *C = nullptr, tot = 0;
            std::vector<uint64_t> noff;
            if (int rc = ordered_compact(B, keep.p, N, off, &C, noff, &tot, st)) return rc;
            (void)hipFree(B);
            B = C;
            off = noff;
        }
        kr->d_keys = B;
        kr->bin_off = off;
        kr->finished = true;
        kr->stats.keys = off[nbin];
        kr->stats.seconds_finish = now_s() - t0;
    }
    if (keys && !kr->have_h_keys) {
        kr->h_keys.resize(kr->bin_off.back());
        if (!kr->h_keys.empty()) GK_TRY(hipMemcpy(kr->h_keys.data(), kr->d_keys, kr->h_keys.size() * sizeof(uint64_t), hipMemcpyDeviceToHost));
        kr->have_h_keys = true;
    }
    if (bin_off) *bin_off = kr->bin_off.data();
    if (keys) *keys = kr->h_keys.data();
    if (d_keys) *d_keys = kr->d_keys;
    return TAXOR_OK;
}

int taxor_gpu_keyer_union_size(taxor_gpu_keyer *kr, const uint32_t *bins, uint64_t n, uint64_t *out)
{
    if (!kr || (n && !bins) || !out) return fail(TAXOR_E_ARG, "keyer_union_size: null argument");
    if (!kr->finished) return fail(TAXOR_E_ARG, "keyer_union_size: call taxor_gpu_keyer_finish first");
    *out = 0;
    GK_TRY(hipSetDevice(kr->device));
    uint64_t tot = 0;
    for (uint64_t i = 0; i < n; ++i) {
        if (bins[i] >= kr->p.n_bins) return fail(TAXOR_E_ARG, "keyer_union_size: user bin out of range");
        tot += kr->bin_off[bins[i] + 1] - kr->bin_off[bins[i]];
    }
    if (!tot) return TAXOR_OK;
    DeviceBuf<uint64_t> cat;
    GK_TRY(want(cat, tot));
    uint64_t at = 0;
    for (uint64_t i = 0; i < n; ++i) {
        const uint64_t lo = kr->bin_off[bins[i]], m = kr->bin_off[bins[i] + 1] - lo;
        if (m) GK_TRY(hipMemcpyAsync(cat.p + at, kr->d_keys + lo, m * sizeof(uint64_t), hipMemcpyDeviceToDevice, kr->st));
        at += m;
    }
    GK_TRY(keyset_count_distinct(cat.p, tot, out, kr->st));
    return TAXOR_OK;
}

int taxor_gpu_keyer_arrange(taxor_gpu_keyer *kr, const uint64_t *first, const uint64_t *count, uint64_t n_ranges, const uint64_t **d_out)
{
    if (!kr || (n_ranges && (!first || !count)) || !d_out) return fail(TAXOR_E_ARG, "keyer_arrange: null argument");
    if (!kr->finished) return fail(TAXOR_E_ARG, "keyer_arrange: call taxor_gpu_keyer_finish first");
    GK_TRY(hipSetDevice(kr->device));
    const uint64_t N = kr->bin_off.back();
    uint64_t tot = 0;
    for (uint64_t i = 0; i < n_ranges; ++i) {
        if (first[i] > N || count[i] > N - first[i]) return fail(TAXOR_E_ARG, "keyer_arrange: range outside the keys");
        tot += count[i];
    }
    if (kr->d_arranged) (void)hipFree(kr->d_arranged);
    kr->d_arranged = nullptr;
    GK_TRY(hipMalloc((void **)&kr->d_arranged, std::max<uint64_t>(tot, 1) * sizeof(uint64_t)));
    uint64_t at = 0;
    for (uint64_t i = 0; i < n_ranges; ++i) {
        if (count[i]) GK_TRY(hipMemcpyAsync(kr->d_arranged + at, kr->d_keys + first[i], count[i] * sizeof(uint64_t), hipMemcpyDeviceToDevice, kr->st));
        at += count[i];
    }
    GK_TRY(hipStreamSynchronize(kr->st));
    *d_out = kr->d_arranged;
    return TAXOR_OK;
}

int taxor_gpu_keyer_stats(const taxor_gpu_keyer *kr, taxor_keyer_stats *out)
{
    if (!kr || !out) return fail(TAXOR_E_ARG, "keyer_stats: null argument");
    *out = kr->stats;
    return TAXOR_OK;
}

int taxor_gpu_device_memory(int device, uint64_t *free_bytes, uint64_t *total_bytes)
{
    if (!free_bytes || !total_bytes) return fail(TAXOR_E_ARG, "device_memory: null argument");
    GK_TRY(hipSetDevice(device));
    size_t f = 0, t = 0;
    GK_TRY(hipMemGetInfo(&f, &t));
    *free_bytes = f;
    *total_bytes = t;
    return TAXOR_OK;
}

} // extern "C"
