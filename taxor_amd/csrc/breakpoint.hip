// breakpoint.hip -- where a read switches reference: the best split of its ordered hash list between two of the references it reported
// (`taxor search --breakpoint-file`).
//
// The object lives beside a resident index for a whole run and keeps nothing between batches but its buffers.  It holds the leaf
// technical bins of every user bin as a CSR (coverage.hip's, hitmap.hip's and confidence.hip's table, restated: those files stay as
// they are) and two bounded staging buffers for hash lists.  A batch brings the searcher's device-resident CSR -- EVERY tuple that
// passed the search threshold, not only the survivors of the 0.8 * max filter -- and the batch's saved hash lists, whose order is the
// order of first occurrence along the read.  The CANDIDATES of a read are its tuples with count > 0, in CSR order; a read is EXAMINED
// when it has a hash and at least two candidates.
//
//   k_bp_count   one wave per read, tuples 64 at a time: M, the read's candidates.  A read without a hash leaves at once.  M goes to
//                the host, which decides who is examined, sums the candidates' offsets and cuts groups, pieces and scratch.
//   k_bp_fill    the same walk over the examined reads; a ballot ranks the candidates of each 64, so tuple index and user bin come out
//                in CSR order.
//   k_bp_probe   one wave per PIECE -- at most BP_SPLIT consecutive hashes of one examined read.  64 hashes per round, one per lane;
//                for each candidate in turn the lookup of section 10.2 (the probe once per IXF among the candidate's leaf bins, three
//                one-byte gathers per leaf bin) and the ballot of the lanes that matched, stored as ONE 64-bit word mask[c][round] by
//                one lane: the whole match matrix at 8 bytes per (candidate, 64 hashes).  Every word is written exactly once, by one
//                wave: nothing is zeroed and nothing is added.
//   k_bp_prefix  one lane per candidate of an examined read, its rounds in order: base[c][k] = the matches in rounds before k, and
//                base[c][rounds] = total_c.  Kept apart from the scan so that no lane reads, within one kernel, what another wrote.
//   k_bp_scan    one wave per examined read, rounds in order, lane = position p = 64 * round + lane.  Per candidate
//                pre = base[c][round] + popcount(mask & lanes below), suf = total_c - pre; P, S and their lowest-index arg-max are
//                updated only on a strictly greater value.  After the candidates a wave arg-max of P + S, ties to the lowest lane,
//                positions >= n masked; carried across rounds only when strictly greater, which keeps the smallest p.  Lane 0 of
//                round 0 is p = 0, where P = 0 and S = max total_c: `single` and `best`.
//
// Every word is an integer maximum or an arg-max with a fixed tie rule over integer sums: nothing depends on the launch geometry nor on
// the cut into pieces, groups and batches.  Every loop is bounded by a count the kernel is given (reads, a read's tuples, a piece's
// hashes, a user bin's leaf bins, a read's candidates and rounds).  No block waits on another.
#include "../../include/taxor_gpu_tools.h"
#include "breakpoint_format.h"
#include "device_prims.h"
#include "hip_host.h"
#include "ixf_arith.h"
#include "kernels.h"
#include "saved_batch.h"
#include "tuning.h"

#include <hip/hip_runtime.h>

#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

// api.hip: the device-resident CSR of a searcher's last run (synchronises it); the searcher's index; an index's IXF descriptors
extern "C" __attribute__((visibility("hidden"))) int taxor_searcher_device_results(taxor_gpu_searcher *s, const uint64_t **d_read_off,
                                                                                   const int64_t **d_user_bin, const uint32_t **d_count,
                                                                                   const uint32_t **d_n_hashes, uint64_t *n_reads,
                                                                                   uint64_t *n_tuples, int *device);
extern "C" __attribute__((visibility("hidden"))) taxor_gpu_index *taxor_searcher_index(taxor_gpu_searcher *s);
extern "C" __attribute__((visibility("hidden"))) int taxor_index_descs(const taxor_gpu_index *idx, const taxor::IxfDesc **d_ixf, const taxor::IxfDesc **h_ixf,
                                                                       uint64_t *n_ixf, uint64_t *n_user_bins, uint32_t *n_passes, int *device);

namespace {

using namespace taxor;

constexpr int BB = 256;                           // threads per block
constexpr int BW = BB / 64;                       // reads / pieces per block pass (one wave each)
constexpr int B_GRID_CAP = 4096;
constexpr uint32_t BP_SPLIT = 2048;               // hashes of one read per piece: a multiple of 64, so a piece's rounds are the read's
constexpr uint64_t STAGE_HASHES = 1ull << 22;     // hashes per staging buffer (32 MiB); there are two
constexpr uint64_t STAGE_PIECES = 1ull << 18;     // pieces per staging buffer (4 MiB); there are two
constexpr uint64_t MAX_READS = 1ull << 31;
constexpr uint64_t BP_BUDGET_WORDS = 1ull << 23;  // mask words of one group of reads (64 MiB; the prefix counts beside them are at most as many bytes)
constexpr int BP_W32 = 9, BP_W64 = 6;             // 32- and 64-bit words per read the scan writes

enum : uint32_t { BP_BAD_BIN = 1u, BP_MISCOUNT = 2u };

struct Piece {
    uint32_t read;       // index in the batch
    uint32_t first;      // offset of the piece's first hash in the staging buffer
    uint32_t n;          // hashes, at most BP_SPLIT
    uint32_t rank0;      // rank of the piece's first hash in the read's list: a multiple of BP_SPLIT
};

__device__ __forceinline__ unsigned long long bp_wave_max(unsigned long long v)
{
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) {
        const unsigned long long t = __shfl_xor(v, d);
        v = t > v ? t : v;
    }
    return v;
}

// a tuple is a candidate when its count is above 0; one that names a user bin outside the index is reported through err
__device__ __forceinline__ bool bp_candidate(const int64_t *__restrict__ ub, const uint32_t *__restrict__ count, uint64_t i, uint64_t hi, uint64_t t0,
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

// the CSR's tuples are indexed from t0 (off[0] == t0)
__global__ __launch_bounds__(BB) void k_bp_count(const uint64_t *__restrict__ off, const int64_t *__restrict__ ub, const uint32_t *__restrict__ count, uint64_t t0,
                                                 const uint32_t *__restrict__ nh, uint64_t n_reads, uint64_t n_bins, uint32_t *__restrict__ n_cand,
                                                 uint32_t *__restrict__ err)
{
    bool bad = false;
    for (uint64_t r = (uint64_t)blockIdx.x * BW + (threadIdx.x >> 6); r < n_reads; r += (uint64_t)gridDim.x * BW) {
        uint32_t m = 0;
        if (nh[r] != 0) {
            const uint64_t lo = off[r], hi = off[r + 1];
            for (uint64_t base = lo; base < hi; base += 64) m += (uint32_t)__popcll(__ballot(bp_candidate(ub, count, base + lane_id(), hi, t0, n_bins, &bad)));
        }
        if (lane_id() == 0) n_cand[r] = m;
    }
    if (bad) atomicOr(err, BP_BAD_BIN);
}

// cand_off is the host's sum of the EXAMINED reads' counts: read r's candidates go to [cand_off[r], cand_off[r + 1]) in CSR order
__global__ __launch_bounds__(BB) void k_bp_fill(const uint64_t *__restrict__ off, const int64_t *__restrict__ ub, const uint32_t *__restrict__ count, uint64_t t0,
                                                uint64_t n_reads, uint64_t n_bins, const uint64_t *__restrict__ cand_off, uint64_t *__restrict__ o_tuple,
                                                int64_t *__restrict__ o_ub, uint32_t *__restrict__ err)
{
    bool bad = false, miscount = false;
    for (uint64_t r = (uint64_t)blockIdx.x * BW + (threadIdx.x >> 6); r < n_reads; r += (uint64_t)gridDim.x * BW) {
        const uint64_t dst0 = cand_off[r], room = cand_off[r + 1] - dst0;
        if (room == 0) continue;
        const uint64_t lo = off[r], hi = off[r + 1];
        uint64_t written = 0;
        for (uint64_t base = lo; base < hi; base += 64) {
            const uint64_t i = base + lane_id();
            const bool k = bp_candidate(ub, count, i, hi, t0, n_bins, &bad);
            const uint64_t m = __ballot(k);
            const uint64_t at = written + (uint64_t)__popcll(m & ((1ull << lane_id()) - 1ull));
            if (k && at < room) {                         // never past the read's room: a walk that disagrees with the count is reported below
                o_tuple[dst0 + at] = i;
                o_ub[dst0 + at] = ub[i - t0];
            }
            written += (uint64_t)__popcll(m);
        }
        miscount = miscount || written != room;
    }
    if (bad) atomicOr(err, BP_BAD_BIN);
    if (miscount) atomicOr(err, BP_MISCOUNT);
}

// what the three kernels after the fill share: the examined reads' candidates and where a read's scratch lies within its group's
struct Layout {
    const uint64_t *cand_off;     // [n_reads + 1]; an empty range: the read is not examined
    const uint64_t *cand_tuple;   // [n_cand] index in the batch CSR
    const int64_t *cand_ub;       // [n_cand] checked against n_bins by the count's walk
    const uint64_t *mask_off;     // [n_reads] first mask word of the read: mask[mask_off[r] + c * rounds + k]
    const uint64_t *base_off;     // [n_reads] first prefix count of the read: base[base_off[r] + c * (rounds + 1) + k]
    const uint32_t *nh;           // [n_reads] rounds = ceil(nh / 64)
    uint64_t *mask;
    uint32_t *base;
};

struct ProbeArgs {
    const IxfDesc *ixf;
    const uint64_t *leaf_off;     // [n_bins + 1] user bin b's leaf technical bins are leaf[leaf_off[b] .. leaf_off[b + 1])
    const uint2 *leaf;            // (IXF, bin)
    Layout l;
    const Piece *pieces;
    const uint64_t *hashes;       // the staged part of the saved lists
    uint32_t n_pieces;
    unsigned long long *lookups;
};

__global__ __launch_bounds__(BB) void k_bp_probe(ProbeArgs a)
{
    unsigned long long lookups = 0;
    const uint32_t lane = lane_id();
    for (uint64_t pi = (uint64_t)blockIdx.x * BW + (threadIdx.x >> 6); pi < a.n_pieces; pi += (uint64_t)gridDim.x * BW) {
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
                const uint64_t l0 = a.leaf_off[b], l1 = a.leaf_off[b + 1];
                bool matched = false;
                uint32_t cur_ixf = 0xFFFFFFFFu;
                IxfDesc d{};
                ixf_probe p{};
                for (uint64_t l = l0; l < l1; ++l) {
                    const uint2 lf = a.leaf[l];
                    if (lf.x != cur_ixf) {                            // a split user bin's parts stand side by side in one IXF: one probe
                        cur_ixf = lf.x;
                        d = a.ixf[lf.x];
                        p = ixf_probe_key_arith(h, d.seed, d.seg_len, d.arith);
                    }
                    if (active && !matched) {
                        const uint8_t f = d.data[(uint64_t)p.row[0] * d.stride + lf.y] ^ d.data[(uint64_t)p.row[1] * d.stride + lf.y] ^
                                          d.data[(uint64_t)p.row[2] * d.stride + lf.y];
                        matched = f == (uint8_t)(p.fp4 & 0xFFu);
                        ++lookups;
                    }
                }
                const uint64_t m = __ballot(matched);
                if (lane == 0) mask[(c - c0) * rounds + round] = m;
            }
        }
    }
    const unsigned long long wave_lookups = wave_incl_add(lookups);     // one atomic per wave
    if (lane == 63 && wave_lookups) atomicAdd(a.lookups, wave_lookups);
}

// reads [r0, r1) of the batch: one group
__global__ __launch_bounds__(BB) void k_bp_prefix(Layout l, uint64_t r0, uint64_t r1)
{
    const uint32_t lane = lane_id();
    for (uint64_t r = r0 + (uint64_t)blockIdx.x * BW + (threadIdx.x >> 6); r < r1; r += (uint64_t)gridDim.x * BW) {
        const uint64_t c0 = l.cand_off[r], m_cand = l.cand_off[r + 1] - c0;
        if (m_cand == 0) continue;
        const uint64_t rounds = ((uint64_t)l.nh[r] + 63) >> 6;
        const uint64_t *mask = l.mask + l.mask_off[r];
        uint32_t *base = l.base + l.base_off[r];
        for (uint64_t c = lane; c < m_cand; c += 64) {
            uint32_t acc = 0;
            for (uint64_t k = 0; k < rounds; ++k) {
                base[c * (rounds + 1) + k] = acc;
                acc += (uint32_t)__popcll(mask[c * rounds + k]);
            }
            base[c * (rounds + 1) + rounds] = acc;
        }
    }
}

// the per-read words, n_reads apart
struct Words {
    uint32_t *gain, *break_hash, *pre_a, *suf_b, *pre_b, *suf_a, *single, *n_cand, *n;
    uint64_t *tuple_a, *tuple_b, *tuple_best;
    int64_t *bin_a, *bin_b, *bin_best;
};

__global__ __launch_bounds__(BB) void k_bp_scan(Layout l, uint64_t r0, uint64_t r1, Words w)
{
    const uint32_t lane = lane_id();
    const uint64_t below = (1ull << lane) - 1ull;
    for (uint64_t r = r0 + (uint64_t)blockIdx.x * BW + (threadIdx.x >> 6); r < r1; r += (uint64_t)gridDim.x * BW) {
        const uint64_t c0 = l.cand_off[r], m_cand = l.cand_off[r + 1] - c0;
        if (m_cand == 0) continue;
        const uint32_t n = l.nh[r];
        const uint64_t rounds = ((uint64_t)n + 63) >> 6;
        const uint64_t *mask = l.mask + l.mask_off[r];
        const uint32_t *base = l.base + l.base_off[r];
        long long top = -1;                                   // max_p split(p) over the rounds so far, and what belongs to its smallest p
        uint32_t t_p = 0, t_P = 0, t_S = 0, t_a = 0, t_b = 0, t_suf_a = 0, t_pre_b = 0, single = 0, best = 0;
        for (uint64_t k = 0; k < rounds; ++k) {
            const uint64_t p = k * 64 + lane;
            uint32_t P = 0, S = 0, arg_p = 0, arg_s = 0, suf_a = 0, pre_b = 0;
            for (uint64_t c = 0; c < m_cand; ++c) {           // the three loads are the same in every lane
                const uint32_t pre = base[c * (rounds + 1) + k] + (uint32_t)__popcll(mask[c * rounds + k] & below);
                const uint32_t suf = base[c * (rounds + 1) + rounds] - pre;
                if (c == 0 || pre > P) { P = pre; arg_p = (uint32_t)c; suf_a = suf; }
                if (c == 0 || suf > S) { S = suf; arg_s = (uint32_t)c; pre_b = pre; }
            }
            if (k == 0) {                                     // p = 0: every prefix is 0, S = max total_c at its lowest c
                single = __shfl(S, 0);
                best = __shfl(arg_s, 0);
            }
            // split(p) above the lane, so that the greatest key is the greatest split at its lowest lane; 0 for p >= n (lane 0 of a round has p < n)
            const unsigned long long key = p < n ? ((((unsigned long long)P + S) << 6) | (63u - lane)) + 1ull : 0ull;
            const unsigned long long mx = bp_wave_max(key) - 1ull;
            const long long v = (long long)(mx >> 6);
            if (v > top) {                                    // strictly: an equal split later in the list does not move the break
                const int src = 63 - (int)(mx & 63ull);
                top = v;
                t_p = (uint32_t)(k * 64) + (uint32_t)src;
                t_P = __shfl(P, src);
                t_S = __shfl(S, src);
                t_a = __shfl(arg_p, src);
                t_b = __shfl(arg_s, src);
                t_suf_a = __shfl(suf_a, src);
                t_pre_b = __shfl(pre_b, src);
            }
        }
        if (lane == 0) {
            w.gain[r] = (uint32_t)top - single;
            w.break_hash[r] = t_p;
            w.pre_a[r] = t_P;
            w.suf_b[r] = t_S;
            w.pre_b[r] = t_pre_b;
            w.suf_a[r] = t_suf_a;
            w.single[r] = single;
            w.n_cand[r] = (uint32_t)m_cand;
            w.n[r] = n;
            w.tuple_a[r] = l.cand_tuple[c0 + t_a];
            w.tuple_b[r] = l.cand_tuple[c0 + t_b];
            w.tuple_best[r] = l.cand_tuple[c0 + best];
            w.bin_a[r] = l.cand_ub[c0 + t_a];
            w.bin_b[r] = l.cand_ub[c0 + t_b];
            w.bin_best[r] = l.cand_ub[c0 + best];
        }
    }
}

#define BP_TRY(expr) TAXOR_HIP_TRY_PREFIX("breakpoint", expr, #expr)

// the results of one caller (a searcher, or add_csr): device words and work arrays, and their page-locked copies
struct Slot {
    DeviceBuf<uint32_t> d_w32, d_n_cand;
    DeviceBuf<uint64_t> d_w64, d_off3, d_cand_tuple;    // d_off3: cand_off[n + 1] | mask_off[n] | base_off[n]
    DeviceBuf<int64_t> d_cand_ub;
    uint32_t *h32 = nullptr;       // BP_W32 words | n_hashes | the candidates' counts, cap each
    uint64_t *h64 = nullptr;       // BP_W64 words, cap each
    uint64_t *h_off3 = nullptr;    // 3 * cap + 1
    uint8_t *h_examined = nullptr;
    uint64_t cap = 0;
    void drop()
    {
        if (h32) (void)hipHostFree(h32);
        if (h64) (void)hipHostFree(h64);
        if (h_off3) (void)hipHostFree(h_off3);
        if (h_examined) (void)hipHostFree(h_examined);
        h32 = nullptr;
        h64 = nullptr;
        h_off3 = nullptr;
        h_examined = nullptr;
        cap = 0;
    }
    ~Slot() { drop(); }
};

struct Group {
    uint64_t r0, r1;               // reads [r0, r1) of the batch
    uint64_t mask_words, base_words;
};

}   // namespace

struct taxor_gpu_breakpoint {
    taxor_gpu_index *idx = nullptr;
    int device = 0;
    uint32_t min_gain = 1;
    uint64_t n_bins = 0, budget_words = BP_BUDGET_WORDS;
    const IxfDesc *d_ixf = nullptr;
    hipStream_t st = nullptr;
    std::mutex mu;                                    // batches may come from several threads
    DeviceBuf<uint64_t> d_leaf_off, d_hashes[2], d_mask;
    DeviceBuf<uint32_t> d_base, d_err;
    DeviceBuf<uint2> d_leaf;
    DeviceBuf<Piece> d_pieces[2];
    DeviceBuf<unsigned long long> d_lookups;
    Piece *h_pieces[2] = {nullptr, nullptr};          // page-locked; ev_free[i] says that buffer i's copy has left it
    hipEvent_t ev_free[2] = {nullptr, nullptr};
    bool ev_used[2] = {false, false};
    std::vector<hipEvent_t> ev_time;                  // pairs around the kernel launches of one call
    std::vector<uint32_t> h_nh;
    std::vector<Group> groups;
    std::map<const void *, std::unique_ptr<Slot>> slots;
    // host arrays of add_csr on the device
    DeviceBuf<uint64_t> c_off;
    DeviceBuf<int64_t> c_ub;
    DeviceBuf<uint32_t> c_cnt, c_nh;
    ~taxor_gpu_breakpoint()
    {
        slots.clear();
        for (int i = 0; i < 2; ++i) {
            if (h_pieces[i]) (void)hipHostFree(h_pieces[i]);
            if (ev_free[i]) (void)hipEventDestroy(ev_free[i]);
        }
        for (hipEvent_t e : ev_time) (void)hipEventDestroy(e);
        if (st) (void)hipStreamDestroy(st);
    }
};

namespace {

// One batch whose CSR is on the object's device (tuples indexed from t0); the hash lists are host arrays (read r's at
// hashes[hash_off[r] .. hash_off[r + 1]), h_nh[r] of them).  The caller holds the mutex and has made every check that needs no launch.
int add_device(taxor_gpu_breakpoint *c, const void *who, uint64_t n, const uint64_t *d_off, const int64_t *d_ub, const uint32_t *d_cnt, const uint32_t *d_nh,
               uint64_t t0, const uint64_t *hash_off, const uint64_t *hashes, const uint32_t *h_nh, taxor_breakpoint_batch *out)
{
    std::unique_ptr<Slot> &sp = c->slots[who];
    if (!sp) sp = std::make_unique<Slot>();
    Slot &sl = *sp;
    if (n > sl.cap) {
        const uint64_t want = std::max<uint64_t>(n + n / 2, 1024);
        sl.drop();
        BP_TRY(sl.d_w32.alloc(BP_W32 * want));
        BP_TRY(sl.d_w64.alloc(BP_W64 * want));
        BP_TRY(sl.d_n_cand.alloc(want));
        BP_TRY(sl.d_off3.alloc(3 * want + 1));
        BP_TRY(hipHostMalloc((void **)&sl.h32, (BP_W32 + 2) * want * sizeof(uint32_t), hipHostMallocDefault));
        BP_TRY(hipHostMalloc((void **)&sl.h64, BP_W64 * want * sizeof(uint64_t), hipHostMallocDefault));
        BP_TRY(hipHostMalloc((void **)&sl.h_off3, (3 * want + 1) * sizeof(uint64_t), hipHostMallocDefault));
        BP_TRY(hipHostMalloc((void **)&sl.h_examined, want, hipHostMallocDefault));
        sl.cap = want;
    }
    uint32_t *h32 = sl.h32;
    uint64_t *h64 = sl.h64;
    out->n_reads = n;
    out->n_examined = out->n_reported = 0;
    out->min_gain = c->min_gain;
    out->reserved = 0;
    out->examined = sl.h_examined;
    out->gain = h32;
    out->break_hash = h32 + n;
    out->pre_a = h32 + 2 * n;
    out->suf_b = h32 + 3 * n;
    out->pre_b = h32 + 4 * n;
    out->suf_a = h32 + 5 * n;
    out->single = h32 + 6 * n;
    out->n_candidates = h32 + 7 * n;
    out->n = h32 + 8 * n;
    out->n_hashes = h32 + 9 * n;
    out->tuple_a = h64;
    out->tuple_b = h64 + n;
    out->tuple_best = h64 + 2 * n;
    out->bin_a = (const int64_t *)(h64 + 3 * n);
    out->bin_b = (const int64_t *)(h64 + 4 * n);
    out->bin_best = (const int64_t *)(h64 + 5 * n);
    out->seconds_kernels = 0;
    out->lookups = 0;
    if (c->ev_used[0] || c->ev_used[1]) {              // a call that failed half-way: its copies out of the page-locked pieces end first
        BP_TRY(hipStreamSynchronize(c->st));
        c->ev_used[0] = c->ev_used[1] = false;
    }
    if (n == 0) return TAXOR_OK;
    uint32_t *d32 = sl.d_w32.p;
    uint64_t *d64 = sl.d_w64.p;
    Words w{d32, d32 + n, d32 + 2 * n, d32 + 3 * n, d32 + 4 * n, d32 + 5 * n, d32 + 6 * n, d32 + 7 * n, d32 + 8 * n,
            d64, d64 + n, d64 + 2 * n, (int64_t *)(d64 + 3 * n), (int64_t *)(d64 + 4 * n), (int64_t *)(d64 + 5 * n)};

    size_t n_ev = 0;
    auto stamp = [&]() -> int {                        // an event on the stream: launches are timed between pairs of them
        if (c->ev_time.size() <= n_ev) {
            hipEvent_t e = nullptr;
            BP_TRY(hipEventCreate(&e));
            c->ev_time.push_back(e);
        }
        BP_TRY(hipEventRecord(c->ev_time[n_ev++], c->st));
        return TAXOR_OK;
    };

    // the words of a read that is not examined are 0
    BP_TRY(hipMemsetAsync(d32, 0, BP_W32 * n * sizeof(uint32_t), c->st));
    BP_TRY(hipMemsetAsync(d64, 0, BP_W64 * n * sizeof(uint64_t), c->st));
    BP_TRY(hipMemsetAsync(c->d_lookups.p, 0, 8, c->st));
    if (int rc = stamp()) return rc;
    k_bp_count<<<grid_for(n, BW, B_GRID_CAP), BB, 0, c->st>>>(d_off, d_ub, d_cnt, t0, d_nh, n, c->n_bins, sl.d_n_cand.p, c->d_err.p);
    BP_TRY(hipGetLastError());
    if (int rc = stamp()) return rc;
    uint32_t *h_m = h32 + (BP_W32 + 1) * n;            // the candidates' counts, behind what the caller sees
    uint32_t err = 0;
    BP_TRY(hipMemcpyAsync(h_m, sl.d_n_cand.p, n * sizeof(uint32_t), hipMemcpyDeviceToHost, c->st));
    BP_TRY(hipMemcpyAsync(&err, c->d_err.p, 4, hipMemcpyDeviceToHost, c->st));
    BP_TRY(hipStreamSynchronize(c->st));
    if (err & BP_BAD_BIN) {
        BP_TRY(hipMemset(c->d_err.p, 0, 4));
        return fail(TAXOR_E_INTERNAL, "breakpoint_add: user_bin: a tuple names a user bin outside the index's %llu", (unsigned long long)c->n_bins);
    }
    // who is examined; the candidates' offsets; groups of reads whose masks stay within the budget, a read that exceeds it by itself
    // alone; where a read's masks and prefix counts lie within its group's scratch
    uint64_t *cand_off = sl.h_off3, *mask_off = cand_off + n + 1, *base_off = mask_off + n;
    c->groups.clear();
    uint64_t n_cand = 0, n_examined = 0, max_mask = 0, max_base = 0, big_read = 0;
    for (uint64_t r = 0; r < n; ++r) {
        cand_off[r] = n_cand;
        mask_off[r] = base_off[r] = 0;
        const bool ex = h_nh[r] != 0 && h_m[r] >= 2;
        sl.h_examined[r] = ex ? 1 : 0;
        if (!ex) continue;
        ++n_examined;
        n_cand += h_m[r];
        const uint64_t rounds = ((uint64_t)h_nh[r] + 63) >> 6, mw = (uint64_t)h_m[r] * rounds, bw = (uint64_t)h_m[r] * (rounds + 1);
        if (c->groups.empty() || c->groups.back().mask_words + mw > c->budget_words) c->groups.push_back(Group{r, r, 0, 0});
        Group &g = c->groups.back();
        mask_off[r] = g.mask_words;
        base_off[r] = g.base_words;
        g.mask_words += mw;
        g.base_words += bw;
        g.r1 = r + 1;
        if (g.mask_words > max_mask) {
            max_mask = g.mask_words;
            big_read = r;
        }
        max_base = std::max(max_base, g.base_words);
    }
    cand_off[n] = n_cand;
    out->n_examined = n_examined;
    memcpy(h32 + BP_W32 * n, h_nh, n * sizeof(uint32_t));
    if (n_examined) {
        const hipError_t e_mask = c->d_mask.reserve(max_mask, max_mask), e_base = e_mask == hipSuccess ? c->d_base.reserve(max_base, max_base) : e_mask;
        if (e_base != hipSuccess) {
            (void)hipGetLastError();
            return fail(TAXOR_E_NOMEM, "breakpoint_add: scratch: %llu bytes of match masks and %llu bytes of prefix counts could not be allocated (%s); the group ends with read %llu, "
                                       "which has %u candidates and %u hashes",
                        (unsigned long long)(max_mask * 8), (unsigned long long)(max_base * 4), hipGetErrorString(e_base), (unsigned long long)big_read, h_m[big_read],
                        h_nh[big_read]);
        }
        BP_TRY(sl.d_cand_tuple.reserve(n_cand, n_cand + n_cand / 2));
        BP_TRY(sl.d_cand_ub.reserve(n_cand, n_cand + n_cand / 2));
        BP_TRY(hipMemcpyAsync(sl.d_off3.p, sl.h_off3, (3 * n + 1) * 8, hipMemcpyHostToDevice, c->st));
        if (int rc = stamp()) return rc;
        k_bp_fill<<<grid_for(n, BW, B_GRID_CAP), BB, 0, c->st>>>(d_off, d_ub, d_cnt, t0, n, c->n_bins, sl.d_off3.p, sl.d_cand_tuple.p, sl.d_cand_ub.p, c->d_err.p);
        BP_TRY(hipGetLastError());
        if (int rc = stamp()) return rc;

        ProbeArgs a{};
        a.ixf = c->d_ixf;
        a.leaf_off = c->d_leaf_off.p;
        a.leaf = c->d_leaf.p;
        a.l = Layout{sl.d_off3.p, sl.d_cand_tuple.p, sl.d_cand_ub.p, sl.d_off3.p + n + 1, sl.d_off3.p + 2 * n + 1, d_nh, c->d_mask.p, c->d_base.p};
        a.lookups = c->d_lookups.p;
        // Pieces are staged and launched in bounded sets (hitmap.hip's scheme): at most STAGE_PIECES pieces whose hashes lie within
        // STAGE_HASHES consecutive entries of the dense host array, copied as one range.  A group's sets come first, then its prefix
        // counts and its scan; the next group writes the same scratch behind them on the stream
        int buf = 0;
        uint32_t n_p = 0;
        uint64_t g0 = 0, g1 = 0;            // the set's hashes: [g0, g1) of hashes
        auto flush = [&]() -> int {
            if (n_p == 0) return TAXOR_OK;
            BP_TRY(hipMemcpyAsync(c->d_hashes[buf].p, hashes + g0, (g1 - g0) * 8, hipMemcpyHostToDevice, c->st));
            BP_TRY(hipMemcpyAsync(c->d_pieces[buf].p, c->h_pieces[buf], (uint64_t)n_p * sizeof(Piece), hipMemcpyHostToDevice, c->st));
            BP_TRY(hipEventRecord(c->ev_free[buf], c->st));
            c->ev_used[buf] = true;
            a.pieces = c->d_pieces[buf].p;
            a.hashes = c->d_hashes[buf].p;
            a.n_pieces = n_p;
            if (int rc = stamp()) return rc;
            k_bp_probe<<<grid_for(n_p, BW, B_GRID_CAP), BB, 0, c->st>>>(a);
            BP_TRY(hipGetLastError());
            if (int rc = stamp()) return rc;
            buf ^= 1;
            n_p = 0;
            if (c->ev_used[buf]) BP_TRY(hipEventSynchronize(c->ev_free[buf]));     // the page-locked pieces of two sets ago have been copied
            return TAXOR_OK;
        };
        for (const Group &g : c->groups) {
            for (uint64_t r = g.r0; r < g.r1; ++r) {
                if (!sl.h_examined[r]) continue;
                const uint64_t h0 = hash_off[r], nh = h_nh[r];
                for (uint64_t done = 0; done < nh;) {
                    const uint32_t take = (uint32_t)std::min<uint64_t>(BP_SPLIT, nh - done);
                    if (n_p && (n_p == STAGE_PIECES || h0 + done + take - g0 > STAGE_HASHES))
                        if (int rc = flush()) return rc;
                    if (n_p == 0) g0 = h0 + done;
                    c->h_pieces[buf][n_p++] = Piece{(uint32_t)r, (uint32_t)(h0 + done - g0), take, (uint32_t)done};
                    done += take;
                    g1 = h0 + done;
                }
            }
            if (int rc = flush()) return rc;
            if (int rc = stamp()) return rc;
            k_bp_prefix<<<grid_for(g.r1 - g.r0, BW, B_GRID_CAP), BB, 0, c->st>>>(a.l, g.r0, g.r1);
            k_bp_scan<<<grid_for(g.r1 - g.r0, BW, B_GRID_CAP), BB, 0, c->st>>>(a.l, g.r0, g.r1, w);
            BP_TRY(hipGetLastError());
            if (int rc = stamp()) return rc;
        }
    }
    BP_TRY(hipMemcpyAsync(h32, d32, BP_W32 * n * sizeof(uint32_t), hipMemcpyDeviceToHost, c->st));
    BP_TRY(hipMemcpyAsync(h64, d64, BP_W64 * n * sizeof(uint64_t), hipMemcpyDeviceToHost, c->st));
    unsigned long long lookups = 0;
    BP_TRY(hipMemcpyAsync(&lookups, c->d_lookups.p, 8, hipMemcpyDeviceToHost, c->st));
    BP_TRY(hipMemcpyAsync(&err, c->d_err.p, 4, hipMemcpyDeviceToHost, c->st));
    BP_TRY(hipStreamSynchronize(c->st));               // the searcher's buffers and the hash lists are the caller's again
    c->ev_used[0] = c->ev_used[1] = false;
    for (size_t i = 0; i + 1 < n_ev; i += 2) {
        float ms = 0;
        BP_TRY(hipEventElapsedTime(&ms, c->ev_time[i], c->ev_time[i + 1]));
        out->seconds_kernels += (double)ms * 1e-3;
    }
    out->lookups = lookups;
    if (err) {                                         // the CSR changed under the call: the second walk did not find what the first counted
        BP_TRY(hipMemset(c->d_err.p, 0, 4));
        return fail(TAXOR_E_INTERNAL, "breakpoint_add: candidates: the walk that writes the candidates disagrees with the walk that counted them (flags %u)", err);
    }
    for (uint64_t r = 0; r < n; ++r) out->n_reported += sl.h_examined[r] && out->gain[r] >= c->min_gain;
    return TAXOR_OK;
}

}   // namespace

extern "C" int taxor_gpu_breakpoint_create(taxor_gpu_index *idx, const taxor_hixf_view *view, uint32_t min_gain, taxor_gpu_breakpoint **out)
{
    if (!out) return fail(TAXOR_E_ARG, "breakpoint_create: null argument");
    *out = nullptr;
    if (!idx || !view) return fail(TAXOR_E_ARG, "breakpoint_create: null argument");
    if (min_gain < 1) return fail(TAXOR_E_ARG, "breakpoint_create: min_gain: %u is below 1 (a read whose best split explains nothing beyond its best reference is never reported)", min_gain);
    const IxfDesc *d_ixf = nullptr, *h_ixf = nullptr;
    uint64_t n_ixf = 0, n_bins = 0;
    uint32_t n_passes = 0;
    int device = 0;
    if (taxor_index_descs(idx, &d_ixf, &h_ixf, &n_ixf, &n_bins, &n_passes, &device)) return fail(TAXOR_E_ARG, "breakpoint_create: null index");
    if (n_passes)
        return fail(TAXOR_E_ARG, "breakpoint_create: a paged index (%u resident pass%s) is refused: its leaf bins are not all resident at once and a read's final tuples exist only after the last pass's merge; finding breaks pass by pass is not built",
                    n_passes, n_passes == 1 ? "" : "es");
    if (view->n_ixf != n_ixf || view->n_user_bins != n_bins || (n_ixf && !view->ixf))
        return fail(TAXOR_E_ARG, "breakpoint_create: the view (%llu IXFs, %llu user bins) is not the index's (%llu IXFs, %llu user bins)", (unsigned long long)view->n_ixf,
                    (unsigned long long)view->n_user_bins, (unsigned long long)n_ixf, (unsigned long long)n_bins);
    if (n_bins >= (1ull << 32) || n_ixf >= (1ull << 32)) return fail(TAXOR_E_ARG, "breakpoint_create: user bins and IXFs are numbered in 32 bits");
    // the inverse of fname_idx: every leaf technical bin of a user bin, root included, as one CSR in index order (the set and the order
    // of coverage.hip's, hitmap.hip's and confidence.hip's tables, restated once more: those files, and their objects, stay as they are)
    std::vector<uint64_t> leaf_off(n_bins + 1, 0);
    for (uint64_t x = 0; x < n_ixf; ++x) {
        const taxor_ixf_view &f = view->ixf[x];
        if (f.bins != h_ixf[x].bins) return fail(TAXOR_E_ARG, "breakpoint_create: IXF %llu has %llu bins in the view, %u in the index", (unsigned long long)x, (unsigned long long)f.bins, h_ixf[x].bins);
        if (!f.fname_idx) return fail(TAXOR_E_ARG, "breakpoint_create: IXF %llu of the view has no fname_idx", (unsigned long long)x);
        for (uint64_t j = 0; j < f.bins; ++j) {
            const int64_t b = f.fname_idx[j];
            if (b < 0) continue;
            if ((uint64_t)b >= n_bins) return fail(TAXOR_E_ARG, "breakpoint_create: bin %llu of IXF %llu names user bin %lld of %llu", (unsigned long long)j, (unsigned long long)x, (long long)b, (unsigned long long)n_bins);
            ++leaf_off[(uint64_t)b + 1];
        }
    }
    for (uint64_t b = 0; b < n_bins; ++b) leaf_off[b + 1] += leaf_off[b];
    std::vector<uint2> leaf(leaf_off[n_bins]);
    {
        std::vector<uint64_t> at(leaf_off.begin(), leaf_off.end() - 1);
        for (uint64_t x = 0; x < n_ixf; ++x)
            for (uint64_t j = 0; j < view->ixf[x].bins; ++j) {
                const int64_t b = view->ixf[x].fname_idx[j];
                if (b >= 0) leaf[at[(uint64_t)b]++] = make_uint2((uint32_t)x, (uint32_t)j);
            }
    }
    BP_TRY(hipSetDevice(device));
    auto c = std::make_unique<taxor_gpu_breakpoint>();
    c->idx = idx;
    c->device = device;
    c->min_gain = min_gain;
    c->n_bins = n_bins;
    c->d_ixf = d_ixf;
    // a measurement knob (tuning.h): the mask words of one group of reads.  It moves the cut into groups, never a result
    if (const char *e = tune_env("TAXOR_BREAKPOINT_BUDGET_WORDS")) {
        const long long v = atoll(e);
        if (v >= 1) c->budget_words = (uint64_t)v;
    }
    BP_TRY(hipStreamCreate(&c->st));
    BP_TRY(c->d_leaf_off.alloc(n_bins + 1));
    BP_TRY(c->d_leaf.alloc(leaf.size() + 1));
    BP_TRY(c->d_err.alloc(1));
    BP_TRY(c->d_lookups.alloc(1));
    for (int i = 0; i < 2; ++i) {
        BP_TRY(c->d_hashes[i].alloc(STAGE_HASHES));
        BP_TRY(c->d_pieces[i].alloc(STAGE_PIECES));
        BP_TRY(hipHostMalloc((void **)&c->h_pieces[i], STAGE_PIECES * sizeof(Piece), hipHostMallocDefault));
        BP_TRY(hipEventCreateWithFlags(&c->ev_free[i], hipEventDisableTiming));
    }
    BP_TRY(hipMemcpy(c->d_leaf_off.p, leaf_off.data(), (n_bins + 1) * 8, hipMemcpyHostToDevice));
    if (!leaf.empty()) BP_TRY(hipMemcpy(c->d_leaf.p, leaf.data(), leaf.size() * 8, hipMemcpyHostToDevice));
    BP_TRY(hipMemset(c->d_err.p, 0, 4));
    *out = c.release();
    return TAXOR_OK;
}

extern "C" void taxor_gpu_breakpoint_destroy(taxor_gpu_breakpoint *c)
{
    if (!c) return;
    (void)hipSetDevice(c->device);
    delete c;
}

extern "C" int taxor_gpu_breakpoint_add_batch(taxor_gpu_breakpoint *c, taxor_gpu_searcher *s, const taxor_gpu_saved *saved, taxor_breakpoint_batch *out)
{
    if (!c || !s || !out) return fail(TAXOR_E_ARG, "breakpoint_add_batch: null argument");
    if (!saved) return fail(TAXOR_E_ARG, "breakpoint_add_batch: saved: no saved batch (the batch ran with capture off, or its lists were not taken)");
    if (taxor_searcher_index(s) != c->idx) return fail(TAXOR_E_ARG, "breakpoint_add_batch: index: the searcher works on another index than the breakpoint object");
    const std::string unsound = saved_validate(*saved);
    if (!unsound.empty()) return fail(TAXOR_E_ARG, "breakpoint_add_batch: " + unsound);
    const uint64_t *d_off = nullptr;
    const int64_t *d_ub = nullptr;
    const uint32_t *d_cnt = nullptr, *d_nh = nullptr;
    uint64_t n = 0, nt = 0;
    int dev = 0;
    if (int rc = taxor_searcher_device_results(s, &d_off, &d_ub, &d_cnt, &d_nh, &n, &nt, &dev)) return rc;
    if (saved->n_reads != n)
        return fail(TAXOR_E_ARG, "breakpoint_add_batch: n_reads: the saved batch holds %llu reads, the searcher's last batch %llu", (unsigned long long)saved->n_reads, (unsigned long long)n);
    if (n >= MAX_READS) return fail(TAXOR_E_ARG, "breakpoint_add_batch: n_reads: a batch of 2^31 reads or more");
    std::lock_guard<std::mutex> lk(c->mu);
    BP_TRY(hipSetDevice(c->device));
    c->h_nh.resize(n);
    if (n) BP_TRY(hipMemcpy(c->h_nh.data(), d_nh, n * 4, hipMemcpyDeviceToHost));
    for (uint64_t r = 0; r < n; ++r)
        if (c->h_nh[r] != saved->n_hashes[r])
            return fail(TAXOR_E_ARG, "breakpoint_add_batch: n_hashes: read %llu has %u hashes in the saved batch, %u in the searcher's last batch", (unsigned long long)r, saved->n_hashes[r], c->h_nh[r]);
    return add_device(c, s, n, d_off, d_ub, d_cnt, d_nh, 0, saved->hash_off.data(), saved->hashes, c->h_nh.data(), out);
}

extern "C" int taxor_gpu_breakpoint_add_csr(taxor_gpu_breakpoint *c, uint64_t n_reads, const uint64_t *read_off, const int64_t *user_bin, const uint32_t *count,
                                            const uint64_t *hash_off, const uint64_t *hashes, taxor_breakpoint_batch *out)
{
    if (!c || !read_off || !hash_off || !out) return fail(TAXOR_E_ARG, "breakpoint_add_csr: null argument");
    if (n_reads >= MAX_READS) return fail(TAXOR_E_ARG, "breakpoint_add_csr: n_reads: 2^31 reads or more");
    for (uint64_t r = 0; r < n_reads; ++r) {
        if (read_off[r + 1] < read_off[r] || read_off[r + 1] - read_off[r] >= (1ull << 32))
            return fail(TAXOR_E_ARG, "breakpoint_add_csr: read_off: the tuples of read %llu are malformed", (unsigned long long)r);
        if (hash_off[r + 1] < hash_off[r] || hash_off[r + 1] - hash_off[r] >= (1ull << 32))
            return fail(TAXOR_E_ARG, "breakpoint_add_csr: hash_off: the list of read %llu is malformed", (unsigned long long)r);
    }
    const uint64_t t0 = read_off[0], nt = read_off[n_reads] - t0;
    if (nt && (!user_bin || !count)) return fail(TAXOR_E_ARG, "breakpoint_add_csr: user_bin / count: null array");
    if (hash_off[n_reads] > hash_off[0] && !hashes) return fail(TAXOR_E_ARG, "breakpoint_add_csr: hashes: null array");
    for (uint64_t i = t0; i < t0 + nt; ++i)
        if (user_bin[i] < 0 || (uint64_t)user_bin[i] >= c->n_bins)
            return fail(TAXOR_E_ARG, "breakpoint_add_csr: user_bin: tuple %llu names user bin %lld, the index has %llu", (unsigned long long)i, (long long)user_bin[i], (unsigned long long)c->n_bins);
    std::lock_guard<std::mutex> lk(c->mu);
    BP_TRY(hipSetDevice(c->device));
    c->h_nh.resize(n_reads);
    for (uint64_t r = 0; r < n_reads; ++r) c->h_nh[r] = (uint32_t)(hash_off[r + 1] - hash_off[r]);
    BP_TRY(c->c_off.reserve(n_reads + 1, n_reads + 1 + n_reads / 2));
    BP_TRY(c->c_nh.reserve(n_reads + 1, n_reads + 1 + n_reads / 2));
    BP_TRY(c->c_ub.reserve(nt + 1, nt + 1 + nt / 2));
    BP_TRY(c->c_cnt.reserve(nt + 1, nt + 1 + nt / 2));
    BP_TRY(hipMemcpy(c->c_off.p, read_off, (n_reads + 1) * 8, hipMemcpyHostToDevice));
    if (nt) {
        BP_TRY(hipMemcpy(c->c_ub.p, user_bin + t0, nt * 8, hipMemcpyHostToDevice));
        BP_TRY(hipMemcpy(c->c_cnt.p, count + t0, nt * 4, hipMemcpyHostToDevice));
    }
    if (n_reads) BP_TRY(hipMemcpy(c->c_nh.p, c->h_nh.data(), n_reads * 4, hipMemcpyHostToDevice));
    return add_device(c, nullptr, n_reads, c->c_off.p, c->c_ub.p, c->c_cnt.p, c->c_nh.p, t0, hash_off, hashes, c->h_nh.data(), out);
}
