// exclusive.hip -- hashes only one reference explains: per read, which of the references it reported holds hashes that none of the others
// on that read's list holds (`taxor search --exclusive-file` / `--exclusive-reads-file`).
//
// The object lives beside a resident index for a whole run.  It holds the leaf technical bins of every user bin as a CSR (coverage.hip's,
// hitmap.hip's, breakpoint.hip's and segments.hip's table, restated: those files stay as they are), two bounded staging buffers for hash
// lists, and per user bin four 64-bit sums and a HyperLogLog sketch of the hashes that were exclusive to it (coverage.hip's byte registers,
// restated).  A batch brings the searcher's device-resident CSR -- EVERY tuple that passed the search threshold -- and the batch's saved hash
// lists.  The CANDIDATES of a read are its tuples with count > 0, in CSR order; a read is EXAMINED when it has a hash and a candidate.
//
//   k_ex_count   one wave per read, tuples 64 at a time: M, the read's candidates.  A read without a hash leaves at once.  M goes to the
//                host, which decides who is examined, sums the candidates' offsets and cuts pieces.
//   k_ex_fill    the same walk over the examined reads; a ballot ranks the candidates of each 64, so tuple index, user bin and the range
//                of the user bin's leaf bins come out in CSR order.
//   k_ex_probe   one wave per PIECE -- at most EX_SPLIT consecutive hashes of one examined read.  64 hashes per round, one per lane; the
//                lane walks ALL M candidates (hits_c needs every lookup: there is no early exit) with the lookup of section 10.2, and
//                keeps two registers: how many candidates matched (0, 1, "2 or more") and the first that did.  Per candidate one lane
//                adds the popcount of the ballot to hits[c].  After the walk the lanes with exactly one match are combined by owner --
//                one ballot and one add to excl[owner] per DISTINCT owner of the round -- and each raises its hash's register in the
//                owner's user bin.  Lanes with two matches or more are ballot-counted into the read's `shared`, lanes with one or more
//                into `matched`; both are kept in registers over the piece and added once.
//   k_ex_tally   a launch of its own, so that a read's words are complete: one lane per candidate of an examined read adds the four
//                per-user-bin sums with 64-bit atomics and writes the candidate's count beside its hits and excl.
//
// The pieces of one read run in different waves.  Their per-read and per-candidate words are 32-bit integer atomic adds on zeroed words
// (as k_cov_accumulate adds its sums) and not per-piece partials summed afterwards: hits and excl ARE the result arrays, so partial words
// would be a second array of M words per PIECE and one more pass, for sums that are order-free either way.  Registers are a maximum.
// Nothing depends on the launch geometry nor on the cut into pieces and batches.  Every loop is bounded by a count the kernel is given
// (reads, a read's tuples, a piece's hashes, a read's candidates, a user bin's leaf bins) or by the 64 lanes of a wave and the
// CAS_ROUNDS of a register update.  No block waits on another.  There is no per-hash or per-round array: reads are not grouped.
#include "../../include/taxor_gpu_tools.h"
#include "device_prims.h"
#include "hip_host.h"
#include "hll.h"
#include "ixf_arith.h"
#include "kernels.h"
#include "saved_batch.h"

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

constexpr int EB = 256;                           // threads per block
constexpr int EW = EB / 64;                       // reads / pieces per block pass (one wave each)
constexpr int E_GRID_CAP = 4096;
constexpr uint32_t EX_SPLIT = 2048;               // hashes of one read per piece: a multiple of 64
constexpr uint64_t STAGE_HASHES = 1ull << 22;     // hashes per staging buffer (32 MiB); there are two
constexpr uint64_t STAGE_PIECES = 1ull << 18;     // pieces per staging buffer (3 MiB); there are two
constexpr uint64_t MAX_READS = 1ull << 31;
constexpr int CAS_ROUNDS = 256;                   // a swap fails only when a byte of the word rose: 4 bytes x at most 61 values

enum : uint32_t { EX_BAD_BIN = 1u, EX_MISCOUNT = 2u, EX_CAS_GAVE_UP = 4u };

struct Piece {
    uint32_t read;       // index in the batch
    uint32_t first;      // offset of the piece's first hash in the staging buffer
    uint32_t n;          // hashes, at most EX_SPLIT
};

struct LeafRange {
    uint64_t l0, l1;     // the candidate's user bin's leaf technical bins are leaf[l0 .. l1)
};

// a tuple is a candidate when its count is above 0; one that names a user bin outside the index is reported through err
__device__ __forceinline__ bool ex_candidate(const int64_t *__restrict__ ub, const uint32_t *__restrict__ count, uint64_t i, uint64_t hi, uint64_t t0,
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
__global__ __launch_bounds__(EB) void k_ex_count(const uint64_t *__restrict__ off, const int64_t *__restrict__ ub, const uint32_t *__restrict__ count, uint64_t t0,
                                                 const uint32_t *__restrict__ nh, uint64_t n_reads, uint64_t n_bins, uint32_t *__restrict__ n_cand,
                                                 uint32_t *__restrict__ err)
{
    bool bad = false;
    for (uint64_t r = (uint64_t)blockIdx.x * EW + (threadIdx.x >> 6); r < n_reads; r += (uint64_t)gridDim.x * EW) {
        uint32_t m = 0;
        if (nh[r] != 0) {
            const uint64_t lo = off[r], hi = off[r + 1];
            for (uint64_t base = lo; base < hi; base += 64) m += (uint32_t)__popcll(__ballot(ex_candidate(ub, count, base + lane_id(), hi, t0, n_bins, &bad)));
        }
        if (lane_id() == 0) n_cand[r] = m;
    }
    if (bad) atomicOr(err, EX_BAD_BIN);
}

// cand_off is the host's sum of the EXAMINED reads' counts: read r's candidates go to [cand_off[r], cand_off[r + 1]) in CSR order
__global__ __launch_bounds__(EB) void k_ex_fill(const uint64_t *__restrict__ off, const int64_t *__restrict__ ub, const uint32_t *__restrict__ count, uint64_t t0,
                                                uint64_t n_reads, uint64_t n_bins, const uint64_t *__restrict__ leaf_off, const uint64_t *__restrict__ cand_off,
                                                uint64_t *__restrict__ o_tuple, int64_t *__restrict__ o_ub, LeafRange *__restrict__ o_leaf, uint32_t *__restrict__ err)
{
    bool bad = false, miscount = false;
    for (uint64_t r = (uint64_t)blockIdx.x * EW + (threadIdx.x >> 6); r < n_reads; r += (uint64_t)gridDim.x * EW) {
        const uint64_t dst0 = cand_off[r], room = cand_off[r + 1] - dst0;
        if (room == 0) continue;
        const uint64_t lo = off[r], hi = off[r + 1];
        uint64_t written = 0;
        for (uint64_t base = lo; base < hi; base += 64) {
            const uint64_t i = base + lane_id();
            const bool k = ex_candidate(ub, count, i, hi, t0, n_bins, &bad);
            const uint64_t m = __ballot(k);
            const uint64_t at = written + (uint64_t)__popcll(m & ((1ull << lane_id()) - 1ull));
            if (k && at < room) {                         // never past the read's room: a walk that disagrees with the count is reported below
                const int64_t b = ub[i - t0];             // inside the index: ex_candidate said so
                o_tuple[dst0 + at] = i;
                o_ub[dst0 + at] = b;
                o_leaf[dst0 + at] = LeafRange{leaf_off[b], leaf_off[b + 1]};
            }
            written += (uint64_t)__popcll(m);
        }
        miscount = miscount || written != room;
    }
    if (bad) atomicOr(err, EX_BAD_BIN);
    if (miscount) atomicOr(err, EX_MISCOUNT);
}

// byte `lane4` of *word = max(that byte, rho): the load in front of the swap ends the update where the register is high enough already
__device__ __forceinline__ bool ex_register_max(uint32_t *word, uint32_t lane4, uint32_t rho)
{
    const uint32_t shift = lane4 * 8u;
    uint32_t cur = __atomic_load_n(word, __ATOMIC_RELAXED);
    for (int it = 0; it < CAS_ROUNDS; ++it) {
        if (((cur >> shift) & 0xFFu) >= rho) return true;
        const uint32_t want = (cur & ~(0xFFu << shift)) | (rho << shift);
        const uint32_t seen = atomicCAS(word, cur, want);
        if (seen == cur) return true;
        cur = seen;
    }
    return false;
}

struct ProbeArgs {
    const IxfDesc *ixf;
    const uint2 *leaf;            // (IXF, bin)
    const uint64_t *cand_off;     // [n_reads + 1]; an empty range: the read is not examined
    const int64_t *cand_ub;       // [n_cand] checked against n_bins by the count's walk
    const LeafRange *cand_leaf;   // [n_cand]
    uint32_t *hits, *excl;        // [n_cand] zeroed before the first piece
    uint32_t *matched, *shared;   // [n_reads] zeroed before the first piece
    const Piece *pieces;
    const uint64_t *hashes;       // the staged part of the saved lists
    uint32_t n_pieces;
    uint32_t precision;
    uint32_t *registers;          // n_bins << precision bytes, four to a word
    unsigned long long *lookups;
    uint32_t *err;
};

__global__ __launch_bounds__(EB) void k_ex_probe(ProbeArgs a)
{
    unsigned long long lookups = 0;
    bool gave_up = false;
    const uint32_t lane = lane_id();
    for (uint64_t pi = (uint64_t)blockIdx.x * EW + (threadIdx.x >> 6); pi < a.n_pieces; pi += (uint64_t)gridDim.x * EW) {
        const Piece pc = a.pieces[pi];
        const uint64_t c0 = a.cand_off[pc.read], c1 = a.cand_off[pc.read + 1];
        uint32_t p_matched = 0, p_shared = 0;                 // the same in every lane
        for (uint32_t h0 = 0; h0 < pc.n; h0 += 64) {
            const uint32_t j = h0 + lane;
            const bool active = j < pc.n;
            const uint64_t h = active ? a.hashes[(uint64_t)pc.first + j] : 0;
            uint32_t k = 0, owner = 0;                        // candidates that matched this lane's hash, 2 = two or more; the first of them
            for (uint64_t c = c0; c < c1; ++c) {
                const LeafRange lr = a.cand_leaf[c];          // the same in every lane
                bool matched = false;
                uint32_t cur_ixf = 0xFFFFFFFFu;
                IxfDesc d{};
                ixf_probe p{};
                for (uint64_t l = lr.l0; l < lr.l1; ++l) {
                    const uint2 lf = a.leaf[l];
                    if (lf.x != cur_ixf) {                    // a split user bin's parts stand side by side in one IXF: one probe
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
                if (lane == 0 && m) atomicAdd(a.hits + c, (uint32_t)__popcll(m));
                if (matched) {
                    if (k == 0) owner = (uint32_t)(c - c0);
                    k = k < 2u ? k + 1u : 2u;
                }
            }
            p_matched += (uint32_t)__popcll(__ballot(k >= 1u));
            p_shared += (uint32_t)__popcll(__ballot(k >= 2u));
            const bool mine = k == 1u;
            // lanes of the round with the same owner are combined: one add per distinct owner, at most 64 of them
            uint64_t rest = __ballot(mine);
            for (int it = 0; it < 64 && rest; ++it) {
                const int src = __ffsll((long long)rest) - 1;
                const uint32_t o = __shfl(owner, src);
                const uint64_t same = __ballot(mine && owner == o);
                if ((int)lane == src) atomicAdd(a.excl + c0 + o, (uint32_t)__popcll(same));
                rest &= ~same;
            }
            if (mine) {
                const uint64_t b = (uint64_t)a.cand_ub[c0 + owner];
                const hll_slot_t s = hll_slot(h, a.precision);
                const uint64_t at = (b << a.precision) + s.index;
                if (!ex_register_max(a.registers + (at >> 2), (uint32_t)(at & 3u), s.rho)) gave_up = true;
            }
        }
        if (lane == 0) {
            if (p_matched) atomicAdd(a.matched + pc.read, p_matched);
            if (p_shared) atomicAdd(a.shared + pc.read, p_shared);
        }
    }
    if (gave_up) atomicOr(a.err, EX_CAS_GAVE_UP);
    const unsigned long long wave_lookups = wave_incl_add(lookups);     // one atomic per wave
    if (lane == 63 && wave_lookups) atomicAdd(a.lookups, wave_lookups);
}

// one lane per candidate of an examined read; sums[4 * n_bins]: cand_reads | hits | exclusive_hits | exclusive_reads
__global__ __launch_bounds__(EB) void k_ex_tally(uint64_t n_cand, const uint64_t *__restrict__ cand_tuple, const int64_t *__restrict__ cand_ub,
                                                 const uint32_t *__restrict__ count, uint64_t t0, const uint32_t *__restrict__ hits, const uint32_t *__restrict__ excl,
                                                 uint32_t *__restrict__ cand_count, uint64_t n_bins, unsigned long long *__restrict__ sums)
{
    for (uint64_t g = (uint64_t)blockIdx.x * EB + threadIdx.x; g < n_cand; g += (uint64_t)gridDim.x * EB) {
        const uint64_t b = (uint64_t)cand_ub[g];
        const uint32_t hc = hits[g], ec = excl[g];
        cand_count[g] = count[cand_tuple[g] - t0];
        atomicAdd(sums + b, 1ull);
        if (hc) atomicAdd(sums + n_bins + b, (unsigned long long)hc);
        if (ec) {
            atomicAdd(sums + 2 * n_bins + b, (unsigned long long)ec);
            atomicAdd(sums + 3 * n_bins + b, 1ull);
        }
    }
}

#define EX_TRY(expr) TAXOR_HIP_TRY_PREFIX("exclusive", expr, #expr)

// the results of one caller (a searcher, or add_csr): device words and work arrays, and their page-locked copies
struct Slot {
    DeviceBuf<uint32_t> d_r32, d_n_cand, d_c32;         // d_r32: matched | shared, cap each; d_c32: hits | excl | count, cap_c each
    DeviceBuf<uint64_t> d_cand_off, d_cand_tuple;
    DeviceBuf<int64_t> d_cand_ub;
    DeviceBuf<LeafRange> d_cand_leaf;
    uint32_t *h_r32 = nullptr;     // matched | shared | n_candidates | n | n_hashes, cap each
    uint64_t *h_cand_off = nullptr;
    uint8_t *h_examined = nullptr;
    uint64_t *h_c64 = nullptr;     // tuple | user bin, cap_c each
    uint32_t *h_c32 = nullptr;     // hits | excl | count, cap_c each
    uint64_t cap = 0, cap_c = 0;
    void drop_reads()
    {
        if (h_r32) (void)hipHostFree(h_r32);
        if (h_cand_off) (void)hipHostFree(h_cand_off);
        if (h_examined) (void)hipHostFree(h_examined);
        h_r32 = nullptr;
        h_cand_off = nullptr;
        h_examined = nullptr;
        cap = 0;
    }
    void drop_cands()
    {
        if (h_c64) (void)hipHostFree(h_c64);
        if (h_c32) (void)hipHostFree(h_c32);
        h_c64 = nullptr;
        h_c32 = nullptr;
        cap_c = 0;
    }
    ~Slot()
    {
        drop_reads();
        drop_cands();
    }
};

}   // namespace

struct taxor_gpu_exclusive {
    taxor_gpu_index *idx = nullptr;
    int device = 0;
    uint32_t precision = 0;
    uint64_t n_bins = 0;
    const IxfDesc *d_ixf = nullptr;
    hipStream_t st = nullptr;
    std::mutex mu;                                    // batches may come from several threads
    DeviceBuf<uint64_t> d_leaf_off, d_hashes[2];
    DeviceBuf<uint2> d_leaf;
    DeviceBuf<Piece> d_pieces[2];
    DeviceBuf<uint32_t> d_registers, d_err;
    DeviceBuf<unsigned long long> d_sums, d_lookups;  // d_sums: cand_reads | hits | exclusive_hits | exclusive_reads
    Piece *h_pieces[2] = {nullptr, nullptr};          // page-locked; ev_free[i] says that buffer i's copy has left it
    hipEvent_t ev_free[2] = {nullptr, nullptr};
    bool ev_used[2] = {false, false};
    std::vector<hipEvent_t> ev_time;                  // pairs around the kernel launches of one call
    std::vector<uint32_t> h_nh;
    std::map<const void *, std::unique_ptr<Slot>> slots;
    double seconds_kernels = 0;
    uint64_t probes = 0;
    // host arrays of add_csr on the device
    DeviceBuf<uint64_t> c_off;
    DeviceBuf<int64_t> c_ub;
    DeviceBuf<uint32_t> c_cnt, c_nh;
    // _results
    std::vector<uint64_t> r_sums;
    std::vector<uint8_t> r_registers;
    ~taxor_gpu_exclusive()
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
int add_device(taxor_gpu_exclusive *c, const void *who, uint64_t n, const uint64_t *d_off, const int64_t *d_ub, const uint32_t *d_cnt, const uint32_t *d_nh,
               uint64_t t0, const uint64_t *hash_off, const uint64_t *hashes, const uint32_t *h_nh, taxor_exclusive_batch *out)
{
    std::unique_ptr<Slot> &sp = c->slots[who];
    if (!sp) sp = std::make_unique<Slot>();
    Slot &sl = *sp;
    if (n > sl.cap || !sl.h_cand_off) {                // an empty first batch still gets its cand_off[0]
        const uint64_t want = std::max<uint64_t>(n + n / 2, 1024);
        sl.drop_reads();
        EX_TRY(sl.d_r32.alloc(2 * want));
        EX_TRY(sl.d_n_cand.alloc(want));
        EX_TRY(sl.d_cand_off.alloc(want + 1));
        EX_TRY(hipHostMalloc((void **)&sl.h_r32, 5 * want * sizeof(uint32_t), hipHostMallocDefault));
        EX_TRY(hipHostMalloc((void **)&sl.h_cand_off, (want + 1) * sizeof(uint64_t), hipHostMallocDefault));
        EX_TRY(hipHostMalloc((void **)&sl.h_examined, want, hipHostMallocDefault));
        sl.cap = want;
    }
    uint32_t *h_matched = sl.h_r32, *h_shared = h_matched + n, *h_m = h_shared + n, *h_n = h_m + n, *h_hashes = h_n + n;
    memset(out, 0, sizeof *out);
    out->n_reads = n;
    out->precision = c->precision;
    out->examined = sl.h_examined;
    out->n_candidates = h_m;
    out->n = h_n;
    out->matched = h_matched;
    out->shared = h_shared;
    out->n_hashes = h_hashes;
    out->cand_off = sl.h_cand_off;
    sl.h_cand_off[0] = 0;
    if (c->ev_used[0] || c->ev_used[1]) {              // a call that failed half-way: its copies out of the page-locked pieces end first
        EX_TRY(hipStreamSynchronize(c->st));
        c->ev_used[0] = c->ev_used[1] = false;
    }
    if (n == 0) return TAXOR_OK;

    size_t n_ev = 0;
    auto stamp = [&]() -> int {                        // an event on the stream: launches are timed between pairs of them
        if (c->ev_time.size() <= n_ev) {
            hipEvent_t e = nullptr;
            EX_TRY(hipEventCreate(&e));
            c->ev_time.push_back(e);
        }
        EX_TRY(hipEventRecord(c->ev_time[n_ev++], c->st));
        return TAXOR_OK;
    };

    // the words of a read that is not examined are 0
    EX_TRY(hipMemsetAsync(sl.d_r32.p, 0, 2 * n * sizeof(uint32_t), c->st));
    EX_TRY(hipMemsetAsync(c->d_lookups.p, 0, 8, c->st));
    if (int rc = stamp()) return rc;
    k_ex_count<<<grid_for(n, EW, E_GRID_CAP), EB, 0, c->st>>>(d_off, d_ub, d_cnt, t0, d_nh, n, c->n_bins, sl.d_n_cand.p, c->d_err.p);
    EX_TRY(hipGetLastError());
    if (int rc = stamp()) return rc;
    uint32_t err = 0;
    EX_TRY(hipMemcpyAsync(h_m, sl.d_n_cand.p, n * sizeof(uint32_t), hipMemcpyDeviceToHost, c->st));
    EX_TRY(hipMemcpyAsync(&err, c->d_err.p, 4, hipMemcpyDeviceToHost, c->st));
    EX_TRY(hipStreamSynchronize(c->st));
    if (err & EX_BAD_BIN) {
        EX_TRY(hipMemset(c->d_err.p, 0, 4));
        return fail(TAXOR_E_INTERNAL, "exclusive_add: user_bin: a tuple names a user bin outside the index's %llu", (unsigned long long)c->n_bins);
    }
    // who is examined (M counts nothing for a read without a hash) and the candidates' offsets
    uint64_t *cand_off = sl.h_cand_off;
    uint64_t n_cand = 0, n_examined = 0;
    for (uint64_t r = 0; r < n; ++r) {
        cand_off[r] = n_cand;
        const bool ex = h_nh[r] != 0 && h_m[r] >= 1;
        sl.h_examined[r] = ex ? 1 : 0;
        h_n[r] = ex ? h_nh[r] : 0;
        if (!ex) continue;
        ++n_examined;
        n_cand += h_m[r];
    }
    cand_off[n] = n_cand;
    out->n_examined = n_examined;
    out->n_cand = n_cand;
    memcpy(h_hashes, h_nh, n * sizeof(uint32_t));
    if (n_cand > sl.cap_c) {
        const uint64_t want = std::max<uint64_t>(n_cand + n_cand / 2, 1024);
        sl.drop_cands();
        EX_TRY(sl.d_c32.alloc(3 * want));
        EX_TRY(sl.d_cand_tuple.alloc(want));
        EX_TRY(sl.d_cand_ub.alloc(want));
        EX_TRY(sl.d_cand_leaf.alloc(want));
        EX_TRY(hipHostMalloc((void **)&sl.h_c64, 2 * want * sizeof(uint64_t), hipHostMallocDefault));
        EX_TRY(hipHostMalloc((void **)&sl.h_c32, 3 * want * sizeof(uint32_t), hipHostMallocDefault));
        sl.cap_c = want;
    }
    unsigned long long lookups = 0;
    if (n_examined) {
        uint32_t *d_hits = sl.d_c32.p, *d_excl = d_hits + n_cand, *d_count = d_excl + n_cand;
        EX_TRY(hipMemsetAsync(d_hits, 0, 2 * n_cand * sizeof(uint32_t), c->st));
        EX_TRY(hipMemcpyAsync(sl.d_cand_off.p, cand_off, (n + 1) * 8, hipMemcpyHostToDevice, c->st));
        if (int rc = stamp()) return rc;
        k_ex_fill<<<grid_for(n, EW, E_GRID_CAP), EB, 0, c->st>>>(d_off, d_ub, d_cnt, t0, n, c->n_bins, c->d_leaf_off.p, sl.d_cand_off.p, sl.d_cand_tuple.p, sl.d_cand_ub.p,
                                                                 sl.d_cand_leaf.p, c->d_err.p);
        EX_TRY(hipGetLastError());
        if (int rc = stamp()) return rc;

        ProbeArgs a{};
        a.ixf = c->d_ixf;
        a.leaf = c->d_leaf.p;
        a.cand_off = sl.d_cand_off.p;
        a.cand_ub = sl.d_cand_ub.p;
        a.cand_leaf = sl.d_cand_leaf.p;
        a.hits = d_hits;
        a.excl = d_excl;
        a.matched = sl.d_r32.p;
        a.shared = sl.d_r32.p + n;
        a.precision = c->precision;
        a.registers = c->d_registers.p;
        a.lookups = c->d_lookups.p;
        a.err = c->d_err.p;
        // Pieces are staged and launched in bounded sets (hitmap.hip's scheme): at most STAGE_PIECES pieces whose hashes lie within
        // STAGE_HASHES consecutive entries of the dense host array, copied as one range
        int buf = 0;
        uint32_t n_p = 0;
        uint64_t g0 = 0, g1 = 0;            // the set's hashes: [g0, g1) of hashes
        auto flush = [&]() -> int {
            if (n_p == 0) return TAXOR_OK;
            EX_TRY(hipMemcpyAsync(c->d_hashes[buf].p, hashes + g0, (g1 - g0) * 8, hipMemcpyHostToDevice, c->st));
            EX_TRY(hipMemcpyAsync(c->d_pieces[buf].p, c->h_pieces[buf], (uint64_t)n_p * sizeof(Piece), hipMemcpyHostToDevice, c->st));
            EX_TRY(hipEventRecord(c->ev_free[buf], c->st));
            c->ev_used[buf] = true;
            a.pieces = c->d_pieces[buf].p;
            a.hashes = c->d_hashes[buf].p;
            a.n_pieces = n_p;
            if (int rc = stamp()) return rc;
            k_ex_probe<<<grid_for(n_p, EW, E_GRID_CAP), EB, 0, c->st>>>(a);
            EX_TRY(hipGetLastError());
            if (int rc = stamp()) return rc;
            buf ^= 1;
            n_p = 0;
            if (c->ev_used[buf]) EX_TRY(hipEventSynchronize(c->ev_free[buf]));     // the page-locked pieces of two sets ago have been copied
            return TAXOR_OK;
        };
        for (uint64_t r = 0; r < n; ++r) {
            if (!sl.h_examined[r]) continue;
            const uint64_t h0 = hash_off[r], nh = h_nh[r];
            for (uint64_t done = 0; done < nh;) {
                const uint32_t take = (uint32_t)std::min<uint64_t>(EX_SPLIT, nh - done);
                if (n_p && (n_p == STAGE_PIECES || h0 + done + take - g0 > STAGE_HASHES))
                    if (int rc = flush()) return rc;
                if (n_p == 0) g0 = h0 + done;
                c->h_pieces[buf][n_p++] = Piece{(uint32_t)r, (uint32_t)(h0 + done - g0), take};
                done += take;
                g1 = h0 + done;
            }
        }
        if (int rc = flush()) return rc;
        if (int rc = stamp()) return rc;
        k_ex_tally<<<grid_for(n_cand, EB, E_GRID_CAP), EB, 0, c->st>>>(n_cand, sl.d_cand_tuple.p, sl.d_cand_ub.p, d_cnt, t0, d_hits, d_excl, d_count, c->n_bins, c->d_sums.p);
        EX_TRY(hipGetLastError());
        if (int rc = stamp()) return rc;
        EX_TRY(hipMemcpyAsync(sl.h_c64, sl.d_cand_tuple.p, n_cand * 8, hipMemcpyDeviceToHost, c->st));
        EX_TRY(hipMemcpyAsync(sl.h_c64 + n_cand, sl.d_cand_ub.p, n_cand * 8, hipMemcpyDeviceToHost, c->st));
        EX_TRY(hipMemcpyAsync(sl.h_c32, sl.d_c32.p, 3 * n_cand * sizeof(uint32_t), hipMemcpyDeviceToHost, c->st));
        out->cand_tuple = sl.h_c64;
        out->cand_bin = (const int64_t *)(sl.h_c64 + n_cand);
        out->cand_hits = sl.h_c32;
        out->cand_excl = sl.h_c32 + n_cand;
        out->cand_count = sl.h_c32 + 2 * n_cand;
    }
    EX_TRY(hipMemcpyAsync(h_matched, sl.d_r32.p, 2 * n * sizeof(uint32_t), hipMemcpyDeviceToHost, c->st));
    EX_TRY(hipMemcpyAsync(&lookups, c->d_lookups.p, 8, hipMemcpyDeviceToHost, c->st));
    EX_TRY(hipMemcpyAsync(&err, c->d_err.p, 4, hipMemcpyDeviceToHost, c->st));
    EX_TRY(hipStreamSynchronize(c->st));               // the searcher's buffers and the hash lists are the caller's again
    c->ev_used[0] = c->ev_used[1] = false;
    for (size_t i = 0; i + 1 < n_ev; i += 2) {
        float ms = 0;
        EX_TRY(hipEventElapsedTime(&ms, c->ev_time[i], c->ev_time[i + 1]));
        out->seconds_kernels += (double)ms * 1e-3;
    }
    out->probes = lookups;
    c->seconds_kernels += out->seconds_kernels;
    c->probes += lookups;
    if (err) {
        EX_TRY(hipMemset(c->d_err.p, 0, 4));
        if (err & EX_CAS_GAVE_UP) return fail(TAXOR_E_INTERNAL, "exclusive_add: registers: a register update did not complete in %d rounds", CAS_ROUNDS);
        // the CSR changed under the call: the second walk did not find what the first counted
        return fail(TAXOR_E_INTERNAL, "exclusive_add: candidates: the walk that writes the candidates disagrees with the walk that counted them (flags %u)", err);
    }
    return TAXOR_OK;
}

}   // namespace

extern "C" int taxor_gpu_exclusive_create(taxor_gpu_index *idx, const taxor_hixf_view *view, uint32_t precision, taxor_gpu_exclusive **out)
{
    if (!out) return fail(TAXOR_E_ARG, "exclusive_create: null argument");
    *out = nullptr;
    if (!idx || !view) return fail(TAXOR_E_ARG, "exclusive_create: null argument");
    if (precision == 0) precision = HLL_DEFAULT_PRECISION;
    if (precision < HLL_MIN_PRECISION || precision > HLL_MAX_PRECISION)
        return fail(TAXOR_E_ARG, "exclusive_create: precision %u is not in [%u, %u] (0 = %u)", precision, HLL_MIN_PRECISION, HLL_MAX_PRECISION, HLL_DEFAULT_PRECISION);
    const IxfDesc *d_ixf = nullptr, *h_ixf = nullptr;
    uint64_t n_ixf = 0, n_bins = 0;
    uint32_t n_passes = 0;
    int device = 0;
    if (taxor_index_descs(idx, &d_ixf, &h_ixf, &n_ixf, &n_bins, &n_passes, &device)) return fail(TAXOR_E_ARG, "exclusive_create: null index");
    if (n_passes)
        return fail(TAXOR_E_ARG, "exclusive_create: a paged index (%u resident pass%s) is refused: its leaf bins are not all resident at once and a read's final tuples exist only after the last pass's merge; counting exclusive hashes pass by pass is not built",
                    n_passes, n_passes == 1 ? "" : "es");
    if (view->n_ixf != n_ixf || view->n_user_bins != n_bins || (n_ixf && !view->ixf))
        return fail(TAXOR_E_ARG, "exclusive_create: the view (%llu IXFs, %llu user bins) is not the index's (%llu IXFs, %llu user bins)", (unsigned long long)view->n_ixf,
                    (unsigned long long)view->n_user_bins, (unsigned long long)n_ixf, (unsigned long long)n_bins);
    if (n_bins >= (1ull << 32) || n_ixf >= (1ull << 32)) return fail(TAXOR_E_ARG, "exclusive_create: user bins and IXFs are numbered in 32 bits");
    // the inverse of fname_idx: every leaf technical bin of a user bin, root included, as one CSR in index order (the set and the order
    // of the other consumers' tables, restated once more: those files, and their objects, stay as they are)
    std::vector<uint64_t> leaf_off(n_bins + 1, 0);
    for (uint64_t x = 0; x < n_ixf; ++x) {
        const taxor_ixf_view &f = view->ixf[x];
        if (f.bins != h_ixf[x].bins) return fail(TAXOR_E_ARG, "exclusive_create: IXF %llu has %llu bins in the view, %u in the index", (unsigned long long)x, (unsigned long long)f.bins, h_ixf[x].bins);
        if (!f.fname_idx) return fail(TAXOR_E_ARG, "exclusive_create: IXF %llu of the view has no fname_idx", (unsigned long long)x);
        for (uint64_t j = 0; j < f.bins; ++j) {
            const int64_t b = f.fname_idx[j];
            if (b < 0) continue;
            if ((uint64_t)b >= n_bins) return fail(TAXOR_E_ARG, "exclusive_create: bin %llu of IXF %llu names user bin %lld of %llu", (unsigned long long)j, (unsigned long long)x, (long long)b, (unsigned long long)n_bins);
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
    EX_TRY(hipSetDevice(device));
    // what the object allocates at once, held against the device's free memory first
    const uint64_t reg_bytes = ((n_bins << precision) + 3) / 4 * 4;
    const uint64_t need = reg_bytes + (4 * n_bins + 1) * 8 + (n_bins + 1) * 8 + leaf.size() * 8 + 2 * (STAGE_HASHES * 8 + STAGE_PIECES * sizeof(Piece)) + 12;
    size_t fr = 0, tot = 0;
    EX_TRY(hipMemGetInfo(&fr, &tot));
    if (need > fr)
        return fail(TAXOR_E_NOMEM, "exclusive_create: the sketches of %llu user bins at precision %u need %llu bytes on the device (%llu of them registers), %llu are free; a smaller --exclusive-precision quarters the registers per two steps",
                    (unsigned long long)n_bins, precision, (unsigned long long)need, (unsigned long long)reg_bytes, (unsigned long long)fr);
    auto c = std::make_unique<taxor_gpu_exclusive>();
    c->idx = idx;
    c->device = device;
    c->precision = precision;
    c->n_bins = n_bins;
    c->d_ixf = d_ixf;
    EX_TRY(hipStreamCreate(&c->st));
    EX_TRY(c->d_leaf_off.alloc(n_bins + 1));
    EX_TRY(c->d_leaf.alloc(leaf.size() + 1));
    EX_TRY(c->d_registers.alloc(reg_bytes / 4 + 1));
    EX_TRY(c->d_sums.alloc(4 * n_bins + 1));
    EX_TRY(c->d_err.alloc(1));
    EX_TRY(c->d_lookups.alloc(1));
    for (int i = 0; i < 2; ++i) {
        EX_TRY(c->d_hashes[i].alloc(STAGE_HASHES));
        EX_TRY(c->d_pieces[i].alloc(STAGE_PIECES));
        EX_TRY(hipHostMalloc((void **)&c->h_pieces[i], STAGE_PIECES * sizeof(Piece), hipHostMallocDefault));
        EX_TRY(hipEventCreateWithFlags(&c->ev_free[i], hipEventDisableTiming));
    }
    EX_TRY(hipMemcpy(c->d_leaf_off.p, leaf_off.data(), (n_bins + 1) * 8, hipMemcpyHostToDevice));
    if (!leaf.empty()) EX_TRY(hipMemcpy(c->d_leaf.p, leaf.data(), leaf.size() * 8, hipMemcpyHostToDevice));
    EX_TRY(hipMemset(c->d_registers.p, 0, (reg_bytes / 4 + 1) * 4));
    EX_TRY(hipMemset(c->d_sums.p, 0, (4 * n_bins + 1) * 8));
    EX_TRY(hipMemset(c->d_err.p, 0, 4));
    *out = c.release();
    return TAXOR_OK;
}

extern "C" void taxor_gpu_exclusive_destroy(taxor_gpu_exclusive *c)
{
    if (!c) return;
    (void)hipSetDevice(c->device);
    delete c;
}

extern "C" int taxor_gpu_exclusive_add_batch(taxor_gpu_exclusive *c, taxor_gpu_searcher *s, const taxor_gpu_saved *saved, taxor_exclusive_batch *out)
{
    if (!c || !s || !out) return fail(TAXOR_E_ARG, "exclusive_add_batch: null argument");
    if (!saved) return fail(TAXOR_E_ARG, "exclusive_add_batch: saved: no saved batch (the batch ran with capture off, or its lists were not taken)");
    if (taxor_searcher_index(s) != c->idx) return fail(TAXOR_E_ARG, "exclusive_add_batch: index: the searcher works on another index than the exclusive object");
    const std::string unsound = saved_validate(*saved);
    if (!unsound.empty()) return fail(TAXOR_E_ARG, "exclusive_add_batch: " + unsound);
    const uint64_t *d_off = nullptr;
    const int64_t *d_ub = nullptr;
    const uint32_t *d_cnt = nullptr, *d_nh = nullptr;
    uint64_t n = 0, nt = 0;
    int dev = 0;
    if (int rc = taxor_searcher_device_results(s, &d_off, &d_ub, &d_cnt, &d_nh, &n, &nt, &dev)) return rc;
    if (saved->n_reads != n)
        return fail(TAXOR_E_ARG, "exclusive_add_batch: n_reads: the saved batch holds %llu reads, the searcher's last batch %llu", (unsigned long long)saved->n_reads, (unsigned long long)n);
    if (n >= MAX_READS) return fail(TAXOR_E_ARG, "exclusive_add_batch: n_reads: a batch of 2^31 reads or more");
    std::lock_guard<std::mutex> lk(c->mu);
    EX_TRY(hipSetDevice(c->device));
    c->h_nh.resize(n);
    if (n) EX_TRY(hipMemcpy(c->h_nh.data(), d_nh, n * 4, hipMemcpyDeviceToHost));
    for (uint64_t r = 0; r < n; ++r)
        if (c->h_nh[r] != saved->n_hashes[r])
            return fail(TAXOR_E_ARG, "exclusive_add_batch: n_hashes: read %llu has %u hashes in the saved batch, %u in the searcher's last batch", (unsigned long long)r, saved->n_hashes[r], c->h_nh[r]);
    return add_device(c, s, n, d_off, d_ub, d_cnt, d_nh, 0, saved->hash_off.data(), saved->hashes, c->h_nh.data(), out);
}

extern "C" int taxor_gpu_exclusive_add_csr(taxor_gpu_exclusive *c, uint64_t n_reads, const uint64_t *read_off, const int64_t *user_bin, const uint32_t *count,
                                           const uint64_t *hash_off, const uint64_t *hashes, taxor_exclusive_batch *out)
{
    if (!c || !read_off || !hash_off || !out) return fail(TAXOR_E_ARG, "exclusive_add_csr: null argument");
    if (n_reads >= MAX_READS) return fail(TAXOR_E_ARG, "exclusive_add_csr: n_reads: 2^31 reads or more");
    for (uint64_t r = 0; r < n_reads; ++r) {
        if (read_off[r + 1] < read_off[r] || read_off[r + 1] - read_off[r] >= (1ull << 32))
            return fail(TAXOR_E_ARG, "exclusive_add_csr: read_off: the tuples of read %llu are malformed", (unsigned long long)r);
        if (hash_off[r + 1] < hash_off[r] || hash_off[r + 1] - hash_off[r] >= (1ull << 32))
            return fail(TAXOR_E_ARG, "exclusive_add_csr: hash_off: the list of read %llu is malformed", (unsigned long long)r);
    }
    const uint64_t t0 = read_off[0], nt = read_off[n_reads] - t0;
    if (nt && (!user_bin || !count)) return fail(TAXOR_E_ARG, "exclusive_add_csr: user_bin / count: null array");
    if (hash_off[n_reads] > hash_off[0] && !hashes) return fail(TAXOR_E_ARG, "exclusive_add_csr: hashes: null array");
    for (uint64_t i = t0; i < t0 + nt; ++i)
        if (user_bin[i] < 0 || (uint64_t)user_bin[i] >= c->n_bins)
            return fail(TAXOR_E_ARG, "exclusive_add_csr: user_bin: tuple %llu names user bin %lld, the index has %llu", (unsigned long long)i, (long long)user_bin[i], (unsigned long long)c->n_bins);
    std::lock_guard<std::mutex> lk(c->mu);
    EX_TRY(hipSetDevice(c->device));
    c->h_nh.resize(n_reads);
    for (uint64_t r = 0; r < n_reads; ++r) c->h_nh[r] = (uint32_t)(hash_off[r + 1] - hash_off[r]);
    EX_TRY(c->c_off.reserve(n_reads + 1, n_reads + 1 + n_reads / 2));
    EX_TRY(c->c_nh.reserve(n_reads + 1, n_reads + 1 + n_reads / 2));
    EX_TRY(c->c_ub.reserve(nt + 1, nt + 1 + nt / 2));
    EX_TRY(c->c_cnt.reserve(nt + 1, nt + 1 + nt / 2));
    EX_TRY(hipMemcpy(c->c_off.p, read_off, (n_reads + 1) * 8, hipMemcpyHostToDevice));
    if (nt) {
        EX_TRY(hipMemcpy(c->c_ub.p, user_bin + t0, nt * 8, hipMemcpyHostToDevice));
        EX_TRY(hipMemcpy(c->c_cnt.p, count + t0, nt * 4, hipMemcpyHostToDevice));
    }
    if (n_reads) EX_TRY(hipMemcpy(c->c_nh.p, c->h_nh.data(), n_reads * 4, hipMemcpyHostToDevice));
    return add_device(c, nullptr, n_reads, c->c_off.p, c->c_ub.p, c->c_cnt.p, c->c_nh.p, t0, hash_off, hashes, c->h_nh.data(), out);
}

extern "C" int taxor_gpu_exclusive_results(taxor_gpu_exclusive *c, taxor_exclusive_results *out)
{
    if (!c || !out) return fail(TAXOR_E_ARG, "exclusive_results: null argument");
    std::lock_guard<std::mutex> lk(c->mu);
    EX_TRY(hipSetDevice(c->device));
    const uint64_t nb = c->n_bins, reg_bytes = nb << c->precision;
    c->r_sums.resize(4 * nb);
    c->r_registers.resize(reg_bytes);
    if (nb) {
        EX_TRY(hipMemcpy(c->r_sums.data(), c->d_sums.p, 4 * nb * 8, hipMemcpyDeviceToHost));
        EX_TRY(hipMemcpy(c->r_registers.data(), c->d_registers.p, reg_bytes, hipMemcpyDeviceToHost));
    }
    out->n_user_bins = nb;
    out->precision = c->precision;
    out->reserved = 0;
    out->cand_reads = c->r_sums.data();
    out->hits = c->r_sums.data() + nb;
    out->exclusive_hits = c->r_sums.data() + 2 * nb;
    out->exclusive_reads = c->r_sums.data() + 3 * nb;
    out->registers = c->r_registers.data();
    out->seconds_kernels = c->seconds_kernels;
    out->probes = c->probes;
    return TAXOR_OK;
}
