// coverage.hip -- distinct matched hashes per reference (`taxor search --coverage-file`; DESIGN.md section 10, "Distinct-hash coverage").
//
// An accumulator lives beside a resident index for a whole run.  Per user bin it keeps the number of reads that reported the bin
// (tuples that survive the search's output filter, taxor_search.cpp:275-286), the sum of their counts, and a HyperLogLog sketch of
// the DISTINCT query hashes that matched the bin.  A batch brings two things: the searcher's device-resident CSR (the buffers
// taxor_gpu_batch_export_device copies from, read where they lie) and the batch's saved hash lists (taxor_gpu_search_take_saved),
// staged to the device through two bounded buffers.
//
//   k_cov_accumulate   one wave per PIECE -- at most COV_SPLIT hashes of one read, cut on the host from the saved counts, so that a
//                      1-Mb read is a hundred waves and not one wave's loop.  The wave finds the read's max count and walks its
//                      tuples 64 at a time; for every surviving tuple (user bin b) it takes the piece's hashes 64 at a time, one per
//                      lane: the probe (three rows, fingerprint) once per IXF among b's leaf bins, three one-byte gathers per leaf
//                      bin at data[row * stride + bin], and for a hash that matched in any of them one register update.  The read's
//                      first piece also adds the tuple to reads[b] and hash_matches[b].
//
// Registers are bytes, four to a 32-bit word, raised by a compare-and-swap on the word: a quarter of the memory of a word per register
// (4 KiB per user bin at P = 12: 113 MB for 27 473 user bins, 410 MB for 100 000), and the load in front of the swap ends the update
// where the register is high enough already -- after the first reads of a reference that is nearly every update.  max is order-free:
// the registers do not depend on the launch geometry, the order of the batches or the cut into pieces.  No block waits on another.
#include "../../include/taxor_gpu_tools.h"
#include "device_prims.h"
#include "hip_host.h"
#include "hll.h"
#include "ixf_arith.h"
#include "kernels.h"
#include "saved_batch.h"

#include <hip/hip_runtime.h>

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

constexpr int CB = 256;                           // threads per block
constexpr int CW = CB / 64;                       // pieces per block pass (one wave each)
constexpr int C_GRID_CAP = 4096;
constexpr uint32_t COV_SPLIT = 2048;              // hashes of one read per piece
constexpr uint64_t STAGE_HASHES = 1ull << 22;     // hashes per staging buffer (32 MiB); there are two
constexpr uint64_t STAGE_PIECES = 1ull << 18;     // pieces per staging buffer (4 MiB); there are two
constexpr int CAS_ROUNDS = 256;                   // a swap fails only when a byte of the word rose: 4 bytes x at most 61 values

enum : uint32_t { COV_BAD_BIN = 1u, COV_CAS_GAVE_UP = 2u };

struct Piece {
    uint32_t read;       // index in the batch
    uint32_t first;      // offset of the piece's first hash in the staging buffer
    uint32_t n;          // hashes, at most COV_SPLIT
    uint32_t head;       // 1: the read's first piece -- it counts the read's tuples
};

struct CovArgs {
    const IxfDesc *ixf;
    const uint64_t *leaf_off;     // [n_bins + 1] user bin b's leaf technical bins are leaf[leaf_off[b] .. leaf_off[b + 1])
    const uint2 *leaf;            // (IXF, bin)
    const uint64_t *off;          // the searcher's CSR
    const int64_t *ub;
    const uint32_t *count;
    const Piece *pieces;
    const uint64_t *hashes;       // the staged part of the saved lists
    uint32_t n_pieces;
    uint32_t precision;
    uint64_t n_bins;
    uint32_t *registers;          // n_bins << precision bytes, four to a word
    unsigned long long *reads, *hash_matches, *probes;
    uint32_t *err;
};

// taxor_search.cpp:285, evaluated as written (profile_feed.hip's ff_keeps without its keep-all switch)
__device__ __forceinline__ bool cov_keeps(uint32_t c, uint32_t mx) { return !((double)c < (double)mx * 0.8); }

// byte `lane4` of *word = max(that byte, rho)
__device__ __forceinline__ bool register_max(uint32_t *word, uint32_t lane4, uint32_t rho)
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

// the piece's hashes against user bin b's leaf bins; returns the lookups this lane made
__device__ __forceinline__ uint32_t cov_bin(const CovArgs &a, const Piece &pc, uint64_t b, bool *gave_up)
{
    const uint64_t l0 = a.leaf_off[b], l1 = a.leaf_off[b + 1];
    uint32_t lookups = 0;
    for (uint32_t h0 = 0; h0 < pc.n; h0 += 64) {
        const uint32_t j = h0 + lane_id();
        const bool active = j < pc.n;
        const uint64_t h = active ? a.hashes[(uint64_t)pc.first + j] : 0;
        bool matched = false;
        uint32_t cur_ixf = 0xFFFFFFFFu;
        IxfDesc d{};
        ixf_probe p{};
        for (uint64_t l = l0; l < l1; ++l) {
            const uint2 lf = a.leaf[l];                       // the same in every lane
            if (lf.x != cur_ixf) {                            // a split user bin's parts stand side by side in one IXF: one probe
                cur_ixf = lf.x;
                d = a.ixf[lf.x];
                p = ixf_probe_key_arith(h, d.seed, d.seg_len, d.arith);
            }
            if (active) {
                const uint8_t f = d.data[(uint64_t)p.row[0] * d.stride + lf.y] ^ d.data[(uint64_t)p.row[1] * d.stride + lf.y] ^
                                  d.data[(uint64_t)p.row[2] * d.stride + lf.y];
                matched |= f == (uint8_t)(p.fp4 & 0xFFu);
                ++lookups;
            }
        }
        if (matched) {
            const hll_slot_t s = hll_slot(h, a.precision);
            const uint64_t at = (b << a.precision) + s.index;
            if (!register_max(a.registers + (at >> 2), (uint32_t)(at & 3u), s.rho)) *gave_up = true;
        }
    }
    return lookups;
}

__global__ __launch_bounds__(CB) void k_cov_accumulate(CovArgs a)
{
    unsigned long long lookups = 0;
    bool bad = false, gave_up = false;
    for (uint64_t pi = (uint64_t)blockIdx.x * CW + (threadIdx.x >> 6); pi < a.n_pieces; pi += (uint64_t)gridDim.x * CW) {
        const Piece pc = a.pieces[pi];
        const uint64_t lo = a.off[pc.read], hi = a.off[pc.read + 1];
        uint32_t mx = 0;
        for (uint64_t i = lo + lane_id(); i < hi; i += 64) {
            const uint32_t c = a.count[i];
            mx = c > mx ? c : mx;
        }
        mx = wave_max(mx);
        for (uint64_t base = lo; base < hi; base += 64) {
            const uint64_t i = base + lane_id();
            uint32_t c = 0, bin = 0;
            bool k = false;
            if (i < hi) {
                const int64_t b = a.ub[i];
                c = a.count[i];
                if (b < 0 || (uint64_t)b >= a.n_bins) bad = true;
                else {
                    bin = (uint32_t)b;
                    k = cov_keeps(c, mx);
                }
            }
            if (k && pc.head) {
                atomicAdd(a.reads + bin, 1ull);
                atomicAdd(a.hash_matches + bin, (unsigned long long)c);
            }
            uint64_t m = __ballot(k);
            while (m) {                                       // the surviving tuples of these 64, one after the other, by the whole wave
                const int src = __ffsll((long long)m) - 1;
                m &= m - 1;
                lookups += cov_bin(a, pc, (uint64_t)__shfl(bin, src), &gave_up);
            }
        }
    }
    if (bad) atomicOr(a.err, COV_BAD_BIN);
    if (gave_up) atomicOr(a.err, COV_CAS_GAVE_UP);
    const unsigned long long wave_lookups = wave_incl_add(lookups);     // one atomic per wave
    if (lane_id() == 63 && wave_lookups) atomicAdd(a.probes, wave_lookups);
}

#define COV_TRY(expr) TAXOR_HIP_TRY_PREFIX("coverage", expr, #expr)

}   // namespace

struct taxor_gpu_coverage {
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
    DeviceBuf<unsigned long long> d_counters;         // reads | hash_matches | probes
    Piece *h_pieces[2] = {nullptr, nullptr};          // page-locked; ev_free[i] says that buffer i's copy has left it
    hipEvent_t ev_free[2] = {nullptr, nullptr};
    bool ev_used[2] = {false, false};
    std::vector<hipEvent_t> ev_time;                  // pairs around the kernel launches of one batch
    double seconds_kernels = 0;
    std::vector<uint32_t> h_nh;
    // _results
    std::vector<uint64_t> r_reads, r_hash_matches;
    std::vector<uint8_t> r_registers;
    ~taxor_gpu_coverage()
    {
        for (int i = 0; i < 2; ++i) {
            if (h_pieces[i]) (void)hipHostFree(h_pieces[i]);
            if (ev_free[i]) (void)hipEventDestroy(ev_free[i]);
        }
        for (hipEvent_t e : ev_time) (void)hipEventDestroy(e);
        if (st) (void)hipStreamDestroy(st);
    }
};

extern "C" int taxor_gpu_coverage_create(taxor_gpu_index *idx, const taxor_hixf_view *view, uint32_t precision, taxor_gpu_coverage **out)
{
    if (!out) return fail(TAXOR_E_ARG, "coverage_create: null argument");
    *out = nullptr;
    if (!idx || !view) return fail(TAXOR_E_ARG, "coverage_create: null argument");
    if (precision == 0) precision = HLL_DEFAULT_PRECISION;
    if (precision < HLL_MIN_PRECISION || precision > HLL_MAX_PRECISION)
        return fail(TAXOR_E_ARG, "coverage_create: precision %u is not in [%u, %u] (0 = %u)", precision, HLL_MIN_PRECISION, HLL_MAX_PRECISION, HLL_DEFAULT_PRECISION);
    const IxfDesc *d_ixf = nullptr, *h_ixf = nullptr;
    uint64_t n_ixf = 0, n_bins = 0;
    uint32_t n_passes = 0;
    int device = 0;
    if (taxor_index_descs(idx, &d_ixf, &h_ixf, &n_ixf, &n_bins, &n_passes, &device)) return fail(TAXOR_E_ARG, "coverage_create: null index");
    if (n_passes)
        return fail(TAXOR_E_ARG, "coverage_create: a paged index (%u resident pass%s) is refused: its leaf bins are not all resident at once, and accumulating pass by pass is not built",
                    n_passes, n_passes == 1 ? "" : "es");
    if (view->n_ixf != n_ixf || view->n_user_bins != n_bins || (n_ixf && !view->ixf))
        return fail(TAXOR_E_ARG, "coverage_create: the view (%llu IXFs, %llu user bins) is not the index's (%llu IXFs, %llu user bins)", (unsigned long long)view->n_ixf,
                    (unsigned long long)view->n_user_bins, (unsigned long long)n_ixf, (unsigned long long)n_bins);
    if (n_bins >= (1ull << 32) || n_ixf >= (1ull << 32)) return fail(TAXOR_E_ARG, "coverage_create: user bins and IXFs are numbered in 32 bits");
    // the inverse of fname_idx: every leaf technical bin of a user bin, root included, as one CSR
    std::vector<uint64_t> leaf_off(n_bins + 1, 0);
    for (uint64_t x = 0; x < n_ixf; ++x) {
        const taxor_ixf_view &f = view->ixf[x];
        if (f.bins != h_ixf[x].bins) return fail(TAXOR_E_ARG, "coverage_create: IXF %llu has %llu bins in the view, %u in the index", (unsigned long long)x, (unsigned long long)f.bins, h_ixf[x].bins);
        if (!f.fname_idx) return fail(TAXOR_E_ARG, "coverage_create: IXF %llu of the view has no fname_idx", (unsigned long long)x);
        for (uint64_t j = 0; j < f.bins; ++j) {
            const int64_t b = f.fname_idx[j];
            if (b < 0) continue;
            if ((uint64_t)b >= n_bins) return fail(TAXOR_E_ARG, "coverage_create: bin %llu of IXF %llu names user bin %lld of %llu", (unsigned long long)j, (unsigned long long)x, (long long)b, (unsigned long long)n_bins);
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
    COV_TRY(hipSetDevice(device));
    // what the accumulator allocates, held against the device's free memory first
    const uint64_t reg_bytes = ((n_bins << precision) + 3) / 4 * 4;
    const uint64_t need = reg_bytes + (2 * n_bins + 1) * 8 + (n_bins + 1) * 8 + leaf.size() * 8 + 2 * (STAGE_HASHES * 8 + STAGE_PIECES * sizeof(Piece)) + 4;
    size_t fr = 0, tot = 0;
    COV_TRY(hipMemGetInfo(&fr, &tot));
    if (need > fr)
        return fail(TAXOR_E_NOMEM, "coverage_create: the sketches of %llu user bins at precision %u need %llu bytes on the device (%llu of them registers), %llu are free; a smaller --coverage-precision quarters the registers per two steps",
                    (unsigned long long)n_bins, precision, (unsigned long long)need, (unsigned long long)reg_bytes, (unsigned long long)fr);
    auto c = std::make_unique<taxor_gpu_coverage>();
    c->idx = idx;
    c->device = device;
    c->precision = precision;
    c->n_bins = n_bins;
    c->d_ixf = d_ixf;
    COV_TRY(hipStreamCreate(&c->st));
    COV_TRY(c->d_leaf_off.alloc(n_bins + 1));
    COV_TRY(c->d_leaf.alloc(leaf.size() + 1));
    COV_TRY(c->d_registers.alloc(reg_bytes / 4 + 1));
    COV_TRY(c->d_counters.alloc(2 * n_bins + 1));
    COV_TRY(c->d_err.alloc(1));
    for (int i = 0; i < 2; ++i) {
        COV_TRY(c->d_hashes[i].alloc(STAGE_HASHES));
        COV_TRY(c->d_pieces[i].alloc(STAGE_PIECES));
        COV_TRY(hipHostMalloc((void **)&c->h_pieces[i], STAGE_PIECES * sizeof(Piece), hipHostMallocDefault));
        COV_TRY(hipEventCreateWithFlags(&c->ev_free[i], hipEventDisableTiming));
    }
    COV_TRY(hipMemcpy(c->d_leaf_off.p, leaf_off.data(), (n_bins + 1) * 8, hipMemcpyHostToDevice));
    if (!leaf.empty()) COV_TRY(hipMemcpy(c->d_leaf.p, leaf.data(), leaf.size() * 8, hipMemcpyHostToDevice));
    COV_TRY(hipMemset(c->d_registers.p, 0, (reg_bytes / 4 + 1) * 4));
    COV_TRY(hipMemset(c->d_counters.p, 0, (2 * n_bins + 1) * 8));
    COV_TRY(hipMemset(c->d_err.p, 0, 4));
    *out = c.release();
    return TAXOR_OK;
}

extern "C" void taxor_gpu_coverage_destroy(taxor_gpu_coverage *c)
{
    if (!c) return;
    (void)hipSetDevice(c->device);
    delete c;
}

extern "C" int taxor_gpu_coverage_add_batch(taxor_gpu_coverage *c, taxor_gpu_searcher *s, const taxor_gpu_saved *saved)
{
    if (!c || !s) return fail(TAXOR_E_ARG, "coverage_add_batch: null argument");
    if (!saved) return fail(TAXOR_E_ARG, "coverage_add_batch: saved: no saved batch (the batch ran with capture off, or its lists were not taken)");
    if (taxor_searcher_index(s) != c->idx) return fail(TAXOR_E_ARG, "coverage_add_batch: index: the searcher works on another index than the accumulator");
    const std::string unsound = saved_validate(*saved);
    if (!unsound.empty()) return fail(TAXOR_E_ARG, "coverage_add_batch: " + unsound);
    const uint64_t *d_off = nullptr;
    const int64_t *d_ub = nullptr;
    const uint32_t *d_cnt = nullptr, *d_nh = nullptr;
    uint64_t n = 0, nt = 0;
    int dev = 0;
    if (int rc = taxor_searcher_device_results(s, &d_off, &d_ub, &d_cnt, &d_nh, &n, &nt, &dev)) return rc;
    if (saved->n_reads != n)
        return fail(TAXOR_E_ARG, "coverage_add_batch: n_reads: the saved batch holds %llu reads, the searcher's last batch %llu", (unsigned long long)saved->n_reads, (unsigned long long)n);
    std::lock_guard<std::mutex> lk(c->mu);
    COV_TRY(hipSetDevice(c->device));
    c->h_nh.resize(n);
    if (n) COV_TRY(hipMemcpy(c->h_nh.data(), d_nh, n * 4, hipMemcpyDeviceToHost));
    for (uint64_t r = 0; r < n; ++r)
        if (c->h_nh[r] != saved->n_hashes[r])
            return fail(TAXOR_E_ARG, "coverage_add_batch: n_hashes: read %llu has %u hashes in the saved batch, %u in the searcher's last batch", (unsigned long long)r, saved->n_hashes[r], c->h_nh[r]);
    if (n == 0) return TAXOR_OK;

    CovArgs a{};
    a.ixf = c->d_ixf;
    a.leaf_off = c->d_leaf_off.p;
    a.leaf = c->d_leaf.p;
    a.off = d_off;
    a.ub = d_ub;
    a.count = d_cnt;
    a.precision = c->precision;
    a.n_bins = c->n_bins;
    a.registers = c->d_registers.p;
    a.reads = c->d_counters.p;
    a.hash_matches = c->d_counters.p + c->n_bins;
    a.probes = c->d_counters.p + 2 * c->n_bins;
    a.err = c->d_err.p;

    // Groups of pieces, each staged and launched by itself: a group never spans two sub-batches of the saved plan, holds at most
    // STAGE_HASHES hashes and STAGE_PIECES pieces.  Its hashes are one contiguous range of the dense saved array.
    size_t n_launch = 0;
    int buf = 0;
    uint32_t n_p = 0;
    uint64_t g0 = 0, g1 = 0;            // the group's hashes: [g0, g1) of saved->hashes
    auto flush = [&]() -> int {
        if (n_p == 0) return TAXOR_OK;
        if (g1 > g0) COV_TRY(hipMemcpyAsync(c->d_hashes[buf].p, saved->hashes + g0, (g1 - g0) * 8, hipMemcpyHostToDevice, c->st));
        COV_TRY(hipMemcpyAsync(c->d_pieces[buf].p, c->h_pieces[buf], (uint64_t)n_p * sizeof(Piece), hipMemcpyHostToDevice, c->st));
        COV_TRY(hipEventRecord(c->ev_free[buf], c->st));
        c->ev_used[buf] = true;
        while (c->ev_time.size() < 2 * (n_launch + 1)) {
            hipEvent_t e = nullptr;
            COV_TRY(hipEventCreate(&e));
            c->ev_time.push_back(e);
        }
        a.pieces = c->d_pieces[buf].p;
        a.hashes = c->d_hashes[buf].p;
        a.n_pieces = n_p;
        COV_TRY(hipEventRecord(c->ev_time[2 * n_launch], c->st));
        k_cov_accumulate<<<grid_for(n_p, CW, C_GRID_CAP), CB, 0, c->st>>>(a);
        COV_TRY(hipGetLastError());
        COV_TRY(hipEventRecord(c->ev_time[2 * n_launch + 1], c->st));
        ++n_launch;
        buf ^= 1;
        n_p = 0;
        g0 = g1;
        if (c->ev_used[buf]) COV_TRY(hipEventSynchronize(c->ev_free[buf]));     // the page-locked pieces of two groups ago have been copied
        return TAXOR_OK;
    };
    for (size_t sb = 0; sb + 1 < saved->sub_first.size(); ++sb) {
        for (uint64_t r = saved->sub_first[sb]; r < saved->sub_first[sb + 1]; ++r) {
            const uint64_t h0 = saved->hash_off[r], nh = saved->n_hashes[r];
            uint64_t done = 0;
            do {                                    // every read has a first piece, hashes or not: it counts the read's tuples
                const uint32_t take = (uint32_t)std::min<uint64_t>(COV_SPLIT, nh - done);
                if (n_p == STAGE_PIECES || g1 - g0 + take > STAGE_HASHES)
                    if (int rc = flush()) return rc;
                c->h_pieces[buf][n_p++] = Piece{(uint32_t)r, (uint32_t)(h0 + done - g0), take, done == 0 ? 1u : 0u};
                done += take;
                g1 = h0 + done;
            } while (done < nh);
        }
        if (int rc = flush()) return rc;
    }
    uint32_t err = 0;
    COV_TRY(hipMemcpyAsync(&err, c->d_err.p, 4, hipMemcpyDeviceToHost, c->st));
    COV_TRY(hipStreamSynchronize(c->st));           // the searcher's buffers and the saved lists are the caller's again
    c->ev_used[0] = c->ev_used[1] = false;
    for (size_t i = 0; i < n_launch; ++i) {
        float ms = 0;
        COV_TRY(hipEventElapsedTime(&ms, c->ev_time[2 * i], c->ev_time[2 * i + 1]));
        c->seconds_kernels += (double)ms * 1e-3;
    }
    if (err & COV_BAD_BIN) return fail(TAXOR_E_INTERNAL, "coverage_add_batch: a tuple names a user bin outside the index's %llu", (unsigned long long)c->n_bins);
    if (err & COV_CAS_GAVE_UP) return fail(TAXOR_E_INTERNAL, "coverage_add_batch: a register update did not complete in %d rounds", CAS_ROUNDS);
    return TAXOR_OK;
}

extern "C" int taxor_gpu_coverage_results(taxor_gpu_coverage *c, taxor_coverage_results *out)
{
    if (!c || !out) return fail(TAXOR_E_ARG, "coverage_results: null argument");
    std::lock_guard<std::mutex> lk(c->mu);
    COV_TRY(hipSetDevice(c->device));
    const uint64_t nb = c->n_bins, reg_bytes = nb << c->precision;
    c->r_reads.resize(nb);
    c->r_hash_matches.resize(nb);
    c->r_registers.resize(reg_bytes);
    unsigned long long probes = 0;
    if (nb) {
        COV_TRY(hipMemcpy(c->r_reads.data(), c->d_counters.p, nb * 8, hipMemcpyDeviceToHost));
        COV_TRY(hipMemcpy(c->r_hash_matches.data(), c->d_counters.p + nb, nb * 8, hipMemcpyDeviceToHost));
        COV_TRY(hipMemcpy(c->r_registers.data(), c->d_registers.p, reg_bytes, hipMemcpyDeviceToHost));
    }
    COV_TRY(hipMemcpy(&probes, c->d_counters.p + 2 * nb, 8, hipMemcpyDeviceToHost));
    out->n_user_bins = nb;
    out->precision = c->precision;
    out->reserved = 0;
    out->reads = c->r_reads.data();
    out->hash_matches = c->r_hash_matches.data();
    out->registers = c->r_registers.data();
    out->seconds_kernels = c->seconds_kernels;
    out->probes = probes;
    return TAXOR_OK;
}
