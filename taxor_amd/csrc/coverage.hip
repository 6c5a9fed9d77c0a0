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
//                      lane: read_probe.h's lookup over ALL of b's leaf bins (`probes` counts them), and for a hash that matched in
//                      any of them one register update.  The read's first piece (rank0 == 0) also adds the tuple to reads[b] and
//                      hash_matches[b].
//
// Registers are bytes, four to a 32-bit word, raised by a compare-and-swap on the word (read_probe.h's hll_register_max): a quarter of the memory of a word per register
// (4 KiB per user bin at P = 12: 113 MB for 27 473 user bins, 410 MB for 100 000), and the load in front of the swap ends the update
// where the register is high enough already -- after the first reads of a reference that is nearly every update.  max is order-free:
// the registers do not depend on the launch geometry, the order of the batches or the cut into pieces.  No block waits on another.
#include "analysis_host.h"
#include "hll.h"

#include <memory>

namespace {

using namespace taxor;

constexpr int CB = READ_BLOCK, CW = READ_WAVES, C_GRID_CAP = READ_GRID_CAP;

enum : uint32_t { COV_BAD_BIN = 1u, COV_CAS_GAVE_UP = 2u };

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

// the piece's hashes against user bin b's leaf bins; returns the lookups this lane made
__device__ __forceinline__ uint32_t cov_bin(const CovArgs &a, const Piece &pc, uint64_t b, bool *gave_up)
{
    const uint64_t l0 = a.leaf_off[b], l1 = a.leaf_off[b + 1];
    uint32_t lookups = 0;
    for (uint32_t h0 = 0; h0 < pc.n; h0 += 64) {
        const uint32_t j = h0 + lane_id();
        const bool active = j < pc.n;
        const uint64_t h = active ? a.hashes[(uint64_t)pc.first + j] : 0;
        if (leaf_lookup<false>(a.ixf, a.leaf, l0, l1, h, active, lookups)) {
            const hll_slot_t s = hll_slot(h, a.precision);
            const uint64_t at = (b << a.precision) + s.index;
            if (!hll_register_max(a.registers + (at >> 2), (uint32_t)(at & 3u), s.rho)) *gave_up = true;
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
                    k = keeps(c, mx);
                }
            }
            if (k && pc.rank0 == 0) {
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
    wave_add_to(a.probes, lookups);
}

#define COV_TRY(expr) TAXOR_HIP_TRY_PREFIX("coverage", expr, #expr)

}   // namespace

struct taxor_gpu_coverage : ReadAnalysis {
    uint32_t precision = 0;
    DeviceBuf<uint32_t> d_registers;
    DeviceBuf<unsigned long long> d_counters;         // reads | hash_matches | probes
    double seconds_kernels = 0;
    // _results
    std::vector<uint64_t> r_reads, r_hash_matches;
    std::vector<uint8_t> r_registers;
};

extern "C" int taxor_gpu_coverage_create(taxor_gpu_index *idx, const taxor_hixf_view *view, uint32_t precision, taxor_gpu_coverage **out)
{
    if (!out) return fail(TAXOR_E_ARG, "coverage_create: null argument");
    *out = nullptr;
    if (!idx || !view) return fail(TAXOR_E_ARG, "coverage_create: null argument");
    if (precision == 0) precision = HLL_DEFAULT_PRECISION;
    if (precision < HLL_MIN_PRECISION || precision > HLL_MAX_PRECISION)
        return fail(TAXOR_E_ARG, "coverage_create: precision %u is not in [%u, %u] (0 = %u)", precision, HLL_MIN_PRECISION, HLL_MAX_PRECISION, HLL_DEFAULT_PRECISION);
    auto c = std::make_unique<taxor_gpu_coverage>();
    if (int rc = c->leaf.build("coverage_create", "its leaf bins are not all resident at once, and accumulating pass by pass is not built", idx, view)) return rc;
    if (int rc = c->stage.configure("coverage_create")) return rc;
    const uint64_t n_bins = c->leaf.n_bins;
    COV_TRY(hipSetDevice(c->leaf.device));
    // what the accumulator allocates, held against the device's free memory first
    const uint64_t reg_bytes = ((n_bins << precision) + 3) / 4 * 4;
    const uint64_t need = reg_bytes + (2 * n_bins + 1) * 8 + c->leaf.device_bytes() + c->stage.device_bytes() + 4;
    size_t fr = 0, tot = 0;
    COV_TRY(hipMemGetInfo(&fr, &tot));
    if (need > fr)
        return fail(TAXOR_E_NOMEM, "coverage_create: the sketches of %llu user bins at precision %u need %llu bytes on the device (%llu of them registers), %llu are free; a smaller --coverage-precision quarters the registers per two steps",
                    (unsigned long long)n_bins, precision, (unsigned long long)need, (unsigned long long)reg_bytes, (unsigned long long)fr);
    c->precision = precision;
    if (int rc = c->open("coverage")) return rc;
    COV_TRY(c->d_registers.alloc(reg_bytes / 4 + 1));
    COV_TRY(c->d_counters.alloc(2 * n_bins + 1));
    COV_TRY(hipMemset(c->d_registers.p, 0, (reg_bytes / 4 + 1) * 4));
    COV_TRY(hipMemset(c->d_counters.p, 0, (2 * n_bins + 1) * 8));
    *out = c.release();
    return TAXOR_OK;
}

extern "C" void taxor_gpu_coverage_destroy(taxor_gpu_coverage *c)
{
    if (!c) return;
    (void)hipSetDevice(c->leaf.device);
    delete c;
}

extern "C" int taxor_gpu_coverage_add_batch(taxor_gpu_coverage *c, taxor_gpu_searcher *s, const taxor_gpu_saved *saved)
{
    if (!c || !s) return fail(TAXOR_E_ARG, "coverage_add_batch: null argument");
    std::unique_lock<std::mutex> lk;
    SearcherBatch b;
    if (int rc = begin_batch("coverage_add_batch", "coverage", "the accumulator", *c, s, saved, lk, &b)) return rc;
    if (int rc = c->stage.recover()) return rc;
    if (b.n == 0) return TAXOR_OK;
    const uint64_t n_bins = c->leaf.n_bins;

    CovArgs a{};
    a.ixf = c->leaf.d_ixf;
    a.leaf_off = c->leaf.d_off.p;
    a.leaf = c->leaf.d_leaf.p;
    a.off = b.d_off;
    a.ub = b.d_ub;
    a.count = b.d_cnt;
    a.precision = c->precision;
    a.n_bins = n_bins;
    a.registers = c->d_registers.p;
    a.reads = c->d_counters.p;
    a.hash_matches = c->d_counters.p + n_bins;
    a.probes = c->d_counters.p + 2 * n_bins;
    a.err = c->d_err.p;
    c->timer.begin();
    c->stage.begin(saved->hashes, [&](const Piece *pieces, const uint64_t *staged, uint32_t n_p) {
        a.pieces = pieces;
        a.hashes = staged;
        a.n_pieces = n_p;
        k_cov_accumulate<<<grid_for(n_p, CW, C_GRID_CAP), CB, 0, c->st>>>(a);
    });
    // every read has a first piece, hashes or not: it counts the read's tuples.  A set never spans two sub-batches of the saved plan
    for (size_t sb = 0; sb + 1 < saved->sub_first.size(); ++sb) {
        for (uint64_t r = saved->sub_first[sb]; r < saved->sub_first[sb + 1]; ++r)
            if (int rc = c->stage.add(r, saved->hash_off[r], saved->n_hashes[r])) return rc;
        if (int rc = c->stage.flush()) return rc;
    }
    uint32_t err = 0;
    COV_TRY(hipMemcpyAsync(&err, c->d_err.p, 4, hipMemcpyDeviceToHost, c->st));
    COV_TRY(hipStreamSynchronize(c->st));           // the searcher's buffers and the saved lists are the caller's again
    c->stage.end();
    if (int rc = c->timer.add_to(&c->seconds_kernels)) return rc;
    if (err)
        if (int rc = c->clear_err()) return rc;
    if (err & COV_BAD_BIN) return fail(TAXOR_E_INTERNAL, "coverage_add_batch: a tuple names a user bin outside the index's %llu", (unsigned long long)n_bins);
    if (err & COV_CAS_GAVE_UP) return fail(TAXOR_E_INTERNAL, "coverage_add_batch: a register update did not complete in %d rounds", HLL_CAS_ROUNDS);
    return TAXOR_OK;
}

extern "C" int taxor_gpu_coverage_results(taxor_gpu_coverage *c, taxor_coverage_results *out)
{
    if (!c || !out) return fail(TAXOR_E_ARG, "coverage_results: null argument");
    std::lock_guard<std::mutex> lk(c->mu);
    COV_TRY(hipSetDevice(c->leaf.device));
    const uint64_t nb = c->leaf.n_bins, reg_bytes = nb << c->precision;
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
