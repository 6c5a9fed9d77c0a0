// exclusive.hip -- hashes only one reference explains: per read, which of the references it reported holds hashes that none of the others
// on that read's list holds (`taxor search --exclusive-file` / `--exclusive-reads-file`).
//
// The object lives beside a resident index for a whole run.  It holds the leaf-bin table and the piece stager of analysis_host.h, and
// per user bin four 64-bit sums and a HyperLogLog sketch of the hashes that were exclusive to it (byte registers, four to a word, raised by
// read_probe.h's hll_register_max).  A batch brings the searcher's device-resident CSR -- EVERY tuple that passed the search threshold --
// and the batch's saved hash lists.  The CANDIDATES of a read are its tuples with count > 0, in CSR order; a read is EXAMINED when it
// has a hash and a candidate.
//
//   read_probe.h's k_cand_count (M per read, to the host, which decides who is examined, sums the candidates' offsets and cuts pieces)
//                and k_cand_fill (tuple index, user bin and the range of the user bin's leaf bins in CSR order).
//   k_ex_probe   one wave per PIECE -- at most EX_SPLIT consecutive hashes of one examined read.  64 hashes per round, one per lane; the
//                lane walks ALL M candidates (hits_c needs every candidate: there is no early exit) with read_probe.h's lookup, which stops at a candidate's first matching leaf bin, and
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
// HLL_CAS_ROUNDS of a register update.  No block waits on another.  There is no per-hash or per-round array: reads are not grouped.
#include "analysis_host.h"
#include "hll.h"

#include <map>
#include <memory>

namespace {

using namespace taxor;

constexpr int EB = READ_BLOCK, EW = READ_WAVES, E_GRID_CAP = READ_GRID_CAP;

enum : uint32_t { EX_CAS_GAVE_UP = 4u };          // beside CAND_BAD_BIN and CAND_MISCOUNT

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
                const bool matched = leaf_lookup<true>(a.ixf, a.leaf, lr.l0, lr.l1, h, active, lookups);
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
                if (!hll_register_max(a.registers + (at >> 2), (uint32_t)(at & 3u), s.rho)) gave_up = true;
            }
        }
        if (lane == 0) {
            if (p_matched) atomicAdd(a.matched + pc.read, p_matched);
            if (p_shared) atomicAdd(a.shared + pc.read, p_shared);
        }
    }
    if (gave_up) atomicOr(a.err, EX_CAS_GAVE_UP);
    wave_add_to(a.lookups, lookups);
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

struct taxor_gpu_exclusive : ReadAnalysis {
    uint32_t precision = 0;
    DeviceBuf<uint32_t> d_registers;
    DeviceBuf<unsigned long long> d_sums, d_lookups;  // d_sums: cand_reads | hits | exclusive_hits | exclusive_reads
    std::map<const void *, std::unique_ptr<Slot>> slots;
    double seconds_kernels = 0;
    uint64_t probes = 0;
    // _results
    std::vector<uint64_t> r_sums;
    std::vector<uint8_t> r_registers;
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
    if (int rc = c->stage.recover()) return rc;
    if (n == 0) return TAXOR_OK;
    const uint64_t n_bins = c->leaf.n_bins;
    c->timer.begin();
    auto stamp = [&]() { return c->timer.stamp(c->st); };

    // the words of a read that is not examined are 0
    EX_TRY(hipMemsetAsync(sl.d_r32.p, 0, 2 * n * sizeof(uint32_t), c->st));
    EX_TRY(hipMemsetAsync(c->d_lookups.p, 0, 8, c->st));
    if (int rc = stamp()) return rc;
    k_cand_count<uint32_t><<<grid_for(n, EW, E_GRID_CAP), EB, 0, c->st>>>(d_off, d_ub, d_cnt, t0, d_nh, n, n_bins, sl.d_n_cand.p, c->d_err.p);
    EX_TRY(hipGetLastError());
    if (int rc = stamp()) return rc;
    uint32_t err = 0;
    EX_TRY(hipMemcpyAsync(h_m, sl.d_n_cand.p, n * sizeof(uint32_t), hipMemcpyDeviceToHost, c->st));
    EX_TRY(hipMemcpyAsync(&err, c->d_err.p, 4, hipMemcpyDeviceToHost, c->st));
    EX_TRY(hipStreamSynchronize(c->st));
    if (err & CAND_BAD_BIN) {
        if (int rc = c->clear_err()) return rc;
        return fail(TAXOR_E_INTERNAL, "exclusive_add: user_bin: a tuple names a user bin outside the index's %llu", (unsigned long long)n_bins);
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
        k_cand_fill<true><<<grid_for(n, EW, E_GRID_CAP), EB, 0, c->st>>>(d_off, d_ub, d_cnt, t0, n, n_bins, c->leaf.d_off.p, sl.d_cand_off.p, sl.d_cand_tuple.p, sl.d_cand_ub.p,
                                                                         sl.d_cand_leaf.p, c->d_err.p);
        EX_TRY(hipGetLastError());
        if (int rc = stamp()) return rc;

        ProbeArgs a{};
        a.ixf = c->leaf.d_ixf;
        a.leaf = c->leaf.d_leaf.p;
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
        c->stage.begin(hashes, [&](const Piece *pieces, const uint64_t *staged, uint32_t n_p) {
            a.pieces = pieces;
            a.hashes = staged;
            a.n_pieces = n_p;
            k_ex_probe<<<grid_for(n_p, EW, E_GRID_CAP), EB, 0, c->st>>>(a);
        });
        for (uint64_t r = 0; r < n; ++r)
            if (sl.h_examined[r])
                if (int rc = c->stage.add(r, hash_off[r], h_nh[r])) return rc;
        if (int rc = c->stage.flush()) return rc;
        if (int rc = stamp()) return rc;
        k_ex_tally<<<grid_for(n_cand, EB, E_GRID_CAP), EB, 0, c->st>>>(n_cand, sl.d_cand_tuple.p, sl.d_cand_ub.p, d_cnt, t0, d_hits, d_excl, d_count, n_bins, c->d_sums.p);
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
    c->stage.end();
    if (int rc = c->timer.add_to(&out->seconds_kernels)) return rc;
    out->probes = lookups;
    c->seconds_kernels += out->seconds_kernels;
    c->probes += lookups;
    if (err) {
        if (int rc = c->clear_err()) return rc;
        if (err & EX_CAS_GAVE_UP) return fail(TAXOR_E_INTERNAL, "exclusive_add: registers: a register update did not complete in %d rounds", HLL_CAS_ROUNDS);
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
    auto c = std::make_unique<taxor_gpu_exclusive>();
    if (int rc = c->leaf.build("exclusive_create", "its leaf bins are not all resident at once and a read's final tuples exist only after the last pass's merge; counting exclusive hashes pass by pass is not built", idx, view))
        return rc;
    if (int rc = c->stage.configure("exclusive_create")) return rc;
    const uint64_t n_bins = c->leaf.n_bins;
    EX_TRY(hipSetDevice(c->leaf.device));
    // what the object allocates at once, held against the device's free memory first
    const uint64_t reg_bytes = ((n_bins << precision) + 3) / 4 * 4;
    const uint64_t need = reg_bytes + (4 * n_bins + 1) * 8 + c->leaf.device_bytes() + c->stage.device_bytes() + 12;
    size_t fr = 0, tot = 0;
    EX_TRY(hipMemGetInfo(&fr, &tot));
    if (need > fr)
        return fail(TAXOR_E_NOMEM, "exclusive_create: the sketches of %llu user bins at precision %u need %llu bytes on the device (%llu of them registers), %llu are free; a smaller --exclusive-precision quarters the registers per two steps",
                    (unsigned long long)n_bins, precision, (unsigned long long)need, (unsigned long long)reg_bytes, (unsigned long long)fr);
    c->precision = precision;
    if (int rc = c->open("exclusive")) return rc;
    EX_TRY(c->d_registers.alloc(reg_bytes / 4 + 1));
    EX_TRY(c->d_sums.alloc(4 * n_bins + 1));
    EX_TRY(c->d_lookups.alloc(1));
    EX_TRY(hipMemset(c->d_registers.p, 0, (reg_bytes / 4 + 1) * 4));
    EX_TRY(hipMemset(c->d_sums.p, 0, (4 * n_bins + 1) * 8));
    *out = c.release();
    return TAXOR_OK;
}

extern "C" void taxor_gpu_exclusive_destroy(taxor_gpu_exclusive *c)
{
    if (!c) return;
    (void)hipSetDevice(c->leaf.device);
    delete c;
}

extern "C" int taxor_gpu_exclusive_add_batch(taxor_gpu_exclusive *c, taxor_gpu_searcher *s, const taxor_gpu_saved *saved, taxor_exclusive_batch *out)
{
    if (!c || !s || !out) return fail(TAXOR_E_ARG, "exclusive_add_batch: null argument");
    std::unique_lock<std::mutex> lk;
    SearcherBatch b;
    if (int rc = begin_batch("exclusive_add_batch", "exclusive", "the exclusive object", *c, s, saved, lk, &b)) return rc;
    return add_device(c, s, b.n, b.d_off, b.d_ub, b.d_cnt, b.d_nh, 0, saved->hash_off.data(), saved->hashes, c->h_nh.data(), out);
}

extern "C" int taxor_gpu_exclusive_add_csr(taxor_gpu_exclusive *c, uint64_t n_reads, const uint64_t *read_off, const int64_t *user_bin, const uint32_t *count,
                                           const uint64_t *hash_off, const uint64_t *hashes, taxor_exclusive_batch *out)
{
    if (!c || !read_off || !hash_off || !out) return fail(TAXOR_E_ARG, "exclusive_add_csr: null argument");
    CsrUpload &u = c->csr;
    std::lock_guard<std::mutex> lk(c->mu);
    if (int rc = u.check("exclusive_add_csr", "index", c->leaf.n_bins, n_reads, read_off, user_bin, count, hash_off, hashes)) return rc;
    EX_TRY(hipSetDevice(c->leaf.device));
    if (int rc = u.upload("exclusive", n_reads, read_off, user_bin, count, hash_off, nullptr, &c->h_nh)) return rc;
    return add_device(c, nullptr, n_reads, u.off.p, u.ub.p, u.cnt.p, u.nh.p, u.t0, hash_off, hashes, c->h_nh.data(), out);
}

extern "C" int taxor_gpu_exclusive_results(taxor_gpu_exclusive *c, taxor_exclusive_results *out)
{
    if (!c || !out) return fail(TAXOR_E_ARG, "exclusive_results: null argument");
    std::lock_guard<std::mutex> lk(c->mu);
    EX_TRY(hipSetDevice(c->leaf.device));
    const uint64_t nb = c->leaf.n_bins, reg_bytes = nb << c->precision;
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
