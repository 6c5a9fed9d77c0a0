// breakpoint.hip -- where a read switches reference: the best split of its ordered hash list between two of the references it reported
// (`taxor search --breakpoint-file`).
//
// The object lives beside a resident index for a whole run and keeps nothing between batches but its buffers: the leaf-bin table and
// the piece stager of analysis_host.h.  A batch brings the searcher's device-resident CSR -- EVERY tuple that passed the search
// threshold, not only the survivors of the 0.8 * max filter -- and the batch's saved hash lists, whose order is the order of first
// occurrence along the read.  The CANDIDATES of a read are its tuples with count > 0, in CSR order; a read is EXAMINED when it has a
// hash and at least two candidates.
//
//   read_probe.h's k_cand_count (M per read, to the host, which decides who is examined, sums the candidates' offsets and cuts groups,
//                pieces and scratch), k_cand_fill (tuple index and user bin in CSR order) and k_probe_mask (one wave per PIECE of an
//                examined read: one 64-bit match word mask[c][round] per candidate and 64 hashes; `lookups` counts its leaf-bin
//                lookups, which stop at a candidate's first matching leaf bin).
//   k_bp_prefix one lane per candidate of an examined read, its rounds in order: base[c][k] = the matches in rounds before k, and
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
#include "analysis_host.h"
#include "breakpoint_format.h"

#include <map>
#include <memory>

namespace {

using namespace taxor;

constexpr int BB = READ_BLOCK, BW = READ_WAVES, B_GRID_CAP = READ_GRID_CAP;
constexpr uint64_t BP_BUDGET_WORDS = 1ull << 23;  // mask words of one group of reads (64 MiB; the prefix counts beside them are at most as many bytes)
constexpr int BP_W32 = 9, BP_W64 = 6;             // 32- and 64-bit words per read the scan writes

// what the kernels after the fill share: the match words (read_probe.h) and where a read's prefix counts lie within its group's scratch
struct Layout : MaskLayout {
    const uint64_t *cand_tuple;   // [n_cand] index in the batch CSR
    const uint64_t *base_off;     // [n_reads] first prefix count of the read: base[base_off[r] + c * (rounds + 1) + k]
    uint32_t *base;
};

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
            const unsigned long long mx = wave_max(key) - 1ull;
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

struct taxor_gpu_breakpoint : ReadAnalysis {
    uint32_t min_gain = 1;
    uint64_t budget_words = BP_BUDGET_WORDS;
    DeviceBuf<uint64_t> d_mask;
    DeviceBuf<uint32_t> d_base;
    DeviceBuf<unsigned long long> d_lookups;
    std::vector<Group> groups;
    std::map<const void *, std::unique_ptr<Slot>> slots;
};

namespace {

// One batch whose CSR is on the object's device (tuples indexed from t0); the hash lists are host arrays (read r's at
// hashes[hash_off[r] .. hash_off[r + 1]), h_nh[r] of them).  The caller holds the mutex and has made every check that needs no launch.
int add_device(taxor_gpu_breakpoint *c, const void *who, uint64_t n, const uint64_t *d_off, const int64_t *d_ub, const uint32_t *d_cnt, const uint32_t *d_nh,
               uint64_t t0, const uint64_t *hash_off, const uint64_t *hashes, const uint32_t *h_nh, taxor_breakpoint_batch *out)
{
    const uint64_t n_bins = c->leaf.n_bins;
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
    if (int rc = c->stage.recover()) return rc;
    if (n == 0) return TAXOR_OK;
    uint32_t *d32 = sl.d_w32.p;
    uint64_t *d64 = sl.d_w64.p;
    Words w{d32, d32 + n, d32 + 2 * n, d32 + 3 * n, d32 + 4 * n, d32 + 5 * n, d32 + 6 * n, d32 + 7 * n, d32 + 8 * n,
            d64, d64 + n, d64 + 2 * n, (int64_t *)(d64 + 3 * n), (int64_t *)(d64 + 4 * n), (int64_t *)(d64 + 5 * n)};
    c->timer.begin();
    auto stamp = [&]() { return c->timer.stamp(c->st); };

    // the words of a read that is not examined are 0
    BP_TRY(hipMemsetAsync(d32, 0, BP_W32 * n * sizeof(uint32_t), c->st));
    BP_TRY(hipMemsetAsync(d64, 0, BP_W64 * n * sizeof(uint64_t), c->st));
    BP_TRY(hipMemsetAsync(c->d_lookups.p, 0, 8, c->st));
    if (int rc = stamp()) return rc;
    k_cand_count<uint32_t><<<grid_for(n, BW, B_GRID_CAP), BB, 0, c->st>>>(d_off, d_ub, d_cnt, t0, d_nh, n, n_bins, sl.d_n_cand.p, c->d_err.p);
    BP_TRY(hipGetLastError());
    if (int rc = stamp()) return rc;
    uint32_t *h_m = h32 + (BP_W32 + 1) * n;            // the candidates' counts, behind what the caller sees
    uint32_t err = 0;
    BP_TRY(hipMemcpyAsync(h_m, sl.d_n_cand.p, n * sizeof(uint32_t), hipMemcpyDeviceToHost, c->st));
    BP_TRY(hipMemcpyAsync(&err, c->d_err.p, 4, hipMemcpyDeviceToHost, c->st));
    BP_TRY(hipStreamSynchronize(c->st));
    if (err & CAND_BAD_BIN) {
        if (int rc = c->clear_err()) return rc;
        return fail(TAXOR_E_INTERNAL, "breakpoint_add: user_bin: a tuple names a user bin outside the index's %llu", (unsigned long long)n_bins);
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
        k_cand_fill<false><<<grid_for(n, BW, B_GRID_CAP), BB, 0, c->st>>>(d_off, d_ub, d_cnt, t0, n, n_bins, nullptr, sl.d_off3.p, sl.d_cand_tuple.p, sl.d_cand_ub.p, nullptr,
                                                                          c->d_err.p);
        BP_TRY(hipGetLastError());
        if (int rc = stamp()) return rc;

        Layout l{};
        l.cand_off = sl.d_off3.p;
        l.cand_ub = sl.d_cand_ub.p;
        l.mask_off = sl.d_off3.p + n + 1;
        l.nh = d_nh;
        l.mask = c->d_mask.p;
        l.cand_tuple = sl.d_cand_tuple.p;
        l.base_off = sl.d_off3.p + 2 * n + 1;
        l.base = c->d_base.p;
        MaskProbeArgs a{c->leaf.d_ixf, c->leaf.d_off.p, c->leaf.d_leaf.p, l, nullptr, nullptr, 0, c->d_lookups.p};
        c->stage.begin(hashes, [&](const Piece *pieces, const uint64_t *staged, uint32_t n_p) {
            a.pieces = pieces;
            a.hashes = staged;
            a.n_pieces = n_p;
            k_probe_mask<true><<<grid_for(n_p, BW, B_GRID_CAP), BB, 0, c->st>>>(a);
        });
        // a group's sets come first, then its prefix counts and its scan; the next group writes the same scratch behind them on the stream
        for (const Group &g : c->groups) {
            for (uint64_t r = g.r0; r < g.r1; ++r)
                if (sl.h_examined[r])
                    if (int rc = c->stage.add(r, hash_off[r], h_nh[r])) return rc;
            if (int rc = c->stage.flush()) return rc;
            if (int rc = stamp()) return rc;
            k_bp_prefix<<<grid_for(g.r1 - g.r0, BW, B_GRID_CAP), BB, 0, c->st>>>(l, g.r0, g.r1);
            k_bp_scan<<<grid_for(g.r1 - g.r0, BW, B_GRID_CAP), BB, 0, c->st>>>(l, g.r0, g.r1, w);
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
    c->stage.end();
    if (int rc = c->timer.add_to(&out->seconds_kernels)) return rc;
    out->lookups = lookups;
    if (err) {                                         // the CSR changed under the call: the second walk did not find what the first counted
        if (int rc = c->clear_err()) return rc;
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
    auto c = std::make_unique<taxor_gpu_breakpoint>();
    if (int rc = c->leaf.build("breakpoint_create", "its leaf bins are not all resident at once and a read's final tuples exist only after the last pass's merge; finding breaks pass by pass is not built", idx, view))
        return rc;
    if (int rc = c->stage.configure("breakpoint_create")) return rc;
    c->min_gain = min_gain;
    // a measurement knob (tuning.h): the mask words of one group of reads.  It moves the cut into groups, never a result
    if (const char *e = tune_env("TAXOR_BREAKPOINT_BUDGET_WORDS")) {
        const long long v = atoll(e);
        if (v >= 1) c->budget_words = (uint64_t)v;
    }
    BP_TRY(hipSetDevice(c->leaf.device));
    if (int rc = c->open("breakpoint")) return rc;
    BP_TRY(c->d_lookups.alloc(1));
    *out = c.release();
    return TAXOR_OK;
}

extern "C" void taxor_gpu_breakpoint_destroy(taxor_gpu_breakpoint *c)
{
    if (!c) return;
    (void)hipSetDevice(c->leaf.device);
    delete c;
}

extern "C" int taxor_gpu_breakpoint_add_batch(taxor_gpu_breakpoint *c, taxor_gpu_searcher *s, const taxor_gpu_saved *saved, taxor_breakpoint_batch *out)
{
    if (!c || !s || !out) return fail(TAXOR_E_ARG, "breakpoint_add_batch: null argument");
    std::unique_lock<std::mutex> lk;
    SearcherBatch b;
    if (int rc = begin_batch("breakpoint_add_batch", "breakpoint", "the breakpoint object", *c, s, saved, lk, &b)) return rc;
    return add_device(c, s, b.n, b.d_off, b.d_ub, b.d_cnt, b.d_nh, 0, saved->hash_off.data(), saved->hashes, c->h_nh.data(), out);
}

extern "C" int taxor_gpu_breakpoint_add_csr(taxor_gpu_breakpoint *c, uint64_t n_reads, const uint64_t *read_off, const int64_t *user_bin, const uint32_t *count,
                                            const uint64_t *hash_off, const uint64_t *hashes, taxor_breakpoint_batch *out)
{
    if (!c || !read_off || !hash_off || !out) return fail(TAXOR_E_ARG, "breakpoint_add_csr: null argument");
    CsrUpload &u = c->csr;
    std::lock_guard<std::mutex> lk(c->mu);
    if (int rc = u.check("breakpoint_add_csr", "index", c->leaf.n_bins, n_reads, read_off, user_bin, count, hash_off, hashes)) return rc;
    BP_TRY(hipSetDevice(c->leaf.device));
    if (int rc = u.upload("breakpoint", n_reads, read_off, user_bin, count, hash_off, nullptr, &c->h_nh)) return rc;
    return add_device(c, nullptr, n_reads, u.off.p, u.ub.p, u.cnt.p, u.nh.p, u.t0, hash_off, hashes, c->h_nh.data(), out);
}
