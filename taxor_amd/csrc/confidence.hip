// confidence.hip -- how many of a read's hashes stand behind its LCA call, and the call a threshold on that leaves
// (`taxor search --lca-confidence`).
//
// The object lives beside a resident index for a whole run.  It holds the lineage's compacted paths as a CSR (lca.hip's table), the
// leaf-bin table and the piece stager of analysis_host.h, and two 64-bit tallies per node plus ROOT and UNCLASSIFIED.  A batch brings the searcher's
// device-resident CSR -- EVERY tuple that passed the search threshold, not only the survivors of the 0.8 * max filter -- and the
// batch's saved hash lists.
//
//   k_cf_agree   one wave per read.  The read's maximum count; a read without a tuple or with maximum 0 is UNCLASSIFIED and leaves.
//                The first survivor's path is the reference (found by a walk that stops at the first round of 64 tuples that holds
//                one).  Then all tuples, 64 at a time: a lane measures how far its tuple's path agrees with the WHOLE reference path
//                and writes that as one byte; the survivors' minimum is D.  agree(t) of section 10.5 is min(byte, D): P is the
//                reference's first D nodes.  A tuple whose user bin lies outside the index gets the byte 0xFF and is reported.
//   k_cf_probe   one wave per PIECE -- at most CF_SPLIT consecutive hashes of one classified read, cut on the host.  64 hashes at a
//                time, one per lane, a = -1.  First the tuples that agree to D (the survivors among them), then the others; a tuple
//                is probed only by the lanes it could still raise (a < agree(t)), skipped when there is none, and the first walk ends
//                when a ballot says every live lane is at D.  Then one atomic add of a popcount per distinct value of a.
//   k_cf_decide  one lane per read: suffix sums of the read's D + 1 words, the deepest depth that holds, the call words, two 64-bit
//                atomic adds.
//
// The histogram is D + 1 words per classified read; the offsets are summed on the host, which has the reads' D anyway (it cuts the
// pieces of classified reads only), so no scan kernel is needed.  Integer sums do not depend on the launch geometry nor on the cut into
// pieces, staged groups and batches.  Every loop is bounded by a count the kernel is given (reads, a read's tuples, a piece's hashes,
// a user bin's leaf bins, a path's length <= LINEAGE_MAX_DEPTH).  No block waits on another.
#include "analysis_host.h"
#include "confidence_format.h"
#include "lineage.h"

#include <map>
#include <memory>

namespace {

using namespace taxor;

constexpr int CB = READ_BLOCK, CW = READ_WAVES, C_GRID_CAP = READ_GRID_CAP;
constexpr uint32_t CF_BAD = 0xFFu;                // the agree byte of a tuple whose user bin lies outside the index
constexpr int CF_WORDS = 9;                       // words per read the kernels write (n_hashes is copied beside them)

enum : uint32_t { CF_BAD_BIN = 1u };

// the per-read words, n_reads apart
struct Words {
    int32_t *node;            // the confident call
    uint32_t *depth;
    int32_t *lca_node;        // section 10.3's call
    uint32_t *lca_depth;      // D
    uint32_t *support, *lca_support, *any_support;
    uint32_t *best, *n_refs;
};

struct AgreeArgs {
    const uint64_t *off;          // the CSR; tuples are indexed from t0 (off[0] == t0)
    const int64_t *ub;
    const uint32_t *count;
    uint64_t t0;
    uint64_t n_reads, n_bins;
    const uint32_t *path_off;     // [n_bins + 1]
    const int32_t *path;
    uint8_t *agree;               // [n_tuples]
    uint32_t *ref_lo;             // [n_reads] where the reference path starts in path[]
    Words w;
    uint32_t *err;
};

__global__ __launch_bounds__(CB) void k_cf_agree(AgreeArgs a)
{
    bool bad = false;
    const uint32_t lane = lane_id();
    for (uint64_t r = (uint64_t)blockIdx.x * CW + (threadIdx.x >> 6); r < a.n_reads; r += (uint64_t)gridDim.x * CW) {
        const uint64_t lo = a.off[r], hi = a.off[r + 1];
        uint32_t mx = 0;
        for (uint64_t i = lo + lane; i < hi; i += 64) {
            const uint32_t c = a.count[i - a.t0];
            mx = c > mx ? c : mx;
        }
        mx = wave_max(mx);
        // the reference: the first survivor that names a user bin of the index
        bool have_ref = false;
        uint32_t ref_lo = 0, ref_len = 0;
        for (uint64_t base = lo; mx != 0 && !have_ref && base < hi; base += 64) {
            const uint64_t i = base + lane;
            bool k = false;
            uint32_t plo = 0, plen = 0;
            if (i < hi) {
                const int64_t b = a.ub[i - a.t0];
                if (b >= 0 && (uint64_t)b < a.n_bins && keeps(a.count[i - a.t0], mx)) {
                    k = true;
                    plo = a.path_off[b];
                    plen = a.path_off[b + 1] - plo;
                    plen = plen < LINEAGE_MAX_DEPTH ? plen : LINEAGE_MAX_DEPTH;
                }
            }
            const uint64_t m = __ballot(k);
            if (m) {
                const int src = __ffsll((long long)m) - 1;
                ref_lo = __shfl(plo, src);
                ref_len = __shfl(plen, src);
                have_ref = true;
            }
        }
        uint32_t common = ref_len, n_refs = 0;
        for (uint64_t base = lo; mx != 0 && base < hi; base += 64) {     // (mx == 0: the read leaves; its bytes are never read)
            const uint64_t i = base + lane;
            bool k = false;
            uint32_t ag = ref_len;
            if (i < hi) {
                const int64_t b = a.ub[i - a.t0];
                uint32_t byte = CF_BAD;
                if (b < 0 || (uint64_t)b >= a.n_bins) bad = true;
                else if (have_ref) {
                    const uint32_t plo = a.path_off[b];
                    uint32_t plen = a.path_off[b + 1] - plo;
                    plen = plen < LINEAGE_MAX_DEPTH ? plen : LINEAGE_MAX_DEPTH;
                    const uint32_t lim = plen < ref_len ? plen : ref_len;
                    byte = 0;
                    while (byte < lim && a.path[plo + byte] == a.path[ref_lo + byte]) ++byte;
                    k = keeps(a.count[i - a.t0], mx);
                    if (k) ag = byte;
                } else byte = 0;
                a.agree[i - a.t0] = (uint8_t)byte;
            }
            n_refs += (uint32_t)__popcll(__ballot(k));
            common = wave_min(ag);      // ag is ref_len on a lane without a survivor, and common never exceeds it
            ref_len = common;              // (later tuples are still compared over the first D nodes at least: min(byte, D) is what counts)
        }
        if (lane == 0) {
            int32_t node = TAXOR_LCA_UNCLASSIFIED;
            if (have_ref) node = common ? a.path[ref_lo + common - 1] : TAXOR_LCA_ROOT;
            a.w.lca_node[r] = node;
            a.w.lca_depth[r] = have_ref ? common : 0;
            a.w.best[r] = have_ref ? mx : 0;
            a.w.n_refs[r] = n_refs;
            a.ref_lo[r] = ref_lo;
        }
    }
    if (bad) atomicOr(a.err, CF_BAD_BIN);
}

struct ProbeArgs {
    const IxfDesc *ixf;
    const uint64_t *leaf_off;     // [n_bins + 1] user bin b's leaf technical bins are leaf[leaf_off[b] .. leaf_off[b + 1])
    const uint2 *leaf;            // (IXF, bin)
    const uint64_t *off;          // the CSR, indexed from t0
    const int64_t *ub;
    uint64_t t0;
    const uint8_t *agree;         // [n_tuples]
    const uint32_t *lca_depth;    // [n_reads] D
    const uint64_t *hist_off;     // [n_reads + 1]
    uint32_t *hist;               // D + 1 words per classified read
    const Piece *pieces;
    const uint64_t *hashes;       // the staged part of the saved lists
    uint32_t n_pieces;
    unsigned long long *counters; // lookups | tuple steps made | tuple steps a full walk would make
};

__global__ __launch_bounds__(CB) void k_cf_probe(ProbeArgs a)
{
    unsigned long long lookups = 0, steps = 0, steps_full = 0;
    const uint32_t lane = lane_id();
    for (uint64_t pi = (uint64_t)blockIdx.x * CW + (threadIdx.x >> 6); pi < a.n_pieces; pi += (uint64_t)gridDim.x * CW) {
        const Piece pc = a.pieces[pi];
        const uint64_t t0 = a.off[pc.read] - a.t0, t1 = a.off[pc.read + 1] - a.t0;
        const int D = (int)a.lca_depth[pc.read];
        uint32_t *hist = a.hist + a.hist_off[pc.read];
        for (uint32_t h0 = 0; h0 < pc.n; h0 += 64) {
            const uint32_t j = h0 + lane;
            const bool active = j < pc.n;
            const uint64_t h = active ? a.hashes[(uint64_t)pc.first + j] : 0;
            int av = -1;                                       // a(i): undefined so far
            bool all_at_d = false;
            steps_full += t1 - t0;                             // what a walk without the exit and the skip makes: every tuple once
            // the tuples that agree to D first (every survivor is one), then the others, which can only fill in below D
            for (int pass = 0; pass < 2 && !all_at_d; ++pass)
                for (uint64_t t = t0; t < t1; ++t) {
                    const uint32_t byte = a.agree[t];              // the same in every lane
                    if (byte == CF_BAD) continue;
                    const int ag = (int)byte < D ? (int)byte : D;
                    if ((ag == D) != (pass == 0)) continue;
                    const bool need = active && av < ag;
                    if (__ballot(need) == 0) continue;            // no lane this tuple could raise
                    ++steps;
                    const uint64_t b = (uint64_t)a.ub[t];
                    if (leaf_lookup<true>(a.ixf, a.leaf, a.leaf_off[b], a.leaf_off[b + 1], h, need, lookups)) av = ag;
                    if (pass == 0 && __ballot(active && av < D) == 0) {
                        all_at_d = true;
                        break;
                    }
                }
            // one add per distinct value of a among the lanes: at most D + 1 rounds
            uint64_t rem = __ballot(active && av >= 0);
            for (int it = 0; it <= D && rem; ++it) {
                const int src = __ffsll((long long)rem) - 1;
                const int v = __shfl(av, src);
                const uint64_t m = __ballot(active && av == v);
                if ((int)lane == src) atomicAdd(hist + v, (uint32_t)__popcll(m));
                rem &= ~m;
            }
        }
    }
    wave_add_to(a.counters, lookups);
    if (lane == 0 && steps_full) {                                      // the step counters are the same in every lane
        atomicAdd(a.counters + 1, steps);
        atomicAdd(a.counters + 2, steps_full);
    }
}

struct DecideArgs {
    uint64_t n_reads;
    double confidence;
    const uint32_t *n_hashes;     // [n_reads]
    const uint32_t *rlen32;       // the reads' lengths: one of the two
    const uint64_t *qlen64;
    const uint64_t *hist_off;     // [n_reads + 1]
    const uint32_t *hist;
    const uint32_t *ref_lo;       // [n_reads]
    const int32_t *path;
    uint32_t n_nodes;
    Words w;
    unsigned long long *direct_reads, *direct_bases;     // [n_nodes + 2]
};

__global__ __launch_bounds__(CB) void k_cf_decide(DecideArgs a)
{
    for (uint64_t r = (uint64_t)blockIdx.x * CB + threadIdx.x; r < a.n_reads; r += (uint64_t)gridDim.x * CB) {
        int32_t node = TAXOR_LCA_UNCLASSIFIED;
        uint32_t depth = 0, sup = 0, sup_d = 0, sup_0 = 0;
        if (a.w.lca_node[r] != TAXOR_LCA_UNCLASSIFIED) {
            const uint32_t D = a.w.lca_depth[r], n = a.n_hashes[r];
            const uint32_t *hist = a.hist + a.hist_off[r];
            uint32_t s = 0;
            bool found = false;
            for (uint32_t d = D + 1; d-- > 0;) {                  // support[d] = the hashes with a >= d; it grows as d falls
                s += hist[d];
                if (d == D) sup_d = s;
                if (!found && confidence_holds(s, a.confidence, n)) {
                    found = true;
                    depth = d;
                    sup = s;
                }
            }
            sup_0 = s;
            if (found) node = depth ? a.path[a.ref_lo[r] + depth - 1] : TAXOR_LCA_ROOT;
            else sup = sup_0;
        }
        a.w.node[r] = node;
        a.w.depth[r] = depth;
        a.w.support[r] = sup;
        a.w.lca_support[r] = sup_d;
        a.w.any_support[r] = sup_0;
        const uint32_t slot = node >= 0 ? (uint32_t)node : node == TAXOR_LCA_ROOT ? a.n_nodes : a.n_nodes + 1;
        const unsigned long long len = a.rlen32 ? (unsigned long long)a.rlen32[r] : (unsigned long long)a.qlen64[r];
        atomicAdd(a.direct_reads + slot, 1ull);
        atomicAdd(a.direct_bases + slot, len);
    }
}

#define CF_TRY(expr) TAXOR_HIP_TRY_PREFIX("confidence", expr, #expr)

// the calls of one caller (a searcher, or add_csr): the device words and work arrays, and the page-locked copy of the words
struct Slot {
    DeviceBuf<uint32_t> d_words, d_ref_lo, d_hist;
    DeviceBuf<uint64_t> d_hist_off;
    DeviceBuf<uint8_t> d_agree;
    uint32_t *h = nullptr;         // (CF_WORDS + 1) * cap words
    uint64_t *h_hist_off = nullptr;
    uint64_t cap = 0;
    ~Slot()
    {
        if (h) (void)hipHostFree(h);
        if (h_hist_off) (void)hipHostFree(h_hist_off);
    }
};

}   // namespace

struct taxor_gpu_confidence : ReadAnalysis {
    double confidence = 0;
    uint64_t n_nodes = 0, n_reads = 0;
    DeviceBuf<uint32_t> d_path_off;
    DeviceBuf<int32_t> d_path;
    DeviceBuf<unsigned long long> d_tally, d_counters;   // direct_reads | direct_bases, n_nodes + 2 each
    std::map<const void *, std::unique_ptr<Slot>> slots;
    double seconds_kernels = 0;
    std::vector<uint64_t> r_tally;
};

namespace {

// One batch whose CSR is on the object's device; the hash lists are host arrays (read r's at hashes[hash_off[r] .. hash_off[r + 1]),
// h_nh[r] of them).  The caller holds the mutex and has made every check that needs no launch.
int add_device(taxor_gpu_confidence *c, const void *who, uint64_t first_read, uint64_t n, uint64_t nt, const uint64_t *d_off, const int64_t *d_ub,
               const uint32_t *d_cnt, const uint32_t *d_nh, const uint32_t *d_rlen32, const uint64_t *d_qlen64, uint64_t t0, const uint64_t *hash_off,
               const uint64_t *hashes, const uint32_t *h_nh, taxor_confidence_calls *calls)
{
    std::unique_ptr<Slot> &sp = c->slots[who];
    if (!sp) sp = std::make_unique<Slot>();
    Slot &sl = *sp;
    if (n > sl.cap) {
        const uint64_t want = std::max<uint64_t>(n + n / 2, 1024);
        if (sl.h) (void)hipHostFree(sl.h);
        if (sl.h_hist_off) (void)hipHostFree(sl.h_hist_off);
        sl.h = nullptr;
        sl.h_hist_off = nullptr;
        sl.cap = 0;
        CF_TRY(sl.d_words.alloc(CF_WORDS * want));
        CF_TRY(sl.d_ref_lo.alloc(want));
        CF_TRY(sl.d_hist_off.alloc(want + 1));
        CF_TRY(hipHostMalloc((void **)&sl.h, (CF_WORDS + 1) * want * sizeof(uint32_t), hipHostMallocDefault));
        CF_TRY(hipHostMalloc((void **)&sl.h_hist_off, (want + 1) * sizeof(uint64_t), hipHostMallocDefault));
        sl.cap = want;
    }
    uint32_t *hw = sl.h;
    calls->n_reads = n;
    calls->first_read = first_read;
    calls->node = (const int32_t *)hw;
    calls->depth = hw + n;
    calls->lca_node = (const int32_t *)(hw + 2 * n);
    calls->lca_depth = hw + 3 * n;
    calls->support = hw + 4 * n;
    calls->lca_support = hw + 5 * n;
    calls->any_support = hw + 6 * n;
    calls->best = hw + 7 * n;
    calls->n_refs = hw + 8 * n;
    calls->n_hashes = hw + 9 * n;
    calls->seconds_kernels = 0;
    calls->probes = calls->tuple_steps = calls->tuple_steps_full = 0;
    if (int rc = c->stage.recover()) return rc;
    if (n == 0) return TAXOR_OK;
    const uint64_t n_bins = c->leaf.n_bins;
    uint32_t *dw = sl.d_words.p;
    Words w{(int32_t *)dw, dw + n, (int32_t *)(dw + 2 * n), dw + 3 * n, dw + 4 * n, dw + 5 * n, dw + 6 * n, dw + 7 * n, dw + 8 * n};

    c->timer.begin();
    auto stamp = [&]() { return c->timer.stamp(c->st); };

    CF_TRY(sl.d_agree.reserve(nt + 1, nt + 1 + nt / 2));
    CF_TRY(hipMemsetAsync(c->d_counters.p, 0, 3 * 8, c->st));
    AgreeArgs ag{};
    ag.off = d_off;
    ag.ub = d_ub;
    ag.count = d_cnt;
    ag.t0 = t0;
    ag.n_reads = n;
    ag.n_bins = n_bins;
    ag.path_off = c->d_path_off.p;
    ag.path = c->d_path.p;
    ag.agree = sl.d_agree.p;
    ag.ref_lo = sl.d_ref_lo.p;
    ag.w = w;
    ag.err = c->d_err.p;
    if (int rc = stamp()) return rc;
    k_cf_agree<<<grid_for(n, CW, C_GRID_CAP), CB, 0, c->st>>>(ag);
    CF_TRY(hipGetLastError());
    if (int rc = stamp()) return rc;
    // section 10.3's call and D come to the host: the pieces are cut from the classified reads, the histogram's offsets from their D
    CF_TRY(hipMemcpyAsync(hw + 2 * n, dw + 2 * n, 2 * n * sizeof(uint32_t), hipMemcpyDeviceToHost, c->st));
    uint32_t err = 0;
    CF_TRY(hipMemcpyAsync(&err, c->d_err.p, 4, hipMemcpyDeviceToHost, c->st));
    CF_TRY(hipStreamSynchronize(c->st));
    if (err & CF_BAD_BIN) {
        if (int rc = c->clear_err()) return rc;
        return fail(TAXOR_E_INTERNAL, "confidence_add: user_bin: a tuple names a user bin outside the lineage's %llu", (unsigned long long)n_bins);
    }
    const int32_t *h_lca = (const int32_t *)(hw + 2 * n);
    const uint32_t *h_D = hw + 3 * n;
    uint64_t words = 0;
    for (uint64_t r = 0; r < n; ++r) {
        sl.h_hist_off[r] = words;
        if (h_lca[r] != TAXOR_LCA_UNCLASSIFIED) words += (uint64_t)h_D[r] + 1;
    }
    sl.h_hist_off[n] = words;
    CF_TRY(sl.d_hist.reserve(words + 1, words + 1 + words / 2));
    CF_TRY(hipMemcpyAsync(sl.d_hist_off.p, sl.h_hist_off, (n + 1) * 8, hipMemcpyHostToDevice, c->st));
    CF_TRY(hipMemsetAsync(sl.d_hist.p, 0, (words + 1) * 4, c->st));

    ProbeArgs a{};
    a.ixf = c->leaf.d_ixf;
    a.leaf_off = c->leaf.d_off.p;
    a.leaf = c->leaf.d_leaf.p;
    a.off = d_off;
    a.ub = d_ub;
    a.t0 = t0;
    a.agree = sl.d_agree.p;
    a.lca_depth = w.lca_depth;
    a.hist_off = sl.d_hist_off.p;
    a.hist = sl.d_hist.p;
    a.counters = c->d_counters.p;
    c->stage.begin(hashes, [&](const Piece *pieces, const uint64_t *staged, uint32_t n_p) {
        a.pieces = pieces;
        a.hashes = staged;
        a.n_pieces = n_p;
        k_cf_probe<<<grid_for(n_p, CW, C_GRID_CAP), CB, 0, c->st>>>(a);
    });
    for (uint64_t r = 0; r < n; ++r)
        if (h_nh[r] != 0 && h_lca[r] != TAXOR_LCA_UNCLASSIFIED)
            if (int rc = c->stage.add(r, hash_off[r], h_nh[r])) return rc;
    if (int rc = c->stage.flush()) return rc;

    DecideArgs d{};
    d.n_reads = n;
    d.confidence = c->confidence;
    d.n_hashes = d_nh;
    d.rlen32 = d_rlen32;
    d.qlen64 = d_qlen64;
    d.hist_off = sl.d_hist_off.p;
    d.hist = sl.d_hist.p;
    d.ref_lo = sl.d_ref_lo.p;
    d.path = c->d_path.p;
    d.n_nodes = (uint32_t)c->n_nodes;
    d.w = w;
    d.direct_reads = c->d_tally.p;
    d.direct_bases = c->d_tally.p + c->n_nodes + 2;
    if (int rc = stamp()) return rc;
    k_cf_decide<<<grid_for(n, CB, C_GRID_CAP), CB, 0, c->st>>>(d);
    CF_TRY(hipGetLastError());
    if (int rc = stamp()) return rc;
    CF_TRY(hipMemcpyAsync(hw, dw, CF_WORDS * n * sizeof(uint32_t), hipMemcpyDeviceToHost, c->st));
    unsigned long long counters[3] = {0, 0, 0};
    CF_TRY(hipMemcpyAsync(counters, c->d_counters.p, 3 * 8, hipMemcpyDeviceToHost, c->st));
    CF_TRY(hipStreamSynchronize(c->st));               // the searcher's buffers and the hash lists are the caller's again
    memcpy(hw + 9 * n, h_nh, n * sizeof(uint32_t));
    c->stage.end();
    if (int rc = c->timer.add_to(&calls->seconds_kernels)) return rc;
    calls->probes = counters[0];
    calls->tuple_steps = counters[1];
    calls->tuple_steps_full = counters[2];
    c->seconds_kernels += calls->seconds_kernels;
    c->n_reads += n;
    return TAXOR_OK;
}

}   // namespace

extern "C" int taxor_gpu_confidence_create(taxor_gpu_index *idx, const taxor_hixf_view *view, const taxor_lineage *lineage, double confidence,
                                           taxor_gpu_confidence **out)
{
    if (!out) return fail(TAXOR_E_ARG, "confidence_create: null argument");
    *out = nullptr;
    if (!idx || !view || !lineage) return fail(TAXOR_E_ARG, "confidence_create: null argument");
    if (!confidence_valid(confidence)) return fail(TAXOR_E_ARG, "confidence_create: confidence: %g is not in [0, 1]", confidence);
    auto c = std::make_unique<taxor_gpu_confidence>();
    if (int rc = c->leaf.build("confidence_create", "its leaf bins are not all resident at once and a read's final tuples exist only after the last pass's merge; weighing calls pass by pass is not built", idx, view))
        return rc;
    if (int rc = c->stage.configure("confidence_create")) return rc;
    const uint64_t n_bins = c->leaf.n_bins;
    // the lineage's paths (lca.hip's table and checks)
    taxor_lineage_view v{};
    if (int rc = taxor_lineage_get_view(lineage, &v)) return rc;
    if (v.n_user_bins != n_bins)
        return fail(TAXOR_E_ARG, "confidence_create: n_user_bins: the lineage was built for %llu user bins, the index has %llu", (unsigned long long)v.n_user_bins, (unsigned long long)n_bins);
    const uint64_t n_path = v.path_off[n_bins];
    if (n_path >= (1ull << 32) || v.n_nodes >= (1ull << 31) - 2) return fail(TAXOR_E_ARG, "confidence_create: nodes and path entries are numbered in 32 bits");
    std::vector<uint32_t> off32(n_bins + 1);
    for (uint64_t b = 0; b <= n_bins; ++b) off32[b] = (uint32_t)v.path_off[b];
    for (uint64_t b = 0; b < n_bins; ++b)
        if (off32[b + 1] < off32[b] || off32[b + 1] - off32[b] > LINEAGE_MAX_DEPTH) return fail(TAXOR_E_ARG, "confidence_create: path_off: the path of user bin %llu is malformed", (unsigned long long)b);
    for (uint64_t i = 0; i < n_path; ++i)
        if (v.path[i] < 0 || (uint64_t)v.path[i] >= v.n_nodes) return fail(TAXOR_E_ARG, "confidence_create: path: entry %llu is not a node", (unsigned long long)i);
    CF_TRY(hipSetDevice(c->leaf.device));
    c->confidence = confidence;
    c->n_nodes = v.n_nodes;
    if (int rc = c->open("confidence")) return rc;
    CF_TRY(c->d_path_off.alloc(n_bins + 1));
    CF_TRY(c->d_path.alloc(n_path + 1));
    CF_TRY(c->d_tally.alloc(2 * (v.n_nodes + 2)));
    CF_TRY(c->d_counters.alloc(3));
    CF_TRY(hipMemcpy(c->d_path_off.p, off32.data(), (n_bins + 1) * 4, hipMemcpyHostToDevice));
    if (n_path) CF_TRY(hipMemcpy(c->d_path.p, v.path, n_path * 4, hipMemcpyHostToDevice));
    CF_TRY(hipMemset(c->d_tally.p, 0, 2 * (v.n_nodes + 2) * 8));
    *out = c.release();
    return TAXOR_OK;
}

extern "C" void taxor_gpu_confidence_destroy(taxor_gpu_confidence *c)
{
    if (!c) return;
    (void)hipSetDevice(c->leaf.device);
    delete c;
}

extern "C" int taxor_gpu_confidence_add_batch(taxor_gpu_confidence *c, taxor_gpu_searcher *s, const taxor_gpu_saved *saved, uint64_t first_read,
                                              taxor_confidence_calls *calls)
{
    if (!c || !s || !calls) return fail(TAXOR_E_ARG, "confidence_add_batch: null argument");
    std::unique_lock<std::mutex> lk;
    SearcherBatch b;
    if (int rc = begin_batch("confidence_add_batch", "confidence", "the confidence object", *c, s, saved, lk, &b)) return rc;
    const uint32_t *d_rlen = nullptr;
    if (int rc = taxor_searcher_device_read_lengths(s, &d_rlen)) return rc;
    return add_device(c, s, first_read, b.n, b.nt, b.d_off, b.d_ub, b.d_cnt, b.d_nh, d_rlen, nullptr, 0, saved->hash_off.data(), saved->hashes, c->h_nh.data(), calls);
}

extern "C" int taxor_gpu_confidence_add_csr(taxor_gpu_confidence *c, uint64_t n_reads, const uint64_t *read_off, const int64_t *user_bin, const uint32_t *count,
                                            const uint64_t *query_len, const uint64_t *hash_off, const uint64_t *hashes, taxor_confidence_calls *calls)
{
    if (!c || !read_off || !hash_off || !calls) return fail(TAXOR_E_ARG, "confidence_add_csr: null argument");
    if (n_reads && !query_len) return fail(TAXOR_E_ARG, "confidence_add_csr: query_len: null array");
    CsrUpload &u = c->csr;
    std::lock_guard<std::mutex> lk(c->mu);
    if (int rc = u.check("confidence_add_csr", "lineage", c->leaf.n_bins, n_reads, read_off, user_bin, count, hash_off, hashes)) return rc;
    CF_TRY(hipSetDevice(c->leaf.device));
    if (int rc = u.upload("confidence", n_reads, read_off, user_bin, count, hash_off, query_len, &c->h_nh)) return rc;
    return add_device(c, nullptr, 0, n_reads, u.nt, u.off.p, u.ub.p, u.cnt.p, u.nh.p, nullptr, u.qlen.p, u.t0, hash_off, hashes, c->h_nh.data(), calls);
}

extern "C" int taxor_gpu_confidence_results(taxor_gpu_confidence *c, taxor_lca_results *out)
{
    if (!c || !out) return fail(TAXOR_E_ARG, "confidence_results: null argument");
    std::lock_guard<std::mutex> lk(c->mu);
    CF_TRY(hipSetDevice(c->leaf.device));
    const uint64_t n = c->n_nodes + 2;
    c->r_tally.resize(2 * n);
    CF_TRY(hipMemcpy(c->r_tally.data(), c->d_tally.p, 2 * n * 8, hipMemcpyDeviceToHost));
    out->n_nodes = c->n_nodes;
    out->direct_reads = c->r_tally.data();
    out->direct_bases = c->r_tally.data() + n;
    out->n_reads = c->n_reads;
    out->seconds_kernel = c->seconds_kernels;
    return TAXOR_OK;
}
