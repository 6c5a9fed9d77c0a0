// lca.hip -- per-read lowest common ancestor and per-taxon tallies (`taxor search --lca-file / --report-file`).
//
// An accumulator lives beside a resident index for a whole run.  It holds the lineage's compacted paths (lineage.h) as a CSR on the
// device and two 64-bit tallies per node, plus ROOT and UNCLASSIFIED.  A batch is the searcher's device-resident CSR (the buffers
// taxor_gpu_batch_export_device copies from, read where they lie) and the reads' lengths, or host arrays (tests).
//
//   k_lca   one wave per read, four reads per block, grid-stride (the convention of profile_feed.hip).  Pass 1: the read's maximum
//           count, lanes over the tuples 64 at a time.  A read without a tuple or with maximum 0 is UNCLASSIFIED and leaves here: the
//           thousands of zero-count tuples of a read without a hash cost this one pass.  Pass 2: the tuples again, 64 at a time; the
//           first survivor's path (the lowest surviving lane of the first round that has one) is the reference, broadcast to the
//           wave; every surviving lane measures how far its path agrees with the reference -- never further than the agreement found
//           so far -- and a wave minimum carries that across the rounds.  Lane 0 writes node / best / n_refs and makes the two
//           64-bit atomic adds.
//
// Most reads have one to five tuples, so most lanes of a wave idle; the kernel is a small share of a batch all the same
// (docs/EXPERIMENTS.md, "Per-read LCA and report"), which is why the simple shape shipped and not groups of 16 lanes per read.
// Every loop is bounded by a count the kernel is given (the reads, a read's tuples, a path's length <= LINEAGE_MAX_DEPTH).  No block
// waits on another.  Integer sums are order-free: the result does not depend on the launch geometry or on the order of the batches.
#include "analysis_host.h"
#include "lineage.h"

#include <map>
#include <memory>

namespace {

using namespace taxor;

constexpr int LB = READ_BLOCK, LW = READ_WAVES;
constexpr int L_GRID_CAP = 2048;

enum : uint32_t { LCA_BAD_BIN = 1u };

struct LcaArgs {
    const uint64_t *off;          // the CSR; tuples are indexed from t0 (off[0] == t0)
    const int64_t *ub;
    const uint32_t *count;
    uint64_t t0;
    const uint32_t *rlen32;       // the reads' lengths: one of the two
    const uint64_t *qlen64;
    uint64_t n_reads, n_bins;
    const uint32_t *path_off;     // [n_bins + 1]
    const int32_t *path;
    uint32_t n_nodes;
    int32_t *o_node;              // [n_reads] each
    uint32_t *o_best, *o_refs;
    unsigned long long *direct_reads, *direct_bases;     // [n_nodes + 2]
    uint32_t *err;
};

__global__ __launch_bounds__(LB) void k_lca(LcaArgs a)
{
    bool bad = false;
    for (uint64_t r = (uint64_t)blockIdx.x * LW + (threadIdx.x >> 6); r < a.n_reads; r += (uint64_t)gridDim.x * LW) {
        const uint64_t lo = a.off[r], hi = a.off[r + 1];
        uint32_t mx = 0;
        for (uint64_t i = lo + lane_id(); i < hi; i += 64) {
            const uint32_t c = a.count[i - a.t0];
            mx = c > mx ? c : mx;
        }
        mx = wave_max(mx);
        int32_t node = TAXOR_LCA_UNCLASSIFIED;
        uint32_t n_refs = 0;
        if (mx != 0) {
            bool have_ref = false;
            uint32_t ref_lo = 0, common = 0;
            for (uint64_t base = lo; base < hi; base += 64) {
                const uint64_t i = base + lane_id();
                bool k = false;
                uint32_t plo = 0, plen = 0;
                if (i < hi) {
                    const int64_t b = a.ub[i - a.t0];
                    if (b < 0 || (uint64_t)b >= a.n_bins) bad = true;
                    else if (keeps(a.count[i - a.t0], mx)) {
                        k = true;
                        plo = a.path_off[b];
                        plen = a.path_off[b + 1] - plo;
                        plen = plen < LINEAGE_MAX_DEPTH ? plen : LINEAGE_MAX_DEPTH;
                    }
                }
                const uint64_t m = __ballot(k);
                if (m == 0) continue;
                n_refs += (uint32_t)__popcll(m);
                if (!have_ref) {                                  // the first survivor's path is the reference
                    const int src = __ffsll((long long)m) - 1;
                    ref_lo = __shfl(plo, src);
                    common = __shfl(plen, src);
                    have_ref = true;
                }
                uint32_t agree = common;
                if (k) {
                    const uint32_t lim = plen < common ? plen : common;
                    agree = 0;
                    while (agree < lim && a.path[plo + agree] == a.path[ref_lo + agree]) ++agree;
                }
                common = wave_min(agree);
            }
            if (have_ref) node = common ? a.path[ref_lo + common - 1] : TAXOR_LCA_ROOT;
            else mx = 0;                                           // (only tuples with a user bin outside the table: reported through err)
        }
        if (lane_id() == 0) {
            a.o_node[r] = node;
            a.o_best[r] = mx;
            a.o_refs[r] = n_refs;
            const uint32_t slot = node >= 0 ? (uint32_t)node : node == TAXOR_LCA_ROOT ? a.n_nodes : a.n_nodes + 1;
            const unsigned long long len = a.rlen32 ? (unsigned long long)a.rlen32[r] : (unsigned long long)a.qlen64[r];
            atomicAdd(a.direct_reads + slot, 1ull);
            atomicAdd(a.direct_bases + slot, len);
        }
    }
    if (bad) atomicOr(a.err, LCA_BAD_BIN);
}

#define LCA_TRY(expr) TAXOR_HIP_TRY_PREFIX("lca", expr, #expr)

// the calls of one caller (a searcher, or add_csr): device words and their page-locked copy, node | best | n_refs | n_hashes
struct Slot {
    DeviceBuf<uint32_t> d;
    uint32_t *h = nullptr;
    uint64_t cap = 0;
    ~Slot()
    {
        if (h) (void)hipHostFree(h);
    }
};

}   // namespace

struct taxor_gpu_lca {
    taxor_gpu_index *idx = nullptr;
    int device = 0;
    uint64_t n_bins = 0, n_nodes = 0, n_reads = 0;
    hipStream_t st = nullptr;
    LaunchTimer timer;
    std::mutex mu;                                    // batches may come from several threads
    DeviceBuf<uint32_t> d_path_off, d_err;
    DeviceBuf<int32_t> d_path;
    DeviceBuf<unsigned long long> d_tally;            // direct_reads | direct_bases, n_nodes + 2 each
    std::map<const void *, std::unique_ptr<Slot>> slots;
    CsrUpload csr;                                    // the host arrays of add_csr on the device
    double seconds_kernel = 0;
    std::vector<uint64_t> r_tally;
    ~taxor_gpu_lca()
    {
        slots.clear();
        if (st) (void)hipStreamDestroy(st);
    }
};

namespace {

// one batch whose arrays are on the accumulator's device; the caller holds the mutex.  d_nh may be null
int add_device(taxor_gpu_lca *c, const void *who, uint64_t first_read, uint64_t n, const uint64_t *d_off, const int64_t *d_ub, const uint32_t *d_cnt,
               const uint32_t *d_nh, const uint32_t *d_rlen32, const uint64_t *d_qlen64, uint64_t t0, taxor_lca_calls *calls)
{
    std::unique_ptr<Slot> &sp = c->slots[who];
    if (!sp) sp = std::make_unique<Slot>();
    Slot &sl = *sp;
    if (n > sl.cap) {
        const uint64_t want = std::max<uint64_t>(n + n / 2, 1024);
        if (sl.h) (void)hipHostFree(sl.h);
        sl.h = nullptr;
        sl.cap = 0;
        LCA_TRY(sl.d.alloc(4 * want));
        LCA_TRY(hipHostMalloc((void **)&sl.h, 4 * want * sizeof(uint32_t), hipHostMallocDefault));
        sl.cap = want;
    }
    calls->n_reads = n;
    calls->first_read = first_read;
    calls->node = (const int32_t *)sl.h;
    calls->best = sl.h + n;
    calls->n_refs = sl.h + 2 * n;
    calls->n_hashes = d_nh ? sl.h + 3 * n : nullptr;
    if (n == 0) return TAXOR_OK;
    LcaArgs a{};
    a.off = d_off;
    a.ub = d_ub;
    a.count = d_cnt;
    a.t0 = t0;
    a.rlen32 = d_rlen32;
    a.qlen64 = d_qlen64;
    a.n_reads = n;
    a.n_bins = c->n_bins;
    a.path_off = c->d_path_off.p;
    a.path = c->d_path.p;
    a.n_nodes = (uint32_t)c->n_nodes;
    a.o_node = (int32_t *)sl.d.p;
    a.o_best = sl.d.p + n;
    a.o_refs = sl.d.p + 2 * n;
    a.direct_reads = c->d_tally.p;
    a.direct_bases = c->d_tally.p + c->n_nodes + 2;
    a.err = c->d_err.p;
    c->timer.begin();
    if (int rc = c->timer.stamp(c->st)) return rc;
    k_lca<<<grid_for(n, LW, L_GRID_CAP), LB, 0, c->st>>>(a);
    LCA_TRY(hipGetLastError());
    if (int rc = c->timer.stamp(c->st)) return rc;
    uint32_t err = 0;
    LCA_TRY(hipMemcpyAsync(sl.h, sl.d.p, 3 * n * sizeof(uint32_t), hipMemcpyDeviceToHost, c->st));
    if (d_nh) LCA_TRY(hipMemcpyAsync(sl.h + 3 * n, d_nh, n * sizeof(uint32_t), hipMemcpyDeviceToHost, c->st));
    LCA_TRY(hipMemcpyAsync(&err, c->d_err.p, 4, hipMemcpyDeviceToHost, c->st));
    LCA_TRY(hipStreamSynchronize(c->st));             // the caller's buffers (a searcher's results) may be reused from here on
    if (int rc = c->timer.add_to(&c->seconds_kernel)) return rc;
    c->n_reads += n;
    if (err & LCA_BAD_BIN) return fail(TAXOR_E_INTERNAL, "lca_add: user_bin: a tuple names a user bin outside the lineage's %llu", (unsigned long long)c->n_bins);
    return TAXOR_OK;
}

}   // namespace

extern "C" int taxor_gpu_lca_create(taxor_gpu_index *idx, const taxor_lineage *lineage, taxor_gpu_lca **out)
{
    if (!out) return fail(TAXOR_E_ARG, "lca_create: null argument");
    *out = nullptr;
    if (!idx || !lineage) return fail(TAXOR_E_ARG, "lca_create: null argument");
    const IxfDesc *d_ixf = nullptr, *h_ixf = nullptr;
    uint64_t n_ixf = 0, n_bins = 0;
    uint32_t n_passes = 0;
    int device = 0;
    if (taxor_index_descs(idx, &d_ixf, &h_ixf, &n_ixf, &n_bins, &n_passes, &device)) return fail(TAXOR_E_ARG, "lca_create: null index");
    if (n_passes)
        return fail(TAXOR_E_ARG, "lca_create: a paged index (%u resident pass%s) is refused: a read's final tuples exist only after the last pass's merge, and calling reads there is not built",
                    n_passes, n_passes == 1 ? "" : "es");
    taxor_lineage_view v{};
    if (int rc = taxor_lineage_get_view(lineage, &v)) return rc;
    if (v.n_user_bins != n_bins)
        return fail(TAXOR_E_ARG, "lca_create: n_user_bins: the lineage was built for %llu user bins, the index has %llu", (unsigned long long)v.n_user_bins, (unsigned long long)n_bins);
    const uint64_t n_path = v.path_off[n_bins];
    if (n_path >= (1ull << 32) || v.n_nodes >= (1ull << 31) - 2) return fail(TAXOR_E_ARG, "lca_create: nodes and path entries are numbered in 32 bits");
    std::vector<uint32_t> off32(n_bins + 1);
    for (uint64_t b = 0; b <= n_bins; ++b) off32[b] = (uint32_t)v.path_off[b];
    for (uint64_t b = 0; b < n_bins; ++b)
        if (off32[b + 1] < off32[b] || off32[b + 1] - off32[b] > LINEAGE_MAX_DEPTH) return fail(TAXOR_E_ARG, "lca_create: path_off: the path of user bin %llu is malformed", (unsigned long long)b);
    for (uint64_t i = 0; i < n_path; ++i)
        if (v.path[i] < 0 || (uint64_t)v.path[i] >= v.n_nodes) return fail(TAXOR_E_ARG, "lca_create: path: entry %llu is not a node", (unsigned long long)i);
    LCA_TRY(hipSetDevice(device));
    auto c = std::make_unique<taxor_gpu_lca>();
    c->idx = idx;
    c->device = device;
    c->n_bins = n_bins;
    c->n_nodes = v.n_nodes;
    c->timer.name = "lca";
    LCA_TRY(hipStreamCreate(&c->st));
    LCA_TRY(c->d_path_off.alloc(n_bins + 1));
    LCA_TRY(c->d_path.alloc(n_path + 1));
    LCA_TRY(c->d_tally.alloc(2 * (v.n_nodes + 2)));
    LCA_TRY(c->d_err.alloc(1));
    LCA_TRY(hipMemcpy(c->d_path_off.p, off32.data(), (n_bins + 1) * 4, hipMemcpyHostToDevice));
    if (n_path) LCA_TRY(hipMemcpy(c->d_path.p, v.path, n_path * 4, hipMemcpyHostToDevice));
    LCA_TRY(hipMemset(c->d_tally.p, 0, 2 * (v.n_nodes + 2) * 8));
    LCA_TRY(hipMemset(c->d_err.p, 0, 4));
    *out = c.release();
    return TAXOR_OK;
}

extern "C" void taxor_gpu_lca_destroy(taxor_gpu_lca *c)
{
    if (!c) return;
    (void)hipSetDevice(c->device);
    delete c;
}

extern "C" int taxor_gpu_lca_add_batch(taxor_gpu_lca *c, taxor_gpu_searcher *s, uint64_t first_read, taxor_lca_calls *calls)
{
    if (!c || !s || !calls) return fail(TAXOR_E_ARG, "lca_add_batch: null argument");
    if (taxor_searcher_index(s) != c->idx) return fail(TAXOR_E_ARG, "lca_add_batch: index: the searcher works on another index than the accumulator");
    const uint64_t *d_off = nullptr;
    const int64_t *d_ub = nullptr;
    const uint32_t *d_cnt = nullptr, *d_nh = nullptr, *d_rlen = nullptr;
    uint64_t n = 0, nt = 0;
    int dev = 0;
    if (int rc = taxor_searcher_device_results(s, &d_off, &d_ub, &d_cnt, &d_nh, &n, &nt, &dev)) return rc;
    if (int rc = taxor_searcher_device_read_lengths(s, &d_rlen)) return rc;
    if (n >= MAX_READS) return fail(TAXOR_E_ARG, "lca_add_batch: n_reads: a batch of 2^31 reads or more");
    std::lock_guard<std::mutex> lk(c->mu);
    LCA_TRY(hipSetDevice(c->device));
    return add_device(c, s, first_read, n, d_off, d_ub, d_cnt, d_nh, d_rlen, nullptr, 0, calls);
}

extern "C" int taxor_gpu_lca_add_csr(taxor_gpu_lca *c, uint64_t n_reads, const uint64_t *read_off, const int64_t *user_bin, const uint32_t *count,
                                     const uint64_t *query_len, taxor_lca_calls *calls)
{
    if (!c || !read_off || !calls) return fail(TAXOR_E_ARG, "lca_add_csr: null argument");
    if (n_reads && !query_len) return fail(TAXOR_E_ARG, "lca_add_csr: query_len: null array");
    CsrUpload &u = c->csr;
    std::lock_guard<std::mutex> lk(c->mu);
    if (int rc = u.check("lca_add_csr", "lineage", c->n_bins, n_reads, read_off, user_bin, count, nullptr, nullptr)) return rc;
    LCA_TRY(hipSetDevice(c->device));
    if (int rc = u.upload("lca", n_reads, read_off, user_bin, count, nullptr, query_len, nullptr)) return rc;
    return add_device(c, nullptr, 0, n_reads, u.off.p, u.ub.p, u.cnt.p, nullptr, nullptr, u.qlen.p, u.t0, calls);
}

extern "C" int taxor_gpu_lca_results(taxor_gpu_lca *c, taxor_lca_results *out)
{
    if (!c || !out) return fail(TAXOR_E_ARG, "lca_results: null argument");
    std::lock_guard<std::mutex> lk(c->mu);
    LCA_TRY(hipSetDevice(c->device));
    const uint64_t n = c->n_nodes + 2;
    c->r_tally.resize(2 * n);
    LCA_TRY(hipMemcpy(c->r_tally.data(), c->d_tally.p, 2 * n * 8, hipMemcpyDeviceToHost));
    out->n_nodes = c->n_nodes;
    out->direct_reads = c->r_tally.data();
    out->direct_bases = c->r_tally.data() + n;
    out->n_reads = c->n_reads;
    out->seconds_kernel = c->seconds_kernel;
    return TAXOR_OK;
}
