// analysis_host.h -- what the per-read analyses share on the host (coverage, lca, confidence, hitmap, breakpoint, segments, exclusive;
// DESIGN.md section 10.10): api.hip's hidden entry points, the leaf-bin table, the piece stager, the launch timer, and the checks and
// uploads of the two batch entry points.  Every function takes the feature's name and puts it in front of its messages.
#pragma once
#include "../../include/taxor_gpu_tools.h"
#include "hip_host.h"
#include "read_probe.h"
#include "saved_batch.h"
#include "tuning.h"

#include <hip/hip_runtime.h>

#include <functional>
#include <mutex>
#include <string>
#include <vector>

// api.hip: the device-resident CSR of a searcher's last run (synchronises it), the reads' lengths in input order, the searcher's
// index, an index's IXF descriptors
extern "C" __attribute__((visibility("hidden"))) int taxor_searcher_device_results(taxor_gpu_searcher *s, const uint64_t **d_read_off,
                                                                                   const int64_t **d_user_bin, const uint32_t **d_count,
                                                                                   const uint32_t **d_n_hashes, uint64_t *n_reads,
                                                                                   uint64_t *n_tuples, int *device);
extern "C" __attribute__((visibility("hidden"))) int taxor_searcher_device_read_lengths(taxor_gpu_searcher *s, const uint32_t **d_rlen);
extern "C" __attribute__((visibility("hidden"))) taxor_gpu_index *taxor_searcher_index(taxor_gpu_searcher *s);
extern "C" __attribute__((visibility("hidden"))) int taxor_index_descs(const taxor_gpu_index *idx, const taxor::IxfDesc **d_ixf, const taxor::IxfDesc **h_ixf,
                                                                       uint64_t *n_ixf, uint64_t *n_user_bins, uint32_t *n_passes, int *device);

namespace taxor {

constexpr int READ_GRID_CAP = 4096;
constexpr uint64_t MAX_READS = 1ull << 31;
constexpr uint64_t STAGE_HASHES = 1ull << 22;     // hashes per staging buffer (32 MiB); there are two
constexpr uint64_t STAGE_PIECES = 1ull << 18;     // pieces per staging buffer (4 MiB); there are two

// "<name>: <expr>: <hip error>", TAXOR_HIP_TRY_PREFIX's shape with a prefix known at run time
#define ANALYSIS_TRY(name, expr)                                                                                                        \
    do {                                                                                                                                \
        const hipError_t e_ = (expr);                                                                                                   \
        if (e_ != hipSuccess) return ::taxor::fail(TAXOR_E_HIP, std::string(name) + ": " #expr ": " + hipGetErrorString(e_));           \
    } while (0)

// Events on a stream: the launches of one call are timed between pairs of them.  The events are kept from call to call
struct LaunchTimer {
    const char *name = "";
    std::vector<hipEvent_t> ev;
    size_t n = 0;
    ~LaunchTimer()
    {
        for (hipEvent_t e : ev) (void)hipEventDestroy(e);
    }
    void begin() { n = 0; }
    int stamp(hipStream_t st)
    {
        if (ev.size() <= n) {
            hipEvent_t e = nullptr;
            ANALYSIS_TRY(name, hipEventCreate(&e));
            ev.push_back(e);
        }
        ANALYSIS_TRY(name, hipEventRecord(ev[n++], st));
        return TAXOR_OK;
    }
    // after the stream was synchronised: the seconds between the pairs since begin(), added to *seconds
    int add_to(double *seconds)
    {
        for (size_t i = 0; i + 1 < n; i += 2) {
            float ms = 0;
            ANALYSIS_TRY(name, hipEventElapsedTime(&ms, ev[i], ev[i + 1]));
            *seconds += (double)ms * 1e-3;
        }
        n = 0;
        return TAXOR_OK;
    }
};

// The inverse of fname_idx: every leaf technical bin of a user bin, root included, as one CSR in index order
struct LeafTable {
    taxor_gpu_index *idx = nullptr;
    int device = 0;
    uint64_t n_bins = 0;
    const IxfDesc *d_ixf = nullptr;
    std::vector<uint64_t> h_off;                      // host copies: gone after upload()
    std::vector<uint2> h_leaf;
    DeviceBuf<uint64_t> d_off;                        // [n_bins + 1] user bin b's leaf bins are d_leaf[d_off[b] .. d_off[b + 1])
    DeviceBuf<uint2> d_leaf;                          // (IXF, bin)

    // fn: "<feature>_create".  paged_why: what follows "is refused: " when the index is searched in resident passes
    int build(const char *fn, const char *paged_why, taxor_gpu_index *index, const taxor_hixf_view *view)
    {
        const IxfDesc *h_ixf = nullptr;
        uint64_t n_ixf = 0;
        uint32_t n_passes = 0;
        if (taxor_index_descs(index, &d_ixf, &h_ixf, &n_ixf, &n_bins, &n_passes, &device)) return fail(TAXOR_E_ARG, "%s: null index", fn);
        if (n_passes) return fail(TAXOR_E_ARG, "%s: a paged index (%u resident pass%s) is refused: %s", fn, n_passes, n_passes == 1 ? "" : "es", paged_why);
        if (view->n_ixf != n_ixf || view->n_user_bins != n_bins || (n_ixf && !view->ixf))
            return fail(TAXOR_E_ARG, "%s: the view (%llu IXFs, %llu user bins) is not the index's (%llu IXFs, %llu user bins)", fn, (unsigned long long)view->n_ixf,
                        (unsigned long long)view->n_user_bins, (unsigned long long)n_ixf, (unsigned long long)n_bins);
        if (n_bins >= (1ull << 32) || n_ixf >= (1ull << 32)) return fail(TAXOR_E_ARG, "%s: user bins and IXFs are numbered in 32 bits", fn);
        h_off.assign(n_bins + 1, 0);
        for (uint64_t x = 0; x < n_ixf; ++x) {
            const taxor_ixf_view &f = view->ixf[x];
            if (f.bins != h_ixf[x].bins)
                return fail(TAXOR_E_ARG, "%s: IXF %llu has %llu bins in the view, %u in the index", fn, (unsigned long long)x, (unsigned long long)f.bins, h_ixf[x].bins);
            if (!f.fname_idx) return fail(TAXOR_E_ARG, "%s: IXF %llu of the view has no fname_idx", fn, (unsigned long long)x);
            for (uint64_t j = 0; j < f.bins; ++j) {
                const int64_t b = f.fname_idx[j];
                if (b < 0) continue;
                if ((uint64_t)b >= n_bins)
                    return fail(TAXOR_E_ARG, "%s: bin %llu of IXF %llu names user bin %lld of %llu", fn, (unsigned long long)j, (unsigned long long)x, (long long)b,
                                (unsigned long long)n_bins);
                ++h_off[(uint64_t)b + 1];
            }
        }
        for (uint64_t b = 0; b < n_bins; ++b) h_off[b + 1] += h_off[b];
        h_leaf.resize(h_off[n_bins]);
        std::vector<uint64_t> at(h_off.begin(), h_off.end() - 1);
        for (uint64_t x = 0; x < n_ixf; ++x)
            for (uint64_t j = 0; j < view->ixf[x].bins; ++j) {
                const int64_t b = view->ixf[x].fname_idx[j];
                if (b >= 0) h_leaf[at[(uint64_t)b]++] = make_uint2((uint32_t)x, (uint32_t)j);
            }
        idx = index;
        return TAXOR_OK;
    }
    uint64_t device_bytes() const { return (n_bins + 1) * 8 + h_leaf.size() * 8; }
    int upload(const char *name)
    {
        ANALYSIS_TRY(name, d_off.alloc(n_bins + 1));
        ANALYSIS_TRY(name, d_leaf.alloc(h_leaf.size() + 1));
        ANALYSIS_TRY(name, hipMemcpy(d_off.p, h_off.data(), (n_bins + 1) * 8, hipMemcpyHostToDevice));
        if (!h_leaf.empty()) ANALYSIS_TRY(name, hipMemcpy(d_leaf.p, h_leaf.data(), h_leaf.size() * 8, hipMemcpyHostToDevice));
        std::vector<uint64_t>().swap(h_off);
        std::vector<uint2>().swap(h_leaf);
        return TAXOR_OK;
    }
};

// Pieces are staged and launched in bounded sets: at most cap_pieces pieces whose hashes lie within cap_hashes consecutive entries of
// the dense host array, copied as one range (lists that lie between two pieces of a set travel with it; those in front of its first
// piece do not).  Two buffers of each kind: the host cuts a set while the set before it is copied and probed.
struct PieceStager {
    const char *name = "";
    hipStream_t st = nullptr;
    LaunchTimer *timer = nullptr;
    uint64_t cap_hashes = STAGE_HASHES, cap_pieces = STAGE_PIECES;
    DeviceBuf<uint64_t> d_hashes[2];
    DeviceBuf<Piece> d_pieces[2];
    Piece *h_pieces[2] = {nullptr, nullptr};          // page-locked; ev_free[i] says that buffer i's copy has left it
    hipEvent_t ev_free[2] = {nullptr, nullptr};
    bool ev_used[2] = {false, false};
    // one call's
    using Launch = std::function<void(const Piece *d_pieces, const uint64_t *d_hashes, uint32_t n_pieces)>;
    Launch launch;
    const uint64_t *hashes = nullptr;
    int buf = 0;
    uint32_t n_p = 0;
    uint64_t g0 = 0, g1 = 0;                          // the set's hashes: [g0, g1) of hashes

    ~PieceStager()
    {
        for (int i = 0; i < 2; ++i) {
            if (h_pieces[i]) (void)hipHostFree(h_pieces[i]);
            if (ev_free[i]) (void)hipEventDestroy(ev_free[i]);
        }
    }
    // the measurement knobs (tuning.h) TAXOR_STAGE_HASHES and TAXOR_STAGE_PIECES: they move the cut into sets, never a result
    int configure(const char *fn)
    {
        if (const char *e = tune_env("TAXOR_STAGE_HASHES")) {
            const long long v = atoll(e);
            if (v < (long long)READ_SPLIT || v > (1ll << 31))
                return fail(TAXOR_E_ARG, "%s: TAXOR_STAGE_HASHES: %lld is outside [%u, 2^31] (a staging buffer holds one piece at least)", fn, v, READ_SPLIT);
            cap_hashes = (uint64_t)v;
        }
        if (const char *e = tune_env("TAXOR_STAGE_PIECES")) {
            const long long v = atoll(e);
            if (v < 1 || v > (1ll << 31)) return fail(TAXOR_E_ARG, "%s: TAXOR_STAGE_PIECES: %lld is outside [1, 2^31]", fn, v);
            cap_pieces = (uint64_t)v;
        }
        return TAXOR_OK;
    }
    uint64_t device_bytes() const { return 2 * (cap_hashes * 8 + cap_pieces * sizeof(Piece)); }
    int alloc(const char *feature, hipStream_t stream, LaunchTimer *t)
    {
        name = feature;
        st = stream;
        timer = t;
        for (int i = 0; i < 2; ++i) {
            ANALYSIS_TRY(name, d_hashes[i].alloc(cap_hashes));
            ANALYSIS_TRY(name, d_pieces[i].alloc(cap_pieces));
            ANALYSIS_TRY(name, hipHostMalloc((void **)&h_pieces[i], cap_pieces * sizeof(Piece), hipHostMallocDefault));
            ANALYSIS_TRY(name, hipEventCreateWithFlags(&ev_free[i], hipEventDisableTiming));
        }
        return TAXOR_OK;
    }
    // a call that failed half-way: its copies out of the page-locked pieces end first
    int recover()
    {
        if (ev_used[0] || ev_used[1]) ANALYSIS_TRY(name, hipStreamSynchronize(st));
        synced();
        return TAXOR_OK;
    }
    // the caller has synchronised the stream
    void synced() { ev_used[0] = ev_used[1] = false; }
    // ... for the last time in this call: the launch, which refers to the caller's locals, goes with it
    void end()
    {
        synced();
        launch = nullptr;
    }
    // host_hashes: the dense array the reads' offsets point into.  l launches the probe of one set on the stream
    void begin(const uint64_t *host_hashes, Launch l)
    {
        hashes = host_hashes;
        launch = std::move(l);
        buf = 0;
        n_p = 0;
        g0 = g1 = 0;
    }
    // the n_hashes hashes of `read` at hashes[hash_off ..]: pieces of READ_SPLIT, the last one shorter; a read without a hash is one
    // empty piece.  A set that is full is launched first
    int add(uint64_t read, uint64_t hash_off, uint64_t n_hashes)
    {
        uint64_t done = 0;
        do {
            const uint32_t take = (uint32_t)std::min<uint64_t>(READ_SPLIT, n_hashes - done);
            if (n_p && (n_p == cap_pieces || hash_off + done + take - g0 > cap_hashes))
                if (int rc = flush()) return rc;
            if (n_p == 0) g0 = hash_off + done;
            h_pieces[buf][n_p++] = Piece{(uint32_t)read, (uint32_t)(hash_off + done - g0), take, (uint32_t)done};
            done += take;
            g1 = hash_off + done;
        } while (done < n_hashes);
        return TAXOR_OK;
    }
    // copy and launch what has been cut
    int flush()
    {
        if (n_p == 0) return TAXOR_OK;
        if (g1 > g0) ANALYSIS_TRY(name, hipMemcpyAsync(d_hashes[buf].p, hashes + g0, (g1 - g0) * 8, hipMemcpyHostToDevice, st));
        ANALYSIS_TRY(name, hipMemcpyAsync(d_pieces[buf].p, h_pieces[buf], (uint64_t)n_p * sizeof(Piece), hipMemcpyHostToDevice, st));
        ANALYSIS_TRY(name, hipEventRecord(ev_free[buf], st));
        ev_used[buf] = true;
        if (int rc = timer->stamp(st)) return rc;
        launch(d_pieces[buf].p, d_hashes[buf].p, n_p);
        ANALYSIS_TRY(name, hipGetLastError());
        if (int rc = timer->stamp(st)) return rc;
        buf ^= 1;
        n_p = 0;
        if (ev_used[buf]) ANALYSIS_TRY(name, hipEventSynchronize(ev_free[buf]));     // the page-locked pieces of two sets ago have been copied
        return TAXOR_OK;
    }
};

// The host arrays of <feature>_add_csr: checked, then copied to the device.  hash_off and query_len may be null (an analysis without
// hash lists, without read lengths)
struct CsrUpload {
    DeviceBuf<uint64_t> off, qlen;
    DeviceBuf<int64_t> ub;
    DeviceBuf<uint32_t> cnt, nh;
    uint64_t t0 = 0, nt = 0;                          // the tuples are indexed from t0 = read_off[0]

    // owner: who numbers the user bins ("index", "lineage").  Needs no device, but the object's lock: t0 and nt are written
    int check(const char *fn, const char *owner, uint64_t n_bins, uint64_t n_reads, const uint64_t *read_off, const int64_t *user_bin, const uint32_t *count,
              const uint64_t *hash_off, const uint64_t *hashes)
    {
        if (n_reads >= MAX_READS) return fail(TAXOR_E_ARG, "%s: n_reads: 2^31 reads or more", fn);
        for (uint64_t r = 0; r < n_reads; ++r) {
            if (read_off[r + 1] < read_off[r] || read_off[r + 1] - read_off[r] >= (1ull << 32))
                return fail(TAXOR_E_ARG, "%s: read_off: the tuples of read %llu are malformed", fn, (unsigned long long)r);
            if (hash_off && (hash_off[r + 1] < hash_off[r] || hash_off[r + 1] - hash_off[r] >= (1ull << 32)))
                return fail(TAXOR_E_ARG, "%s: hash_off: the list of read %llu is malformed", fn, (unsigned long long)r);
        }
        t0 = read_off[0];
        nt = read_off[n_reads] - t0;
        if (nt && (!user_bin || !count)) return fail(TAXOR_E_ARG, "%s: user_bin / count: null array", fn);
        if (hash_off && hash_off[n_reads] > hash_off[0] && !hashes) return fail(TAXOR_E_ARG, "%s: hashes: null array", fn);
        for (uint64_t i = t0; i < t0 + nt; ++i)
            if (user_bin[i] < 0 || (uint64_t)user_bin[i] >= n_bins)
                return fail(TAXOR_E_ARG, "%s: user_bin: tuple %llu names user bin %lld, the %s has %llu", fn, (unsigned long long)i, (long long)user_bin[i], owner,
                            (unsigned long long)n_bins);
        return TAXOR_OK;
    }
    // under the lock, on the object's device.  With hash_off the reads' hash counts go to *h_nh and to nh
    int upload(const char *name, uint64_t n_reads, const uint64_t *read_off, const int64_t *user_bin, const uint32_t *count, const uint64_t *hash_off,
               const uint64_t *query_len, std::vector<uint32_t> *h_nh)
    {
        ANALYSIS_TRY(name, off.reserve(n_reads + 1, n_reads + 1 + n_reads / 2));
        ANALYSIS_TRY(name, ub.reserve(nt + 1, nt + 1 + nt / 2));
        ANALYSIS_TRY(name, cnt.reserve(nt + 1, nt + 1 + nt / 2));
        ANALYSIS_TRY(name, hipMemcpy(off.p, read_off, (n_reads + 1) * 8, hipMemcpyHostToDevice));
        if (nt) {
            ANALYSIS_TRY(name, hipMemcpy(ub.p, user_bin + t0, nt * 8, hipMemcpyHostToDevice));
            ANALYSIS_TRY(name, hipMemcpy(cnt.p, count + t0, nt * 4, hipMemcpyHostToDevice));
        }
        if (hash_off) {
            h_nh->resize(n_reads);
            for (uint64_t r = 0; r < n_reads; ++r) (*h_nh)[r] = (uint32_t)(hash_off[r + 1] - hash_off[r]);
            ANALYSIS_TRY(name, nh.reserve(n_reads + 1, n_reads + 1 + n_reads / 2));
            if (n_reads) ANALYSIS_TRY(name, hipMemcpy(nh.p, h_nh->data(), n_reads * 4, hipMemcpyHostToDevice));
        }
        if (query_len) {
            ANALYSIS_TRY(name, qlen.reserve(n_reads + 1, n_reads + 1 + n_reads / 2));
            if (n_reads) ANALYSIS_TRY(name, hipMemcpy(qlen.p, query_len, n_reads * 8, hipMemcpyHostToDevice));
        }
        return TAXOR_OK;
    }
};

// What every analysis object holds: the table, the stager, the timer, a stream and the error word of its kernels
struct ReadAnalysis {
    LeafTable leaf;
    PieceStager stage;
    LaunchTimer timer;
    hipStream_t st = nullptr;
    std::mutex mu;                                    // batches may come from several threads
    DeviceBuf<uint32_t> d_err;
    std::vector<uint32_t> h_nh;
    CsrUpload csr;                                    // the host arrays of add_csr on the device
    ~ReadAnalysis()
    {
        if (st) (void)hipStreamDestroy(st);
    }
    // after leaf.build() and stage.configure(), on the index's device
    int open(const char *name)
    {
        timer.name = name;
        ANALYSIS_TRY(name, hipStreamCreate(&st));
        if (int rc = leaf.upload(name)) return rc;
        if (int rc = stage.alloc(name, st, &timer)) return rc;
        ANALYSIS_TRY(name, d_err.alloc(1));
        ANALYSIS_TRY(name, hipMemset(d_err.p, 0, 4));
        return TAXOR_OK;
    }
    // the error word of the kernels, read after a synchronisation; a word that is set is cleared for the next call
    int clear_err()
    {
        ANALYSIS_TRY(timer.name, hipMemset(d_err.p, 0, 4));
        return TAXOR_OK;
    }
};

// The device-resident results of a searcher's last batch
struct SearcherBatch {
    const uint64_t *d_off = nullptr;
    const int64_t *d_ub = nullptr;
    const uint32_t *d_cnt = nullptr, *d_nh = nullptr;
    uint64_t n = 0, nt = 0;
};

// The checks of <feature>_add_batch behind the null arguments: the saved batch is the searcher's last batch, read by read.  Takes the
// object's lock, selects its device and leaves the reads' hash counts in a.h_nh.  object: what the message calls the analysis object
inline int begin_batch(const char *fn, const char *name, const char *object, ReadAnalysis &a, taxor_gpu_searcher *s, const taxor_gpu_saved *saved,
                       std::unique_lock<std::mutex> &lk, SearcherBatch *b)
{
    if (!saved) return fail(TAXOR_E_ARG, "%s: saved: no saved batch (the batch ran with capture off, or its lists were not taken)", fn);
    if (taxor_searcher_index(s) != a.leaf.idx) return fail(TAXOR_E_ARG, "%s: index: the searcher works on another index than %s", fn, object);
    const std::string unsound = saved_validate(*saved);
    if (!unsound.empty()) return fail(TAXOR_E_ARG, std::string(fn) + ": " + unsound);
    int dev = 0;
    if (int rc = taxor_searcher_device_results(s, &b->d_off, &b->d_ub, &b->d_cnt, &b->d_nh, &b->n, &b->nt, &dev)) return rc;
    const uint64_t n = b->n;
    if (saved->n_reads != n)
        return fail(TAXOR_E_ARG, "%s: n_reads: the saved batch holds %llu reads, the searcher's last batch %llu", fn, (unsigned long long)saved->n_reads, (unsigned long long)n);
    if (n >= MAX_READS) return fail(TAXOR_E_ARG, "%s: n_reads: a batch of 2^31 reads or more", fn);
    lk = std::unique_lock<std::mutex>(a.mu);
    ANALYSIS_TRY(name, hipSetDevice(a.leaf.device));
    a.h_nh.resize(n);
    if (n) ANALYSIS_TRY(name, hipMemcpy(a.h_nh.data(), b->d_nh, n * 4, hipMemcpyDeviceToHost));
    for (uint64_t r = 0; r < n; ++r)
        if (a.h_nh[r] != saved->n_hashes[r])
            return fail(TAXOR_E_ARG, "%s: n_hashes: read %llu has %u hashes in the saved batch, %u in the searcher's last batch", fn, (unsigned long long)r, saved->n_hashes[r],
                        a.h_nh[r]);
    return TAXOR_OK;
}

} // namespace taxor
