// profile_feed.hip -- search results -> the CSR of `taxor profile`, on the device ("search to profile in one run").
//
// A feed collects, batch by batch and in any order, what taxor_gpu_profile_create takes from the host today: per read the matches
// that survive the search's output filter (taxor_search.cpp:268-306), as (reference id, ref_len, QHASH_MATCH), plus QUERY_LEN and
// QHASH_COUNT.  A batch comes from a searcher's device-resident results (the buffers taxor_gpu_batch_export_device copies from)
// or, for tests and other callers, from host arrays.  _finish permutes the reads into byte-wise id order and hands the device
// arrays to a taxor_gpu_profile (profile.hip, taxor_profile_adopt_device).
//
// One wave per read, lanes over the tuples 64 at a time, four reads per block, grid-stride: the convention of profile.hip.
//
//   k_ff_count     per read: max count, then the tuples with !((double)count < (double)max * 0.8) (:282-286, fp64 as written; every
//                  tuple under TAXOR_FEED_KEEP_ALL); a read with none contributes ONE match (ref -1, :268-273)
//   k_ff_scan_*    exclusive scan of 64-bit counts (tile sums, one block over the sums, add back).  The CSR-assembly scan of
//                  kernels.hip is 32-bit, local to a sub-batch and part of FinalizeArgs; this one scans up to every read of a run
//   k_ff_scatter   the surviving tuples in CSR order: ref_of_bin / ref_len_of_bin / count / user_bin; per read start, count,
//                  QUERY_LEN and QHASH_COUNT (0 for a "-" read, like profile_parse_range leaves it for a six-column line)
//   k_ff_counts_by_rank / k_ff_permute   finish: per-read counts gathered by rank, scanned, each read's segment copied
#include "../../include/taxor_gpu_tools.h"
#include "device_prims.h"
#include "hip_host.h"
#include "profile_host.h"
#include "read_probe.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

// api.hip: the device-resident CSR of a searcher's last run (synchronises it), and the reads' lengths in input order
extern "C" __attribute__((visibility("hidden"))) int taxor_searcher_device_results(taxor_gpu_searcher *s, const uint64_t **d_read_off,
                                                                                   const int64_t **d_user_bin, const uint32_t **d_count,
                                                                                   const uint32_t **d_n_hashes, uint64_t *n_reads,
                                                                                   uint64_t *n_tuples, int *device);
extern "C" __attribute__((visibility("hidden"))) int taxor_searcher_device_read_lengths(taxor_gpu_searcher *s, const uint32_t **d_rlen);
// profile.hip: a profile over device arrays; on success it owns them, and shares the host arrays
extern "C" __attribute__((visibility("hidden"))) int taxor_profile_adopt_device(int device, const std::shared_ptr<taxor_profile_host_csr> *host, uint64_t n_refs,
                                                                                uint64_t *d_off, int32_t *d_ref, uint64_t *d_ref_len, uint64_t *d_hash_match,
                                                                                uint64_t *d_query_len, uint64_t *d_hash_count, taxor_gpu_profile **out);

namespace {

using namespace taxor;

constexpr int FB = 256;                  // threads per block
constexpr int FW = FB / 64;              // reads per block pass (one wave each)
constexpr int F_GRID_CAP = 2048;
constexpr int SCAN_ITEMS = 8;            // values per thread of a scan tile
constexpr int SCAN_TILE = FB * SCAN_ITEMS;
constexpr uint64_t MAX_READS = 1ull << 36;

enum : uint32_t { FF_BAD_BIN = 1u };

__device__ __forceinline__ uint64_t ff_first_read() { return (uint64_t)blockIdx.x * FW + (threadIdx.x >> 6); }
__device__ __forceinline__ uint64_t ff_read_step() { return (uint64_t)gridDim.x * FW; }

// the largest count among tuples [lo, hi) of `count` (indexed from t0); the same in every lane
__device__ __forceinline__ uint32_t ff_read_max(const uint32_t *__restrict__ count, uint64_t t0, uint64_t lo, uint64_t hi)
{
    uint32_t mx = 0;
    for (uint64_t i = lo + lane_id(); i < hi; i += 64) {
        const uint32_t c = count[i - t0];
        mx = c > mx ? c : mx;
    }
    return wave_max(mx);
}

// read_probe.h's output filter, with the keep-all switch in front
__device__ __forceinline__ bool ff_keeps(uint32_t c, uint32_t mx, bool keep_all) { return keep_all || keeps(c, mx); }

__global__ __launch_bounds__(FB) void k_ff_count(const uint64_t *__restrict__ off, const int64_t *__restrict__ ub, const uint32_t *__restrict__ count,
                                                 uint64_t t0, uint64_t n_reads, uint64_t n_bins, int keep_all, uint64_t *__restrict__ kept,
                                                 uint32_t *__restrict__ err)
{
    for (uint64_t r = ff_first_read(); r < n_reads; r += ff_read_step()) {
        const uint64_t lo = off[r], hi = off[r + 1];
        const uint32_t mx = ff_read_max(count, t0, lo, hi);
        uint64_t n = 0;
        bool bad = false;
        for (uint64_t base = lo; base < hi; base += 64) {
            const uint64_t i = base + lane_id();
            bool k = false;
            if (i < hi) {
                const int64_t b = ub[i - t0];
                bad |= b < 0 || (uint64_t)b >= n_bins;
                k = ff_keeps(count[i - t0], mx, keep_all != 0);
            }
            n += (uint64_t)__popcll(__ballot(k));
        }
        if (bad) atomicOr(err, FF_BAD_BIN);
        if (lane_id() == 0) kept[r] = n ? n : 1;
    }
}

// ---- exclusive scan of in[n] into out[n + 1] (out[n] = the total): tile-local scan and tile sums, the sums by one block, add back
__global__ __launch_bounds__(FB) void k_ff_scan_tiles(const uint64_t *__restrict__ in, uint64_t n, uint64_t *__restrict__ out, uint64_t *__restrict__ sums)
{
    const uint64_t first = (uint64_t)blockIdx.x * SCAN_TILE + (uint64_t)threadIdx.x * SCAN_ITEMS;
    uint64_t v[SCAN_ITEMS], mine = 0;
#pragma unroll
    for (int j = 0; j < SCAN_ITEMS; ++j) {
        v[j] = first + j < n ? in[first + j] : 0;
        mine += v[j];
    }
    __shared__ uint64_t sScr[FW];
    uint64_t total;
    uint64_t run = block_excl_add<FW>(mine, sScr, &total);
#pragma unroll
    for (int j = 0; j < SCAN_ITEMS; ++j) {
        if (first + j < n) out[first + j] = run;
        run += v[j];
    }
    if (threadIdx.x == 0) sums[blockIdx.x] = total;
}

// one block: sums[n_tiles] -> exclusive, in place; out_total[0] = everything
__global__ __launch_bounds__(FB) void k_ff_scan_sums(uint64_t *__restrict__ sums, uint64_t n_tiles, uint64_t *__restrict__ out_total)
{
    __shared__ uint64_t sScr[FW];
    uint64_t carry = 0;
    for (uint64_t base = 0; base < n_tiles; base += FB) {
        const uint64_t i = base + threadIdx.x;
        const uint64_t v = i < n_tiles ? sums[i] : 0;
        uint64_t total;
        const uint64_t ex = block_excl_add<FW>(v, sScr, &total);
        if (i < n_tiles) sums[i] = carry + ex;
        carry += total;
    }
    if (threadIdx.x == 0) out_total[0] = carry;
}

__global__ __launch_bounds__(FB) void k_ff_scan_add(uint64_t *__restrict__ out, uint64_t n, const uint64_t *__restrict__ sums)
{
    const uint64_t first = (uint64_t)blockIdx.x * SCAN_TILE + (uint64_t)threadIdx.x * SCAN_ITEMS;
    const uint64_t add = sums[blockIdx.x];
#pragma unroll
    for (int j = 0; j < SCAN_ITEMS; ++j)
        if (first + j < n) out[first + j] += add;
}

struct FeedStore {                       // where the matches and the per-read records of a feed live
    int32_t *m_ref;
    uint64_t *m_ref_len, *m_hash_match;
    int64_t *m_user_bin;
    uint64_t *r_start, *r_count, *r_query_len, *r_hash_count;
};

// pos = exclusive scan of the batch's kept counts; the batch's matches start at `base` of the store, its reads at first_read
__global__ __launch_bounds__(FB) void k_ff_scatter(const uint64_t *__restrict__ off, const int64_t *__restrict__ ub, const uint32_t *__restrict__ count,
                                                   const uint32_t *__restrict__ n_hashes, const uint32_t *__restrict__ rlen32,
                                                   const uint64_t *__restrict__ qlen64, uint64_t t0, uint64_t n_reads, int keep_all,
                                                   const uint64_t *__restrict__ pos, uint64_t base, uint64_t first_read,
                                                   const int32_t *__restrict__ ref_of_bin, const uint64_t *__restrict__ ref_len_of_bin, FeedStore st)
{
    for (uint64_t r = ff_first_read(); r < n_reads; r += ff_read_step()) {
        const uint64_t lo = off[r], hi = off[r + 1];
        const uint32_t mx = ff_read_max(count, t0, lo, hi);
        const uint64_t dst0 = base + pos[r];
        uint64_t written = 0;
        for (uint64_t b0 = lo; b0 < hi; b0 += 64) {
            const uint64_t i = b0 + lane_id();
            uint32_t c = 0;
            int64_t bin = 0;
            bool k = false;
            if (i < hi) {
                c = count[i - t0];
                bin = ub[i - t0];
                k = ff_keeps(c, mx, keep_all != 0);
            }
            const uint64_t m = __ballot(k);
            if (k) {
                const uint64_t d = dst0 + written + (uint64_t)__popcll(m & ((1ull << lane_id()) - 1ull));
                st.m_ref[d] = ref_of_bin[bin];
                st.m_ref_len[d] = ref_len_of_bin[bin];
                st.m_hash_match[d] = c;
                st.m_user_bin[d] = bin;
            }
            written += (uint64_t)__popcll(m);
        }
        if (lane_id() == 0) {
            if (written == 0) {                        // the read's "-" line
                st.m_ref[dst0] = -1;
                st.m_ref_len[dst0] = 0;
                st.m_hash_match[dst0] = 0;
                st.m_user_bin[dst0] = -1;
            }
            const uint64_t g = first_read + r;
            st.r_start[g] = dst0;
            st.r_count[g] = written ? written : 1;
            st.r_query_len[g] = rlen32 ? (uint64_t)rlen32[r] : qlen64[r];
            st.r_hash_count[g] = written ? (uint64_t)n_hashes[r] : 0;
        }
    }
}

__global__ __launch_bounds__(FB) void k_ff_counts_by_rank(const uint64_t *__restrict__ rank, const uint64_t *__restrict__ r_count, uint64_t n,
                                                          uint64_t *__restrict__ by_rank)
{
    for (uint64_t i = (uint64_t)blockIdx.x * FB + threadIdx.x; i < n; i += (uint64_t)gridDim.x * FB) by_rank[rank[i]] = r_count[i];
}

__global__ __launch_bounds__(FB) void k_ff_permute(const uint64_t *__restrict__ rank, uint64_t n, const uint64_t *__restrict__ off, FeedStore st,
                                                   int32_t *__restrict__ o_ref, uint64_t *__restrict__ o_ref_len, uint64_t *__restrict__ o_hash_match,
                                                   int64_t *__restrict__ o_user_bin, uint64_t *__restrict__ o_query_len,
                                                   uint64_t *__restrict__ o_hash_count)
{
    for (uint64_t r = ff_first_read(); r < n; r += ff_read_step()) {
        const uint64_t k = rank[r], src = st.r_start[r], dst = off[k], c = st.r_count[r];
        for (uint64_t j = lane_id(); j < c; j += 64) {
            o_ref[dst + j] = st.m_ref[src + j];
            o_ref_len[dst + j] = st.m_ref_len[src + j];
            o_hash_match[dst + j] = st.m_hash_match[src + j];
            o_user_bin[dst + j] = st.m_user_bin[src + j];
        }
        if (lane_id() == 0) {
            o_query_len[k] = st.r_query_len[r];
            o_hash_count[k] = st.r_hash_count[r];
        }
    }
}

#define FF_TRY(expr) TAXOR_HIP_TRY_PREFIX("profile_feed", expr, #expr)

// a feed's arrays grow geometrically and keep their first `keep` elements
template <class T> hipError_t grow(DeviceBuf<T> &b, uint64_t want, uint64_t keep, hipStream_t st)
{
    return b.grow(want, std::max<uint64_t>({want, b.cap + b.cap / 2, 1024}), keep, st);
}

}   // namespace

struct taxor_gpu_profile_feed {
    int device = 0;
    uint64_t n_bins = 0, n_refs = 0;
    hipStream_t st = nullptr;
    std::mutex mu;                                   // batches may come from several threads
    DeviceBuf<int32_t> d_ref_of_bin, m_ref, o_ref;
    DeviceBuf<uint64_t> d_ref_len_of_bin, m_ref_len, m_hash_match, r_start, r_count, r_query_len, r_hash_count;
    DeviceBuf<int64_t> m_user_bin, o_user_bin;
    DeviceBuf<uint64_t> b_kept, b_pos, b_sums;            // per batch: kept counts, their scan, the scan's tile sums
    DeviceBuf<uint32_t> d_err;
    // host arrays of add_csr on the device
    DeviceBuf<uint64_t> c_off, c_qlen;
    DeviceBuf<int64_t> c_ub;
    DeviceBuf<uint32_t> c_cnt, c_nh;
    uint64_t m_used = 0, r_cap_used = 0;
    std::vector<std::pair<uint64_t, uint64_t>> ranges;   // (first_read, n_reads) of every batch
    bool finished = false;
    // the finished CSR on the host (taxor_gpu_profile_feed_matches); all but ref and user_bin are shared with the profile, which
    // reads them in its host stages: one copy in host memory
    std::shared_ptr<taxor_profile_host_csr> h;
    std::vector<int32_t> h_ref;
    std::vector<int64_t> h_user_bin;
    ~taxor_gpu_profile_feed()
    {
        if (st) (void)hipStreamDestroy(st);
    }
};

namespace {

FeedStore store_of(taxor_gpu_profile_feed *f)
{
    return FeedStore{f->m_ref.p, f->m_ref_len.p, f->m_hash_match.p, f->m_user_bin.p, f->r_start.p, f->r_count.p, f->r_query_len.p, f->r_hash_count.p};
}

// in[n] on the device -> out[n + 1]; *total on the host.  Synchronises the feed's stream.
int scan_counts(taxor_gpu_profile_feed *f, const uint64_t *in, uint64_t n, uint64_t *out, uint64_t *total)
{
    if (n == 0) {
        FF_TRY(hipMemsetAsync(out, 0, 8, f->st));
        FF_TRY(hipStreamSynchronize(f->st));
        *total = 0;
        return TAXOR_OK;
    }
    const uint64_t tiles = (n + SCAN_TILE - 1) / SCAN_TILE;
    FF_TRY(grow(f->b_sums, tiles, 0, f->st));
    k_ff_scan_tiles<<<(int)tiles, FB, 0, f->st>>>(in, n, out, f->b_sums.p);
    k_ff_scan_sums<<<1, FB, 0, f->st>>>(f->b_sums.p, tiles, out + n);
    k_ff_scan_add<<<(int)tiles, FB, 0, f->st>>>(out, n, f->b_sums.p);
    FF_TRY(hipGetLastError());
    FF_TRY(hipMemcpyAsync(total, out + n, 8, hipMemcpyDeviceToHost, f->st));
    FF_TRY(hipStreamSynchronize(f->st));
    return TAXOR_OK;
}

// one batch whose arrays are on the feed's device; tuples are indexed from t0 (off[0] == t0)
int add_device(taxor_gpu_profile_feed *f, uint64_t first_read, uint64_t n, const uint64_t *d_off, const int64_t *d_ub, const uint32_t *d_cnt,
               const uint32_t *d_nh, const uint32_t *d_rlen32, const uint64_t *d_qlen64, uint64_t t0, uint32_t flags)
{
    if (f->finished) return fail(TAXOR_E_ARG, "profile_feed_add: the feed is finished");
    if (flags & ~TAXOR_FEED_KEEP_ALL) return fail(TAXOR_E_ARG, "profile_feed_add: unknown flag");
    if (first_read >= MAX_READS || n >= MAX_READS) return fail(TAXOR_E_ARG, "profile_feed_add: read index beyond 2^36");
    if (n == 0) {
        f->ranges.emplace_back(first_read, n);
        return TAXOR_OK;
    }
    const int keep_all = (flags & TAXOR_FEED_KEEP_ALL) ? 1 : 0;
    FF_TRY(grow(f->b_kept, n, 0, f->st));
    FF_TRY(grow(f->b_pos, n + 1, 0, f->st));
    FF_TRY(hipMemsetAsync(f->d_err.p, 0, 4, f->st));
    k_ff_count<<<grid_for(n, FW, F_GRID_CAP), FB, 0, f->st>>>(d_off, d_ub, d_cnt, t0, n, f->n_bins, keep_all, f->b_kept.p, f->d_err.p);
    FF_TRY(hipGetLastError());
    uint64_t total = 0;
    uint32_t err = 0;
    FF_TRY(hipMemcpyAsync(&err, f->d_err.p, 4, hipMemcpyDeviceToHost, f->st));
    if (int rc = scan_counts(f, f->b_kept.p, n, f->b_pos.p, &total)) return rc;     // synchronises the stream
    if (err & FF_BAD_BIN)
        return fail(TAXOR_E_ARG, "profile_feed_add: a user bin lies outside the feed's table of " + std::to_string(f->n_bins) + " user bins");
    // a batch is never truncated: the stores grow to hold it
    const uint64_t need_m = f->m_used + total, need_r = first_read + n;
    FF_TRY(grow(f->m_ref, need_m, f->m_used, f->st));
    FF_TRY(grow(f->m_ref_len, need_m, f->m_used, f->st));
    FF_TRY(grow(f->m_hash_match, need_m, f->m_used, f->st));
    FF_TRY(grow(f->m_user_bin, need_m, f->m_used, f->st));
    FF_TRY(grow(f->r_start, need_r, f->r_cap_used, f->st));
    FF_TRY(grow(f->r_count, need_r, f->r_cap_used, f->st));
    FF_TRY(grow(f->r_query_len, need_r, f->r_cap_used, f->st));
    FF_TRY(grow(f->r_hash_count, need_r, f->r_cap_used, f->st));
    f->r_cap_used = std::max(f->r_cap_used, need_r);
    k_ff_scatter<<<grid_for(n, FW, F_GRID_CAP), FB, 0, f->st>>>(d_off, d_ub, d_cnt, d_nh, d_rlen32, d_qlen64, t0, n, keep_all, f->b_pos.p, f->m_used, first_read,
                                                  f->d_ref_of_bin.p, f->d_ref_len_of_bin.p, store_of(f));
    FF_TRY(hipGetLastError());
    FF_TRY(hipStreamSynchronize(f->st));              // the caller's buffers (a searcher's results) may be reused from here on
    f->m_used += total;
    f->ranges.emplace_back(first_read, n);            // only now: a batch that failed on the way has added no reads, and may be added again
    return TAXOR_OK;
}

}   // namespace

extern "C" int taxor_gpu_profile_feed_create(int device, uint64_t n_user_bins, const int32_t *ref_of_bin, const uint64_t *ref_len_of_bin, uint64_t n_refs,
                                             taxor_gpu_profile_feed **out)
{
    if (!out) return fail(TAXOR_E_ARG, "profile_feed_create: null argument");
    *out = nullptr;
    if (n_user_bins && (!ref_of_bin || !ref_len_of_bin)) return fail(TAXOR_E_ARG, "profile_feed_create: null array");
    if (n_refs >= (1ull << 31)) return fail(TAXOR_E_ARG, "profile_feed_create: more than 2^31 - 1 references");
    for (uint64_t u = 0; u < n_user_bins; ++u)
        if (ref_of_bin[u] < 0 || (uint64_t)ref_of_bin[u] >= n_refs) return fail(TAXOR_E_ARG, "profile_feed_create: reference id of user bin " + std::to_string(u) + " out of range");
    FF_TRY(hipSetDevice(device));
    auto f = std::make_unique<taxor_gpu_profile_feed>();
    f->device = device;
    f->n_bins = n_user_bins;
    f->n_refs = n_refs;
    FF_TRY(hipStreamCreate(&f->st));
    FF_TRY(grow(f->d_ref_of_bin, n_user_bins, 0, f->st));
    FF_TRY(grow(f->d_ref_len_of_bin, n_user_bins, 0, f->st));
    FF_TRY(grow(f->d_err, 1, 0, f->st));
    if (n_user_bins) {
        FF_TRY(hipMemcpy(f->d_ref_of_bin.p, ref_of_bin, n_user_bins * 4, hipMemcpyHostToDevice));
        FF_TRY(hipMemcpy(f->d_ref_len_of_bin.p, ref_len_of_bin, n_user_bins * 8, hipMemcpyHostToDevice));
    }
    *out = f.release();
    return TAXOR_OK;
}

extern "C" void taxor_gpu_profile_feed_destroy(taxor_gpu_profile_feed *f)
{
    if (!f) return;
    (void)hipSetDevice(f->device);
    delete f;
}

extern "C" int taxor_gpu_profile_feed_add_batch(taxor_gpu_profile_feed *f, taxor_gpu_searcher *s, uint64_t first_read, uint32_t flags)
{
    if (!f || !s) return fail(TAXOR_E_ARG, "profile_feed_add_batch: null argument");
    const uint64_t *d_off = nullptr;
    const int64_t *d_ub = nullptr;
    const uint32_t *d_cnt = nullptr, *d_nh = nullptr, *d_rlen = nullptr;
    uint64_t n = 0, nt = 0;
    int dev = 0;
    if (int rc = taxor_searcher_device_results(s, &d_off, &d_ub, &d_cnt, &d_nh, &n, &nt, &dev)) return rc;
    if (dev != f->device) return fail(TAXOR_E_ARG, "profile_feed_add_batch: the searcher runs on device " + std::to_string(dev) + ", the feed on " + std::to_string(f->device));
    if (int rc = taxor_searcher_device_read_lengths(s, &d_rlen)) return rc;
    std::lock_guard<std::mutex> lk(f->mu);
    FF_TRY(hipSetDevice(f->device));
    return add_device(f, first_read, n, d_off, d_ub, d_cnt, d_nh, d_rlen, nullptr, 0, flags);
}

extern "C" int taxor_gpu_profile_feed_add_csr(taxor_gpu_profile_feed *f, uint64_t first_read, uint64_t n_reads, const uint64_t *read_off, const int64_t *user_bin,
                                              const uint32_t *count, const uint32_t *n_hashes, const uint64_t *query_len, uint32_t flags)
{
    if (!f || !read_off) return fail(TAXOR_E_ARG, "profile_feed_add_csr: null argument");
    if (n_reads && (!n_hashes || !query_len)) return fail(TAXOR_E_ARG, "profile_feed_add_csr: null array");
    if (n_reads >= MAX_READS) return fail(TAXOR_E_ARG, "profile_feed_add_csr: read index beyond 2^36");
    for (uint64_t r = 0; r < n_reads; ++r)
        if (read_off[r + 1] < read_off[r]) return fail(TAXOR_E_ARG, "profile_feed_add_csr: read_off decreases");
    const uint64_t t0 = read_off[0], nt = read_off[n_reads] - t0;
    if (nt && (!user_bin || !count)) return fail(TAXOR_E_ARG, "profile_feed_add_csr: null array");
    std::lock_guard<std::mutex> lk(f->mu);
    FF_TRY(hipSetDevice(f->device));
    FF_TRY(grow(f->c_off, n_reads + 1, 0, f->st));
    FF_TRY(grow(f->c_ub, nt, 0, f->st));
    FF_TRY(grow(f->c_cnt, nt, 0, f->st));
    FF_TRY(grow(f->c_nh, n_reads, 0, f->st));
    FF_TRY(grow(f->c_qlen, n_reads, 0, f->st));
    FF_TRY(hipMemcpy(f->c_off.p, read_off, (n_reads + 1) * 8, hipMemcpyHostToDevice));
    if (nt) {
        FF_TRY(hipMemcpy(f->c_ub.p, user_bin + t0, nt * 8, hipMemcpyHostToDevice));
        FF_TRY(hipMemcpy(f->c_cnt.p, count + t0, nt * 4, hipMemcpyHostToDevice));
    }
    if (n_reads) {
        FF_TRY(hipMemcpy(f->c_nh.p, n_hashes, n_reads * 4, hipMemcpyHostToDevice));
        FF_TRY(hipMemcpy(f->c_qlen.p, query_len, n_reads * 8, hipMemcpyHostToDevice));
    }
    return add_device(f, first_read, n_reads, f->c_off.p, f->c_ub.p, f->c_cnt.p, f->c_nh.p, nullptr, f->c_qlen.p, t0, flags);
}

extern "C" int taxor_gpu_profile_feed_finish(taxor_gpu_profile_feed *f, const uint64_t *rank_of_read, uint64_t n_reads_total, taxor_gpu_profile **profile)
{
    if (!f || !profile) return fail(TAXOR_E_ARG, "profile_feed_finish: null argument");
    *profile = nullptr;
    if (n_reads_total && !rank_of_read) return fail(TAXOR_E_ARG, "profile_feed_finish: null argument");
    std::lock_guard<std::mutex> lk(f->mu);
    if (f->finished) return fail(TAXOR_E_ARG, "profile_feed_finish: the feed is finished");
    // the batches' ranges cover [0, n_reads_total) exactly, once
    {
        std::vector<std::pair<uint64_t, uint64_t>> rg;
        for (const auto &x : f->ranges)
            if (x.second) rg.push_back(x);
        std::sort(rg.begin(), rg.end());
        uint64_t next = 0;
        for (const auto &x : rg) {
            if (x.first > next)
                return fail(TAXOR_E_ARG, "profile_feed_finish: reads " + std::to_string(next) + " to " + std::to_string(x.first - 1) + " were never added (a gap between the batches)");
            if (x.first < next)
                return fail(TAXOR_E_ARG, "profile_feed_finish: read " + std::to_string(x.first) + " was added twice (the batches' ranges overlap)");
            next = x.first + x.second;
        }
        if (next != n_reads_total)
            return fail(TAXOR_E_ARG, "profile_feed_finish: " + std::to_string(next) + " reads were added, " + std::to_string(n_reads_total) + " are to be ranked");
    }
    const uint64_t R = n_reads_total, M = f->m_used;
    {
        std::vector<uint8_t> seen(R, 0);
        for (uint64_t i = 0; i < R; ++i) {
            const uint64_t k = rank_of_read[i];
            if (k >= R) return fail(TAXOR_E_ARG, "profile_feed_finish: rank " + std::to_string(k) + " of read " + std::to_string(i) + " is not below the number of reads");
            if (seen[k]) return fail(TAXOR_E_ARG, "profile_feed_finish: rank " + std::to_string(k) + " is used twice (rank_of_read is not a permutation)");
            seen[k] = 1;
        }
    }
    FF_TRY(hipSetDevice(f->device));
    hipStream_t st = f->st;
    DeviceBuf<uint64_t> d_rank, d_by_rank, o_off, o_ref_len, o_hash_match, o_query_len, o_hash_count;
    FF_TRY(grow(d_rank, R, 0, st));
    FF_TRY(grow(d_by_rank, R, 0, st));
    FF_TRY(grow(o_off, R + 1, 0, st));
    FF_TRY(grow(f->o_ref, M, 0, st));
    FF_TRY(grow(o_ref_len, M, 0, st));
    FF_TRY(grow(o_hash_match, M, 0, st));
    FF_TRY(grow(f->o_user_bin, M, 0, st));
    FF_TRY(grow(o_query_len, R, 0, st));
    FF_TRY(grow(o_hash_count, R, 0, st));
    if (R) {
        FF_TRY(hipMemcpyAsync(d_rank.p, rank_of_read, R * 8, hipMemcpyHostToDevice, st));
        k_ff_counts_by_rank<<<grid_for(R, FB, F_GRID_CAP), FB, 0, st>>>(d_rank.p, f->r_count.p, R, d_by_rank.p);
        FF_TRY(hipGetLastError());
    }
    uint64_t total = 0;
    if (int rc = scan_counts(f, d_by_rank.p, R, o_off.p, &total)) return rc;
    if (total != M) return fail(TAXOR_E_INTERNAL, "profile_feed_finish: the reads hold " + std::to_string(total) + " matches, the store " + std::to_string(M));
    if (R) {
        k_ff_permute<<<grid_for(R, FW, F_GRID_CAP), FB, 0, st>>>(d_rank.p, R, o_off.p, store_of(f), f->o_ref.p, o_ref_len.p, o_hash_match.p, f->o_user_bin.p, o_query_len.p,
                                                   o_hash_count.p);
        FF_TRY(hipGetLastError());
    }
    // the finished CSR once on the host: the profile's host stages read it, the caller's binning file needs user_bin and read_off
    auto h = std::make_shared<taxor_profile_host_csr>();
    h->off.resize(R + 1);
    f->h_ref.resize(M);
    h->ref_len.resize(M);
    h->hash_match.resize(M);
    f->h_user_bin.resize(M);
    h->query_len.resize(R);
    h->hash_count.resize(R);
    FF_TRY(hipMemcpyAsync(h->off.data(), o_off.p, (R + 1) * 8, hipMemcpyDeviceToHost, st));
    if (M) {
        FF_TRY(hipMemcpyAsync(f->h_ref.data(), f->o_ref.p, M * 4, hipMemcpyDeviceToHost, st));
        FF_TRY(hipMemcpyAsync(h->ref_len.data(), o_ref_len.p, M * 8, hipMemcpyDeviceToHost, st));
        FF_TRY(hipMemcpyAsync(h->hash_match.data(), o_hash_match.p, M * 8, hipMemcpyDeviceToHost, st));
        FF_TRY(hipMemcpyAsync(f->h_user_bin.data(), f->o_user_bin.p, M * 8, hipMemcpyDeviceToHost, st));
    }
    if (R) {
        FF_TRY(hipMemcpyAsync(h->query_len.data(), o_query_len.p, R * 8, hipMemcpyDeviceToHost, st));
        FF_TRY(hipMemcpyAsync(h->hash_count.data(), o_hash_count.p, R * 8, hipMemcpyDeviceToHost, st));
    }
    FF_TRY(hipStreamSynchronize(st));
    if (int rc = taxor_profile_adopt_device(f->device, &h, f->n_refs, o_off.p, f->o_ref.p, o_ref_len.p, o_hash_match.p, o_query_len.p, o_hash_count.p, profile)) return rc;
    f->h = std::move(h);
    (void)o_off.take();                               // the profile owns them now
    (void)f->o_ref.take();
    (void)o_ref_len.take();
    (void)o_hash_match.take();
    (void)o_query_len.take();
    (void)o_hash_count.take();
    f->finished = true;
    f->o_user_bin.release();
    f->m_ref.release();
    f->m_ref_len.release();
    f->m_hash_match.release();
    f->m_user_bin.release();
    f->r_start.release();
    f->r_count.release();
    f->r_query_len.release();
    f->r_hash_count.release();
    return TAXOR_OK;
}

extern "C" int taxor_gpu_profile_feed_matches(const taxor_gpu_profile_feed *f, taxor_profile_csr *csr, const int64_t **user_bin)
{
    if (!f || (!csr && !user_bin)) return fail(TAXOR_E_ARG, "profile_feed_matches: null argument");
    if (!f->finished) return fail(TAXOR_E_ARG, "profile_feed_matches: the feed is not finished");
    if (csr) {
        csr->n_reads = f->h->query_len.size();
        csr->n_refs = f->n_refs;
        csr->n_matches = f->h_ref.size();
        csr->read_off = f->h->off.data();
        csr->ref = f->h_ref.data();
        csr->ref_len = f->h->ref_len.data();
        csr->hash_match = f->h->hash_match.data();
        csr->query_len = f->h->query_len.data();
        csr->hash_count = f->h->hash_count.data();
    }
    if (user_bin) *user_bin = f->h_user_bin.data();
    return TAXOR_OK;
}
