// hitmap.hip -- where along a read each reference matched (`taxor search --hitmap-file`).
//
// A hit map lives beside a resident index for a whole run and keeps nothing between batches but its buffers.  A batch brings the
// searcher's device-resident CSR (the buffers taxor_gpu_batch_export_device copies from, read where they lie) and the batch's saved
// hash lists (taxor_gpu_search_take_saved), whose order is the order of first occurrence along the read.  Per read the MAPPED tuples
// are those that survive the search's output filter, provided the read has a hash; per mapped tuple (user bin b) the read's ordered
// list is cut into S segments -- hash i of n lies in segment floor(i * S / n) -- and hits[t][j] counts the hashes of segment j found
// in at least one leaf technical bin of b.
//
//   k_hm_count   one wave per read, tuples 64 at a time: the read's maximum count, then its mapped tuples counted.  A read without a
//                hash leaves at once: its thousands of zero-count tuples cost one load.
//   k_hm_scan_*  exclusive scan of the counts (tile scan, the tile sums by one block, add back): map_off.
//   k_hm_fill    the same walk; a ballot ranks the mapped tuples of each 64, so tuple / user_bin / count come out in CSR order.
//   k_hm_probe   one wave per PIECE -- at most READ_SPLIT consecutive hashes of one read that has a mapped tuple, cut on the host from the
//                saved counts, so that a 1-Mb read is a hundred waves.  The piece's hashes 64 at a time, one per lane; a lane knows its
//                hash's segment, and because the segment ascends with the lane the 64 fall into a few runs whose first lanes each
//                know their run's lanes as a mask.  Then the read's mapped tuples one after the other: read_probe.h's lookup over
//                ALL the tuple's leaf bins (`probes` counts them), a ballot of the lanes that matched, and per run one atomic add of
//                popcount(ballot & run) -- none where it is 0.
//
// hits is zeroed before the probe and only ever added to: integer sums do not depend on the launch geometry nor on the cut into
// pieces, staged groups and batches.  Every loop is bounded by a count the kernel is given (reads, a read's tuples, a piece's hashes,
// a user bin's leaf bins).  No block waits on another.
#include "analysis_host.h"
#include "hitmap_format.h"

#include <map>
#include <memory>

namespace {

using namespace taxor;

constexpr int HB = READ_BLOCK, HW = READ_WAVES, H_GRID_CAP = READ_GRID_CAP;
constexpr int SCAN_ITEMS = 4;
constexpr uint64_t SCAN_TILE = (uint64_t)HB * SCAN_ITEMS;

enum : uint32_t { HM_BAD_BIN = 1u };

__device__ __forceinline__ uint32_t hm_read_max(const uint32_t *__restrict__ count, uint64_t lo, uint64_t hi)
{
    uint32_t mx = 0;
    for (uint64_t i = lo + lane_id(); i < hi; i += 64) {
        const uint32_t c = count[i];
        mx = c > mx ? c : mx;
    }
    return wave_max(mx);
}

// a tuple is mapped when it survives the filter and names a user bin of the index (one outside is reported through err)
__device__ __forceinline__ bool hm_mapped(const int64_t *__restrict__ ub, const uint32_t *__restrict__ count, uint64_t i, uint64_t hi, uint32_t mx,
                                          uint64_t n_bins, bool *bad)
{
    if (i >= hi) return false;
    const int64_t b = ub[i];
    if (b < 0 || (uint64_t)b >= n_bins) {
        *bad = true;
        return false;
    }
    return keeps(count[i], mx);
}

__global__ __launch_bounds__(HB) void k_hm_count(const uint64_t *__restrict__ off, const int64_t *__restrict__ ub, const uint32_t *__restrict__ count,
                                                 const uint32_t *__restrict__ nh, uint64_t n_reads, uint64_t n_bins, uint64_t *__restrict__ mapped,
                                                 uint32_t *__restrict__ err)
{
    bool bad = false;
    for (uint64_t r = (uint64_t)blockIdx.x * HW + (threadIdx.x >> 6); r < n_reads; r += (uint64_t)gridDim.x * HW) {
        uint64_t n = 0;
        if (nh[r] != 0) {
            const uint64_t lo = off[r], hi = off[r + 1];
            const uint32_t mx = hm_read_max(count, lo, hi);
            for (uint64_t base = lo; base < hi; base += 64) n += (uint64_t)__popcll(__ballot(hm_mapped(ub, count, base + lane_id(), hi, mx, n_bins, &bad)));
        }
        if (lane_id() == 0) mapped[r] = n;
    }
    if (bad) atomicOr(err, HM_BAD_BIN);
}

// ---- exclusive scan of in[n] into out[n + 1] (out[n] = the total): tile-local scan and tile sums, the sums by one block, add back
// (profile_feed.hip's three launches)
__global__ __launch_bounds__(HB) void k_hm_scan_tiles(const uint64_t *__restrict__ in, uint64_t n, uint64_t *__restrict__ out, uint64_t *__restrict__ sums)
{
    const uint64_t first = (uint64_t)blockIdx.x * SCAN_TILE + (uint64_t)threadIdx.x * SCAN_ITEMS;
    uint64_t v[SCAN_ITEMS], mine = 0;
#pragma unroll
    for (int j = 0; j < SCAN_ITEMS; ++j) {
        v[j] = first + j < n ? in[first + j] : 0;
        mine += v[j];
    }
    __shared__ uint64_t sScr[HW];
    uint64_t total;
    uint64_t run = block_excl_add<HW>(mine, sScr, &total);
#pragma unroll
    for (int j = 0; j < SCAN_ITEMS; ++j) {
        if (first + j < n) out[first + j] = run;
        run += v[j];
    }
    if (threadIdx.x == 0) sums[blockIdx.x] = total;
}

__global__ __launch_bounds__(HB) void k_hm_scan_sums(uint64_t *__restrict__ sums, uint64_t n_tiles, uint64_t *__restrict__ out_total)
{
    __shared__ uint64_t sScr[HW];
    uint64_t carry = 0;
    for (uint64_t base = 0; base < n_tiles; base += HB) {
        const uint64_t i = base + threadIdx.x;
        const uint64_t v = i < n_tiles ? sums[i] : 0;
        uint64_t total;
        const uint64_t ex = block_excl_add<HW>(v, sScr, &total);
        if (i < n_tiles) sums[i] = carry + ex;
        carry += total;
    }
    if (threadIdx.x == 0) out_total[0] = carry;
}

__global__ __launch_bounds__(HB) void k_hm_scan_add(uint64_t *__restrict__ out, uint64_t n, const uint64_t *__restrict__ sums)
{
    const uint64_t first = (uint64_t)blockIdx.x * SCAN_TILE + (uint64_t)threadIdx.x * SCAN_ITEMS;
    const uint64_t add = sums[blockIdx.x];
#pragma unroll
    for (int j = 0; j < SCAN_ITEMS; ++j)
        if (first + j < n) out[first + j] += add;
}

// map_off = the scan of k_hm_count's counts: read r's mapped tuples go to [map_off[r], map_off[r + 1]) in CSR order
__global__ __launch_bounds__(HB) void k_hm_fill(const uint64_t *__restrict__ off, const int64_t *__restrict__ ub, const uint32_t *__restrict__ count,
                                                const uint32_t *__restrict__ nh, uint64_t n_reads, uint64_t n_bins, const uint64_t *__restrict__ map_off,
                                                uint64_t *__restrict__ o_tuple, int64_t *__restrict__ o_ub, uint32_t *__restrict__ o_count)
{
    for (uint64_t r = (uint64_t)blockIdx.x * HW + (threadIdx.x >> 6); r < n_reads; r += (uint64_t)gridDim.x * HW) {
        if (nh[r] == 0) continue;
        const uint64_t lo = off[r], hi = off[r + 1], dst0 = map_off[r], room = map_off[r + 1] - dst0;
        const uint32_t mx = hm_read_max(count, lo, hi);
        uint64_t written = 0;
        bool bad = false;
        for (uint64_t base = lo; base < hi; base += 64) {
            const uint64_t i = base + lane_id();
            const bool k = hm_mapped(ub, count, i, hi, mx, n_bins, &bad);
            const uint64_t m = __ballot(k);
            const uint64_t at = written + (uint64_t)__popcll(m & ((1ull << lane_id()) - 1ull));
            if (k && at < room) {                         // (at < room always: the same walk counted them)
                o_tuple[dst0 + at] = i;
                o_ub[dst0 + at] = ub[i];
                o_count[dst0 + at] = count[i];
            }
            written += (uint64_t)__popcll(m);
        }
    }
}

struct ProbeArgs {
    const IxfDesc *ixf;
    const uint64_t *leaf_off;     // [n_bins + 1] user bin b's leaf technical bins are leaf[leaf_off[b] .. leaf_off[b + 1])
    const uint2 *leaf;            // (IXF, bin)
    const uint64_t *map_off;      // [n_reads + 1]
    const uint32_t *nh;           // [n_reads] the reads' hashes
    const int64_t *map_ub;        // [n_mapped] checked against n_bins by k_hm_fill's walk
    const Piece *pieces;
    const uint64_t *hashes;       // the staged part of the saved lists
    uint32_t n_pieces;
    uint32_t segments;
    uint32_t *hits;               // [n_mapped * segments]
    unsigned long long *probes;
};

__global__ __launch_bounds__(HB) void k_hm_probe(ProbeArgs a)
{
    unsigned long long lookups = 0;
    const uint32_t lane = lane_id();
    for (uint64_t pi = (uint64_t)blockIdx.x * HW + (threadIdx.x >> 6); pi < a.n_pieces; pi += (uint64_t)gridDim.x * HW) {
        const Piece pc = a.pieces[pi];
        const uint64_t t0 = a.map_off[pc.read], t1 = a.map_off[pc.read + 1];
        const uint32_t total = a.nh[pc.read];                 // rank0 + n <= total
        for (uint32_t h0 = 0; h0 < pc.n; h0 += 64) {
            const uint32_t j = h0 + lane;
            const bool active = j < pc.n;
            const uint64_t h = active ? a.hashes[(uint64_t)pc.first + j] : 0;
            // hitmap_format.h's hitmap_seg; rank < total on an active lane, so seg < segments
            const uint32_t seg = active ? (uint32_t)((uint64_t)(pc.rank0 + j) * a.segments / total) : 0xFFFFFFFFu;
            // seg ascends with the lane: the first lane of every run of equal segments, and the lanes from itself up to the next run
            const uint32_t before = __shfl_up(seg, 1);
            const bool head = active && (lane == 0 || before != seg);
            const uint64_t heads = __ballot(head);
            const uint64_t above = lane == 63 ? 0ull : heads & ~((2ull << lane) - 1ull);
            const int end = above ? __ffsll((long long)above) - 1 : 64;
            const uint64_t run = (end == 64 ? ~0ull : (1ull << end) - 1ull) & ~((1ull << lane) - 1ull);
            for (uint64_t t = t0; t < t1; ++t) {
                const uint64_t b = (uint64_t)a.map_ub[t];                 // the same in every lane
                const uint64_t m = __ballot(leaf_lookup<false>(a.ixf, a.leaf, a.leaf_off[b], a.leaf_off[b + 1], h, active, lookups));
                if (head) {
                    const uint32_t c = (uint32_t)__popcll(m & run);
                    if (c) atomicAdd(a.hits + t * a.segments + seg, c);
                }
            }
        }
    }
    wave_add_to(a.probes, lookups);
}

#define HM_TRY(expr) TAXOR_HIP_TRY_PREFIX("hitmap", expr, #expr)

// the results of one searcher's calls: device arrays and their page-locked copy.  The host block holds, in this order,
// map_off[n + 1] | tuple[m] | user_bin[m] | count[m] | hits[m * S] | n_hashes[n]
struct Slot {
    DeviceBuf<uint64_t> d_mapped, d_map_off, d_sums, d_tuple;
    DeviceBuf<int64_t> d_ub;
    DeviceBuf<uint32_t> d_count, d_hits;
    char *h = nullptr;
    uint64_t h_cap = 0;
    ~Slot()
    {
        if (h) (void)hipHostFree(h);
    }
};

}   // namespace

struct taxor_gpu_hitmap : ReadAnalysis {
    uint32_t segments = 0;
    DeviceBuf<unsigned long long> d_probes;
    std::map<const void *, std::unique_ptr<Slot>> slots;
};

extern "C" int taxor_gpu_hitmap_create(taxor_gpu_index *idx, const taxor_hixf_view *view, uint32_t segments, taxor_gpu_hitmap **out)
{
    if (!out) return fail(TAXOR_E_ARG, "hitmap_create: null argument");
    *out = nullptr;
    if (!idx || !view) return fail(TAXOR_E_ARG, "hitmap_create: null argument");
    if (segments < 1 || segments > HITMAP_MAX_SEGMENTS) return fail(TAXOR_E_ARG, "hitmap_create: segments: %u is not in [1, %u]", segments, HITMAP_MAX_SEGMENTS);
    auto c = std::make_unique<taxor_gpu_hitmap>();
    if (int rc = c->leaf.build("hitmap_create", "its leaf bins are not all resident at once, and locating hits pass by pass is not built", idx, view)) return rc;
    if (int rc = c->stage.configure("hitmap_create")) return rc;
    c->segments = segments;
    HM_TRY(hipSetDevice(c->leaf.device));
    if (int rc = c->open("hitmap")) return rc;
    HM_TRY(c->d_probes.alloc(1));
    *out = c.release();
    return TAXOR_OK;
}

extern "C" void taxor_gpu_hitmap_destroy(taxor_gpu_hitmap *c)
{
    if (!c) return;
    (void)hipSetDevice(c->leaf.device);
    delete c;
}

extern "C" int taxor_gpu_hitmap_add_batch(taxor_gpu_hitmap *c, taxor_gpu_searcher *s, const taxor_gpu_saved *saved, taxor_hitmap_batch *out)
{
    if (!c || !s || !out) return fail(TAXOR_E_ARG, "hitmap_add_batch: null argument");
    std::unique_lock<std::mutex> lk;
    SearcherBatch b;
    if (int rc = begin_batch("hitmap_add_batch", "hitmap", "the hit map", *c, s, saved, lk, &b)) return rc;
    const uint64_t n = b.n, nt = b.nt, n_bins = c->leaf.n_bins;
    const uint64_t *d_off = b.d_off;
    const int64_t *d_ub = b.d_ub;
    const uint32_t *d_cnt = b.d_cnt, *d_nh = b.d_nh;

    const uint32_t S = c->segments;
    std::unique_ptr<Slot> &sp = c->slots[s];
    if (!sp) sp = std::make_unique<Slot>();
    Slot &sl = *sp;
    // the page-locked block for n reads and m mapped tuples; what it held is gone
    auto host_block = [&](uint64_t m) -> int {
        const uint64_t need = (n + 1) * 8 + m * (8 + 8 + 4 + 4ull * S) + n * 4;
        if (need > sl.h_cap) {
            const uint64_t want = std::max<uint64_t>(need + need / 2, 1u << 16);
            if (sl.h) (void)hipHostFree(sl.h);
            sl.h = nullptr;
            sl.h_cap = 0;
            HM_TRY(hipHostMalloc((void **)&sl.h, want, hipHostMallocDefault));
            sl.h_cap = want;
        }
        uint64_t *map_off = (uint64_t *)sl.h;
        uint64_t *tuple = map_off + n + 1;
        int64_t *ub = (int64_t *)(tuple + m);
        uint32_t *count = (uint32_t *)(ub + m);
        uint32_t *hits = count + m;
        uint32_t *nh = hits + m * S;
        out->n_reads = n;
        out->n_mapped = m;
        out->segments = S;
        out->reserved = 0;
        out->map_off = map_off;
        out->tuple = tuple;
        out->user_bin = ub;
        out->count = count;
        out->hits = hits;
        out->n_hashes = nh;
        out->seconds_kernels = 0;
        out->probes = 0;
        return TAXOR_OK;
    };
    if (int rc = c->stage.recover()) return rc;
    if (n == 0) {
        if (int rc = host_block(0)) return rc;
        ((uint64_t *)sl.h)[0] = 0;
        return TAXOR_OK;
    }
    c->timer.begin();
    auto stamp = [&]() { return c->timer.stamp(c->st); };

    // the mapped tuples: counted, scanned, written in CSR order
    const uint64_t tiles = (n + SCAN_TILE - 1) / SCAN_TILE;
    HM_TRY(sl.d_mapped.reserve(n, n + n / 2));
    HM_TRY(sl.d_map_off.reserve(n + 1, n + 1 + n / 2));
    HM_TRY(sl.d_sums.reserve(tiles, tiles + tiles / 2));
    HM_TRY(hipMemsetAsync(c->d_probes.p, 0, 8, c->st));
    if (int rc = stamp()) return rc;
    k_hm_count<<<grid_for(n, HW, H_GRID_CAP), HB, 0, c->st>>>(d_off, d_ub, d_cnt, d_nh, n, n_bins, sl.d_mapped.p, c->d_err.p);
    k_hm_scan_tiles<<<(int)tiles, HB, 0, c->st>>>(sl.d_mapped.p, n, sl.d_map_off.p, sl.d_sums.p);
    k_hm_scan_sums<<<1, HB, 0, c->st>>>(sl.d_sums.p, tiles, sl.d_map_off.p + n);
    k_hm_scan_add<<<(int)tiles, HB, 0, c->st>>>(sl.d_map_off.p, n, sl.d_sums.p);
    HM_TRY(hipGetLastError());
    if (int rc = stamp()) return rc;
    uint64_t m = 0;
    HM_TRY(hipMemcpyAsync(&m, sl.d_map_off.p + n, 8, hipMemcpyDeviceToHost, c->st));
    HM_TRY(hipStreamSynchronize(c->st));
    if (m > nt) return fail(TAXOR_E_INTERNAL, "hitmap_add_batch: %llu mapped tuples of %llu", (unsigned long long)m, (unsigned long long)nt);
    if (int rc = host_block(m)) return rc;
    uint64_t *h_map_off = (uint64_t *)sl.h;
    HM_TRY(hipMemcpyAsync(h_map_off, sl.d_map_off.p, (n + 1) * 8, hipMemcpyDeviceToHost, c->st));
    memcpy((void *)out->n_hashes, c->h_nh.data(), n * 4);
    uint32_t err = 0;
    if (m) {
        HM_TRY(sl.d_tuple.reserve(m, m + m / 2));
        HM_TRY(sl.d_ub.reserve(m, m + m / 2));
        HM_TRY(sl.d_count.reserve(m, m + m / 2));
        HM_TRY(sl.d_hits.reserve(m * S, (m + m / 2) * S));
        HM_TRY(hipMemsetAsync(sl.d_hits.p, 0, m * S * 4, c->st));
        if (int rc = stamp()) return rc;
        k_hm_fill<<<grid_for(n, HW, H_GRID_CAP), HB, 0, c->st>>>(d_off, d_ub, d_cnt, d_nh, n, n_bins, sl.d_map_off.p, sl.d_tuple.p, sl.d_ub.p, sl.d_count.p);
        HM_TRY(hipGetLastError());
        if (int rc = stamp()) return rc;
        HM_TRY(hipStreamSynchronize(c->st));           // map_off is on the host: the pieces are cut from it

        ProbeArgs a{};
        a.ixf = c->leaf.d_ixf;
        a.leaf_off = c->leaf.d_off.p;
        a.leaf = c->leaf.d_leaf.p;
        a.map_off = sl.d_map_off.p;
        a.nh = d_nh;
        a.map_ub = sl.d_ub.p;
        a.segments = S;
        a.hits = sl.d_hits.p;
        a.probes = c->d_probes.p;
        c->stage.begin(saved->hashes, [&](const Piece *pieces, const uint64_t *staged, uint32_t n_p) {
            a.pieces = pieces;
            a.hashes = staged;
            a.n_pieces = n_p;
            k_hm_probe<<<grid_for(n_p, HW, H_GRID_CAP), HB, 0, c->st>>>(a);
        });
        for (uint64_t r = 0; r < n; ++r)
            if (saved->n_hashes[r] != 0 && h_map_off[r + 1] != h_map_off[r])
                if (int rc = c->stage.add(r, saved->hash_off[r], saved->n_hashes[r])) return rc;
        if (int rc = c->stage.flush()) return rc;
        HM_TRY(hipMemcpyAsync((void *)out->tuple, sl.d_tuple.p, m * 8, hipMemcpyDeviceToHost, c->st));
        HM_TRY(hipMemcpyAsync((void *)out->user_bin, sl.d_ub.p, m * 8, hipMemcpyDeviceToHost, c->st));
        HM_TRY(hipMemcpyAsync((void *)out->count, sl.d_count.p, m * 4, hipMemcpyDeviceToHost, c->st));
        HM_TRY(hipMemcpyAsync((void *)out->hits, sl.d_hits.p, m * S * 4, hipMemcpyDeviceToHost, c->st));
    }
    unsigned long long probes = 0;
    HM_TRY(hipMemcpyAsync(&probes, c->d_probes.p, 8, hipMemcpyDeviceToHost, c->st));
    HM_TRY(hipMemcpyAsync(&err, c->d_err.p, 4, hipMemcpyDeviceToHost, c->st));
    HM_TRY(hipStreamSynchronize(c->st));               // the searcher's buffers and the saved lists are the caller's again
    c->stage.end();
    if (int rc = c->timer.add_to(&out->seconds_kernels)) return rc;
    out->probes = probes;
    if (err & HM_BAD_BIN) {
        if (int rc = c->clear_err()) return rc;
        return fail(TAXOR_E_INTERNAL, "hitmap_add_batch: a tuple names a user bin outside the index's %llu", (unsigned long long)n_bins);
    }
    return TAXOR_OK;
}
