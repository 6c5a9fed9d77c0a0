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
//   k_hm_probe   one wave per PIECE -- at most HM_SPLIT consecutive hashes of one read that has a mapped tuple, cut on the host from the
//                saved counts, so that a 1-Mb read is a hundred waves.  The piece's hashes 64 at a time, one per lane; a lane knows its
//                hash's segment, and because the segment ascends with the lane the 64 fall into a few runs whose first lanes each
//                know their run's lanes as a mask.  Then the read's mapped tuples one after the other: the probe (three rows,
//                fingerprint) once per IXF among the tuple's leaf bins, three one-byte gathers per leaf bin at data[row * stride +
//                bin], a ballot of the lanes that matched, and per run one atomic add of popcount(ballot & run) -- none where it is 0.
//
// hits is zeroed before the probe and only ever added to: integer sums do not depend on the launch geometry nor on the cut into
// pieces, staged groups and batches.  Every loop is bounded by a count the kernel is given (reads, a read's tuples, a piece's hashes,
// a user bin's leaf bins).  No block waits on another.
#include "../../include/taxor_gpu_tools.h"
#include "device_prims.h"
#include "hip_host.h"
#include "hitmap_format.h"
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

constexpr int HB = 256;                           // threads per block
constexpr int HW = HB / 64;                       // reads / pieces per block pass (one wave each)
constexpr int H_GRID_CAP = 4096;
constexpr int SCAN_ITEMS = 4;
constexpr uint64_t SCAN_TILE = (uint64_t)HB * SCAN_ITEMS;
constexpr uint32_t HM_SPLIT = 2048;               // hashes of one read per piece
constexpr uint64_t STAGE_HASHES = 1ull << 22;     // hashes per staging buffer (32 MiB); there are two
constexpr uint64_t STAGE_PIECES = 1ull << 18;     // pieces per staging buffer (5 MiB); there are two
constexpr uint64_t MAX_READS = 1ull << 31;

enum : uint32_t { HM_BAD_BIN = 1u };

struct Piece {
    uint32_t read;       // index in the batch
    uint32_t first;      // offset of the piece's first hash in the staging buffer
    uint32_t n;          // hashes, at most HM_SPLIT
    uint32_t rank0;      // rank of the piece's first hash in the read's list
    uint32_t total;      // hashes of the whole read (rank0 + n <= total)
};

// taxor_search.cpp:285, evaluated as written: the expression of taxor_classify_filter, k_ff_count, cov_keeps and lca_keeps.  Restated
// here, and not moved into device_prims.h, for lca.hip's reason: that header is part of every kernel file of the search path, and this
// change leaves those files' sources, and with them their objects, exactly as they were
__device__ __forceinline__ bool hm_keeps(uint32_t c, uint32_t mx) { return !((double)c < (double)mx * 0.8); }

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
    return hm_keeps(count[i], mx);
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
        for (uint32_t h0 = 0; h0 < pc.n; h0 += 64) {
            const uint32_t j = h0 + lane;
            const bool active = j < pc.n;
            const uint64_t h = active ? a.hashes[(uint64_t)pc.first + j] : 0;
            // hitmap_format.h's hitmap_seg; rank < total on an active lane, so seg < segments
            const uint32_t seg = active ? (uint32_t)((uint64_t)(pc.rank0 + j) * a.segments / pc.total) : 0xFFFFFFFFu;
            // seg ascends with the lane: the first lane of every run of equal segments, and the lanes from itself up to the next run
            const uint32_t before = __shfl_up(seg, 1);
            const bool head = active && (lane == 0 || before != seg);
            const uint64_t heads = __ballot(head);
            const uint64_t above = lane == 63 ? 0ull : heads & ~((2ull << lane) - 1ull);
            const int end = above ? __ffsll((long long)above) - 1 : 64;
            const uint64_t run = (end == 64 ? ~0ull : (1ull << end) - 1ull) & ~((1ull << lane) - 1ull);
            for (uint64_t t = t0; t < t1; ++t) {
                const uint64_t b = (uint64_t)a.map_ub[t];                 // the same in every lane
                const uint64_t l0 = a.leaf_off[b], l1 = a.leaf_off[b + 1];
                bool matched = false;
                uint32_t cur_ixf = 0xFFFFFFFFu;
                IxfDesc d{};
                ixf_probe p{};
                for (uint64_t l = l0; l < l1; ++l) {
                    const uint2 lf = a.leaf[l];
                    if (lf.x != cur_ixf) {                                // a split user bin's parts stand side by side in one IXF: one probe
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
                const uint64_t m = __ballot(matched);
                if (head) {
                    const uint32_t c = (uint32_t)__popcll(m & run);
                    if (c) atomicAdd(a.hits + t * a.segments + seg, c);
                }
            }
        }
    }
    const unsigned long long wave_lookups = wave_incl_add(lookups);     // one atomic per wave
    if (lane == 63 && wave_lookups) atomicAdd(a.probes, wave_lookups);
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

struct taxor_gpu_hitmap {
    taxor_gpu_index *idx = nullptr;
    int device = 0;
    uint32_t segments = 0;
    uint64_t n_bins = 0;
    const IxfDesc *d_ixf = nullptr;
    hipStream_t st = nullptr;
    std::mutex mu;                                    // batches may come from several threads
    DeviceBuf<uint64_t> d_leaf_off, d_hashes[2];
    DeviceBuf<uint2> d_leaf;
    DeviceBuf<Piece> d_pieces[2];
    DeviceBuf<uint32_t> d_err;
    DeviceBuf<unsigned long long> d_probes;
    Piece *h_pieces[2] = {nullptr, nullptr};          // page-locked; ev_free[i] says that buffer i's copy has left it
    hipEvent_t ev_free[2] = {nullptr, nullptr};
    bool ev_used[2] = {false, false};
    std::vector<hipEvent_t> ev_time;                  // pairs around the kernel launches of one batch
    std::vector<uint32_t> h_nh;
    std::map<const void *, std::unique_ptr<Slot>> slots;
    ~taxor_gpu_hitmap()
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

extern "C" int taxor_gpu_hitmap_create(taxor_gpu_index *idx, const taxor_hixf_view *view, uint32_t segments, taxor_gpu_hitmap **out)
{
    if (!out) return fail(TAXOR_E_ARG, "hitmap_create: null argument");
    *out = nullptr;
    if (!idx || !view) return fail(TAXOR_E_ARG, "hitmap_create: null argument");
    if (segments < 1 || segments > HITMAP_MAX_SEGMENTS) return fail(TAXOR_E_ARG, "hitmap_create: segments: %u is not in [1, %u]", segments, HITMAP_MAX_SEGMENTS);
    const IxfDesc *d_ixf = nullptr, *h_ixf = nullptr;
    uint64_t n_ixf = 0, n_bins = 0;
    uint32_t n_passes = 0;
    int device = 0;
    if (taxor_index_descs(idx, &d_ixf, &h_ixf, &n_ixf, &n_bins, &n_passes, &device)) return fail(TAXOR_E_ARG, "hitmap_create: null index");
    if (n_passes)
        return fail(TAXOR_E_ARG, "hitmap_create: a paged index (%u resident pass%s) is refused: its leaf bins are not all resident at once, and locating hits pass by pass is not built",
                    n_passes, n_passes == 1 ? "" : "es");
    if (view->n_ixf != n_ixf || view->n_user_bins != n_bins || (n_ixf && !view->ixf))
        return fail(TAXOR_E_ARG, "hitmap_create: the view (%llu IXFs, %llu user bins) is not the index's (%llu IXFs, %llu user bins)", (unsigned long long)view->n_ixf,
                    (unsigned long long)view->n_user_bins, (unsigned long long)n_ixf, (unsigned long long)n_bins);
    if (n_bins >= (1ull << 32) || n_ixf >= (1ull << 32)) return fail(TAXOR_E_ARG, "hitmap_create: user bins and IXFs are numbered in 32 bits");
    // the inverse of fname_idx: every leaf technical bin of a user bin, root included, as one CSR in index order (the set and the
    // order of coverage.hip's accumulator, restated: that file stays as it is)
    std::vector<uint64_t> leaf_off(n_bins + 1, 0);
    for (uint64_t x = 0; x < n_ixf; ++x) {
        const taxor_ixf_view &f = view->ixf[x];
        if (f.bins != h_ixf[x].bins) return fail(TAXOR_E_ARG, "hitmap_create: IXF %llu has %llu bins in the view, %u in the index", (unsigned long long)x, (unsigned long long)f.bins, h_ixf[x].bins);
        if (!f.fname_idx) return fail(TAXOR_E_ARG, "hitmap_create: IXF %llu of the view has no fname_idx", (unsigned long long)x);
        for (uint64_t j = 0; j < f.bins; ++j) {
            const int64_t b = f.fname_idx[j];
            if (b < 0) continue;
            if ((uint64_t)b >= n_bins) return fail(TAXOR_E_ARG, "hitmap_create: bin %llu of IXF %llu names user bin %lld of %llu", (unsigned long long)j, (unsigned long long)x, (long long)b, (unsigned long long)n_bins);
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
    HM_TRY(hipSetDevice(device));
    auto c = std::make_unique<taxor_gpu_hitmap>();
    c->idx = idx;
    c->device = device;
    c->segments = segments;
    c->n_bins = n_bins;
    c->d_ixf = d_ixf;
    HM_TRY(hipStreamCreate(&c->st));
    HM_TRY(c->d_leaf_off.alloc(n_bins + 1));
    HM_TRY(c->d_leaf.alloc(leaf.size() + 1));
    HM_TRY(c->d_err.alloc(1));
    HM_TRY(c->d_probes.alloc(1));
    for (int i = 0; i < 2; ++i) {
        HM_TRY(c->d_hashes[i].alloc(STAGE_HASHES));
        HM_TRY(c->d_pieces[i].alloc(STAGE_PIECES));
        HM_TRY(hipHostMalloc((void **)&c->h_pieces[i], STAGE_PIECES * sizeof(Piece), hipHostMallocDefault));
        HM_TRY(hipEventCreateWithFlags(&c->ev_free[i], hipEventDisableTiming));
    }
    HM_TRY(hipMemcpy(c->d_leaf_off.p, leaf_off.data(), (n_bins + 1) * 8, hipMemcpyHostToDevice));
    if (!leaf.empty()) HM_TRY(hipMemcpy(c->d_leaf.p, leaf.data(), leaf.size() * 8, hipMemcpyHostToDevice));
    HM_TRY(hipMemset(c->d_err.p, 0, 4));
    *out = c.release();
    return TAXOR_OK;
}

extern "C" void taxor_gpu_hitmap_destroy(taxor_gpu_hitmap *c)
{
    if (!c) return;
    (void)hipSetDevice(c->device);
    delete c;
}

extern "C" int taxor_gpu_hitmap_add_batch(taxor_gpu_hitmap *c, taxor_gpu_searcher *s, const taxor_gpu_saved *saved, taxor_hitmap_batch *out)
{
    if (!c || !s || !out) return fail(TAXOR_E_ARG, "hitmap_add_batch: null argument");
    if (!saved) return fail(TAXOR_E_ARG, "hitmap_add_batch: saved: no saved batch (the batch ran with capture off, or its lists were not taken)");
    if (taxor_searcher_index(s) != c->idx) return fail(TAXOR_E_ARG, "hitmap_add_batch: index: the searcher works on another index than the hit map");
    const std::string unsound = saved_validate(*saved);
    if (!unsound.empty()) return fail(TAXOR_E_ARG, "hitmap_add_batch: " + unsound);
    const uint64_t *d_off = nullptr;
    const int64_t *d_ub = nullptr;
    const uint32_t *d_cnt = nullptr, *d_nh = nullptr;
    uint64_t n = 0, nt = 0;
    int dev = 0;
    if (int rc = taxor_searcher_device_results(s, &d_off, &d_ub, &d_cnt, &d_nh, &n, &nt, &dev)) return rc;
    if (saved->n_reads != n)
        return fail(TAXOR_E_ARG, "hitmap_add_batch: n_reads: the saved batch holds %llu reads, the searcher's last batch %llu", (unsigned long long)saved->n_reads, (unsigned long long)n);
    if (n >= MAX_READS) return fail(TAXOR_E_ARG, "hitmap_add_batch: n_reads: a batch of 2^31 reads or more");
    std::lock_guard<std::mutex> lk(c->mu);
    HM_TRY(hipSetDevice(c->device));
    c->h_nh.resize(n);
    if (n) HM_TRY(hipMemcpy(c->h_nh.data(), d_nh, n * 4, hipMemcpyDeviceToHost));
    for (uint64_t r = 0; r < n; ++r)
        if (c->h_nh[r] != saved->n_hashes[r])
            return fail(TAXOR_E_ARG, "hitmap_add_batch: n_hashes: read %llu has %u hashes in the saved batch, %u in the searcher's last batch", (unsigned long long)r, saved->n_hashes[r], c->h_nh[r]);

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
    if (n == 0) {
        if (int rc = host_block(0)) return rc;
        ((uint64_t *)sl.h)[0] = 0;
        return TAXOR_OK;
    }

    size_t n_ev = 0;
    auto stamp = [&]() -> int {                        // an event on the stream: launches are timed between pairs of them
        if (c->ev_time.size() <= n_ev) {
            hipEvent_t e = nullptr;
            HM_TRY(hipEventCreate(&e));
            c->ev_time.push_back(e);
        }
        HM_TRY(hipEventRecord(c->ev_time[n_ev++], c->st));
        return TAXOR_OK;
    };

    // the mapped tuples: counted, scanned, written in CSR order
    const uint64_t tiles = (n + SCAN_TILE - 1) / SCAN_TILE;
    HM_TRY(sl.d_mapped.reserve(n, n + n / 2));
    HM_TRY(sl.d_map_off.reserve(n + 1, n + 1 + n / 2));
    HM_TRY(sl.d_sums.reserve(tiles, tiles + tiles / 2));
    HM_TRY(hipMemsetAsync(c->d_probes.p, 0, 8, c->st));
    if (int rc = stamp()) return rc;
    k_hm_count<<<grid_for(n, HW, H_GRID_CAP), HB, 0, c->st>>>(d_off, d_ub, d_cnt, d_nh, n, c->n_bins, sl.d_mapped.p, c->d_err.p);
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
        k_hm_fill<<<grid_for(n, HW, H_GRID_CAP), HB, 0, c->st>>>(d_off, d_ub, d_cnt, d_nh, n, c->n_bins, sl.d_map_off.p, sl.d_tuple.p, sl.d_ub.p, sl.d_count.p);
        HM_TRY(hipGetLastError());
        if (int rc = stamp()) return rc;
        HM_TRY(hipStreamSynchronize(c->st));           // map_off is on the host: the pieces are cut from it

        ProbeArgs a{};
        a.ixf = c->d_ixf;
        a.leaf_off = c->d_leaf_off.p;
        a.leaf = c->d_leaf.p;
        a.map_off = sl.d_map_off.p;
        a.map_ub = sl.d_ub.p;
        a.segments = S;
        a.hits = sl.d_hits.p;
        a.probes = c->d_probes.p;
        // Groups of pieces, each staged and launched by itself: at most STAGE_PIECES pieces whose hashes lie within STAGE_HASHES
        // consecutive entries of the dense saved array, copied as one range (the lists of reads without a mapped tuple that lie
        // between two pieces travel with it; those in front of a group's first piece do not).
        int buf = 0;
        uint32_t n_p = 0;
        uint64_t g0 = 0, g1 = 0;            // the group's hashes: [g0, g1) of saved->hashes
        auto flush = [&]() -> int {
            if (n_p == 0) return TAXOR_OK;
            HM_TRY(hipMemcpyAsync(c->d_hashes[buf].p, saved->hashes + g0, (g1 - g0) * 8, hipMemcpyHostToDevice, c->st));
            HM_TRY(hipMemcpyAsync(c->d_pieces[buf].p, c->h_pieces[buf], (uint64_t)n_p * sizeof(Piece), hipMemcpyHostToDevice, c->st));
            HM_TRY(hipEventRecord(c->ev_free[buf], c->st));
            c->ev_used[buf] = true;
            a.pieces = c->d_pieces[buf].p;
            a.hashes = c->d_hashes[buf].p;
            a.n_pieces = n_p;
            if (int rc = stamp()) return rc;
            k_hm_probe<<<grid_for(n_p, HW, H_GRID_CAP), HB, 0, c->st>>>(a);
            HM_TRY(hipGetLastError());
            if (int rc = stamp()) return rc;
            buf ^= 1;
            n_p = 0;
            if (c->ev_used[buf]) HM_TRY(hipEventSynchronize(c->ev_free[buf]));     // the page-locked pieces of two groups ago have been copied
            return TAXOR_OK;
        };
        for (uint64_t r = 0; r < n; ++r) {
            const uint64_t h0 = saved->hash_off[r], nh = saved->n_hashes[r];
            if (nh == 0 || h_map_off[r + 1] == h_map_off[r]) continue;
            for (uint64_t done = 0; done < nh;) {
                const uint32_t take = (uint32_t)std::min<uint64_t>(HM_SPLIT, nh - done);
                if (n_p && (n_p == STAGE_PIECES || h0 + done + take - g0 > STAGE_HASHES))
                    if (int rc = flush()) return rc;
                if (n_p == 0) g0 = h0 + done;
                c->h_pieces[buf][n_p++] = Piece{(uint32_t)r, (uint32_t)(h0 + done - g0), take, (uint32_t)done, (uint32_t)nh};
                done += take;
                g1 = h0 + done;
            }
        }
        if (int rc = flush()) return rc;
        HM_TRY(hipMemcpyAsync((void *)out->tuple, sl.d_tuple.p, m * 8, hipMemcpyDeviceToHost, c->st));
        HM_TRY(hipMemcpyAsync((void *)out->user_bin, sl.d_ub.p, m * 8, hipMemcpyDeviceToHost, c->st));
        HM_TRY(hipMemcpyAsync((void *)out->count, sl.d_count.p, m * 4, hipMemcpyDeviceToHost, c->st));
        HM_TRY(hipMemcpyAsync((void *)out->hits, sl.d_hits.p, m * S * 4, hipMemcpyDeviceToHost, c->st));
    }
    unsigned long long probes = 0;
    HM_TRY(hipMemcpyAsync(&probes, c->d_probes.p, 8, hipMemcpyDeviceToHost, c->st));
    HM_TRY(hipMemcpyAsync(&err, c->d_err.p, 4, hipMemcpyDeviceToHost, c->st));
    HM_TRY(hipStreamSynchronize(c->st));               // the searcher's buffers and the saved lists are the caller's again
    c->ev_used[0] = c->ev_used[1] = false;
    for (size_t i = 0; i + 1 < n_ev; i += 2) {
        float ms = 0;
        HM_TRY(hipEventElapsedTime(&ms, c->ev_time[i], c->ev_time[i + 1]));
        out->seconds_kernels += (double)ms * 1e-3;
    }
    out->probes = probes;
    if (err & HM_BAD_BIN) {
        HM_TRY(hipMemset(c->d_err.p, 0, 4));
        return fail(TAXOR_E_INTERNAL, "hitmap_add_batch: a tuple names a user bin outside the index's %llu", (unsigned long long)c->n_bins);
    }
    return TAXOR_OK;
}
