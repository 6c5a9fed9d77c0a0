// census.hip -- index hashes per reference, read off the resident filter (`taxor census`, `taxor search --coverage-breadth`;
// DESIGN.md section 10.9).  A bin of an interleaved XOR filter gives each of its n keys one slot of its column and leaves every other
// slot at the 0 the builder cleared it to; an assigned slot holds fp ^ (two other slots), uniform over 256 values.  So the nonzero
// bytes of a column are Binomial(n, 255/256) and nonzero * 256 / 255 estimates n (census_format.h).  Counting them is one streaming
// pass over the fingerprints:
//
//   k_census   one block per TILE of a work list the host cuts once per census: a tile is `rows` rows of a column chunk of cw 16-byte
//              units of one IXF, cw a power of two in 4 .. 64 (a stride of S bytes is S / 16 units, a multiple of 4: whole chunks of
//              64, then the binary digits of the rest).  Thread t owns unit t % cw -- 16 bins for the whole tile -- and rows
//              t / cw, t / cw + 256 / cw, ...: with cw = 4 (stride 64) a wave reads 16 consecutive rows, 1 KiB in one piece.  Each
//              16-byte load is tested a dword at a time into four packed byte counters (0x01 per nonzero byte); after at most 252
//              rows the bytes are added to sixteen 32-bit registers.  Lanes of a wave that own the same unit are added by xor
//              shuffles, the block's four waves through LDS, and every bin < `bins` of the chunk gets ONE 64-bit atomic add per tile
//              on a word zeroed before the launch.  Padding columns are read (they lie in the same 16-byte units) and never added.
//
// Sums are integer additions: the words do not depend on the tile size, the grid or the order of the blocks.  Every loop runs to a
// count the tile carries; no block waits on another.
#include "../../include/taxor_gpu_tools.h"
#include "census_format.h"
#include "hip_host.h"
#include "kernels.h"

#include <hip/hip_runtime.h>

#include <cstring>
#include <memory>
#include <string>
#include <vector>

extern "C" __attribute__((visibility("hidden"))) int taxor_index_descs(const taxor_gpu_index *idx, const taxor::IxfDesc **d_ixf, const taxor::IxfDesc **h_ixf,
                                                                       uint64_t *n_ixf, uint64_t *n_user_bins, uint32_t *n_passes, int *device);

namespace {

using namespace taxor;

constexpr int NB = 256;                           // threads per block
constexpr int NW = NB / 64;
constexpr uint32_t CW_MAX = 64;                   // widest column chunk, in 16-byte units (1 KiB of a row)
constexpr uint32_t FLUSH_ROWS = 252;              // rows between two flushes of the packed byte counters: a multiple of the unroll, below 256
constexpr uint32_t UNROLL = 4;
constexpr uint32_t TILE_ITERS_DEFAULT = 512;      // rows per thread and tile: 2 MiB of a 64-unit chunk
constexpr uint32_t TILE_ITERS_MAX = 1u << 20;
constexpr uint32_t GRID_DEFAULT = 2048;           // 256 CUs x 8 blocks
constexpr uint64_t LAUNCH_TILES = 1ull << 24;     // tiles per launch

struct Tile {
    uint32_t ixf;
    uint32_t unit0;      // first 16-byte unit of the column chunk
    uint32_t cw;         // units of the chunk: 4, 8, 16, 32 or 64
    uint32_t row0;
    uint32_t rows;       // at most iters * (NB / cw)
    uint32_t iters;      // rows per thread: ceil(rows / (NB / cw))
};

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef const u32x4 __attribute__((address_space(1))) *gptr128;

// 0x01 in every byte of w that is not zero
__device__ __forceinline__ uint32_t nonzero_bytes(uint32_t w)
{
    return ((w | ((w & 0x7F7F7F7Fu) + 0x7F7F7F7Fu)) >> 7) & 0x01010101u;
}

__global__ __launch_bounds__(NB) void k_census(const IxfDesc *__restrict__ ixf, const Tile *__restrict__ tiles, uint64_t n_tiles, unsigned long long *__restrict__ nonzero)
{
    __shared__ uint32_t s_sum[NW][16 * CW_MAX];   // [wave][byte * 64 + unit]
    const uint32_t t = threadIdx.x, lane = t & 63u, wave = t >> 6;
    for (uint64_t ti = blockIdx.x; ti < n_tiles; ti += gridDim.x) {
        const Tile tl = tiles[ti];
        const IxfDesc d = ixf[tl.ixf];
        const uint32_t unit = tl.unit0 + (t & (tl.cw - 1u)), step = NB / tl.cw;
        const uint64_t row_end = (uint64_t)tl.row0 + tl.rows;      // 64 bits: a row number past the tile must not wrap into it
        const uint8_t *col = d.data + (uint64_t)unit * 16u;
        uint32_t acc[16];
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[i] = 0;
        uint64_t r = (uint64_t)tl.row0 + t / tl.cw;
        for (uint32_t k0 = 0; k0 < tl.iters; k0 += FLUSH_ROWS) {
            const uint32_t k1 = k0 + FLUSH_ROWS < tl.iters ? k0 + FLUSH_ROWS : tl.iters;
            uint32_t pk[4] = {0, 0, 0, 0};
            for (uint32_t k = k0; k < k1; k += UNROLL) {
                u32x4 v[UNROLL];
                if (k + UNROLL <= k1 && r + (UNROLL - 1) * step < row_end) {      // all four rows are the tile's: four loads in flight
#pragma unroll
                    for (uint32_t u = 0; u < UNROLL; ++u) v[u] = __builtin_nontemporal_load((gptr128)(uintptr_t)(col + (r + u * step) * d.stride));
                } else {
#pragma unroll
                    for (uint32_t u = 0; u < UNROLL; ++u) {
                        const uint64_t ru = r + u * step;
                        v[u] = (u32x4){0, 0, 0, 0};
                        if (k + u < k1 && ru < row_end) v[u] = __builtin_nontemporal_load((gptr128)(uintptr_t)(col + ru * d.stride));
                    }
                }
#pragma unroll
                for (uint32_t u = 0; u < UNROLL; ++u) {
                    pk[0] += nonzero_bytes(v[u].x);
                    pk[1] += nonzero_bytes(v[u].y);
                    pk[2] += nonzero_bytes(v[u].z);
                    pk[3] += nonzero_bytes(v[u].w);
                }
                r += UNROLL * step;
            }
#pragma unroll
            for (int i = 0; i < 16; ++i) acc[i] += (pk[i >> 2] >> (8 * (i & 3))) & 0xFFu;
        }
        // lanes l, l + cw, l + 2 cw, ... of a wave own the same unit
        for (uint32_t o = 32; o >= tl.cw; o >>= 1) {
#pragma unroll
            for (int i = 0; i < 16; ++i) acc[i] += __shfl_xor(acc[i], (int)o);
        }
        if (lane < tl.cw) {
#pragma unroll
            for (int i = 0; i < 16; ++i) s_sum[wave][i * CW_MAX + lane] = acc[i];
        }
        __syncthreads();
        for (uint32_t c = t; c < tl.cw * 16u; c += NB) {
            const uint32_t bin = tl.unit0 * 16u + c, at = (c & 15u) * CW_MAX + (c >> 4);
            const uint32_t sum = s_sum[0][at] + s_sum[1][at] + s_sum[2][at] + s_sum[3][at];
            if (bin < d.bins && sum) atomicAdd(nonzero + d.bin_base + bin, (unsigned long long)sum);
        }
        __syncthreads();
    }
}

#define CEN_TRY(expr) TAXOR_HIP_TRY_PREFIX("census", expr, #expr)

}   // namespace

struct taxor_gpu_census {
    taxor_gpu_index *idx = nullptr;
    int device = 0;
    const IxfDesc *d_ixf = nullptr;
    std::vector<IxfDesc> h_ixf;
    uint64_t n_user_bins = 0, total_bins = 0, bytes = 0;
    uint32_t tile_iters = 0;                      // the cut the work list on the device follows; 0 = none yet
    uint64_t n_tiles = 0;
    hipStream_t st = nullptr;
    hipEvent_t ev[2] = {nullptr, nullptr};
    DeviceBuf<Tile> d_tiles;
    DeviceBuf<unsigned long long> d_nonzero;
    std::vector<uint64_t> r_nonzero, r_bin_first;
    ~taxor_gpu_census()
    {
        for (hipEvent_t e : ev)
            if (e) (void)hipEventDestroy(e);
        if (st) (void)hipStreamDestroy(st);
    }
};

extern "C" int taxor_gpu_census_create(taxor_gpu_index *idx, taxor_gpu_census **out)
{
    if (!out) return fail(TAXOR_E_ARG, "census_create: null argument");
    *out = nullptr;
    if (!idx) return fail(TAXOR_E_ARG, "census_create: null argument");
    const IxfDesc *d_ixf = nullptr, *h_ixf = nullptr;
    uint64_t n_ixf = 0, n_bins = 0;
    uint32_t n_passes = 0;
    int device = 0;
    if (taxor_index_descs(idx, &d_ixf, &h_ixf, &n_ixf, &n_bins, &n_passes, &device)) return fail(TAXOR_E_ARG, "census_create: null index");
    if (n_passes)
        return fail(TAXOR_E_ARG, "census_create: a paged index (%u resident pass%s) is refused: its IXFs are not all resident at once, and counting pass by pass is not built",
                    n_passes, n_passes == 1 ? "" : "es");
    auto c = std::make_unique<taxor_gpu_census>();
    c->idx = idx;
    c->device = device;
    c->d_ixf = d_ixf;
    c->h_ixf.assign(h_ixf, h_ixf + n_ixf);
    c->n_user_bins = n_bins;
    c->r_bin_first.resize(n_ixf + 1);
    for (uint64_t x = 0; x < n_ixf; ++x) {
        const IxfDesc &d = c->h_ixf[x];
        if (d.stride % 64 != 0 || d.stride < d.bins || d.bin_base != c->total_bins)
            return fail(TAXOR_E_INTERNAL, "census_create: IXF %llu: stride %u, %u bins from bin %u do not follow the search layout", (unsigned long long)x, d.stride, d.bins, d.bin_base);
        c->r_bin_first[x] = c->total_bins;
        c->total_bins += d.bins;
        c->bytes += 3ull * d.seg_len * d.stride;
    }
    c->r_bin_first[n_ixf] = c->total_bins;
    CEN_TRY(hipSetDevice(device));
    CEN_TRY(hipStreamCreateWithFlags(&c->st, hipStreamNonBlocking));
    CEN_TRY(hipEventCreate(&c->ev[0]));
    CEN_TRY(hipEventCreate(&c->ev[1]));
    CEN_TRY(c->d_nonzero.alloc(c->total_bins + 1));
    *out = c.release();
    return TAXOR_OK;
}

extern "C" void taxor_gpu_census_destroy(taxor_gpu_census *c)
{
    if (!c) return;
    (void)hipSetDevice(c->device);
    delete c;
}

// the work list for `tile_iters` rows per thread and tile, in index order
static void census_cut(const std::vector<IxfDesc> &ixf, uint32_t tile_iters, std::vector<Tile> &tiles)
{
    tiles.clear();
    for (size_t x = 0; x < ixf.size(); ++x) {
        const uint32_t units = ixf[x].stride / 16, rows = 3u * ixf[x].seg_len;
        for (uint32_t u0 = 0; u0 < units;) {
            uint32_t cw = CW_MAX;
            while (cw > units - u0) cw >>= 1;     // units - u0 is a multiple of 4: cw ends at 4 or above
            const uint64_t tile_rows = (uint64_t)tile_iters * (NB / cw);
            for (uint64_t r0 = 0; r0 < rows; r0 += tile_rows) {
                const uint32_t n = (uint32_t)std::min<uint64_t>(tile_rows, rows - r0);
                tiles.push_back(Tile{(uint32_t)x, u0, cw, (uint32_t)r0, n, (n + NB / cw - 1) / (NB / cw)});
            }
            u0 += cw;
        }
    }
}

extern "C" int taxor_gpu_census_run(taxor_gpu_census *c, uint32_t tile_iters, uint32_t max_blocks, taxor_census_results *out)
{
    if (!c || !out) return fail(TAXOR_E_ARG, "census_run: null argument");
    if (tile_iters == 0) tile_iters = TILE_ITERS_DEFAULT;
    if (tile_iters > TILE_ITERS_MAX) return fail(TAXOR_E_ARG, "census_run: tile_iters %u above %u", tile_iters, TILE_ITERS_MAX);
    if (max_blocks == 0) max_blocks = GRID_DEFAULT;
    if (max_blocks > (1u << 20)) return fail(TAXOR_E_ARG, "census_run: max_blocks %u above %u", max_blocks, 1u << 20);
    CEN_TRY(hipSetDevice(c->device));
    if (c->tile_iters != tile_iters) {
        std::vector<Tile> tiles;
        census_cut(c->h_ixf, tile_iters, tiles);
        CEN_TRY(c->d_tiles.reserve(tiles.size() + 1, tiles.size() + 1));
        if (!tiles.empty()) CEN_TRY(hipMemcpy(c->d_tiles.p, tiles.data(), tiles.size() * sizeof(Tile), hipMemcpyHostToDevice));
        c->n_tiles = tiles.size();
        c->tile_iters = tile_iters;
    }
    CEN_TRY(hipMemsetAsync(c->d_nonzero.p, 0, (c->total_bins + 1) * 8, c->st));     // counters are zeroed per call
    CEN_TRY(hipEventRecord(c->ev[0], c->st));
    uint32_t launches = 0;
    for (uint64_t t0 = 0; t0 < c->n_tiles; t0 += LAUNCH_TILES, ++launches) {
        const uint64_t n = std::min<uint64_t>(LAUNCH_TILES, c->n_tiles - t0);
        k_census<<<grid_for(n, 1, max_blocks), NB, 0, c->st>>>(c->d_ixf, c->d_tiles.p + t0, n, c->d_nonzero.p);
        CEN_TRY(hipGetLastError());
    }
    CEN_TRY(hipEventRecord(c->ev[1], c->st));
    c->r_nonzero.resize(c->total_bins);
    if (c->total_bins) CEN_TRY(hipMemcpyAsync(c->r_nonzero.data(), c->d_nonzero.p, c->total_bins * 8, hipMemcpyDeviceToHost, c->st));
    CEN_TRY(hipStreamSynchronize(c->st));
    float ms = 0;
    CEN_TRY(hipEventElapsedTime(&ms, c->ev[0], c->ev[1]));
    out->n_ixf = c->h_ixf.size();
    out->n_bins = c->total_bins;
    out->n_user_bins = c->n_user_bins;
    out->bin_first = c->r_bin_first.data();
    out->nonzero = c->r_nonzero.data();
    out->seconds_kernel = (double)ms * 1e-3;
    out->bytes_read = c->bytes;
    out->n_tiles = c->n_tiles;
    out->launches = launches;
    out->reserved = 0;
    return TAXOR_OK;
}

// ---- host only: census_format.h for a binding (tests/test_census_cpu.py compares these with restatements)
extern "C" uint64_t taxor_census_keys_est(uint64_t nonzero) { return census_keys_est(nonzero); }
extern "C" uint64_t taxor_census_capacity(uint64_t seg_len) { return census_capacity(seg_len); }
extern "C" int taxor_census_peeled(uint64_t nonzero, uint64_t seg_len) { return census_peeled(nonzero, census_capacity(seg_len)) ? 1 : 0; }

static uint64_t census_copy_out(const std::string &s, char *buf, uint64_t cap)
{
    if (buf && cap) {
        const uint64_t n = std::min<uint64_t>(cap - 1, s.size());
        memcpy(buf, s.data(), n);
        buf[n] = '\0';
    }
    return s.size();
}

extern "C" uint64_t taxor_census_ref_line(const char *accession, const char *name, const char *taxid, uint64_t ref_len, uint64_t leaf_bins, uint64_t index_hashes, int flagged,
                                          char *buf, uint64_t cap)
{
    std::string s;
    census_ref_line(s, accession, name, taxid, ref_len, leaf_bins, census_count{index_hashes, flagged != 0});
    return census_copy_out(s, buf, cap);
}

extern "C" uint64_t taxor_census_ixf_line(uint64_t ixf, uint64_t bins, uint64_t leaf_bins, uint64_t seg_len, uint64_t stride, uint64_t max_bin_keys, int flagged, char *buf,
                                          uint64_t cap)
{
    std::string s;
    census_ixf_line(s, ixf, bins, leaf_bins, seg_len, stride, census_count{max_bin_keys, flagged != 0});
    return census_copy_out(s, buf, cap);
}

extern "C" uint64_t taxor_census_breadth_columns(uint64_t distinct, uint64_t hash_matches, uint64_t index_hashes, int flagged, char *buf, uint64_t cap)
{
    std::string s;
    census_breadth_columns(s, distinct, hash_matches, census_count{index_hashes, flagged != 0});
    return census_copy_out(s, buf, cap);
}
