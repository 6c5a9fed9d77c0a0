// fastx_scan.hip -- FASTA / four-line FASTQ record scanning on the device: raw file bytes in, the
// searcher's packed batch and a per-record table out.  The host's part per base is the copy of the bytes; per record it reads
// the table (id position, id length, read length).
//
// Grammar: that of fastx::FastxReader::next in range mode (fastx.h; strict4 for FASTQ).  A line ends at '\n' or at the end of the
// buffer; exactly one '\r' directly before that end belongs to the terminator, any other '\r' is an ordinary byte (and fails
// the alphabet check).  FASTA: blank lines before the first record are skipped; a record is a line beginning with '>' and every
// line up to the next such line, its sequence those lines without terminators.  FASTQ: between the first and the last
// non-blank line, line 4i begins with '@', line 4i+2 with '+', line 4i+3 is as long as line 4i+1 (lines past the end of the
// buffer count as empty: the last record's empty quality line may be missing).  Anything else -- a blank line between two
// FASTQ records, a wrapped FASTQ sequence, a length mismatch, a first non-blank byte that is not the record character -- raises
// TAXOR_FASTX_IRREGULAR: one status word, nothing else is written, the caller parses the range on the host.
//
//   k_fx_count_nl      newlines per tile of FX_TILE bytes: ballot + popcount, a wave over 64 bytes at a time
//   k_fx_line_starts   the same ballots again, ranked by the scanned tile counts: ls[j] = first byte of line j
//   k_fx_lines         per line: content length (without terminator); FASTA: header flag, base count; FASTQ: first/last non-blank line
//   k_fx_fasta_records per header line: record -> line, id position and length (the scan of the header flags numbers the records)
//   k_fx_fasta_lens    per record: read length from the per-line base prefix
//   k_fx_fastq_records per record: the four-line checks, id, sequence position, read length
//   k_fx_pack_fasta    16 bases per thread; a word finds its first line by bisection of the base prefix within its record
//   k_fx_pack_fastq    16 bases per thread from one contiguous line
//   k_fx_scan_*        exclusive 64-bit scan in three launches (tile-local, the tile sums by one block, add back): the pattern of
//                      k_ff_scan_* in profile_feed.hip.  No block waits on another; every loop is bounded by a count it is given.
//
// All positions are 64-bit.  A buffer of 2^40 bytes or more is refused with TAXOR_E_ARG (one block per tile: the grid).
#include "../../include/taxor_gpu_tools.h"
#include "device_prims.h"
#include "fastx_scan.h"
#include "hip_host.h"
#include "tuning.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <vector>

namespace taxor {

namespace {

constexpr int XB = 256;                  // threads per block
constexpr int XW = XB / 64;
constexpr int FX_STEPS = 16;             // 64-byte steps of a wave
constexpr uint64_t FX_WAVE_BYTES = 64 * FX_STEPS;
constexpr uint64_t FX_TILE = XW * FX_WAVE_BYTES;   // 4096 bytes per block
constexpr int SCAN_ITEMS = 8;
constexpr int SCAN_TILE = XB * SCAN_ITEMS;
constexpr int X_GRID_CAP = 4096;
constexpr uint64_t FX_MAX_BYTES = 1ull << 40;

// state words on the device
enum { ST_STATUS = 0, ST_FIRST = 1, ST_LAST = 2, ST_WORDS = 4 };

__device__ __forceinline__ uint64_t fx_tid() { return (uint64_t)blockIdx.x * XB + threadIdx.x; }
__device__ __forceinline__ uint64_t fx_step() { return (uint64_t)gridDim.x * XB; }

__global__ __launch_bounds__(XB) void k_fx_count_nl(const uint8_t *__restrict__ raw, uint64_t n, uint64_t *__restrict__ tile_cnt)
{
    const uint64_t wbase = (uint64_t)blockIdx.x * FX_TILE + (uint64_t)(threadIdx.x >> 6) * FX_WAVE_BYTES;
    uint32_t cnt = 0;
#pragma unroll
    for (int s = 0; s < FX_STEPS; ++s) {
        const uint64_t pos = wbase + (uint64_t)s * 64 + lane_id();
        cnt += (uint32_t)__popcll(__ballot(pos < n && raw[pos] == '\n'));
    }
    __shared__ uint32_t sW[XW];
    if (lane_id() == 0) sW[threadIdx.x >> 6] = cnt;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint64_t t = 0;
#pragma unroll
        for (int w = 0; w < XW; ++w) t += sW[w];
        tile_cnt[blockIdx.x] = t;
    }
}

// tile_off = exclusive scan of the tile counts, tile_off[n_tiles] = all newlines.  ls[0] = 0, ls[i + 1] = the byte after newline i;
// a last line without a newline ends as if one stood at raw[n]: ls[lines] = n + 1
__global__ __launch_bounds__(XB) void k_fx_line_starts(const uint8_t *__restrict__ raw, uint64_t n, const uint64_t *__restrict__ tile_off,
                                                       uint64_t n_tiles, uint64_t *__restrict__ ls)
{
    const uint32_t w = threadIdx.x >> 6;
    const uint64_t wbase = (uint64_t)blockIdx.x * FX_TILE + (uint64_t)w * FX_WAVE_BYTES;
    uint64_t m[FX_STEPS];
    uint32_t cnt = 0;
#pragma unroll
    for (int s = 0; s < FX_STEPS; ++s) {
        const uint64_t pos = wbase + (uint64_t)s * 64 + lane_id();
        m[s] = __ballot(pos < n && raw[pos] == '\n');
        cnt += (uint32_t)__popcll(m[s]);
    }
    __shared__ uint32_t sW[XW];
    if (lane_id() == 0) sW[w] = cnt;
    __syncthreads();
    uint64_t rank = tile_off[blockIdx.x];
#pragma unroll
    for (uint32_t i = 0; i < (uint32_t)XW; ++i)
        if (i < w) rank += sW[i];
    const uint64_t below = (1ull << lane_id()) - 1ull;
#pragma unroll
    for (int s = 0; s < FX_STEPS; ++s) {
        if ((m[s] >> lane_id()) & 1ull) ls[1 + rank + (uint64_t)__popcll(m[s] & below)] = wbase + (uint64_t)s * 64 + lane_id() + 1;
        rank += (uint64_t)__popcll(m[s]);
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        ls[0] = 0;
        if (raw[n - 1] != '\n') ls[tile_off[n_tiles] + 1] = n + 1;
    }
}

// line j is raw[ls[j], ls[j + 1] - 1) followed by its terminator; clen = its length without one trailing '\r'
__global__ __launch_bounds__(XB) void k_fx_lines(const uint8_t *__restrict__ raw, const uint64_t *__restrict__ ls, uint64_t n_lines, int kind,
                                                 uint64_t *__restrict__ clen, uint64_t *__restrict__ hflag, uint64_t *__restrict__ nbase,
                                                 unsigned long long *__restrict__ state)
{
    unsigned long long first = ~0ull, last = 0;
    bool any = false;
    for (uint64_t j = fx_tid(); j < n_lines; j += fx_step()) {
        const uint64_t s = ls[j], t = ls[j + 1] - 1;
        uint64_t len = t - s;
        if (len && raw[t - 1] == '\r') --len;
        clen[j] = len;
        if (kind == '>') {
            const bool h = t > s && raw[s] == '>';
            hflag[j] = h ? 1 : 0;
            nbase[j] = h ? 0 : len;
        } else if (len) {
            first = any ? first : j;
            last = j;
            any = true;
        }
    }
    if (kind != '>' && any) {
        atomicMin(&state[ST_FIRST], first);
        atomicMax(&state[ST_LAST], last);
    }
}

// H = exclusive scan of hflag (H[n_lines] = records), so header line j opens record H[j]
__global__ __launch_bounds__(XB) void k_fx_fasta_records(const uint64_t *__restrict__ ls, const uint64_t *__restrict__ clen,
                                                         const uint64_t *__restrict__ hflag, const uint64_t *__restrict__ H,
                                                         const uint64_t *__restrict__ nbase, uint64_t n_lines, uint64_t *__restrict__ rec_line,
                                                         uint64_t *__restrict__ id_off, uint64_t *__restrict__ id_len,
                                                         unsigned long long *__restrict__ state)
{
    bool bad = false;
    for (uint64_t j = fx_tid(); j < n_lines; j += fx_step()) {
        const uint64_t r = H[j];
        if (hflag[j]) {
            rec_line[r] = j;
            id_off[r] = ls[j] + 1;
            id_len[r] = clen[j] - 1;
        } else if (nbase[j] && r == 0) {
            bad = true;                                   // sequence before the first header
        }
    }
    if (bad) atomicOr(&state[ST_STATUS], (unsigned long long)TAXOR_FASTX_IRREGULAR);
    if (fx_tid() == 0) rec_line[H[n_lines]] = n_lines;
}

// B = exclusive scan of nbase: record r holds bases [B[rec_line[r]], B[rec_line[r + 1]])
__global__ __launch_bounds__(XB) void k_fx_fasta_lens(const uint64_t *__restrict__ rec_line, const uint64_t *__restrict__ B,
                                                      const uint64_t *__restrict__ n_recs, uint64_t *__restrict__ rlen)
{
    const uint64_t n = n_recs[0];
    for (uint64_t r = fx_tid(); r < n; r += fx_step()) rlen[r] = B[rec_line[r + 1]] - B[rec_line[r]];
}

// record r = lines first + 4r .. first + 4r + 3; a line past the buffer is empty
__global__ __launch_bounds__(XB) void k_fx_fastq_records(const uint8_t *__restrict__ raw, const uint64_t *__restrict__ ls,
                                                         const uint64_t *__restrict__ clen, uint64_t n_lines, uint64_t first, uint64_t n_recs,
                                                         uint64_t *__restrict__ id_off, uint64_t *__restrict__ id_len,
                                                         uint64_t *__restrict__ rlen, uint64_t *__restrict__ seq_off,
                                                         unsigned long long *__restrict__ state)
{
    bool bad = false;
    for (uint64_t r = fx_tid(); r < n_recs; r += fx_step()) {
        const uint64_t j = first + 4 * r;                 // < n_lines: the host counted the records from the last non-blank line
        const uint64_t l0 = clen[j];
        const uint64_t l1 = j + 1 < n_lines ? clen[j + 1] : 0, l3 = j + 3 < n_lines ? clen[j + 3] : 0;
        const bool at = l0 && raw[ls[j]] == '@';
        const bool plus = j + 2 < n_lines && clen[j + 2] && raw[ls[j + 2]] == '+';
        bad |= !at || !plus || l1 != l3;
        id_off[r] = ls[j] + 1;
        id_len[r] = l0 ? l0 - 1 : 0;
        rlen[r] = l1;
        seq_off[r] = j + 1 < n_lines ? ls[j + 1] : 0;
    }
    if (bad) atomicOr(&state[ST_STATUS], (unsigned long long)TAXOR_FASTX_IRREGULAR);
}

// ---- packing: one block per read (grid-stride), one thread per 16-base word, the words of a read padded to a multiple of four
__global__ __launch_bounds__(XB) void k_fx_pack_fastq(const uint8_t *__restrict__ raw, const uint64_t *__restrict__ seq_off,
                                                      const uint32_t *__restrict__ rlen, const uint64_t *__restrict__ poff,
                                                      uint32_t *__restrict__ packed, uint64_t n_reads, Counters *ctr)
{
    for (uint64_t r = blockIdx.x; r < n_reads; r += gridDim.x) {
        const uint8_t *src = raw + seq_off[r];
        const uint32_t len = rlen[r];
        const uint32_t nw = (len + 15u) >> 4, nw_pad = (nw + 3u) & ~3u;
        uint32_t *dst = packed + poff[r];
        bool bad = false;
        for (uint32_t w = threadIdx.x; w < nw_pad; w += XB) {
            uint32_t word = 0;
#pragma unroll
            for (uint32_t c = 0; c < 16; ++c) {
                const uint32_t pos = (w << 4) + c;
                if (w < nw && pos < len) {
                    uint32_t code = dna4_code(src[pos]);
                    if (code == 0xFFu) { bad = true; code = 0; }
                    word |= code << (30u - 2u * c);
                }
            }
            dst[w] = word;
        }
        if (__any(bad) && lane_id() == 0) atomicOr(&ctr->flags, FLAG_ALPHABET);
    }
}

__global__ __launch_bounds__(XB) void k_fx_pack_fasta(const uint8_t *__restrict__ raw, const uint64_t *__restrict__ ls,
                                                      const uint64_t *__restrict__ nbase, const uint64_t *__restrict__ B,
                                                      const uint64_t *__restrict__ rec_line, const uint32_t *__restrict__ rlen,
                                                      const uint64_t *__restrict__ poff, uint32_t *__restrict__ packed, uint64_t n_reads,
                                                      Counters *ctr)
{
    for (uint64_t r = blockIdx.x; r < n_reads; r += gridDim.x) {
        const uint64_t hdr = rec_line[r], end = rec_line[r + 1];   // the record's lines are (hdr, end)
        const uint64_t g0 = B[hdr];
        const uint32_t len = rlen[r];
        const uint32_t nw = (len + 15u) >> 4, nw_pad = (nw + 3u) & ~3u;
        uint32_t *dst = packed + poff[r];
        bool bad = false;
        for (uint32_t w = threadIdx.x; w < nw_pad; w += XB) {
            uint32_t word = 0;
            if (w < nw) {
                // the last line of the record whose first base is at or before base g: B does not decrease, and among lines
                // that share a B (empty ones) the last is the one that holds the base
                const uint64_t g = g0 + ((uint64_t)w << 4);
                uint64_t a = hdr + 1, z = end;
                for (int it = 0; it < 64 && z - a > 1; ++it) {
                    const uint64_t mid = a + ((z - a) >> 1);
                    if (B[mid] <= g) a = mid;
                    else z = mid;
                }
                uint64_t j = a, in = g - B[a], have = nbase[a];
                const uint32_t nb = min(16u, len - (w << 4));
                for (uint32_t c = 0; c < nb; ++c) {
                    while (in >= have && j + 1 < end) {          // next line of the record; bounded by its line count
                        in -= have;
                        have = nbase[++j];
                    }
                    uint32_t code = dna4_code(raw[ls[j] + in]);
                    ++in;
                    if (code == 0xFFu) { bad = true; code = 0; }
                    word |= code << (30u - 2u * c);
                }
            }
            dst[w] = word;
        }
        if (__any(bad) && lane_id() == 0) atomicOr(&ctr->flags, FLAG_ALPHABET);
    }
}

// ---- exclusive scan of in[n] into out[n + 1] (out[n] = the total)
__global__ __launch_bounds__(XB) void k_fx_scan_tiles(const uint64_t *__restrict__ in, uint64_t n, uint64_t *__restrict__ out, uint64_t *__restrict__ sums)
{
    const uint64_t first = (uint64_t)blockIdx.x * SCAN_TILE + (uint64_t)threadIdx.x * SCAN_ITEMS;
    uint64_t v[SCAN_ITEMS], mine = 0;
#pragma unroll
    for (int j = 0; j < SCAN_ITEMS; ++j) {
        v[j] = first + j < n ? in[first + j] : 0;
        mine += v[j];
    }
    __shared__ uint64_t sScr[XW];
    uint64_t total;
    uint64_t run = block_excl_add<XW>(mine, sScr, &total);
#pragma unroll
    for (int j = 0; j < SCAN_ITEMS; ++j) {
        if (first + j < n) out[first + j] = run;
        run += v[j];
    }
    if (threadIdx.x == 0) sums[blockIdx.x] = total;
}

__global__ __launch_bounds__(XB) void k_fx_scan_sums(uint64_t *__restrict__ sums, uint64_t n_tiles, uint64_t *__restrict__ out_total)
{
    __shared__ uint64_t sScr[XW];
    uint64_t carry = 0;
    for (uint64_t base = 0; base < n_tiles; base += XB) {
        const uint64_t i = base + threadIdx.x;
        const uint64_t v = i < n_tiles ? sums[i] : 0;
        uint64_t total;
        const uint64_t ex = block_excl_add<XW>(v, sScr, &total);
        if (i < n_tiles) sums[i] = carry + ex;
        carry += total;
    }
    if (threadIdx.x == 0) out_total[0] = carry;
}

__global__ __launch_bounds__(XB) void k_fx_scan_add(uint64_t *__restrict__ out, uint64_t n, const uint64_t *__restrict__ sums)
{
    const uint64_t first = (uint64_t)blockIdx.x * SCAN_TILE + (uint64_t)threadIdx.x * SCAN_ITEMS;
    const uint64_t add = sums[blockIdx.x];
#pragma unroll
    for (int j = 0; j < SCAN_ITEMS; ++j)
        if (first + j < n) out[first + j] += add;
}

#define FX_TRY(expr) TAXOR_HIP_TRY_PREFIX("fastx_scan", expr, #expr)

hipError_t room(DeviceBuf<uint64_t> &b, uint64_t n) { return b.reserve(n, n + n / 8 + 64); }

}   // namespace

struct FastxScan {
    DeviceBuf<uint64_t> tile_cnt, tile_off, sums, ls, clen, hflag, H, nbase, B, rec_line, id_off, id_len, rlen, seq_off, state;
    std::vector<uint64_t> h_id_off, h_id_len, h_rlen;
    int kind = 0;
    uint64_t n_lines = 0, n_recs = 0;
    // TAXOR_FASTX_TRACE (under TAXOR_TUNING): HIP-event time of the kernels, segment by segment between the host's waits; the sum
    // goes to stderr when the scanner is destroyed
    bool timed = false;
    hipEvent_t ev[8] = {};
    int ev_open = 0;                     // pairs recorded since the last harvest
    double ms = 0;
    uint64_t calls = 0, bytes = 0;
    void mark(hipStream_t st) { if (timed && ev_open < 8) (void)hipEventRecord(ev[ev_open++], st); }
    void harvest()                       // after a wait on the stream: every recorded pair has finished
    {
        for (int i = 0; i + 1 < ev_open; i += 2) {
            float t = 0;
            if (hipEventElapsedTime(&t, ev[i], ev[i + 1]) == hipSuccess) ms += t;
        }
        ev_open = 0;
    }
};

namespace {

// in[n] -> out[n + 1] on st (n > 0)
int scan64(FastxScan *fx, const uint64_t *in, uint64_t n, uint64_t *out, hipStream_t st)
{
    const uint64_t tiles = (n + SCAN_TILE - 1) / SCAN_TILE;
    FX_TRY(room(fx->sums, tiles));
    k_fx_scan_tiles<<<(int)tiles, XB, 0, st>>>(in, n, out, fx->sums.p);
    k_fx_scan_sums<<<1, XB, 0, st>>>(fx->sums.p, tiles, out + n);
    k_fx_scan_add<<<(int)tiles, XB, 0, st>>>(out, n, fx->sums.p);
    FX_TRY(hipGetLastError());
    return TAXOR_OK;
}

}   // namespace

FastxScan *fastx_scan_create()
{
    FastxScan *fx = new FastxScan();
    if (tune_env("TAXOR_FASTX_TRACE")) {
        fx->timed = true;
        for (auto &e : fx->ev)
            if (hipEventCreate(&e) != hipSuccess) fx->timed = false;
    }
    return fx;
}

void fastx_scan_destroy(FastxScan *fx)
{
    if (fx->timed) {
        fx->harvest();                   // (the searcher has waited for its streams)
        fprintf(stderr, "[fastx_scan] %llu calls, %llu bytes: %.3f ms in the scan and pack kernels (HIP events)\n", (unsigned long long)fx->calls,
                (unsigned long long)fx->bytes, fx->ms);
        for (auto &e : fx->ev)
            if (e) (void)hipEventDestroy(e);
    }
    delete fx;
}

int fastx_scan_records(FastxScan *fx, const uint8_t *d_raw, uint64_t n_bytes, int kind, uint8_t last_byte, hipStream_t st, FastxTable *out)
{
    if (kind != '>' && kind != '@') return fail(TAXOR_E_ARG, "search_fastx_begin: kind is neither '>' (FASTA) nor '@' (FASTQ)");
    if (n_bytes >= FX_MAX_BYTES) return fail(TAXOR_E_ARG, "search_fastx_begin: a buffer of 2^40 bytes or more is not scanned in one call");
    fx->kind = kind;
    fx->n_lines = fx->n_recs = 0;
    *out = FastxTable{0, nullptr, nullptr, nullptr, 0};
    if (n_bytes == 0) return TAXOR_OK;
    if (fx->timed) {
        if (hipStreamSynchronize(st) == hipSuccess) fx->harvest();      // the previous call's pack kernel
        ++fx->calls;
        fx->bytes += n_bytes;
    }
    // lines
    const uint64_t tiles = (n_bytes + FX_TILE - 1) / FX_TILE;
    FX_TRY(room(fx->tile_cnt, tiles));
    FX_TRY(room(fx->tile_off, tiles + 1));
    FX_TRY(room(fx->state, ST_WORDS));
    fx->mark(st);
    k_fx_count_nl<<<(int)tiles, XB, 0, st>>>(d_raw, n_bytes, fx->tile_cnt.p);
    FX_TRY(hipGetLastError());
    if (int rc = scan64(fx, fx->tile_cnt.p, tiles, fx->tile_off.p, st)) return rc;
    fx->mark(st);
    uint64_t n_nl = 0;
    FX_TRY(hipMemcpyAsync(&n_nl, fx->tile_off.p + tiles, 8, hipMemcpyDeviceToHost, st));
    FX_TRY(hipStreamSynchronize(st));
    const uint64_t L = n_nl + (last_byte != '\n' ? 1 : 0);
    fx->n_lines = L;
    FX_TRY(room(fx->ls, L + 2));
    FX_TRY(room(fx->clen, L));
    static const uint64_t h_state[ST_WORDS] = {0, ~0ull, 0, 0};
    FX_TRY(hipMemcpyAsync(fx->state.p, h_state, sizeof h_state, hipMemcpyHostToDevice, st));
    fx->mark(st);
    k_fx_line_starts<<<(int)tiles, XB, 0, st>>>(d_raw, n_bytes, fx->tile_off.p, tiles, fx->ls.p);
    FX_TRY(hipGetLastError());
    unsigned long long *d_state = reinterpret_cast<unsigned long long *>(fx->state.p);
    const int g_lines = grid_for(L, XB, X_GRID_CAP);
    uint64_t h_back[ST_WORDS] = {0, 0, 0, 0};
    uint64_t R = 0;
    if (kind == '>') {
        FX_TRY(room(fx->hflag, L));
        FX_TRY(room(fx->H, L + 1));
        FX_TRY(room(fx->nbase, L));
        FX_TRY(room(fx->B, L + 1));
        FX_TRY(room(fx->rec_line, L + 1));
        FX_TRY(room(fx->id_off, L));
        FX_TRY(room(fx->id_len, L));
        FX_TRY(room(fx->rlen, L));
        k_fx_lines<<<g_lines, XB, 0, st>>>(d_raw, fx->ls.p, L, kind, fx->clen.p, fx->hflag.p, fx->nbase.p, d_state);
        FX_TRY(hipGetLastError());
        if (int rc = scan64(fx, fx->hflag.p, L, fx->H.p, st)) return rc;
        if (int rc = scan64(fx, fx->nbase.p, L, fx->B.p, st)) return rc;
        k_fx_fasta_records<<<g_lines, XB, 0, st>>>(fx->ls.p, fx->clen.p, fx->hflag.p, fx->H.p, fx->nbase.p, L, fx->rec_line.p, fx->id_off.p,
                                                   fx->id_len.p, d_state);
        k_fx_fasta_lens<<<g_lines, XB, 0, st>>>(fx->rec_line.p, fx->B.p, fx->H.p + L, fx->rlen.p);
        FX_TRY(hipGetLastError());
        fx->mark(st);
        FX_TRY(hipMemcpyAsync(h_back, fx->state.p, sizeof h_back, hipMemcpyDeviceToHost, st));
        FX_TRY(hipMemcpyAsync(&R, fx->H.p + L, 8, hipMemcpyDeviceToHost, st));
        FX_TRY(hipStreamSynchronize(st));
    } else {
        k_fx_lines<<<g_lines, XB, 0, st>>>(d_raw, fx->ls.p, L, kind, fx->clen.p, nullptr, nullptr, d_state);
        FX_TRY(hipGetLastError());
        fx->mark(st);
        FX_TRY(hipMemcpyAsync(h_back, fx->state.p, sizeof h_back, hipMemcpyDeviceToHost, st));
        FX_TRY(hipStreamSynchronize(st));
        if (h_back[ST_FIRST] != ~0ull) {
            const uint64_t first = h_back[ST_FIRST], last = h_back[ST_LAST];
            R = (last - first + 4) / 4;
            FX_TRY(room(fx->id_off, R));
            FX_TRY(room(fx->id_len, R));
            FX_TRY(room(fx->rlen, R));
            FX_TRY(room(fx->seq_off, R));
            fx->mark(st);
            k_fx_fastq_records<<<grid_for(R, XB, X_GRID_CAP), XB, 0, st>>>(d_raw, fx->ls.p, fx->clen.p, L, first, R, fx->id_off.p, fx->id_len.p,
                                                                           fx->rlen.p, fx->seq_off.p, d_state);
            FX_TRY(hipGetLastError());
            fx->mark(st);
            FX_TRY(hipMemcpyAsync(h_back, fx->state.p, sizeof h_back, hipMemcpyDeviceToHost, st));
            FX_TRY(hipStreamSynchronize(st));
        }
    }
    fx->harvest();
    if (h_back[ST_STATUS]) {
        out->status = TAXOR_FASTX_IRREGULAR;
        return TAXOR_OK;
    }
    fx->n_recs = R;
    fx->h_id_off.resize(R);
    fx->h_id_len.resize(R);
    fx->h_rlen.resize(R);
    if (R) {
        FX_TRY(hipMemcpyAsync(fx->h_id_off.data(), fx->id_off.p, R * 8, hipMemcpyDeviceToHost, st));
        FX_TRY(hipMemcpyAsync(fx->h_id_len.data(), fx->id_len.p, R * 8, hipMemcpyDeviceToHost, st));
        FX_TRY(hipMemcpyAsync(fx->h_rlen.data(), fx->rlen.p, R * 8, hipMemcpyDeviceToHost, st));
        FX_TRY(hipStreamSynchronize(st));
    }
    out->n_reads = R;
    out->id_off = fx->h_id_off.data();
    out->id_len = fx->h_id_len.data();
    out->read_len = fx->h_rlen.data();
    return TAXOR_OK;
}

int fastx_scan_pack(FastxScan *fx, const uint8_t *d_raw, const uint64_t *d_poff, const uint32_t *d_rlen, uint32_t *d_packed,
                    uint64_t n_reads, Counters *ctr, hipStream_t st)
{
    if (n_reads != fx->n_recs) return fail(TAXOR_E_INTERNAL, "fastx_scan_pack: the batch is not the one that was scanned");
    if (!n_reads) return TAXOR_OK;
    const int grid = grid_for(n_reads, 1, 8192);
    fx->mark(st);
    if (fx->kind == '>')
        k_fx_pack_fasta<<<grid, XB, 0, st>>>(d_raw, fx->ls.p, fx->nbase.p, fx->B.p, fx->rec_line.p, d_rlen, d_poff, d_packed, n_reads, ctr);
    else
        k_fx_pack_fastq<<<grid, XB, 0, st>>>(d_raw, fx->seq_off.p, d_rlen, d_poff, d_packed, n_reads, ctr);
    fx->mark(st);
    FX_TRY(hipGetLastError());
    return TAXOR_OK;
}

}   // namespace taxor
