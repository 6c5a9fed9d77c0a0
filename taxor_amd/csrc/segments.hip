// segments.hip -- paint a read with its references: the optimal segmentation of its ordered hash list among ALL the references it
// reported, with a cost per switch (`taxor search --segments-file`).
//
// The object lives beside a resident index for a whole run and keeps nothing between batches but its buffers: the leaf-bin table and
// the piece stager of analysis_host.h.  A batch brings the searcher's device-resident CSR and the batch's saved hash lists.  The
// CANDIDATES of a read are its tuples with count > 0, in CSR order; a read is EXAMINED when it has a hash and at least two candidates
// (section 10.6's words).
//
//   read_probe.h's k_cand_count, k_cand_fill and k_probe_mask, as in breakpoint.hip: M per read to the host; the candidates compacted
//                in CSR order; one 64-bit match word mask[c][round] per candidate and 64 hashes.  `lookups` counts the leaf-bin lookups
//                of the last, which stop at a candidate's first matching leaf bin.
//   k_sg_single  one wave per examined read, a lane per candidate (c % 64 == lane): total_c by popcounts, then a wave maximum of
//                (total_c, lowest c): `single` and `best`.
//   k_sg_viterbi one wave per examined read, positions in order.  A lane owns the candidates c with c % 64 == lane.  With
//                STEP = L * 2^32 + 1:  V_c(0) = x_c(0) * 2^32;  J = B(i-1) - STEP;  sw_c(i) = V_c(i-1) < J;
//                V_c(i) = x_c(i) * 2^32 + max(V_c(i-1), J).  B and a (the lowest c that attains it) come from a wave maximum of V and
//                a ballot of the lanes that hold it, lowest lane first; across chunks of 64 candidates only a strictly greater value
//                replaces the carried one.  a(i) is buffered one position per lane and stored as one row per round.  M <= 64: V, the
//                lane's mask word and its switch bits live in registers, one load and one store per (candidate, round).  M > 64: V
//                lives in device scratch, 8 bytes per candidate, and the lane's switch word is read, changed and written back per
//                position; lane c % 64 is the only lane that ever touches V[c], mask[c][.] and sw[c][.], so no lane reads within this
//                kernel what another lane wrote.  Per read the kernel writes e = a(n-1), value = B(n-1) and nothing else.
//                   V never decreases and is never negative (max(V, J) >= V).  sw_{a(i-1)}(i) is never set (V_a = B > J), so every
//                switch changes the candidate.  The path that stays on `best` has value single * 2^32, so hits - L * switches >= single.
//   k_sg_trace_count / k_sg_trace_fill   launches of their own, so the switch words are complete: one lane per examined read walks
//                back from n-1, skipping whole switch words and finding the highest set bit at or below its position with a count of
//                leading zeros (n / 64 + K steps, not n).  The first pass writes K; the host sums K over the reported reads (K >= 2) into
//                seg_off; the second pass writes start, end and candidate of each segment from the back, so they stand in list order.
//   k_sg_hits    one wave per reported read: per segment the lanes stride the mask words of the segment's candidate and of `best`
//                between start and end, with edge masks, and a wave sum of the popcounts gives hits and best_hits.
//
// Every word is an integer maximum, an arg-max with a fixed tie rule or a sum of integers: nothing depends on the launch geometry nor on
// the cut into pieces, groups and batches.  Every loop is bounded by a count the kernel is given.  No block waits on another.
#include "analysis_host.h"
#include "segments_format.h"

#include <climits>
#include <cstring>
#include <map>
#include <memory>

namespace {

using namespace taxor;

constexpr int SB = READ_BLOCK, SWV = READ_WAVES, S_GRID_CAP = READ_GRID_CAP;
constexpr uint64_t MAX_HASHES = 1ull << 31;       // of one read: value = hits * 2^32 - ... stays within 63 bits below it
constexpr uint64_t SG_BUDGET_WORDS = 1ull << 23;  // mask words of one group of reads (64 MiB), and as many switch words
constexpr long long SG_NONE = LLONG_MIN;          // a lane without a candidate, in a wave maximum of V >= 0

enum : uint32_t { SG_BAD_TRACE = 4u };            // beside CAND_BAD_BIN and CAND_MISCOUNT

// what the kernels after the fill share: the match words (read_probe.h) and where a read's other scratch lies within its group's.
// The read's switch words lie at the place of its mask words, mask_off[r], in sw
struct Layout : MaskLayout {
    const uint64_t *cand_tuple;   // [n_cand] index in the batch CSR
    const uint64_t *a_off;        // [n_reads] first word of the read's a: a[a_off[r] + i], 64 * rounds of them
    uint64_t *sw;
    uint32_t *a;
    long long *state;             // V[cand_off[r] + c], for reads with more than 64 candidates
};

// reads [r0, r1) of the batch: one group.  single = max_c total_c; best = the lowest c that attains it
__global__ __launch_bounds__(SB) void k_sg_single(Layout l, uint64_t r0, uint64_t r1, uint32_t *__restrict__ single, uint32_t *__restrict__ best,
                                                  uint64_t *__restrict__ tuple_best, int64_t *__restrict__ bin_best)
{
    const uint32_t lane = lane_id();
    for (uint64_t r = r0 + (uint64_t)blockIdx.x * SWV + (threadIdx.x >> 6); r < r1; r += (uint64_t)gridDim.x * SWV) {
        const uint64_t c0 = l.cand_off[r], m_cand = l.cand_off[r + 1] - c0;
        if (m_cand == 0) continue;
        const uint64_t rounds = ((uint64_t)l.nh[r] + 63) >> 6;
        const uint64_t *mask = l.mask + l.mask_off[r];
        unsigned long long key = 0;                       // total above (2^32 - 1 - c): the greatest key is the greatest total at its lowest c
        for (uint64_t c = lane; c < m_cand; c += 64) {    // m_cand < 2^32: a read's tuples are counted in 32 bits
            uint32_t total = 0;
            for (uint64_t k = 0; k < rounds; ++k) total += (uint32_t)__popcll(mask[c * rounds + k]);
            const unsigned long long kc = ((unsigned long long)total << 32) | (0xFFFFFFFFull - c);
            key = kc > key ? kc : key;
        }
        key = wave_max(key);                              // lane 0 holds c = 0, so the key names a candidate
        if (lane == 0) {
            const uint32_t b = 0xFFFFFFFFu - (uint32_t)key;
            single[r] = (uint32_t)(key >> 32);
            best[r] = b;
            tuple_best[r] = l.cand_tuple[c0 + b];
            bin_best[r] = l.cand_ub[c0 + b];
        }
    }
}

// cost = L, the switch cost.  Writes sw[c][round] and a[i] into the group's scratch, and per read e and value
__global__ __launch_bounds__(SB) void k_sg_viterbi(Layout l, uint64_t r0, uint64_t r1, uint64_t cost, uint32_t *__restrict__ e_out, long long *__restrict__ value_out)
{
    const uint32_t lane = lane_id();
    const long long step = (long long)((cost << 32) + 1ull);          // cost <= 2^20
    for (uint64_t r = r0 + (uint64_t)blockIdx.x * SWV + (threadIdx.x >> 6); r < r1; r += (uint64_t)gridDim.x * SWV) {
        const uint64_t c0 = l.cand_off[r], m_cand = l.cand_off[r + 1] - c0;
        if (m_cand == 0) continue;
        const uint32_t n = l.nh[r];                                   // > 0 and < 2^31 for an examined read
        const uint64_t rounds = ((uint64_t)n + 63) >> 6;
        const uint64_t *mask = l.mask + l.mask_off[r];
        uint64_t *sw = l.sw + l.mask_off[r];
        uint32_t *arow = l.a + l.a_off[r];
        long long B = 0;                                              // B(i-1), then B(i)
        uint32_t a = 0;                                               // a(i)
        if (m_cand <= 64) {
            const bool act = lane < m_cand;
            long long V = 0;
            for (uint64_t k = 0; k < rounds; ++k) {
                const uint64_t m = act ? mask[(uint64_t)lane * rounds + k] : 0ull;
                const uint32_t cnt = (uint32_t)((uint64_t)n - k * 64 < 64 ? (uint64_t)n - k * 64 : 64);
                uint64_t bits = 0;
                uint32_t a_mine = 0;
                for (uint32_t j = 0; j < cnt; ++j) {
                    const long long x = (long long)(((m >> j) & 1ull) << 32);
                    if (k == 0 && j == 0) {
                        V = x;
                    } else {
                        const long long J = B - step;
                        bits |= (uint64_t)(V < J) << j;                // a tie stays
                        V = x + (V > J ? V : J);
                    }
                    B = wave_max(act ? V : SG_NONE);
                    a = (uint32_t)__ffsll((long long)__ballot(act && V == B)) - 1u;     // lane 0 is a candidate and some lane holds B: never 0 - 1
                    if (lane == j) a_mine = a;
                }
                if (act) sw[(uint64_t)lane * rounds + k] = bits;
                arow[k * 64 + lane] = a_mine;                         // one row per round; 0 behind the read's end
            }
        } else {
            long long *V = l.state + c0;
            for (uint64_t k = 0; k < rounds; ++k) {
                const uint32_t cnt = (uint32_t)((uint64_t)n - k * 64 < 64 ? (uint64_t)n - k * 64 : 64);
                uint32_t a_mine = 0;
                for (uint32_t j = 0; j < cnt; ++j) {
                    const bool first = k == 0 && j == 0;
                    const long long J = B - step;
                    long long nb = SG_NONE;
                    uint32_t na = 0;
                    for (uint64_t q0 = 0; q0 < m_cand; q0 += 64) {    // chunks of 64 candidates, in order
                        const uint64_t c = q0 + lane;
                        const bool act = c < m_cand;
                        long long v = SG_NONE;
                        if (act) {
                            const long long x = (long long)(((mask[c * rounds + k] >> j) & 1ull) << 32);
                            uint64_t bits = j == 0 ? 0ull : sw[c * rounds + k];       // this lane's own word, as it left it
                            if (first) {
                                v = x;
                            } else {
                                const long long v0 = V[c];                            // this lane's own store of the position before
                                bits |= (uint64_t)(v0 < J) << j;
                                v = x + (v0 > J ? v0 : J);
                            }
                            sw[c * rounds + k] = bits;
                            V[c] = v;
                        }
                        const long long cm = wave_max(v);
                        if (cm > nb) {                                // strictly: an equal value in a later chunk does not take over
                            nb = cm;
                            na = (uint32_t)q0 + (uint32_t)__ffsll((long long)__ballot(act && v == cm)) - 1u;
                        }
                    }
                    B = nb;
                    a = na;
                    if (lane == j) a_mine = a;
                }
                arow[k * 64 + lane] = a_mine;
            }
        }
        if (lane == 0) {
            e_out[r] = a;
            value_out[r] = B;
        }
    }
}

struct SegOut {
    const uint64_t *seg_off;      // [n_reads + 1] a reported read's segments go to [seg_off[r], seg_off[r + 1]); an empty range otherwise
    uint32_t *start, *end, *cand;
    uint64_t *tuple;
    int64_t *bin;
};

// One lane walks read r back from its end.  FILL: the segments are written from the back into the read's room.  Returns K
template <bool FILL> __device__ __forceinline__ uint32_t sg_walk(const Layout &l, uint64_t r, uint32_t e, uint32_t k_known, const SegOut &o, bool *bad)
{
    const uint64_t c0 = l.cand_off[r], m_cand = l.cand_off[r + 1] - c0;
    const uint32_t n = l.nh[r];
    const uint64_t rounds = ((uint64_t)n + 63) >> 6;
    const uint64_t *sw = l.sw + l.mask_off[r];
    const uint32_t *arow = l.a + l.a_off[r];
    const uint64_t dst = FILL ? o.seg_off[r] : 0;
    uint32_t cur = e, end = n, k_seg = 0;
    for (uint32_t seg = 0; seg < n; ++seg) {              // a read of n hashes has at most n segments
        if (cur >= m_cand) {                              // never: e and a name candidates
            *bad = true;
            break;
        }
        // the highest switch bit of `cur` at or below position end - 1
        const uint32_t pos = end - 1;
        uint64_t kw = pos >> 6;
        uint64_t w = sw[(uint64_t)cur * rounds + kw] & (~0ull >> (63u - (pos & 63u)));
        while (w == 0 && kw > 0) {                        // at most `rounds` words
            --kw;
            w = sw[(uint64_t)cur * rounds + kw];
        }
        const uint32_t start = w ? (uint32_t)(kw * 64) + 63u - (uint32_t)__clzll((long long)w) : 0u;
        if (FILL && k_seg < k_known) {                    // from the back: list order
            const uint64_t at = dst + (k_known - 1 - k_seg);
            o.start[at] = start;
            o.end[at] = end;
            o.cand[at] = cur;
            o.tuple[at] = l.cand_tuple[c0 + cur];
            o.bin[at] = l.cand_ub[c0 + cur];
        }
        ++k_seg;
        if (start == 0) break;                            // position 0 never carries a switch bit: this is the first segment
        cur = arow[start - 1];                            // a(start - 1): where the path came from
        end = start;
    }
    return k_seg;
}

__global__ __launch_bounds__(SB) void k_sg_trace_count(Layout l, uint64_t r0, uint64_t r1, const uint32_t *__restrict__ e, uint32_t *__restrict__ n_seg,
                                                       uint32_t *__restrict__ err)
{
    bool bad = false;
    const SegOut none{};
    for (uint64_t r = r0 + (uint64_t)blockIdx.x * SB + threadIdx.x; r < r1; r += (uint64_t)gridDim.x * SB) {
        if (l.cand_off[r + 1] == l.cand_off[r]) continue;
        n_seg[r] = sg_walk<false>(l, r, e[r], 0, none, &bad);
    }
    if (bad) atomicOr(err, SG_BAD_TRACE);
}

__global__ __launch_bounds__(SB) void k_sg_trace_fill(Layout l, uint64_t r0, uint64_t r1, const uint32_t *__restrict__ e, const uint32_t *__restrict__ n_seg, SegOut o,
                                                      uint32_t *__restrict__ err)
{
    bool bad = false;
    for (uint64_t r = r0 + (uint64_t)blockIdx.x * SB + threadIdx.x; r < r1; r += (uint64_t)gridDim.x * SB) {
        const uint64_t room = o.seg_off[r + 1] - o.seg_off[r];
        if (room == 0) continue;                          // not examined, or unbroken
        const uint32_t k = n_seg[r];
        if (k != room) {                                  // never: the host summed these very counts
            bad = true;
            continue;
        }
        if (sg_walk<true>(l, r, e[r], k, o, &bad) != k) bad = true;
    }
    if (bad) atomicOr(err, SG_BAD_TRACE);
}

__global__ __launch_bounds__(SB) void k_sg_hits(Layout l, uint64_t r0, uint64_t r1, const uint32_t *__restrict__ best, SegOut o, uint32_t *__restrict__ seg_hits,
                                                uint32_t *__restrict__ seg_best_hits)
{
    const uint32_t lane = lane_id();
    for (uint64_t r = r0 + (uint64_t)blockIdx.x * SWV + (threadIdx.x >> 6); r < r1; r += (uint64_t)gridDim.x * SWV) {
        const uint64_t s0 = o.seg_off[r], s1 = o.seg_off[r + 1];
        if (s0 == s1) continue;
        const uint64_t m_cand = l.cand_off[r + 1] - l.cand_off[r];
        const uint32_t n = l.nh[r];
        const uint64_t rounds = ((uint64_t)n + 63) >> 6;
        const uint64_t *mask = l.mask + l.mask_off[r];
        const uint64_t b = best[r];
        for (uint64_t s = s0; s < s1; ++s) {
            const uint32_t st = o.start[s], en = o.end[s];
            const uint64_t c = o.cand[s];
            uint32_t h = 0, hb = 0;
            if (c < m_cand && b < m_cand && st < en && en <= n) {     // what the trace wrote; a word outside the read's masks is never read
                const uint64_t k0 = st >> 6, k1 = (uint64_t)(en - 1) >> 6;
                for (uint64_t k = k0 + lane; k <= k1; k += 64) {
                    uint64_t edge = ~0ull;
                    if (k == k0) edge &= ~0ull << (st & 63u);
                    if (k == k1) edge &= ~0ull >> (63u - ((en - 1) & 63u));
                    h += (uint32_t)__popcll(mask[c * rounds + k] & edge);
                    hb += (uint32_t)__popcll(mask[b * rounds + k] & edge);
                }
            }
            h = wave_incl_add(h);
            hb = wave_incl_add(hb);
            if (lane == 63) {
                seg_hits[s] = h;
                seg_best_hits[s] = hb;
            }
        }
    }
}

#define SG_TRY(expr) TAXOR_HIP_TRY_PREFIX("segments", expr, #expr)

constexpr int SG_H32 = 7, SG_H64 = 3;                 // 32- and 64-bit words per read in the page-locked result

// the results of one caller (a searcher, or add_csr): device words and work arrays, and their page-locked copies
struct Slot {
    DeviceBuf<uint32_t> d_n_cand, d_e, d_nseg, d_single, d_best;
    DeviceBuf<uint64_t> d_off3, d_cand_tuple, d_tuple_best, d_seg_off;     // d_off3: cand_off[n + 1] | mask_off[n] | a_off[n]
    DeviceBuf<int64_t> d_cand_ub, d_bin_best;
    DeviceBuf<long long> d_value, d_state;
    DeviceBuf<uint32_t> d_seg_start, d_seg_end, d_seg_cand, d_seg_hits, d_seg_best;
    DeviceBuf<uint64_t> d_seg_tuple;
    DeviceBuf<int64_t> d_seg_bin;
    uint64_t seg_cap = 0;          // segments the seven arrays above hold
    uint32_t *h32 = nullptr;       // n_candidates | n | n_hashes | n_segments | path_hits | path_switches | single, cap each
    uint64_t *h64 = nullptr;       // tuple_best | bin_best | value, cap each
    uint64_t *h_off3 = nullptr;    // 3 * cap + 1
    uint64_t *h_seg_off = nullptr; // cap + 1
    uint8_t *h_examined = nullptr;
    uint32_t *hs32 = nullptr;      // seg_start | seg_end | seg_hits | seg_best_hits, hseg_cap each
    uint64_t *hs64 = nullptr;      // seg_tuple | seg_bin, hseg_cap each
    uint64_t cap = 0, hseg_cap = 0;
    void drop_segs()
    {
        if (hs32) (void)hipHostFree(hs32);
        if (hs64) (void)hipHostFree(hs64);
        hs32 = nullptr;
        hs64 = nullptr;
        hseg_cap = 0;
    }
    void drop()
    {
        if (h32) (void)hipHostFree(h32);
        if (h64) (void)hipHostFree(h64);
        if (h_off3) (void)hipHostFree(h_off3);
        if (h_seg_off) (void)hipHostFree(h_seg_off);
        if (h_examined) (void)hipHostFree(h_examined);
        h32 = nullptr;
        h64 = nullptr;
        h_off3 = nullptr;
        h_seg_off = nullptr;
        h_examined = nullptr;
        cap = 0;
    }
    ~Slot()
    {
        drop();
        drop_segs();
    }
};

struct Group {
    uint64_t r0, r1;               // reads [r0, r1) of the batch
    uint64_t mask_words, a_words;
};

}   // namespace

struct taxor_gpu_segments : ReadAnalysis {
    uint32_t switch_cost = SEGMENTS_DEFAULT_SWITCH_COST;
    uint64_t budget_words = SG_BUDGET_WORDS;
    DeviceBuf<uint64_t> d_mask, d_sw;
    DeviceBuf<uint32_t> d_a;
    DeviceBuf<unsigned long long> d_lookups;
    std::vector<Group> groups;
    std::map<const void *, std::unique_ptr<Slot>> slots;
};

namespace {

// One batch whose CSR is on the object's device (tuples indexed from t0); the hash lists are host arrays (read r's at
// hashes[hash_off[r] .. hash_off[r + 1]), h_nh[r] of them).  The caller holds the mutex and has made every check that needs no launch
// but one: a read of 2^31 hashes or more is refused here, first.
int add_device(taxor_gpu_segments *c, const void *who, uint64_t n, const uint64_t *d_off, const int64_t *d_ub, const uint32_t *d_cnt, const uint32_t *d_nh,
               uint64_t t0, const uint64_t *hash_off, const uint64_t *hashes, const uint32_t *h_nh, taxor_segments_batch *out)
{
    for (uint64_t r = 0; r < n; ++r)
        if (h_nh[r] >= MAX_HASHES)
            return fail(TAXOR_E_ARG, "segments_add: n: read %llu has %u hashes; with 2^31 or more the value of a path (hits * 2^32 - switches) leaves 63 bits", (unsigned long long)r,
                        h_nh[r]);
    std::unique_ptr<Slot> &sp = c->slots[who];
    if (!sp) sp = std::make_unique<Slot>();
    Slot &sl = *sp;
    if (n > sl.cap || sl.cap == 0) {                   // an empty batch has a seg_off of one entry as well
        const uint64_t want = std::max<uint64_t>(n + n / 2, 1024);
        sl.drop();
        SG_TRY(sl.d_n_cand.alloc(want));
        SG_TRY(sl.d_e.alloc(want));
        SG_TRY(sl.d_nseg.alloc(want));
        SG_TRY(sl.d_single.alloc(want));
        SG_TRY(sl.d_best.alloc(want));
        SG_TRY(sl.d_tuple_best.alloc(want));
        SG_TRY(sl.d_bin_best.alloc(want));
        SG_TRY(sl.d_value.alloc(want));
        SG_TRY(sl.d_off3.alloc(3 * want + 1));
        SG_TRY(sl.d_seg_off.alloc(want + 1));
        SG_TRY(hipHostMalloc((void **)&sl.h32, SG_H32 * want * sizeof(uint32_t), hipHostMallocDefault));
        SG_TRY(hipHostMalloc((void **)&sl.h64, SG_H64 * want * sizeof(uint64_t), hipHostMallocDefault));
        SG_TRY(hipHostMalloc((void **)&sl.h_off3, (3 * want + 1) * sizeof(uint64_t), hipHostMallocDefault));
        SG_TRY(hipHostMalloc((void **)&sl.h_seg_off, (want + 1) * sizeof(uint64_t), hipHostMallocDefault));
        SG_TRY(hipHostMalloc((void **)&sl.h_examined, want, hipHostMallocDefault));
        sl.cap = want;
    }
    uint32_t *h32 = sl.h32;
    uint64_t *h64 = sl.h64;
    uint32_t *h_m = h32, *h_n = h32 + n, *h_nseg = h32 + 3 * n, *h_hits = h32 + 4 * n, *h_switches = h32 + 5 * n;
    const long long *h_value = (const long long *)(h64 + 2 * n);
    out->n_reads = n;
    out->n_examined = out->n_reported = 0;
    out->switch_cost = c->switch_cost;
    out->n_groups = 0;
    out->examined = sl.h_examined;
    out->n_candidates = h_m;
    out->n = h_n;
    out->n_hashes = h32 + 2 * n;
    out->n_segments = h_nseg;
    out->path_hits = h_hits;
    out->path_switches = h_switches;
    out->single = h32 + 6 * n;
    out->tuple_best = h64;
    out->bin_best = (const int64_t *)(h64 + n);
    out->seg_off = sl.h_seg_off;
    out->seg_start = out->seg_end = out->seg_hits = out->seg_best_hits = nullptr;
    out->seg_tuple = nullptr;
    out->seg_bin = nullptr;
    out->seconds_kernels = 0;
    out->lookups = 0;
    sl.h_seg_off[0] = 0;
    if (int rc = c->stage.recover()) return rc;
    if (n == 0) return TAXOR_OK;
    const uint64_t n_bins = c->leaf.n_bins;
    c->timer.begin();
    auto stamp = [&]() { return c->timer.stamp(c->st); };

    // the words of a read that is not examined are 0
    SG_TRY(hipMemsetAsync(sl.d_nseg.p, 0, n * sizeof(uint32_t), c->st));
    SG_TRY(hipMemsetAsync(sl.d_single.p, 0, n * sizeof(uint32_t), c->st));
    SG_TRY(hipMemsetAsync(sl.d_best.p, 0, n * sizeof(uint32_t), c->st));
    SG_TRY(hipMemsetAsync(sl.d_e.p, 0, n * sizeof(uint32_t), c->st));
    SG_TRY(hipMemsetAsync(sl.d_tuple_best.p, 0, n * sizeof(uint64_t), c->st));
    SG_TRY(hipMemsetAsync(sl.d_bin_best.p, 0, n * sizeof(int64_t), c->st));
    SG_TRY(hipMemsetAsync(sl.d_value.p, 0, n * sizeof(long long), c->st));
    SG_TRY(hipMemsetAsync(c->d_lookups.p, 0, 8, c->st));
    if (int rc = stamp()) return rc;
    k_cand_count<uint32_t><<<grid_for(n, SWV, S_GRID_CAP), SB, 0, c->st>>>(d_off, d_ub, d_cnt, t0, d_nh, n, n_bins, sl.d_n_cand.p, c->d_err.p);
    SG_TRY(hipGetLastError());
    if (int rc = stamp()) return rc;
    uint32_t err = 0;
    SG_TRY(hipMemcpyAsync(h_m, sl.d_n_cand.p, n * sizeof(uint32_t), hipMemcpyDeviceToHost, c->st));
    SG_TRY(hipMemcpyAsync(&err, c->d_err.p, 4, hipMemcpyDeviceToHost, c->st));
    SG_TRY(hipStreamSynchronize(c->st));
    if (err & CAND_BAD_BIN) {
        if (int rc = c->clear_err()) return rc;
        return fail(TAXOR_E_INTERNAL, "segments_add: user_bin: a tuple names a user bin outside the index's %llu", (unsigned long long)n_bins);
    }
    // who is examined; the candidates' offsets; groups of reads whose masks stay within the budget, a read that exceeds it by itself
    // alone; where a read's masks (and switch words) and its a lie within its group's scratch
    uint64_t *cand_off = sl.h_off3, *mask_off = cand_off + n + 1, *a_off = mask_off + n;
    c->groups.clear();
    uint64_t n_cand = 0, n_examined = 0, max_mask = 0, max_a = 0, big_read = 0;
    for (uint64_t r = 0; r < n; ++r) {
        cand_off[r] = n_cand;
        mask_off[r] = a_off[r] = 0;
        const bool ex = h_nh[r] != 0 && h_m[r] >= 2;
        sl.h_examined[r] = ex ? 1 : 0;
        h_n[r] = ex ? h_nh[r] : 0;
        h_nseg[r] = h_hits[r] = h_switches[r] = 0;
        if (!ex) {
            h_m[r] = 0;
            continue;
        }
        ++n_examined;
        n_cand += h_m[r];
        const uint64_t rounds = ((uint64_t)h_nh[r] + 63) >> 6, mw = (uint64_t)h_m[r] * rounds;
        if (c->groups.empty() || c->groups.back().mask_words + mw > c->budget_words) c->groups.push_back(Group{r, r, 0, 0});
        Group &g = c->groups.back();
        mask_off[r] = g.mask_words;
        a_off[r] = g.a_words;
        g.mask_words += mw;
        g.a_words += 64 * rounds;
        g.r1 = r + 1;
        if (g.mask_words > max_mask) {
            max_mask = g.mask_words;
            big_read = r;
        }
        max_a = std::max(max_a, g.a_words);
    }
    cand_off[n] = n_cand;
    out->n_examined = n_examined;
    out->n_groups = (uint32_t)c->groups.size();
    memcpy(h32 + 2 * n, h_nh, n * sizeof(uint32_t));
    uint64_t seg_total = 0;
    if (n_examined) {
        hipError_t e_scr = c->d_mask.reserve(max_mask, max_mask);
        if (e_scr == hipSuccess) e_scr = c->d_sw.reserve(max_mask, max_mask);
        if (e_scr == hipSuccess) e_scr = c->d_a.reserve(max_a, max_a);
        if (e_scr == hipSuccess) e_scr = sl.d_state.reserve(n_cand, n_cand + n_cand / 2);
        if (e_scr != hipSuccess) {
            (void)hipGetLastError();
            return fail(TAXOR_E_NOMEM, "segments_add: scratch: %llu bytes of match masks, as many of switch words, %llu bytes of predecessors and %llu bytes of state could not be "
                                       "allocated (%s); the group ends with read %llu, which has %u candidates and %u hashes",
                        (unsigned long long)(max_mask * 8), (unsigned long long)(max_a * 4), (unsigned long long)(n_cand * 8), hipGetErrorString(e_scr),
                        (unsigned long long)big_read, h_m[big_read], h_nh[big_read]);
        }
        SG_TRY(sl.d_cand_tuple.reserve(n_cand, n_cand + n_cand / 2));
        SG_TRY(sl.d_cand_ub.reserve(n_cand, n_cand + n_cand / 2));
        SG_TRY(hipMemcpyAsync(sl.d_off3.p, sl.h_off3, (3 * n + 1) * 8, hipMemcpyHostToDevice, c->st));
        if (int rc = stamp()) return rc;
        k_cand_fill<false><<<grid_for(n, SWV, S_GRID_CAP), SB, 0, c->st>>>(d_off, d_ub, d_cnt, t0, n, n_bins, nullptr, sl.d_off3.p, sl.d_cand_tuple.p, sl.d_cand_ub.p, nullptr,
                                                                           c->d_err.p);
        SG_TRY(hipGetLastError());
        if (int rc = stamp()) return rc;

        Layout l{};
        l.cand_off = sl.d_off3.p;
        l.cand_ub = sl.d_cand_ub.p;
        l.mask_off = sl.d_off3.p + n + 1;
        l.nh = d_nh;
        l.mask = c->d_mask.p;
        l.cand_tuple = sl.d_cand_tuple.p;
        l.a_off = sl.d_off3.p + 2 * n + 1;
        l.sw = c->d_sw.p;
        l.a = c->d_a.p;
        l.state = sl.d_state.p;
        MaskProbeArgs a{c->leaf.d_ixf, c->leaf.d_off.p, c->leaf.d_leaf.p, l, nullptr, nullptr, 0, c->d_lookups.p};
        c->stage.begin(hashes, [&](const Piece *pieces, const uint64_t *staged, uint32_t n_p) {
            a.pieces = pieces;
            a.hashes = staged;
            a.n_pieces = n_p;
            k_probe_mask<true><<<grid_for(n_p, SWV, S_GRID_CAP), SB, 0, c->st>>>(a);
        });
        // A group's sets come first, then its Viterbi pass and the first trace; the host sums the group's K, and the second trace and
        // the segments' hits follow before the next group writes the same scratch behind them on the stream
        uint64_t r_done = 0;                // seg_off[0 .. r_done] is final
        for (const Group &g : c->groups) {
            for (uint64_t r = g.r0; r < g.r1; ++r)
                if (sl.h_examined[r])
                    if (int rc = c->stage.add(r, hash_off[r], h_nh[r])) return rc;
            if (int rc = c->stage.flush()) return rc;
            const uint64_t gn = g.r1 - g.r0;
            if (int rc = stamp()) return rc;
            k_sg_single<<<grid_for(gn, SWV, S_GRID_CAP), SB, 0, c->st>>>(l, g.r0, g.r1, sl.d_single.p, sl.d_best.p, sl.d_tuple_best.p, sl.d_bin_best.p);
            k_sg_viterbi<<<grid_for(gn, SWV, S_GRID_CAP), SB, 0, c->st>>>(l, g.r0, g.r1, (uint64_t)c->switch_cost, sl.d_e.p, sl.d_value.p);
            k_sg_trace_count<<<grid_for(gn, SB, S_GRID_CAP), SB, 0, c->st>>>(l, g.r0, g.r1, sl.d_e.p, sl.d_nseg.p, c->d_err.p);
            SG_TRY(hipGetLastError());
            if (int rc = stamp()) return rc;
            SG_TRY(hipMemcpyAsync(h_nseg + g.r0, sl.d_nseg.p + g.r0, gn * sizeof(uint32_t), hipMemcpyDeviceToHost, c->st));
            SG_TRY(hipStreamSynchronize(c->st));
            c->stage.synced();
            // K summed over the reported reads, like M above
            for (uint64_t r = r_done; r < g.r1; ++r) {
                sl.h_seg_off[r] = seg_total;
                if (r >= g.r0 && sl.h_examined[r] && h_nseg[r] >= 2) seg_total += h_nseg[r];
            }
            sl.h_seg_off[g.r1] = seg_total;
            r_done = g.r1;
            if (seg_total > sl.seg_cap) {                  // the segments of the groups before stay
                const uint64_t want = std::max<uint64_t>(seg_total + seg_total / 2, 4096), keep = sl.h_seg_off[g.r0];
                SG_TRY(sl.d_seg_start.grow(seg_total, want, keep, c->st));
                SG_TRY(sl.d_seg_end.grow(seg_total, want, keep, c->st));
                SG_TRY(sl.d_seg_cand.grow(seg_total, want, keep, c->st));
                SG_TRY(sl.d_seg_hits.grow(seg_total, want, keep, c->st));
                SG_TRY(sl.d_seg_best.grow(seg_total, want, keep, c->st));
                SG_TRY(sl.d_seg_tuple.grow(seg_total, want, keep, c->st));
                SG_TRY(sl.d_seg_bin.grow(seg_total, want, keep, c->st));
                sl.seg_cap = want;
            }
            if (seg_total == sl.h_seg_off[g.r0]) continue; // no read of the group is reported
            SG_TRY(hipMemcpyAsync(sl.d_seg_off.p + g.r0, sl.h_seg_off + g.r0, (gn + 1) * 8, hipMemcpyHostToDevice, c->st));
            const SegOut so{sl.d_seg_off.p, sl.d_seg_start.p, sl.d_seg_end.p, sl.d_seg_cand.p, sl.d_seg_tuple.p, sl.d_seg_bin.p};
            if (int rc = stamp()) return rc;
            k_sg_trace_fill<<<grid_for(gn, SB, S_GRID_CAP), SB, 0, c->st>>>(l, g.r0, g.r1, sl.d_e.p, sl.d_nseg.p, so, c->d_err.p);
            k_sg_hits<<<grid_for(gn, SWV, S_GRID_CAP), SB, 0, c->st>>>(l, g.r0, g.r1, sl.d_best.p, so, sl.d_seg_hits.p, sl.d_seg_best.p);
            SG_TRY(hipGetLastError());
            if (int rc = stamp()) return rc;
        }
        for (uint64_t r = r_done; r <= n; ++r) sl.h_seg_off[r] = seg_total;
    } else {
        for (uint64_t r = 0; r <= n; ++r) sl.h_seg_off[r] = 0;
    }
    if (seg_total > sl.hseg_cap) {
        const uint64_t want = std::max<uint64_t>(seg_total + seg_total / 2, 4096);
        sl.drop_segs();
        SG_TRY(hipHostMalloc((void **)&sl.hs32, 4 * want * sizeof(uint32_t), hipHostMallocDefault));
        SG_TRY(hipHostMalloc((void **)&sl.hs64, 2 * want * sizeof(uint64_t), hipHostMallocDefault));
        sl.hseg_cap = want;
    }
    SG_TRY(hipMemcpyAsync(h32 + 6 * n, sl.d_single.p, n * sizeof(uint32_t), hipMemcpyDeviceToHost, c->st));
    SG_TRY(hipMemcpyAsync(h64, sl.d_tuple_best.p, n * sizeof(uint64_t), hipMemcpyDeviceToHost, c->st));
    SG_TRY(hipMemcpyAsync(h64 + n, sl.d_bin_best.p, n * sizeof(int64_t), hipMemcpyDeviceToHost, c->st));
    SG_TRY(hipMemcpyAsync(h64 + 2 * n, sl.d_value.p, n * sizeof(long long), hipMemcpyDeviceToHost, c->st));
    if (seg_total) {
        const uint64_t s = seg_total;
        SG_TRY(hipMemcpyAsync(sl.hs32, sl.d_seg_start.p, s * 4, hipMemcpyDeviceToHost, c->st));
        SG_TRY(hipMemcpyAsync(sl.hs32 + s, sl.d_seg_end.p, s * 4, hipMemcpyDeviceToHost, c->st));
        SG_TRY(hipMemcpyAsync(sl.hs32 + 2 * s, sl.d_seg_hits.p, s * 4, hipMemcpyDeviceToHost, c->st));
        SG_TRY(hipMemcpyAsync(sl.hs32 + 3 * s, sl.d_seg_best.p, s * 4, hipMemcpyDeviceToHost, c->st));
        SG_TRY(hipMemcpyAsync(sl.hs64, sl.d_seg_tuple.p, s * 8, hipMemcpyDeviceToHost, c->st));
        SG_TRY(hipMemcpyAsync(sl.hs64 + s, sl.d_seg_bin.p, s * 8, hipMemcpyDeviceToHost, c->st));
        out->seg_start = sl.hs32;
        out->seg_end = sl.hs32 + s;
        out->seg_hits = sl.hs32 + 2 * s;
        out->seg_best_hits = sl.hs32 + 3 * s;
        out->seg_tuple = sl.hs64;
        out->seg_bin = (const int64_t *)(sl.hs64 + s);
    }
    unsigned long long lookups = 0;
    SG_TRY(hipMemcpyAsync(&lookups, c->d_lookups.p, 8, hipMemcpyDeviceToHost, c->st));
    SG_TRY(hipMemcpyAsync(&err, c->d_err.p, 4, hipMemcpyDeviceToHost, c->st));
    SG_TRY(hipStreamSynchronize(c->st));               // the searcher's buffers and the hash lists are the caller's again
    c->stage.end();
    if (int rc = c->timer.add_to(&out->seconds_kernels)) return rc;
    out->lookups = lookups;
    if (err) {                                         // the CSR changed under the call, or a trace left the read's candidates
        if (int rc = c->clear_err()) return rc;
        return fail(TAXOR_E_INTERNAL, "segments_add: candidates: a second walk disagrees with the first (the candidates' or the trace's; flags %u)", err);
    }
    // value = (hits - L * switches) * 2^32 - switches, and switches = K - 1
    const uint64_t L = c->switch_cost;
    for (uint64_t r = 0; r < n; ++r) {
        if (!sl.h_examined[r]) continue;
        const uint64_t k = h_nseg[r];
        const long long v = h_value[r];
        if (k < 1 || v < 0 || (((uint64_t)v + (k - 1)) & 0xFFFFFFFFull) != 0)
            return fail(TAXOR_E_INTERNAL, "segments_add: value: read %llu has value %lld and %llu segments, which do not belong together", (unsigned long long)r, v,
                        (unsigned long long)k);
        h_switches[r] = (uint32_t)(k - 1);
        h_hits[r] = (uint32_t)((((uint64_t)v + (k - 1)) >> 32) + L * (k - 1));
        out->n_reported += k >= 2;
    }
    return TAXOR_OK;
}

}   // namespace

extern "C" int taxor_gpu_segments_create(taxor_gpu_index *idx, const taxor_hixf_view *view, uint32_t switch_cost, taxor_gpu_segments **out)
{
    if (!out) return fail(TAXOR_E_ARG, "segments_create: null argument");
    *out = nullptr;
    if (!idx || !view) return fail(TAXOR_E_ARG, "segments_create: null argument");
    if (switch_cost < 1 || switch_cost > SEGMENTS_MAX_SWITCH_COST)
        return fail(TAXOR_E_ARG, "segments_create: switch_cost: %u is outside [1, %u] (a switch that costs nothing is taken at every hash; above 2^20 the cost leaves the value's 63 bits)",
                    switch_cost, SEGMENTS_MAX_SWITCH_COST);
    auto c = std::make_unique<taxor_gpu_segments>();
    if (int rc = c->leaf.build("segments_create", "its leaf bins are not all resident at once and a read's final tuples exist only after the last pass's merge; segmenting pass by pass is not built", idx, view))
        return rc;
    if (int rc = c->stage.configure("segments_create")) return rc;
    c->switch_cost = switch_cost;
    // a measurement knob (tuning.h): the mask words of one group of reads.  It moves the cut into groups, never a result
    if (const char *e = tune_env("TAXOR_SEGMENTS_BUDGET_WORDS")) {
        const long long v = atoll(e);
        if (v >= 1) c->budget_words = (uint64_t)v;
    }
    SG_TRY(hipSetDevice(c->leaf.device));
    if (int rc = c->open("segments")) return rc;
    SG_TRY(c->d_lookups.alloc(1));
    *out = c.release();
    return TAXOR_OK;
}

extern "C" void taxor_gpu_segments_destroy(taxor_gpu_segments *c)
{
    if (!c) return;
    (void)hipSetDevice(c->leaf.device);
    delete c;
}

extern "C" int taxor_gpu_segments_add_batch(taxor_gpu_segments *c, taxor_gpu_searcher *s, const taxor_gpu_saved *saved, taxor_segments_batch *out)
{
    if (!c || !s || !out) return fail(TAXOR_E_ARG, "segments_add_batch: null argument");
    std::unique_lock<std::mutex> lk;
    SearcherBatch b;
    if (int rc = begin_batch("segments_add_batch", "segments", "the segments object", *c, s, saved, lk, &b)) return rc;
    return add_device(c, s, b.n, b.d_off, b.d_ub, b.d_cnt, b.d_nh, 0, saved->hash_off.data(), saved->hashes, c->h_nh.data(), out);
}

extern "C" int taxor_gpu_segments_add_csr(taxor_gpu_segments *c, uint64_t n_reads, const uint64_t *read_off, const int64_t *user_bin, const uint32_t *count,
                                          const uint64_t *hash_off, const uint64_t *hashes, taxor_segments_batch *out)
{
    if (!c || !read_off || !hash_off || !out) return fail(TAXOR_E_ARG, "segments_add_csr: null argument");
    CsrUpload &u = c->csr;
    std::lock_guard<std::mutex> lk(c->mu);
    if (int rc = u.check("segments_add_csr", "index", c->leaf.n_bins, n_reads, read_off, user_bin, count, hash_off, hashes)) return rc;
    SG_TRY(hipSetDevice(c->leaf.device));
    if (int rc = u.upload("segments", n_reads, read_off, user_bin, count, hash_off, nullptr, &c->h_nh)) return rc;
    return add_device(c, nullptr, n_reads, u.off.p, u.ub.p, u.cnt.p, u.nh.p, u.t0, hash_off, hashes, c->h_nh.data(), out);
}
