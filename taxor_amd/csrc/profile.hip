// profile.hip -- `taxor profile` on the device: the filtering rounds and the EM of src/main/taxor_profile.cpp over a CSR
// read -> matches (reads and references numbered in byte-wise string order, matches in file order).
//
// A match never moves: every stage keeps an ALIVE byte per match and reads "the read's matches in order" as the alive ones in
// CSR order, which is what the reference's vector erase leaves.  One wave per read, four reads per block, grid-stride.
//
//   k_pf_flag_single   round 1 (:166-180): references with a single-match read
//   k_pf_filter        :186-229: a multi-match read that touches a flagged reference keeps only its flagged matches
//   k_pf_hist          round 2 (:232-264): per reference (unique, ambiguous) counts
//   k_pf_accept        :266-277: unique >= 3 && (float)unique / (float)(unique + ambiguous) >= 0.01f
//   k_pf_assoc         round 3 (:293-346): unique_assign_reads, all_assigned_reads, the first match of every reference (its
//                      ref_len is taxa_lengths'), and the pair table: reads shared by (ref1, ref2) over all ordered pairs
//                      inside a multi-match read -- keyset.h's slot rule on the key ref1 << 32 | ref2, a 32-bit counter beside it
//   (host)             :349-399: the explained-by rule in map order and the chain resolution -- O(pairs), order-dependent
//   k_pf_explain       :405-451: erase a match whose explaining reference is in the read, else rename it and its ref_len
//   k_pf_dup           matches that repeat an earlier reference of their read (a rename can collide): they take the FIRST
//                      occurrence's likelihood, like the insert of :497
//   k_pf_sum_ratio     EM (:487-491): sum of match / count ratios of a multi-match read, added in match order
//   k_pf_em            :658-720 and :527-540: posteriors, the best set, the erased match, the nucleotide sums
//
// EM arithmetic: the device does integer sums, IEEE double add / subtract / divide and comparisons (this file is compiled with
// -ffp-contract=off); every log and the one sequential sum of posteriors are the host's (run(), below).
#include "../../include/taxor_gpu_tools.h"
#include "device_prims.h"
#include "hip_host.h"
#include "keyset.h"
#include "profile_host.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstring>
#include <memory>
#include <string>
#include <unordered_map>
#include <vector>

namespace {

using namespace taxor;

constexpr int PB = 256;                  // threads per block
constexpr int PW = PB / 64;              // reads per block pass (one wave each)
constexpr int P_GRID_CAP = 2048;
constexpr uint64_t NO_POS = ~0ull;

enum : uint32_t { PF_TABLE_FULL = 1u, PF_NO_PRIOR = 2u };

__device__ __forceinline__ uint64_t pf_first_read() { return (uint64_t)blockIdx.x * PW + (threadIdx.x >> 6); }
__device__ __forceinline__ uint64_t pf_read_step() { return (uint64_t)gridDim.x * PW; }

// alive matches of [lo, hi); *mine = this lane's last alive position (NO_POS if none).  Uniform control flow.
__device__ __forceinline__ uint64_t pf_count(const uint8_t *__restrict__ alive, uint64_t lo, uint64_t hi, uint64_t *mine)
{
    uint64_t n = 0;
    *mine = NO_POS;
    for (uint64_t base = lo; base < hi; base += 64) {
        const uint64_t i = base + lane_id();
        const bool a = i < hi && alive[i];
        if (a) *mine = i;
        n += (uint64_t)__popcll(__ballot(a));
    }
    return n;
}

__global__ __launch_bounds__(PB) void k_pf_flag_single(const uint64_t *__restrict__ off, const int32_t *__restrict__ ref,
                                                       const uint8_t *__restrict__ alive, uint64_t n_reads, uint8_t *__restrict__ flag)
{
    for (uint64_t r = pf_first_read(); r < n_reads; r += pf_read_step()) {
        uint64_t mine;
        const uint64_t n = pf_count(alive, off[r], off[r + 1], &mine);
        if (n == 1 && mine != NO_POS && ref[mine] >= 0) flag[ref[mine]] = 1;
    }
}

__global__ __launch_bounds__(PB) void k_pf_filter(const uint64_t *__restrict__ off, const int32_t *__restrict__ ref, uint8_t *__restrict__ alive,
                                                  uint64_t n_reads, const uint8_t *__restrict__ flag)
{
    for (uint64_t r = pf_first_read(); r < n_reads; r += pf_read_step()) {
        const uint64_t lo = off[r], hi = off[r + 1];
        uint64_t n = 0;
        bool any = false;
        for (uint64_t base = lo; base < hi; base += 64) {
            const uint64_t i = base + lane_id();
            const bool a = i < hi && alive[i];
            const bool f = a && ref[i] >= 0 && flag[ref[i]];
            n += (uint64_t)__popcll(__ballot(a));
            any |= __ballot(f) != 0;
        }
        if (n < 2 || !any) continue;
        for (uint64_t i = lo + lane_id(); i < hi; i += 64)
            if (alive[i] && !(ref[i] >= 0 && flag[ref[i]])) alive[i] = 0;
    }
}

__global__ __launch_bounds__(PB) void k_pf_hist(const uint64_t *__restrict__ off, const int32_t *__restrict__ ref, const uint8_t *__restrict__ alive,
                                                uint64_t n_reads, uint32_t *__restrict__ uniq, uint32_t *__restrict__ amb)
{
    for (uint64_t r = pf_first_read(); r < n_reads; r += pf_read_step()) {
        const uint64_t lo = off[r], hi = off[r + 1];
        uint64_t mine;
        const uint64_t n = pf_count(alive, lo, hi, &mine);
        if (n == 1) {
            if (mine != NO_POS && ref[mine] >= 0) atomicAdd(&uniq[ref[mine]], 1u);
        } else if (n > 1) {
            for (uint64_t i = lo + lane_id(); i < hi; i += 64)
                if (alive[i] && ref[i] >= 0) atomicAdd(&amb[ref[i]], 1u);
        }
    }
}

__global__ __launch_bounds__(PB) void k_pf_accept(const uint32_t *__restrict__ uniq, const uint32_t *__restrict__ amb, uint64_t n_refs,
                                                  uint8_t *__restrict__ flag)
{
    for (uint64_t t = (uint64_t)blockIdx.x * PB + threadIdx.x; t < n_refs; t += (uint64_t)gridDim.x * PB) {
        const uint32_t u = uniq[t], a = amb[t];
        // single precision, like remove_low_confidence_references' static_cast<float> on both sides (:275)
        flag[t] = (u >= 3u && (float)u / (float)((uint64_t)u + a) >= 0.01f) ? 1 : 0;
    }
}

__device__ __forceinline__ void pf_pair_add(uint64_t *__restrict__ keys, uint32_t *__restrict__ cnt, uint64_t mask, uint64_t key,
                                            uint32_t *__restrict__ err)
{
    uint64_t s = keyset_slot_hash(key) & mask;
    for (uint64_t probes = 0; probes <= mask; ++probes) {
        const uint64_t old = atomicCAS((unsigned long long *)&keys[s], (unsigned long long)KEYSET_EMPTY, (unsigned long long)key);
        if (old == KEYSET_EMPTY || old == key) {
            atomicAdd(&cnt[s], 1u);
            return;
        }
        s = (s + 1) & mask;
    }
    atomicOr(err, PF_TABLE_FULL);
}

__global__ __launch_bounds__(PB) void k_pf_assoc(const uint64_t *__restrict__ off, const int32_t *__restrict__ ref, const uint8_t *__restrict__ alive,
                                                 uint64_t n_reads, uint32_t *__restrict__ uniq, uint32_t *__restrict__ all,
                                                 unsigned long long *__restrict__ first_pos, uint64_t *__restrict__ keys,
                                                 uint32_t *__restrict__ cnt, uint64_t mask, uint32_t *__restrict__ err)
{
    for (uint64_t r = pf_first_read(); r < n_reads; r += pf_read_step()) {
        const uint64_t lo = off[r], hi = off[r + 1];
        uint64_t mine;
        const uint64_t n = pf_count(alive, lo, hi, &mine);
        if (n == 1) {
            if (mine != NO_POS && ref[mine] >= 0) {
                atomicAdd(&uniq[ref[mine]], 1u);
                atomicAdd(&all[ref[mine]], 1u);
                atomicMin(&first_pos[ref[mine]], (unsigned long long)mine);
            }
        } else if (n > 1) {
            for (uint64_t i = lo + lane_id(); i < hi; i += 64)
                if (alive[i] && ref[i] >= 0) {
                    atomicAdd(&all[ref[i]], 1u);
                    atomicMin(&first_pos[ref[i]], (unsigned long long)i);
                }
            for (uint64_t a = lo; a < hi; ++a) {                           // a is the same in every lane
                if (!alive[a] || ref[a] < 0) continue;
                const uint64_t ra = (uint64_t)(uint32_t)ref[a];
                for (uint64_t j = lo + lane_id(); j < hi; j += 64)
                    if (alive[j] && ref[j] >= 0 && (uint64_t)(uint32_t)ref[j] != ra) pf_pair_add(keys, cnt, mask, ra << 32 | (uint32_t)ref[j], err);
            }
        }
    }
}

// reads ref_in / alive_in (the read as it was: the reference collects acc_ids before its loop), writes every match of ref_out / alive_out
__global__ __launch_bounds__(PB) void k_pf_explain(const uint64_t *__restrict__ off, const int32_t *__restrict__ ref_in, const uint8_t *__restrict__ alive_in,
                                                   uint64_t n_reads, const int32_t *__restrict__ expl, const uint64_t *__restrict__ taxa_len,
                                                   int32_t *__restrict__ ref_out, uint8_t *__restrict__ alive_out, uint64_t *__restrict__ ref_len)
{
    for (uint64_t r = pf_first_read(); r < n_reads; r += pf_read_step()) {
        const uint64_t lo = off[r], hi = off[r + 1];
        uint64_t mine;
        const uint64_t n = pf_count(alive_in, lo, hi, &mine);
        for (uint64_t i = lo + lane_id(); i < hi; i += 64) {
            int32_t x = ref_in[i];
            uint8_t a = alive_in[i];
            if (n > 1 && a && x >= 0 && expl[x] >= 0) {
                const int32_t y = expl[x];
                bool present = false;
                for (uint64_t j = lo; j < hi && !present; ++j) present = alive_in[j] && ref_in[j] == y;
                if (present) a = 0;
                else {
                    x = y;
                    ref_len[i] = taxa_len[y];
                }
            }
            ref_out[i] = x;
            alive_out[i] = a;
        }
    }
}

__global__ __launch_bounds__(PB) void k_pf_dup(const uint64_t *__restrict__ off, const int32_t *__restrict__ ref, const uint8_t *__restrict__ alive,
                                               uint64_t n_reads, uint8_t *__restrict__ dup)
{
    for (uint64_t r = pf_first_read(); r < n_reads; r += pf_read_step()) {
        const uint64_t lo = off[r], hi = off[r + 1];
        for (uint64_t i = lo + lane_id(); i < hi; i += 64) {
            bool d = false;
            if (alive[i] && ref[i] >= 0)
                for (uint64_t j = lo; j < i && !d; ++j) d = alive[j] && ref[j] == ref[i];
            dup[i] = d ? 1 : 0;
        }
    }
}

// sum[r] = the ratios of read r's alive matches added in match order, or -1 for a read with fewer than two matches
__global__ __launch_bounds__(PB) void k_pf_sum_ratio(const uint64_t *__restrict__ off, const uint8_t *__restrict__ alive, const uint64_t *__restrict__ hash_match,
                                                     const uint64_t *__restrict__ hash_count, uint64_t n_reads, double *__restrict__ sum)
{
    for (uint64_t r = pf_first_read(); r < n_reads; r += pf_read_step()) {
        const uint64_t lo = off[r], hi = off[r + 1];
        const double c = (double)hash_count[r];
        double s = 0.0;
        uint64_t n = 0;
        for (uint64_t base = lo; base < hi; base += 64) {
            const uint64_t i = base + lane_id();
            const bool a = i < hi && alive[i];
            const double ratio = a ? (double)hash_match[i] / c : 0.0;
            uint64_t m = __ballot(a);
            n += (uint64_t)__popcll(m);
            while (m) {                                                    // m is the same in every lane: one chain, in match order
                const int k = __ffsll((unsigned long long)m) - 1;
                s = s + __shfl(ratio, k);
                m &= m - 1;
            }
        }
        if (lane_id() == 0) sum[r] = n > 1 ? s : -1.0;
    }
}

// One EM iteration's device part.  post / valid / best are written for every match of every read; totals = {all_nts, unclassified_nts}.
__global__ __launch_bounds__(PB) void k_pf_em(const uint64_t *__restrict__ off, const int32_t *__restrict__ ref, uint8_t *__restrict__ alive,
                                              const uint8_t *__restrict__ dup, const double *__restrict__ log_match, const double *__restrict__ log_count,
                                              const double *__restrict__ log_sum, const uint64_t *__restrict__ query_len, uint64_t n_reads,
                                              const double *__restrict__ prior, const uint8_t *__restrict__ has_prior, double *__restrict__ post,
                                              uint8_t *__restrict__ valid, uint8_t *__restrict__ best, unsigned long long *__restrict__ ref_nts,
                                              unsigned long long *__restrict__ totals, uint32_t *__restrict__ err)
{
    unsigned long long acc_all = 0, acc_un = 0;                             // the same in every lane of the wave
    for (uint64_t r = pf_first_read(); r < n_reads; r += pf_read_step()) {
        const uint64_t lo = off[r], hi = off[r + 1];
        const unsigned long long qlen = query_len[r];
        uint64_t mine;
        const uint64_t n = pf_count(alive, lo, hi, &mine);
        if (n <= 1) {
            bool counted = false, unclassified = false;
            for (uint64_t i = lo + lane_id(); i < hi; i += 64) {
                uint8_t v = 0, b = 0;
                if (n == 1 && i == mine) {
                    const int32_t x = ref[i];
                    if (x < 0) {                                            // the read's "-" line (:670-676)
                        b = 1;
                        counted = unclassified = true;
                    } else if (has_prior[x]) {
                        post[i] = 0.0 + prior[x];                           // the single match's likelihood is 0.0 (:505)
                        v = b = 1;
                        counted = true;
                        atomicAdd(&ref_nts[x], qlen);
                    }
                }
                valid[i] = v;
                best[i] = b;
            }
            if (__ballot(counted)) acc_all += qlen;
            if (__ballot(unclassified)) acc_un += qlen;
            continue;
        }
        const double lc = log_count[r], ls = log_sum[r];
        double mx = -DBL_MAX;
        long long last = -1;
        for (uint64_t i = lo + lane_id(); i < hi; i += 64) {
            uint8_t v = 0;
            const int32_t x = ref[i];
            if (alive[i] && x >= 0 && has_prior[x]) {
                uint64_t src = i;
                if (dup[i])
                    for (uint64_t j = lo; j < i; ++j)
                        if (alive[j] && ref[j] == x) {
                            src = j;
                            break;
                        }
                const double p = ((log_match[src] - lc) - ls) + prior[x];
                post[i] = p;
                v = 1;
                if (p > mx) mx = p;
                last = (long long)i;                                        // min_post is never lowered (:709): the LAST such match goes
            }
            valid[i] = v;
        }
        mx = wave_max(mx);
        last = wave_max(last);
        bool any_best = false;
        for (uint64_t i = lo + lane_id(); i < hi; i += 64) {
            const bool b = valid[i] && post[i] >= mx;                       // ties stay, in match order (:699-707)
            best[i] = b ? 1 : 0;
            if (b) {
                any_best = true;
                atomicAdd(&ref_nts[ref[i]], qlen);
            }
        }
        if (__ballot(any_best)) acc_all += qlen;
        if (last < 0) {
            if (lane_id() == 0) atomicOr(err, PF_NO_PRIOR);
        } else if (lane_id() == 0)
            alive[last] = 0;
    }
    if (lane_id() == 0) {
        if (acc_all) atomicAdd(&totals[0], acc_all);
        if (acc_un) atomicAdd(&totals[1], acc_un);
    }
}

#define PF_TRY(expr) TAXOR_HIP_TRY_PREFIX("profile", expr, #expr)

// every array is allocated anew, with at least one element
template <class T> hipError_t alloc(DeviceBuf<T> &b, uint64_t n) { return b.alloc(std::max<uint64_t>(n, 1)); }

}   // namespace

struct taxor_gpu_profile {
    explicit taxor_gpu_profile(std::shared_ptr<taxor_profile_host_csr> h = std::make_shared<taxor_profile_host_csr>()) : host(std::move(h)) {}
    int device = 0;
    uint64_t n_reads = 0, n_refs = 0, n_matches = 0;
    hipStream_t st = nullptr;
    // the CSR as given (host copies the host stages read; never written after the constructor functions -- a feed shares them)
    std::shared_ptr<taxor_profile_host_csr> host;
    std::vector<uint64_t> &h_off = host->off, &h_ref_len0 = host->ref_len, &h_hash_match = host->hash_match, &h_query_len = host->query_len,
                          &h_hash_count = host->hash_count;
    DeviceBuf<uint64_t> d_off, d_ref_len, d_hash_match, d_query_len, d_hash_count, d_taxa_len, d_keys;
    DeviceBuf<int32_t> d_ref, d_ref2, d_expl;
    DeviceBuf<uint8_t> d_alive, d_alive2, d_flag, d_dup, d_valid, d_best, d_has_prior;
    DeviceBuf<uint32_t> d_uniq, d_all, d_cnt, d_err;
    DeviceBuf<unsigned long long> d_first, d_ref_nts, d_totals;
    DeviceBuf<double> d_log_match, d_log_count, d_sum, d_prior, d_post;
    uint64_t pair_slots = 0;
    // results
    std::vector<int32_t> r_ref, r_explained;
    std::vector<uint64_t> r_ref_len, r_taxa_len, r_ref_nts, r_pair_key, r_iter_ref_nts;
    std::vector<uint32_t> r_pair_count, r_unique, r_all;
    std::vector<uint8_t> r_alive, r_best, r_has_prior, r_alive1, r_alive2, r_alive3;
    std::vector<double> r_log_prior;
    taxor_profile_results res{};
    bool ran = false, done = false;
    ~taxor_gpu_profile()
    {
        if (st) (void)hipStreamDestroy(st);
    }
};

namespace {

// :349-399 over the downloaded counts.  expl[x] = the reference that explains x, or -1.  Map order is id order.
int explained_by(uint64_t n_refs, const std::vector<uint32_t> &uniq, const std::vector<uint32_t> &all, const std::vector<uint64_t> &pair_key,
                 const std::vector<uint32_t> &pair_count, std::vector<int32_t> &expl)
{
    const uint64_t np = pair_key.size();
    std::vector<uint64_t> order(np);
    for (uint64_t i = 0; i < np; ++i) order[i] = i;
    std::sort(order.begin(), order.end(), [&](uint64_t a, uint64_t b) { return pair_key[a] < pair_key[b]; });
    std::vector<uint64_t> key(np);
    std::vector<uint64_t> shared(np);
    for (uint64_t i = 0; i < np; ++i) {
        key[i] = pair_key[order[i]];
        shared[i] = pair_count[order[i]];
    }
    auto lookup = [&](uint64_t a, uint64_t b) -> uint64_t {
        const uint64_t k = a << 32 | b;
        const auto it = std::lower_bound(key.begin(), key.end(), k);
        return it != key.end() && *it == k ? shared[(uint64_t)(it - key.begin())] : 0;
    };
    expl.assign(n_refs, -1);
    for (uint64_t i = 0; i < np; ++i) {                                     // sorted by (ref, assoc): the two nested maps' order
        const uint64_t a = key[i] >> 32, b = key[i] & 0xffffffffull;
        const uint64_t a_u = uniq[a], a_all = all[a], b_u = uniq[b], b_all = all[b];
        if (a_u > b_u || a_all > b_all) {
            if (a_all - shared[i] < (uint64_t)(0.05 * (double)a_all) && expl[a] < 0) expl[a] = (int32_t)b;
        } else {
            if (b_all - lookup(b, a) < (uint64_t)(0.05 * (double)b_all) && expl[b] < 0) expl[b] = (int32_t)a;
        }
    }
    // :385-399, pass by pass in map order with the updates in place.  A chain that ends at a reference nobody explains is
    // resolved after at most as many passes as there are entries; one that runs into a cycle changes for ever.
    uint64_t entries = 0;
    for (uint64_t x = 0; x < n_refs; ++x) entries += expl[x] >= 0;
    bool found = true;
    for (uint64_t pass = 0; found; ++pass) {
        if (pass > entries + 1)
            return fail(TAXOR_E_ARG, "profile: the explained-by relation between references runs into a cycle (a reference is explained, through "
                                      "others, by itself); the chain resolution of the reference implementation does not end on such input");
        found = false;
        for (uint64_t x = 0; x < n_refs; ++x) {
            if (expl[x] < 0) continue;
            const int32_t y = expl[x];
            if (expl[y] >= 0 && (int32_t)x != expl[y]) {
                expl[x] = expl[y];
                found = true;
            }
        }
    }
    return TAXOR_OK;
}

// everything a run works in, beside the six arrays of the CSR
int alloc_work(taxor_gpu_profile *p)
{
    const uint64_t R = p->n_reads, F = p->n_refs, M = p->n_matches;
    PF_TRY(alloc(p->d_ref2, M));
    PF_TRY(alloc(p->d_alive, M));
    PF_TRY(alloc(p->d_alive2, M));
    PF_TRY(alloc(p->d_dup, M));
    PF_TRY(alloc(p->d_valid, M));
    PF_TRY(alloc(p->d_best, M));
    PF_TRY(alloc(p->d_post, M));
    PF_TRY(alloc(p->d_log_match, M));
    PF_TRY(alloc(p->d_log_count, R));
    PF_TRY(alloc(p->d_sum, R));
    PF_TRY(alloc(p->d_flag, F));
    PF_TRY(alloc(p->d_has_prior, F));
    PF_TRY(alloc(p->d_uniq, F));
    PF_TRY(alloc(p->d_all, F));
    PF_TRY(alloc(p->d_first, F));
    PF_TRY(alloc(p->d_ref_nts, F));
    PF_TRY(alloc(p->d_prior, F));
    PF_TRY(alloc(p->d_expl, F));
    PF_TRY(alloc(p->d_taxa_len, F));
    PF_TRY(alloc(p->d_totals, 2));
    PF_TRY(alloc(p->d_err, 1));
    return TAXOR_OK;
}

}   // namespace

extern "C" int taxor_gpu_profile_create(int device, const taxor_profile_csr *csr, taxor_gpu_profile **out)
{
    if (!csr || !out) return fail(TAXOR_E_ARG, "profile_create: null argument");
    *out = nullptr;
    const uint64_t R = csr->n_reads, F = csr->n_refs, M = csr->n_matches;
    if (!csr->read_off || (M && (!csr->ref || !csr->ref_len || !csr->hash_match)) || (R && (!csr->query_len || !csr->hash_count)))
        return fail(TAXOR_E_ARG, "profile_create: null array");
    if (F >= (1ull << 31)) return fail(TAXOR_E_ARG, "profile_create: more than 2^31 - 1 references");
    if (csr->read_off[0] != 0 || csr->read_off[R] != M) return fail(TAXOR_E_ARG, "profile_create: read_off does not span the matches");
    for (uint64_t r = 0; r < R; ++r)
        if (csr->read_off[r + 1] < csr->read_off[r]) return fail(TAXOR_E_ARG, "profile_create: read_off decreases");
    for (uint64_t i = 0; i < M; ++i)
        if (csr->ref[i] < -1 || (csr->ref[i] >= 0 && (uint64_t)csr->ref[i] >= F)) return fail(TAXOR_E_ARG, "profile_create: reference id out of range");
    PF_TRY(hipSetDevice(device));
    auto p = std::make_unique<taxor_gpu_profile>();
    p->device = device;
    p->n_reads = R;
    p->n_refs = F;
    p->n_matches = M;
    p->h_off.assign(csr->read_off, csr->read_off + R + 1);
    p->h_ref_len0.assign(csr->ref_len, csr->ref_len + M);
    p->h_hash_match.assign(csr->hash_match, csr->hash_match + M);
    p->h_query_len.assign(csr->query_len, csr->query_len + R);
    p->h_hash_count.assign(csr->hash_count, csr->hash_count + R);
    PF_TRY(hipStreamCreate(&p->st));
    PF_TRY(alloc(p->d_off, R + 1));
    PF_TRY(alloc(p->d_ref, M));
    PF_TRY(alloc(p->d_ref_len, M));
    PF_TRY(alloc(p->d_hash_match, M));
    PF_TRY(alloc(p->d_query_len, R));
    PF_TRY(alloc(p->d_hash_count, R));
    if (int rc = alloc_work(p.get())) return rc;
    PF_TRY(hipMemcpy(p->d_off.p, csr->read_off, (R + 1) * 8, hipMemcpyHostToDevice));
    if (M) {
        PF_TRY(hipMemcpy(p->d_ref.p, csr->ref, M * 4, hipMemcpyHostToDevice));
        PF_TRY(hipMemcpy(p->d_hash_match.p, csr->hash_match, M * 8, hipMemcpyHostToDevice));
    }
    if (R) {
        PF_TRY(hipMemcpy(p->d_query_len.p, csr->query_len, R * 8, hipMemcpyHostToDevice));
        PF_TRY(hipMemcpy(p->d_hash_count.p, csr->hash_count, R * 8, hipMemcpyHostToDevice));
    }
    *out = p.release();
    return TAXOR_OK;
}

// library-internal (profile_feed.hip): a profile over a CSR that is on the device already.  `host` holds the same CSR in host memory
// (the host stages of run() read it; shared with the caller, not copied); the six device arrays are single hipMalloc blocks of at
// least one element, matches' reference ids within [-1, n_refs).  On success the profile owns them, on failure the caller still does.
extern "C" __attribute__((visibility("hidden"))) int taxor_profile_adopt_device(int device, const std::shared_ptr<taxor_profile_host_csr> *host, uint64_t n_refs,
                                                                                uint64_t *d_off, int32_t *d_ref, uint64_t *d_ref_len, uint64_t *d_hash_match,
                                                                                uint64_t *d_query_len, uint64_t *d_hash_count, taxor_gpu_profile **out)
{
    if (!host || !*host || !out || !d_off || !d_ref || !d_ref_len || !d_hash_match || !d_query_len || !d_hash_count) return fail(TAXOR_E_ARG, "profile_adopt: null argument");
    *out = nullptr;
    const taxor_profile_host_csr &h = **host;
    if (h.off.empty()) return fail(TAXOR_E_ARG, "profile_adopt: read_off is empty");
    const uint64_t R = h.off.size() - 1, F = n_refs, M = h.off[R];
    if (F >= (1ull << 31)) return fail(TAXOR_E_ARG, "profile_adopt: more than 2^31 - 1 references");
    if (h.off[0] != 0 || h.ref_len.size() != M || h.hash_match.size() != M || h.query_len.size() != R || h.hash_count.size() != R)
        return fail(TAXOR_E_ARG, "profile_adopt: the host arrays do not span the reads and the matches");
    PF_TRY(hipSetDevice(device));
    auto p = std::make_unique<taxor_gpu_profile>(*host);
    p->device = device;
    p->n_reads = R;
    p->n_refs = F;
    p->n_matches = M;
    PF_TRY(hipStreamCreate(&p->st));
    if (int rc = alloc_work(p.get())) return rc;
    p->d_off.p = d_off;
    p->d_ref.p = d_ref;
    p->d_ref_len.p = d_ref_len;
    p->d_hash_match.p = d_hash_match;
    p->d_query_len.p = d_query_len;
    p->d_hash_count.p = d_hash_count;
    *out = p.release();
    return TAXOR_OK;
}

extern "C" void taxor_gpu_profile_destroy(taxor_gpu_profile *p)
{
    if (!p) return;
    (void)hipSetDevice(p->device);
    delete p;
}

extern "C" int taxor_gpu_profile_run(taxor_gpu_profile *p, uint32_t em_steps, uint32_t flags)
{
    if (!p) return fail(TAXOR_E_ARG, "profile_run: null argument");
    if (em_steps < 1) return fail(TAXOR_E_ARG, "profile_run: em_steps < 1");
    if (p->ran) return fail(TAXOR_E_ARG, "profile_run: this object has run already (the rounds consume its matches)");
    p->ran = true;
    const bool trace = (flags & TAXOR_PROFILE_TRACE) != 0;
    const uint64_t R = p->n_reads, F = p->n_refs, M = p->n_matches;
    const double t0 = now_s();
    PF_TRY(hipSetDevice(p->device));
    hipStream_t st = p->st;
    const int g = grid_for(R, PW, P_GRID_CAP), gf = grid_for(F, PB, P_GRID_CAP);
    auto snapshot = [&](std::vector<uint8_t> &v) -> hipError_t {
        v.resize(M);
        return M ? hipMemcpyAsync(v.data(), p->d_alive.p, M, hipMemcpyDeviceToHost, st) : hipSuccess;
    };
    PF_TRY(hipMemsetAsync(p->d_alive.p, 1, std::max<uint64_t>(M, 1), st));
    PF_TRY(hipMemsetAsync(p->d_err.p, 0, 4, st));
    if (M) PF_TRY(hipMemcpyAsync(p->d_ref_len.p, p->h_ref_len0.data(), M * 8, hipMemcpyHostToDevice, st));
    // ---- round 1
    PF_TRY(hipMemsetAsync(p->d_flag.p, 0, std::max<uint64_t>(F, 1), st));
    k_pf_flag_single<<<g, PB, 0, st>>>(p->d_off.p, p->d_ref.p, p->d_alive.p, R, p->d_flag.p);
    k_pf_filter<<<g, PB, 0, st>>>(p->d_off.p, p->d_ref.p, p->d_alive.p, R, p->d_flag.p);
    if (trace) PF_TRY(snapshot(p->r_alive1));
    // ---- round 2
    PF_TRY(hipMemsetAsync(p->d_uniq.p, 0, std::max<uint64_t>(F, 1) * 4, st));
    PF_TRY(hipMemsetAsync(p->d_all.p, 0, std::max<uint64_t>(F, 1) * 4, st));
    k_pf_hist<<<g, PB, 0, st>>>(p->d_off.p, p->d_ref.p, p->d_alive.p, R, p->d_uniq.p, p->d_all.p);
    k_pf_accept<<<gf, PB, 0, st>>>(p->d_uniq.p, p->d_all.p, F, p->d_flag.p);
    k_pf_filter<<<g, PB, 0, st>>>(p->d_off.p, p->d_ref.p, p->d_alive.p, R, p->d_flag.p);
    if (trace) PF_TRY(snapshot(p->r_alive2));
    // ---- round 3: counts and the pair table, sized from the ordered pairs the reads can hold (and no more than the references admit)
    std::vector<uint8_t> h_alive(M);
    if (M) PF_TRY(hipMemcpyAsync(h_alive.data(), p->d_alive.p, M, hipMemcpyDeviceToHost, st));
    PF_TRY(hipStreamSynchronize(st));
    uint64_t pair_bound = 0;
    for (uint64_t r = 0; r < R; ++r) {
        uint64_t m = 0;
        for (uint64_t i = p->h_off[r]; i < p->h_off[r + 1]; ++i) m += h_alive[i];
        if (m > 1) pair_bound += m * (m - 1);
    }
    if (F > 1) pair_bound = std::min(pair_bound, F * (F - 1));
    else pair_bound = 0;
    uint64_t slots = 64;
    while (slots < 2 * pair_bound) slots <<= 1;
    p->pair_slots = slots;
    PF_TRY(alloc(p->d_keys, slots));
    PF_TRY(alloc(p->d_cnt, slots));
    PF_TRY(hipMemsetAsync(p->d_keys.p, 0xFF, slots * 8, st));
    PF_TRY(hipMemsetAsync(p->d_cnt.p, 0, slots * 4, st));
    PF_TRY(hipMemsetAsync(p->d_uniq.p, 0, std::max<uint64_t>(F, 1) * 4, st));
    PF_TRY(hipMemsetAsync(p->d_all.p, 0, std::max<uint64_t>(F, 1) * 4, st));
    PF_TRY(hipMemsetAsync(p->d_first.p, 0xFF, std::max<uint64_t>(F, 1) * 8, st));
    k_pf_assoc<<<g, PB, 0, st>>>(p->d_off.p, p->d_ref.p, p->d_alive.p, R, p->d_uniq.p, p->d_all.p, p->d_first.p, p->d_keys.p, p->d_cnt.p, slots - 1,
                                 p->d_err.p);
    std::vector<uint64_t> h_keys(slots), h_first(F);
    std::vector<uint32_t> h_cnt(slots);
    p->r_unique.resize(F);
    p->r_all.resize(F);
    uint32_t h_err = 0;
    PF_TRY(hipMemcpyAsync(h_keys.data(), p->d_keys.p, slots * 8, hipMemcpyDeviceToHost, st));
    PF_TRY(hipMemcpyAsync(h_cnt.data(), p->d_cnt.p, slots * 4, hipMemcpyDeviceToHost, st));
    if (F) {
        PF_TRY(hipMemcpyAsync(p->r_unique.data(), p->d_uniq.p, F * 4, hipMemcpyDeviceToHost, st));
        PF_TRY(hipMemcpyAsync(p->r_all.data(), p->d_all.p, F * 4, hipMemcpyDeviceToHost, st));
        PF_TRY(hipMemcpyAsync(h_first.data(), p->d_first.p, F * 8, hipMemcpyDeviceToHost, st));
    }
    PF_TRY(hipMemcpyAsync(&h_err, p->d_err.p, 4, hipMemcpyDeviceToHost, st));
    PF_TRY(hipStreamSynchronize(st));
    if (h_err & PF_TABLE_FULL) return fail(TAXOR_E_INTERNAL, "profile: the pair table overflowed its sizing bound");
    p->r_pair_key.clear();
    p->r_pair_count.clear();
    for (uint64_t s = 0; s < slots; ++s)
        if (h_keys[s] != KEYSET_EMPTY) {
            p->r_pair_key.push_back(h_keys[s]);
            p->r_pair_count.push_back(h_cnt[s]);
        }
    {
        const int rc = explained_by(F, p->r_unique, p->r_all, p->r_pair_key, p->r_pair_count, p->r_explained);
        if (rc != TAXOR_OK) return rc;
    }
    // taxa_lengths (:309-310,:326-327,:453-462): the ref_len of a reference's first match, explained references dropped
    p->r_taxa_len.assign(F, 0);
    p->r_has_prior.assign(F, 0);
    uint64_t n_taxa = 0;
    for (uint64_t x = 0; x < F; ++x)
        if (p->r_all[x] > 0) {
            p->r_taxa_len[x] = p->h_ref_len0[h_first[x]];
            if (p->r_explained[x] < 0) {
                p->r_has_prior[x] = 1;
                ++n_taxa;
            }
        }
    if (F) {
        PF_TRY(hipMemcpyAsync(p->d_expl.p, p->r_explained.data(), F * 4, hipMemcpyHostToDevice, st));
        PF_TRY(hipMemcpyAsync(p->d_taxa_len.p, p->r_taxa_len.data(), F * 8, hipMemcpyHostToDevice, st));
        PF_TRY(hipMemcpyAsync(p->d_has_prior.p, p->r_has_prior.data(), F, hipMemcpyHostToDevice, st));
    }
    k_pf_explain<<<g, PB, 0, st>>>(p->d_off.p, p->d_ref.p, p->d_alive.p, R, p->d_expl.p, p->d_taxa_len.p, p->d_ref2.p, p->d_alive2.p, p->d_ref_len.p);
    std::swap(p->d_ref.p, p->d_ref2.p);
    std::swap(p->d_alive.p, p->d_alive2.p);
    k_pf_dup<<<g, PB, 0, st>>>(p->d_off.p, p->d_ref.p, p->d_alive.p, R, p->d_dup.p);
    if (trace) PF_TRY(snapshot(p->r_alive3));
    p->r_ref.resize(M);
    p->r_ref_len.resize(M);
    if (M) {
        PF_TRY(hipMemcpyAsync(p->r_ref.data(), p->d_ref.p, M * 4, hipMemcpyDeviceToHost, st));
        PF_TRY(hipMemcpyAsync(p->r_ref_len.data(), p->d_ref_len.p, M * 8, hipMemcpyDeviceToHost, st));
    }
    // ---- EM.  log(match) and log(count) never change: one log per distinct integer
    {
        std::unordered_map<uint64_t, double> log_of;
        auto lg = [&](uint64_t v) {
            auto it = log_of.find(v);
            if (it == log_of.end()) it = log_of.emplace(v, log((double)v)).first;
            return it->second;
        };
        std::vector<double> lm(M), lc(R);
        for (uint64_t i = 0; i < M; ++i) lm[i] = lg(p->h_hash_match[i]);
        for (uint64_t r = 0; r < R; ++r) lc[r] = lg(p->h_hash_count[r]);
        if (M) PF_TRY(hipMemcpyAsync(p->d_log_match.p, lm.data(), M * 8, hipMemcpyHostToDevice, st));
        if (R) PF_TRY(hipMemcpyAsync(p->d_log_count.p, lc.data(), R * 8, hipMemcpyHostToDevice, st));
        PF_TRY(hipStreamSynchronize(st));
    }
    p->r_log_prior.assign(F, 0.0);
    for (uint64_t x = 0; x < F; ++x)
        if (p->r_has_prior[x]) p->r_log_prior[x] = log(1.0 / (double)n_taxa);       // :472
    p->r_ref_nts.assign(F, 0);
    p->r_iter_ref_nts.clear();
    std::vector<double> h_sum(R), h_post(M);
    std::vector<uint8_t> h_valid(M);
    unsigned long long h_tot[2] = {0, 0};
    double cond = -DBL_MAX, log_unclassified = 0.0;
    uint32_t step = 0, iterations = 0;
    const double t_em = now_s();
    while (step < em_steps) {
        k_pf_sum_ratio<<<g, PB, 0, st>>>(p->d_off.p, p->d_alive.p, p->d_hash_match.p, p->d_hash_count.p, R, p->d_sum.p);
        if (R) PF_TRY(hipMemcpyAsync(h_sum.data(), p->d_sum.p, R * 8, hipMemcpyDeviceToHost, st));
        PF_TRY(hipStreamSynchronize(st));
        for (uint64_t r = 0; r < R; ++r)
            if (h_sum[r] >= 0.0) h_sum[r] = log(h_sum[r]);                          // :496
        if (R) PF_TRY(hipMemcpyAsync(p->d_sum.p, h_sum.data(), R * 8, hipMemcpyHostToDevice, st));
        if (F) PF_TRY(hipMemcpyAsync(p->d_prior.p, p->r_log_prior.data(), F * 8, hipMemcpyHostToDevice, st));
        PF_TRY(hipMemsetAsync(p->d_ref_nts.p, 0, std::max<uint64_t>(F, 1) * 8, st));
        PF_TRY(hipMemsetAsync(p->d_totals.p, 0, 16, st));
        k_pf_em<<<g, PB, 0, st>>>(p->d_off.p, p->d_ref.p, p->d_alive.p, p->d_dup.p, p->d_log_match.p, p->d_log_count.p, p->d_sum.p, p->d_query_len.p, R,
                                  p->d_prior.p, p->d_has_prior.p, p->d_post.p, p->d_valid.p, p->d_best.p, p->d_ref_nts.p, p->d_totals.p, p->d_err.p);
        if (M) {
            PF_TRY(hipMemcpyAsync(h_post.data(), p->d_post.p, M * 8, hipMemcpyDeviceToHost, st));
            PF_TRY(hipMemcpyAsync(h_valid.data(), p->d_valid.p, M, hipMemcpyDeviceToHost, st));
        }
        if (F) PF_TRY(hipMemcpyAsync(p->r_ref_nts.data(), p->d_ref_nts.p, F * 8, hipMemcpyDeviceToHost, st));
        PF_TRY(hipMemcpyAsync(h_tot, p->d_totals.p, 16, hipMemcpyDeviceToHost, st));
        PF_TRY(hipMemcpyAsync(&h_err, p->d_err.p, 4, hipMemcpyDeviceToHost, st));
        PF_TRY(hipStreamSynchronize(st));
        if (h_err & PF_NO_PRIOR)
            return fail(TAXOR_E_ARG, "profile: in EM iteration " + std::to_string(iterations) + " a read with several matches has none whose reference "
                                      "carries a prior (all of them were explained away); the reference implementation erases an invalid iterator there");
        ++iterations;
        if (trace) p->r_iter_ref_nts.insert(p->r_iter_ref_nts.end(), p->r_ref_nts.begin(), p->r_ref_nts.end());
        double new_cond = 0;
        for (uint64_t i = 0; i < M; ++i)
            if (h_valid[i]) new_cond += h_post[i];                                  // :697, one chain in map order
        const double log_all = log((double)h_tot[0]);
        for (uint64_t x = 0; x < F; ++x)
            if (p->r_has_prior[x]) p->r_log_prior[x] = log((double)p->r_ref_nts[x] + 0.000000000001) - log_all;     // :561
        log_unclassified = log((double)h_tot[1] + 0.000000000001) - log_all;       // :564
        const double diff = new_cond - cond;
        if (diff < fabs(log(0.0001))) break;                                        // :726
        cond = new_cond;
        ++step;
    }
    p->r_alive.resize(M);
    p->r_best.resize(M);
    if (M) {
        PF_TRY(hipMemcpyAsync(p->r_alive.data(), p->d_alive.p, M, hipMemcpyDeviceToHost, st));
        PF_TRY(hipMemcpyAsync(p->r_best.data(), p->d_best.p, M, hipMemcpyDeviceToHost, st));
    }
    PF_TRY(hipStreamSynchronize(st));
    const double t1 = now_s();
    taxor_profile_results &o = p->res;
    memset(&o, 0, sizeof o);
    o.n_reads = R;
    o.n_refs = F;
    o.n_matches = M;
    o.ref = p->r_ref.data();
    o.ref_len = p->r_ref_len.data();
    o.alive = p->r_alive.data();
    o.best = p->r_best.data();
    o.has_prior = p->r_has_prior.data();
    o.taxa_len = p->r_taxa_len.data();
    o.ref_nts = p->r_ref_nts.data();
    o.log_prior = p->r_log_prior.data();
    o.explained_by = p->r_explained.data();
    o.unique_reads = p->r_unique.data();
    o.all_reads = p->r_all.data();
    o.all_nts = h_tot[0];
    o.unclassified_nts = h_tot[1];
    o.log_unclassified = log_unclassified;
    o.em_steps_needed = step;
    o.em_iterations = iterations;
    o.n_pairs = p->r_pair_key.size();
    o.pair_slots = p->pair_slots;
    o.pair_key = p->r_pair_key.data();
    o.pair_count = p->r_pair_count.data();
    if (trace) {
        o.alive_round1 = p->r_alive1.data();
        o.alive_round2 = p->r_alive2.data();
        o.alive_round3 = p->r_alive3.data();
        o.iter_ref_nts = p->r_iter_ref_nts.data();
    }
    o.seconds_filter = t_em - t0;
    o.seconds_em = t1 - t_em;
    p->done = true;
    return TAXOR_OK;
}

extern "C" int taxor_gpu_profile_results(taxor_gpu_profile *p, taxor_profile_results *out)
{
    if (!p || !out) return fail(TAXOR_E_ARG, "profile_results: null argument");
    if (!p->done) return fail(TAXOR_E_ARG, "profile_results: no completed run");
    *out = p->res;
    return TAXOR_OK;
}
