// sketch.hip -- similarity between the key sets of user bins, on the device (`taxor build --group-similar`; DESIGN.md section 9,
// "Similarity-aware layout").  The reference leaves this to chopper (HyperLogLog sketches, clustering of user bins of similar size;
// src/main/taxor_build.cpp:470-472); here it is exact arithmetic over bottom-m sketches:
//
//   sketch of a bin   the min(m, n) smallest values of mix(key) over the bin's distinct keys, ascending.  mix is one fixed bijection on
//                     64-bit values (sk_mix below), so distinct keys give distinct values and one rule serves every hashing mode.
//     k_sk_select     a bin keeps the values under a threshold guessed from (2m + 32) / n: counted first, then written to the bin's
//                     segment of a candidate array.  A bin that comes out with fewer than min(m, n) candidates is counted again under a
//                     threshold 16 times as wide, so after at most 16 steps every bin has enough (the last threshold keeps every key)
//     rocPRIM         segmented radix sort of the candidates
//     k_sk_gather     the first min(m, n) of every segment
//   pairs             tau_b = 2^64 - 1 when the sketch holds every key of b (count <= m), else b's largest sketch value.  Below
//                     tau = min(tau_a, tau_b) both sketches hold EVERY mixed key of their bins, so
//                       shared[a][b] = |{v <= tau} in both|,  uni[a][b] = |A <= tau| + |B <= tau| - shared
//                     is the Jaccard index of an unbiased sample, and the exact one when both sketches are complete.
//     k_sketch_pairs  a block holds P_COLS column sketches in LDS and streams P_ROWS rows past them; a wave takes one row, keeps its
//                     values in registers (m / 64 per lane) and searches them in each column by binary search; ballot + popcount count.
#include "../../include/taxor_gpu_tools.h"
#include "device_prims.h"
#include "hip_host.h"

#include <hip/hip_runtime.h>
#include <rocprim/device/device_segmented_radix_sort.hpp>

#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

namespace {

using namespace taxor;

constexpr int SB = 256;                          // threads per block, both stages
constexpr uint64_t SK_TILE = 4096;               // keys of one bin a block takes at a time
constexpr uint32_t SK_MAX_M = 1024;
constexpr uint64_t SK_BATCH = 1ull << 26;        // candidates, and sketch slots, on the device at a time
constexpr uint64_t SK_UPLOAD_KEYS = 1ull << 27;  // keys of a host array on the device at a time
constexpr int SK_STEPS = 16;                     // threshold widenings: 16^16 = 2^64
constexpr int P_COLS = 4;                        // column sketches in LDS (8 KB each at m = 1024)
constexpr int P_ROWS = 32;                       // rows a block streams past them: 8 per wave
constexpr int P_VALS = SK_MAX_M / 64;            // a row's values per lane

// the mixer: the splitmix64 step -- add the golden-ratio constant, then two xor-shift-multiply rounds and a
// final xor-shift.  Every step is invertible on 64-bit values
__device__ __forceinline__ uint64_t sk_mix(uint64_t x)
{
    x += 0x9E3779B97F4A7C15ull;
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
    return x ^ (x >> 31);
}

// tile ti: keys [first, min(first + SK_TILE, off[bin + 1])) of bin tile_bin[ti].  SCATTER = false: cnt[bin] += values <= thr[bin].
// SCATTER = true: the same values go to cand[cbase[bin] + slot], slots handed out through cnt[bin] (any order: they are sorted next);
// ccnt[bin] is the count the first form found, and bounds the slots
template <bool SCATTER>
__global__ __launch_bounds__(SB) void k_sk_select(const uint64_t *__restrict__ keys, const uint64_t *__restrict__ off, const uint64_t *__restrict__ thr,
                                                  const uint32_t *__restrict__ tile_bin, const uint64_t *__restrict__ tile_first, uint32_t n_tiles,
                                                  uint32_t *cnt, const uint32_t *__restrict__ ccnt, const uint32_t *__restrict__ cbase,
                                                  uint64_t *__restrict__ cand)
{
    for (uint32_t ti = blockIdx.x; ti < n_tiles; ti += gridDim.x) {
        const uint32_t b = tile_bin[ti];
        const uint64_t i0 = tile_first[ti], i1 = min(i0 + SK_TILE, off[b + 1]), T = thr[b];
        for (uint64_t j = i0; j < i1; j += SB) {                  // (uniform trip count: wave_append is a wave operation)
            const uint64_t i = j + threadIdx.x;
            const uint64_t v = i < i1 ? sk_mix(keys[i]) : 0;
            const bool c = i < i1 && v <= T;
            const uint32_t slot = wave_append(c, &cnt[b]);
            if (SCATTER && c && slot < ccnt[b]) cand[(uint64_t)cbase[b] + slot] = v;
        }
    }
}

__global__ __launch_bounds__(SB) void k_sk_gather(const uint64_t *__restrict__ sorted, const uint32_t *__restrict__ cbase, const uint32_t *__restrict__ len,
                                                  uint64_t n_bins, uint32_t m, uint64_t *__restrict__ out)
{
    const uint64_t total = n_bins * m;
    for (uint64_t x = (uint64_t)blockIdx.x * SB + threadIdx.x; x < total; x += (uint64_t)gridDim.x * SB) {
        const uint64_t b = x / m;
        const uint32_t j = (uint32_t)(x - b * m);
        out[x] = j < len[b] ? sorted[(uint64_t)cbase[b] + j] : 0;
    }
}

// number of values <= t in the ascending B[0, n)
__device__ __forceinline__ uint32_t sk_upper(const uint64_t *B, uint32_t n, uint64_t t)
{
    uint32_t lo = 0, hi = n;
    while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        if (B[mid] <= t) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

// grid (columns / P_COLS, rows / P_ROWS); dynamic LDS: P_COLS * m values
__global__ __launch_bounds__(SB) void k_sketch_pairs(const uint64_t *__restrict__ sketch, const uint32_t *__restrict__ len, const uint64_t *__restrict__ tau,
                                                     uint32_t n, uint32_t m, uint32_t *__restrict__ shared, uint32_t *__restrict__ uni)
{
    extern __shared__ uint64_t sB[];
    const uint32_t c0 = blockIdx.x * P_COLS, r0 = blockIdx.y * P_ROWS;
    const uint32_t n_cols = min((uint32_t)P_COLS, n - c0);
    for (uint32_t c = 0; c < n_cols; ++c) {
        const uint32_t L = min(len[c0 + c], m);
        const uint64_t *__restrict__ src = sketch + (uint64_t)(c0 + c) * m;
        for (uint32_t i = threadIdx.x; i < L; i += SB) sB[c * m + i] = src[i];
    }
    __syncthreads();
    const uint32_t lane = lane_id(), r1 = min(r0 + (uint32_t)P_ROWS, n);
    for (uint32_t r = r0 + (threadIdx.x >> 6); r < r1; r += SB / 64) {
        const uint32_t la = min(len[r], m);
        const uint64_t ta = tau[r];
        const uint64_t *__restrict__ A = sketch + (uint64_t)r * m;
        uint64_t av[P_VALS];
#pragma unroll
        for (int q = 0; q < P_VALS; ++q) {
            const uint32_t i = (uint32_t)q * 64u + lane;
            av[q] = i < la ? A[i] : ~0ull;
        }
        uint32_t my_shared = 0, my_uni = 0;
        for (uint32_t c = 0; c < n_cols; ++c) {
            const uint64_t *B = sB + c * m;
            const uint64_t t = min(ta, tau[c0 + c]);
            const uint32_t nB = sk_upper(B, min(len[c0 + c], m), t);      // (the same in every lane: LDS broadcasts)
            uint32_t nA = 0, sh = 0;
#pragma unroll
            for (int q = 0; q < P_VALS; ++q) {
                if ((uint32_t)q * 64u < la) {                             // (la is the wave's: the lanes stay together)
                    const uint64_t v = av[q];
                    const bool in = (uint32_t)q * 64u + lane < la && v <= t;
                    // v, if B[0, nB) holds it, is at [base, base + cnt): the trip count follows nB alone, the same in every lane
                    uint32_t base = 0, cnt = nB;
                    while (cnt > 1) {
                        const uint32_t half = cnt >> 1;
                        if (B[base + half] <= v) base += half;
                        cnt -= half;
                    }
                    const bool found = in && nB > 0 && B[base] == v;
                    nA += (uint32_t)__popcll(__ballot(in));
                    sh += (uint32_t)__popcll(__ballot(found));
                }
            }
            if (lane == c) { my_shared = sh; my_uni = nA + nB - sh; }
        }
        if (lane < n_cols) {
            shared[(uint64_t)r * n + c0 + lane] = my_shared;
            uni[(uint64_t)r * n + c0 + lane] = my_uni;
        }
    }
}

#define SK_TRY(expr) TAXOR_HIP_TRY_PREFIX("sketch", expr, #expr)

// threshold under which a bin of n keys is expected to keep 2m + 32 values, widened 16-fold per step; 2^64 - 1 keeps every key
uint64_t sk_threshold(uint64_t n, uint32_t m, int step)
{
    double p = (2.0 * m + 32.0) / (double)std::max<uint64_t>(n, 1);
    for (int s = 0; s < step && p < 1.0; ++s) p *= 16.0;
    if (p >= 1.0 || step >= SK_STEPS) return UINT64_MAX;
    return (uint64_t)(p * 18446744073709551616.0);
}

// bins [0, nb) whose keys lie at d_keys[off[b] .. off[b + 1]) (off: host); sketch / len: host, for these bins
int sketch_bins(const uint64_t *d_keys, const uint64_t *off, uint64_t nb, uint32_t m, uint64_t *sketch, uint32_t *len, hipStream_t st)
{
    for (uint64_t b = 0; b < nb; ++b) len[b] = (uint32_t)std::min<uint64_t>(m, off[b + 1] - off[b]);
    if (off[nb] == off[0]) return TAXOR_OK;
    // tiles in bin order, and where each bin's tiles begin
    std::vector<uint32_t> tile_bin;
    std::vector<uint64_t> tile_first, bin_tile0(nb + 1);
    for (uint64_t b = 0; b < nb; ++b) {
        bin_tile0[b] = tile_bin.size();
        for (uint64_t i = off[b]; i < off[b + 1]; i += SK_TILE) { tile_bin.push_back((uint32_t)b); tile_first.push_back(i); }
    }
    bin_tile0[nb] = tile_bin.size();
    if (tile_bin.size() >= (1ull << 32)) return fail(TAXOR_E_ARG, "keys_sketch: too many keys in one call");
    DeviceBuf<uint64_t> d_off, d_thr, d_tfirst;
    DeviceBuf<uint32_t> d_tbin, d_cnt, d_ccnt, d_cbase, d_len;
    SK_TRY(d_off.alloc(nb + 1));
    SK_TRY(d_thr.alloc(nb));
    SK_TRY(d_cnt.alloc(nb));
    SK_TRY(d_ccnt.alloc(nb));
    SK_TRY(d_cbase.alloc(nb));
    SK_TRY(d_len.alloc(nb));
    SK_TRY(d_tbin.alloc(tile_bin.size()));
    SK_TRY(d_tfirst.alloc(tile_bin.size()));
    SK_TRY(hipMemcpyAsync(d_off.p, off, (nb + 1) * sizeof(uint64_t), hipMemcpyHostToDevice, st));
    SK_TRY(hipMemcpyAsync(d_len.p, len, nb * sizeof(uint32_t), hipMemcpyHostToDevice, st));
    SK_TRY(hipMemcpyAsync(d_tbin.p, tile_bin.data(), tile_bin.size() * sizeof(uint32_t), hipMemcpyHostToDevice, st));
    SK_TRY(hipMemcpyAsync(d_tfirst.p, tile_first.data(), tile_first.size() * sizeof(uint64_t), hipMemcpyHostToDevice, st));
    // ---- thresholds and candidate counts; a bin that keeps too few is counted again under a wider threshold
    std::vector<uint64_t> thr(nb);
    std::vector<uint32_t> ccnt(nb, 0), cnt(nb);
    std::vector<uint64_t> pending(nb);
    for (uint64_t b = 0; b < nb; ++b) pending[b] = b;
    for (int step = 0; !pending.empty(); ++step) {
        if (step > SK_STEPS) return fail(TAXOR_E_INTERNAL, "keys_sketch: a bin kept fewer values than it has keys under the widest threshold");
        std::vector<uint32_t> tb;
        std::vector<uint64_t> tf;
        for (uint64_t b : pending) {
            thr[b] = sk_threshold(off[b + 1] - off[b], m, step);
            if (step == 0) continue;                                  // (the first step runs every tile)
            tb.insert(tb.end(), tile_bin.begin() + bin_tile0[b], tile_bin.begin() + bin_tile0[b + 1]);
            tf.insert(tf.end(), tile_first.begin() + bin_tile0[b], tile_first.begin() + bin_tile0[b + 1]);
        }
        DeviceBuf<uint32_t> d_tb;
        DeviceBuf<uint64_t> d_tf;
        const uint32_t *p_tb = d_tbin.p;
        const uint64_t *p_tf = d_tfirst.p;
        uint64_t nt = tile_bin.size();
        if (step > 0) {
            nt = tb.size();
            SK_TRY(d_tb.alloc(std::max<uint64_t>(nt, 1)));
            SK_TRY(d_tf.alloc(std::max<uint64_t>(nt, 1)));
            SK_TRY(hipMemcpyAsync(d_tb.p, tb.data(), nt * sizeof(uint32_t), hipMemcpyHostToDevice, st));
            SK_TRY(hipMemcpyAsync(d_tf.p, tf.data(), nt * sizeof(uint64_t), hipMemcpyHostToDevice, st));
            p_tb = d_tb.p;
            p_tf = d_tf.p;
        }
        SK_TRY(hipMemcpyAsync(d_thr.p, thr.data(), nb * sizeof(uint64_t), hipMemcpyHostToDevice, st));
        SK_TRY(hipMemsetAsync(d_cnt.p, 0, nb * sizeof(uint32_t), st));
        if (nt) hipLaunchKernelGGL(k_sk_select<false>, dim3(grid_for(nt, 1, 16384)), dim3(SB), 0, st, d_keys, d_off.p, d_thr.p, p_tb, p_tf, (uint32_t)nt, d_cnt.p,
                                   (const uint32_t *)nullptr, (const uint32_t *)nullptr, (uint64_t *)nullptr);
        SK_TRY(hipGetLastError());
        SK_TRY(hipMemcpyAsync(cnt.data(), d_cnt.p, nb * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
        SK_TRY(hipStreamSynchronize(st));
        std::vector<uint64_t> again;
        for (uint64_t b : pending) {
            if (cnt[b] >= len[b]) ccnt[b] = cnt[b];
            else again.push_back(b);
        }
        pending.swap(again);
    }
    SK_TRY(hipMemcpyAsync(d_thr.p, thr.data(), nb * sizeof(uint64_t), hipMemcpyHostToDevice, st));
    SK_TRY(hipMemcpyAsync(d_ccnt.p, ccnt.data(), nb * sizeof(uint32_t), hipMemcpyHostToDevice, st));
    // ---- batches of bins: candidates out, sorted per bin, the first len[b] of each to the host
    DeviceBuf<uint64_t> cand, sorted, d_sk;
    DeviceBuf<uint32_t> d_end;
    DeviceBuf<uint8_t> tmp;
    std::vector<uint32_t> cbase(nb, 0), cend(nb, 0);
    for (uint64_t b0 = 0; b0 < nb;) {
        uint64_t b1 = b0, total = 0;
        while (b1 < nb && (b1 == b0 || (total + ccnt[b1] <= SK_BATCH && (b1 - b0 + 1) * m <= SK_BATCH))) {
            cbase[b1] = (uint32_t)total;
            total += ccnt[b1];
            cend[b1] = (uint32_t)total;
            ++b1;
        }
        if (total >= (1ull << 32)) return fail(TAXOR_E_ARG, "keys_sketch: a bin keeps 2^32 values or more under its threshold");
        const uint64_t n = b1 - b0;
        SK_TRY(d_sk.reserve(n * m, n * m));
        if (total) {
            SK_TRY(cand.reserve(total, total));
            SK_TRY(sorted.reserve(total, total));
            SK_TRY(d_end.reserve(n, n));
            SK_TRY(hipMemcpyAsync(d_cbase.p + b0, cbase.data() + b0, n * sizeof(uint32_t), hipMemcpyHostToDevice, st));
            SK_TRY(hipMemcpyAsync(d_end.p, cend.data() + b0, n * sizeof(uint32_t), hipMemcpyHostToDevice, st));
            SK_TRY(hipMemsetAsync(d_cnt.p + b0, 0, n * sizeof(uint32_t), st));
            const uint64_t t0 = bin_tile0[b0], nt = bin_tile0[b1] - t0;
            if (nt) hipLaunchKernelGGL(k_sk_select<true>, dim3(grid_for(nt, 1, 16384)), dim3(SB), 0, st, d_keys, d_off.p, d_thr.p, d_tbin.p + t0, d_tfirst.p + t0,
                                       (uint32_t)nt, d_cnt.p, (const uint32_t *)d_ccnt.p, (const uint32_t *)d_cbase.p, cand.p);
            SK_TRY(hipGetLastError());
            size_t tmp_bytes = 0;
            SK_TRY(rocprim::segmented_radix_sort_keys(nullptr, tmp_bytes, cand.p, sorted.p, (unsigned)total, (unsigned)n, d_cbase.p + b0, d_end.p, 0, 64, st));
            SK_TRY(tmp.reserve(tmp_bytes, std::max<uint64_t>(tmp_bytes, 16)));
            SK_TRY(rocprim::segmented_radix_sort_keys((void *)tmp.p, tmp_bytes, cand.p, sorted.p, (unsigned)total, (unsigned)n, d_cbase.p + b0, d_end.p, 0, 64, st));
            hipLaunchKernelGGL(k_sk_gather, dim3(grid_for(n * m, SB, 16384)), dim3(SB), 0, st, sorted.p, d_cbase.p + b0, d_len.p + b0, n, m, d_sk.p);
            SK_TRY(hipGetLastError());
        } else
            SK_TRY(hipMemsetAsync(d_sk.p, 0, n * m * sizeof(uint64_t), st));
        SK_TRY(hipMemcpyAsync(sketch + b0 * m, d_sk.p, n * m * sizeof(uint64_t), hipMemcpyDeviceToHost, st));
        SK_TRY(hipStreamSynchronize(st));
        b0 = b1;
    }
    return TAXOR_OK;
}

} // namespace

extern "C" {

int taxor_gpu_keys_sketch(int device, const uint64_t *keys, int keys_on_device, const uint64_t *off, uint64_t n_bins, uint32_t m, uint64_t *sketch,
                          uint32_t *len)
{
    if (!off || !sketch || !len || n_bins == 0) return fail(TAXOR_E_ARG, "keys_sketch: null argument");
    if (m < 1 || m > SK_MAX_M) return fail(TAXOR_E_ARG, "keys_sketch: the sketch size must be in [1, %u]", SK_MAX_M);
    if (n_bins >= (1ull << 32)) return fail(TAXOR_E_ARG, "keys_sketch: n_bins must be below 2^32");
    for (uint64_t b = 0; b < n_bins; ++b)
        if (off[b + 1] < off[b] || off[b + 1] - off[b] >= (1ull << 32)) return fail(TAXOR_E_ARG, "keys_sketch: bin offsets decrease, or a bin of 2^32 keys or more");
    if (off[n_bins] == off[0]) {
        std::fill(len, len + n_bins, 0u);
        return TAXOR_OK;
    }
    if (!keys) return fail(TAXOR_E_ARG, "keys_sketch: null keys");
    SK_TRY(hipSetDevice(device));
    if (keys_on_device) {
        std::vector<uint64_t> rel(off, off + n_bins + 1);
        for (uint64_t &x : rel) x -= off[0];
        return sketch_bins(keys + off[0], rel.data(), n_bins, m, sketch, len, nullptr);
    }
    // host keys: ranges of bins whose keys go up together
    DeviceBuf<uint64_t> d_keys;
    for (uint64_t b0 = 0; b0 < n_bins;) {
        uint64_t b1 = b0 + 1;
        while (b1 < n_bins && off[b1 + 1] - off[b0] <= SK_UPLOAD_KEYS) ++b1;
        const uint64_t nk = off[b1] - off[b0];
        SK_TRY(d_keys.reserve(nk, std::max<uint64_t>(nk, 16)));
        if (nk) SK_TRY(hipMemcpy(d_keys.p, keys + off[b0], nk * sizeof(uint64_t), hipMemcpyHostToDevice));
        std::vector<uint64_t> rel(off + b0, off + b1 + 1);
        for (uint64_t &x : rel) x -= off[b0];
        if (int rc = sketch_bins(d_keys.p, rel.data(), b1 - b0, m, sketch + b0 * m, len + b0, nullptr)) return rc;
        b0 = b1;
    }
    return TAXOR_OK;
}

int taxor_gpu_sketch_pairs(int device, const uint64_t *sketch, const uint32_t *len, const uint64_t *count, uint64_t n, uint32_t m, uint32_t *shared,
                           uint32_t *uni, float *kernel_ms)
{
    if (!sketch || !len || !count || !shared || !uni) return fail(TAXOR_E_ARG, "sketch_pairs: null argument");
    if (n < 1 || n > 8192) return fail(TAXOR_E_ARG, "sketch_pairs: n must be in [1, 8192]");
    if (m < 1 || m > SK_MAX_M) return fail(TAXOR_E_ARG, "sketch_pairs: the sketch size must be in [1, %u]", SK_MAX_M);
    std::vector<uint64_t> tau(n);
    for (uint64_t b = 0; b < n; ++b) {
        if (len[b] != std::min<uint64_t>(count[b], m))
            return fail(TAXOR_E_ARG, "sketch_pairs: bin %llu has %u sketch values, its %llu keys give %llu", (unsigned long long)b, len[b],
                        (unsigned long long)count[b], (unsigned long long)std::min<uint64_t>(count[b], m));
        tau[b] = count[b] <= m ? UINT64_MAX : sketch[b * m + len[b] - 1];
    }
    SK_TRY(hipSetDevice(device));
    DeviceBuf<uint64_t> d_sk, d_tau;
    DeviceBuf<uint32_t> d_len, d_shared, d_uni;
    SK_TRY(d_sk.alloc(n * m));
    SK_TRY(d_tau.alloc(n));
    SK_TRY(d_len.alloc(n));
    SK_TRY(d_shared.alloc(n * n));
    SK_TRY(d_uni.alloc(n * n));
    SK_TRY(hipMemcpy(d_sk.p, sketch, n * m * sizeof(uint64_t), hipMemcpyHostToDevice));
    SK_TRY(hipMemcpy(d_tau.p, tau.data(), n * sizeof(uint64_t), hipMemcpyHostToDevice));
    SK_TRY(hipMemcpy(d_len.p, len, n * sizeof(uint32_t), hipMemcpyHostToDevice));
    hipEvent_t e0 = nullptr, e1 = nullptr;
    SK_TRY(hipEventCreate(&e0));
    if (hipEventCreate(&e1) != hipSuccess) {
        (void)hipEventDestroy(e0);
        return fail(TAXOR_E_HIP, "sketch_pairs: event creation failed");
    }
    const dim3 grid((uint32_t)((n + P_COLS - 1) / P_COLS), (uint32_t)((n + P_ROWS - 1) / P_ROWS));
    hipError_t e = hipEventRecord(e0, nullptr);
    hipLaunchKernelGGL(k_sketch_pairs, grid, dim3(SB), (size_t)P_COLS * m * sizeof(uint64_t), nullptr, d_sk.p, d_len.p, d_tau.p, (uint32_t)n, m, d_shared.p,
                       d_uni.p);
    if (e == hipSuccess) e = hipGetLastError();
    if (e == hipSuccess) e = hipEventRecord(e1, nullptr);
    if (e == hipSuccess) e = hipMemcpy(shared, d_shared.p, n * n * sizeof(uint32_t), hipMemcpyDeviceToHost);
    if (e == hipSuccess) e = hipMemcpy(uni, d_uni.p, n * n * sizeof(uint32_t), hipMemcpyDeviceToHost);
    float ms = 0.f;
    if (e == hipSuccess) e = hipEventElapsedTime(&ms, e0, e1);
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
    SK_TRY(e);
    if (kernel_ms) *kernel_ms = ms;
    return TAXOR_OK;
}

// the global rank (host code around the pairs kernel): windows of bins of similar size, each paired on the device and cluster-ordered
int taxor_similarity_rank(int device, const uint64_t *sketch, const uint32_t *len, const uint64_t *counts, uint64_t n, uint32_t m, uint64_t window,
                          double jmin, uint64_t *rank, uint64_t *n_multi, float *pairs_ms)
{
    if (!sketch || !len || !counts || !rank || n == 0 || n >= (1ull << 31) || m == 0 || window < 2 || window > 8192 || !(jmin > 0.0) || jmin > 1.0)
        return TAXOR_E_ARG;
    std::vector<uint64_t> P(n);
    for (uint64_t i = 0; i < n; ++i) P[i] = i;
    std::sort(P.begin(), P.end(), [&](uint64_t a, uint64_t b) { return counts[a] > counts[b] || (counts[a] == counts[b] && a < b); });
    const uint64_t w_max = std::min(window, n);
    std::vector<uint64_t> sk(w_max * m), cnt(w_max), order(w_max), cluster(w_max), members;
    std::vector<uint32_t> ln(w_max), shared(w_max * w_max), uni(w_max * w_max);
    uint64_t multi = 0;
    float ms_sum = 0.f;
    for (uint64_t w0 = 0; w0 < n; w0 += window) {
        const uint64_t w = std::min(window, n - w0);
        for (uint64_t i = 0; i < w; ++i) {
            const uint64_t u = P[w0 + i];
            memcpy(sk.data() + i * m, sketch + u * m, (size_t)m * sizeof(uint64_t));
            ln[i] = len[u];
            cnt[i] = counts[u];
        }
        float ms = 0.f;
        if (int rc = taxor_gpu_sketch_pairs(device, sk.data(), ln.data(), cnt.data(), w, m, shared.data(), uni.data(), &ms)) return rc;
        ms_sum += ms;
        if (int rc = taxor_cluster_order(shared.data(), uni.data(), w, jmin, order.data(), cluster.data())) return rc;
        members.assign(w, 0);
        for (uint64_t i = 0; i < w; ++i) {
            rank[P[w0 + order[i]]] = w0 + i;
            if (++members[cluster[i]] == 2) ++multi;
        }
    }
    if (n_multi) *n_multi = multi;
    if (pairs_ms) *pairs_ms = ms_sum;
    return TAXOR_OK;
}

} // extern "C"
