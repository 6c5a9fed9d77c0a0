// host_util.cpp -- host-side scalars of the path and the tools the tests / bench need around it
// (threshold ratio, classification filter, XOR-filter bin construction, synthetic reads).
#include "../../include/taxor_gpu_tools.h"
#include "ixf_arith.h"
#include "saved_batch.h"
#include "hll.h"
#include "lineage.h"

#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <queue>
#include <set>
#include <thread>
#include <vector>

namespace {

// src/hixf/search/syncmer_model.hpp:14-36 -- minimal matching ratios; rows = read accuracy 80..100 %,
// columns = k 12,14,...,30.  (Data of the reference's empirical model; needed for identical thresholds.)
const double kMatchingRatios[21][10] = {
    {0.552077, 0.195989, 0.151428, 0.118475, 0.0946177, 0.0797244, 0.0604658, 0.0480255, 0.0367569, 0.0252911},
    {0.552385, 0.207533, 0.161204, 0.127368, 0.103704, 0.0881939, 0.0689396, 0.0556991, 0.044185, 0.0298818},
    {0.552239, 0.220393, 0.17382, 0.139866, 0.113736, 0.0966358, 0.0783558, 0.0639223, 0.0523452, 0.0389549},
    {0.552682, 0.236329, 0.188152, 0.152267, 0.126191, 0.106106, 0.0876917, 0.0730642, 0.0621864, 0.0489249},
    {0.553172, 0.254091, 0.202686, 0.165344, 0.137087, 0.116649, 0.098822, 0.0831266, 0.0703342, 0.0582562},
    {0.553716, 0.271183, 0.219848, 0.181959, 0.152163, 0.130048, 0.110622, 0.0942414, 0.0810792, 0.0688187},
    {0.554532, 0.292154, 0.240059, 0.199738, 0.168952, 0.144956, 0.122726, 0.105878, 0.0940805, 0.0777557},
    {0.557957, 0.313553, 0.260912, 0.220014, 0.186567, 0.16101, 0.137399, 0.119867, 0.10453, 0.0900014},
    {0.563925, 0.338316, 0.283689, 0.2401, 0.206963, 0.179541, 0.155347, 0.135128, 0.121575, 0.104741},
    {0.568519, 0.364594, 0.310373, 0.267578, 0.231083, 0.20088, 0.174376, 0.153111, 0.139339, 0.120042},
    {0.579726, 0.395595, 0.338947, 0.295287, 0.258713, 0.22876, 0.200759, 0.175309, 0.161306, 0.139616},
    {0.599258, 0.430241, 0.371291, 0.325596, 0.289651, 0.257329, 0.228011, 0.201799, 0.186956, 0.164794},
    {0.611572, 0.468953, 0.410482, 0.363923, 0.325828, 0.293046, 0.26167, 0.235216, 0.216716, 0.192162},
    {0.624341, 0.510411, 0.452122, 0.407016, 0.370022, 0.334601, 0.303413, 0.275232, 0.254563, 0.227871},
    {0.655724, 0.555245, 0.498564, 0.453201, 0.416285, 0.381883, 0.352291, 0.322556, 0.299739, 0.271481},
    {0.694872, 0.608367, 0.552085, 0.509395, 0.471692, 0.437803, 0.405938, 0.377117, 0.354352, 0.325132},
    {0.742071, 0.669034, 0.613738, 0.57366, 0.539215, 0.50832, 0.476855, 0.449152, 0.42683, 0.397277},
    {0.795543, 0.733694, 0.68341, 0.647737, 0.617382, 0.588448, 0.56083, 0.533714, 0.514757, 0.486399},
    {0.853121, 0.802585, 0.763169, 0.733734, 0.708902, 0.684331, 0.660171, 0.637633, 0.621567, 0.596993},
    {0.918163, 0.882314, 0.854479, 0.835831, 0.819643, 0.804269, 0.788526, 0.771895, 0.763059, 0.742114},
    {1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0}};

inline uint64_t splitmix64(uint64_t &x)
{
    uint64_t z = (x += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

} // namespace

extern "C" {

double taxor_threshold_ratio(uint32_t kmer_size, double error_rate, double percentage)
{
    if (percentage > 0.0 && percentage <= 1.0) return percentage;           // threshold.hpp:27-32,76-79
    // the asserts at syncmer_model.hpp:40-44 are compiled out of the reference's Release build and the
    // lookup would read out of bounds; reject instead
    if (kmer_size % 2 != 0 || kmer_size < 12 || kmer_size > 30) return -1.0;
    if (!(error_rate >= 0.0) || !(error_rate <= 0.2)) return -1.0;
    const size_t row = (size_t)std::ceil((1.0 - error_rate) * 100.0 - 80.0); // syncmer_model.hpp:47
    const size_t col = kmer_size - 10 - ((kmer_size - 10) / 2) - 1;          // :48
    if (row > 20 || col > 9) return -1.0;
    return kMatchingRatios[row][col];
}

int taxor_threshold_kind(int use_syncmer, uint32_t kmer_size, uint64_t window_size, double percentage)
{
    const uint64_t kmers_per_window = window_size - kmer_size + 1;          // threshold.hpp:26
    if (percentage > 0.0 && percentage <= 1.0) return TAXOR_THR_PERCENTAGE; // :28
    if (use_syncmer) return TAXOR_THR_SYNCMER;                              // :34
    // the `fracminhash` member is always false here (search_arguments.hpp:61-75), so the window decides
    return kmers_per_window == 1 ? TAXOR_THR_KMER : TAXOR_THR_FRACMINHASH;  // :39-47
}

namespace {

// static_cast<size_t>(double) as the reference's stock build performs it.  For very short reads the reference casts
// NaN (sqrt of a negative variance) or a negative bound to size_t, which is undefined in C++; its build sets no
// -march (src/CMakeLists.txt:17-29), so GCC emits the baseline x86-64 cvttsd2si sequence, whose results are spelled
// out here instead of being left to whatever this compiler and this CPU would do.
uint64_t to_size_like_reference(double x)
{
    constexpr double two63 = 9223372036854775808.0;
    constexpr uint64_t indefinite = 0x8000000000000000ull;
    if (std::isnan(x) || x <= -two63) return indefinite;
    if (x < two63) return (uint64_t)(int64_t)x;
    const double y = x - two63;
    return y >= two63 ? 0 : ((uint64_t)(int64_t)y ^ indefinite);
}

double normal_cdf_inverse(double p)                                         // gaussian_inverse.cpp:13-50
{
    auto approx = [](double t) {
        constexpr double c0 = 2.515517, c1 = 0.802853, c2 = 0.010328, d0 = 1.432788, d1 = 0.189269, d2 = 0.001308;
        return t - ((c2 * t + c1) * t + c0) / (((d2 * t + d1) * t + d0) * t + 1.0);
    };
    return p < 0.5 ? -approx(std::sqrt(-2.0 * std::log(p))) : approx(std::sqrt(-2.0 * std::log(1.0 - p)));
}

// moments of the number of mutated k-mers (Blanca et al.), kmer_model.cpp:26-46; the operand order is the
// reference's, because double arithmetic is not associative and the result is truncated to an integer threshold
struct NmutMoments {
    double q, expected, variance;
    NmutMoments(double r, double k, double n)
    {
        q = 1.0 - std::pow(1.0 - r, k);
        expected = n * q;
        variance = n * (1.0 - q) * (q * (2.0 * k + (2.0 / r) - 1.0) - 2.0 * k) + k * (k - 1.0) * std::pow((1.0 - q), 2.0) +
                   (2.0 * (1.0 - q) / (std::pow(r, 2.0))) * ((1.0 + (k - 1.0) * (1.0 - q)) * r - q);
    }
};

} // namespace

uint64_t taxor_threshold_model(int kind, uint64_t count, uint32_t kmer_size, double error_rate, double percentage,
                               double scaling_factor)
{
    const uint64_t fp_correction = (uint64_t)((double)count * 0.0039);      // threshold.hpp:53
    const double n = (double)count, k = (double)kmer_size;
    switch (kind) {
    case TAXOR_THR_SYNCMER: return (uint64_t)(n * taxor_threshold_ratio(kmer_size, error_rate, -1.0)); // :57-61
    case TAXOR_THR_KMER: {                                                  // :62-67, kmer_model.cpp:10-23
        const NmutMoments m(error_rate, k, n);
        const double z = normal_cdf_inverse(1.0 - (1 - 0.95) / 2.0);
        const uint64_t high = to_size_like_reference(std::ceil(n * m.q + z * std::sqrt(m.variance)));
        return count - high - fp_correction;                               // size_t arithmetic: may wrap
    }
    case TAXOR_THR_FRACMINHASH: {                                           // :68-75, fracminhash_model.cpp:8-33
        const NmutMoments m(error_rate, k, n);
        const double z = normal_cdf_inverse(1.0 - (1.0 - 0.95) / 2.0);
        const double term3 = m.variance / std::pow(n, 2);
        const double term2 = n * m.expected - (std::pow(m.expected, 2) + m.variance);
        const double denominator = scaling_factor * std::pow(n, 3) * std::pow(1.0 - std::pow(1.0 - scaling_factor, n), 2);
        const double term1 = (1.0 - scaling_factor) / denominator;
        const double c_low = std::pow((1.0 - error_rate), k) - z * std::sqrt(term1 * term2 + term3);
        return to_size_like_reference(c_low * n) - fp_correction;
    }
    default: return (uint64_t)(n * percentage);                             // :76-79
    }
}

int taxor_threshold_select(const taxor_hixf_view *view, double error_rate, double percentage, taxor_gpu_search_params *prm)
{
    if (!view || !prm) return TAXOR_E_ARG;
    prm->model = (uint32_t)taxor_threshold_kind(view->use_syncmer, view->kmer_size, view->window_size, percentage);
    prm->error_rate = error_rate;
    prm->ratio = 0.0;
    if (prm->model == TAXOR_THR_PERCENTAGE) prm->ratio = percentage;
    else if (prm->model == TAXOR_THR_SYNCMER) {
        prm->ratio = taxor_threshold_ratio(view->kmer_size, error_rate, -1.0);
        if (prm->ratio < 0.0) return TAXOR_E_ARG;
    } else if (!(error_rate > 0.0) || !(error_rate < 1.0)) return TAXOR_E_ARG; // the models divide by r and take log-free powers of 1-r
    return TAXOR_OK;
}

uint64_t taxor_threshold(uint64_t hash_count, double ratio)
{
    return (uint64_t)((double)hash_count * ratio); // threshold.hpp:60
}

void taxor_classify_filter(const uint32_t *count, uint64_t n, uint8_t *keep)
{
    uint64_t max_count = 0; // taxor_search.cpp:275-280
    for (uint64_t i = 0; i < n; ++i)
        if (count[i] > max_count) max_count = count[i];
    for (uint64_t i = 0; i < n; ++i) // :285
        keep[i] = !(static_cast<double>(count[i]) < static_cast<double>(max_count) * 0.8);
}

uint64_t taxor_ixf_seg_len(uint64_t max_bin_elements) { return taxor::ixf_seg_len(max_bin_elements); }

// the sketch of `taxor search --coverage-file` (hll.h): the slot function the device uses, and the estimator.  A precision outside
// [4, 16] has no sketch: slot 0 / rho 0, estimate NaN
void taxor_hll_slot(uint64_t hash, uint32_t precision, uint32_t *index, uint8_t *rho)
{
    taxor::hll_slot_t s{0, 0};
    if (precision >= taxor::HLL_MIN_PRECISION && precision <= taxor::HLL_MAX_PRECISION) s = taxor::hll_slot(hash, precision);
    if (index) *index = s.index;
    if (rho) *rho = (uint8_t)s.rho;
}

double taxor_hll_estimate(const uint8_t *registers, uint32_t precision)
{
    if (!registers || precision < taxor::HLL_MIN_PRECISION || precision > taxor::HLL_MAX_PRECISION) return std::nan("");
    return taxor::hll_estimate(registers, precision);
}

// XOR-filter construction for one bin: peel the 3-uniform hypergraph, assign fingerprints in reverse// (the algorithm family of src/main/xorfilter.hpp:142-334; queue formulation).  The dense per-row scratch is
// kept per thread and only the touched rows are cleared, so sparse bins of a very tall IXF cost O(n).
int taxor_ixf_build_bin(const uint64_t *keys, uint64_t n, uint64_t seed, uint64_t seg_len, uint8_t *column)
{
    return taxor_ixf_build_bin_arith(keys, n, seed, seg_len, 0, column);
}

int taxor_ixf_build_bin_arith(const uint64_t *keys, uint64_t n, uint64_t seed, uint64_t seg_len, uint32_t arith, uint8_t *column)
{
    const uint64_t rows = 3 * seg_len;
    std::memset(column, 0, rows);
    if (n == 0) return 0;
    if (seg_len == 0 || seg_len > 0x55555555ull) return 1;
    static thread_local std::vector<uint32_t> cnt;
    static thread_local std::vector<uint64_t> xr;
    if (cnt.size() < rows) {
        cnt.assign(rows, 0);
        xr.assign(rows, 0);
    }
    std::vector<uint32_t> touched;
    touched.reserve(3 * n);
    for (uint64_t i = 0; i < n; ++i) {
        const taxor::ixf_probe p = taxor::ixf_probe_key_arith(keys[i], seed, (uint32_t)seg_len, arith);
        for (int j = 0; j < 3; ++j) {
            if (cnt[p.row[j]]++ == 0) touched.push_back(p.row[j]);
            xr[p.row[j]] ^= keys[i];
        }
    }
    std::vector<uint32_t> queue;
    queue.reserve(touched.size());
    for (uint32_t r : touched)
        if (cnt[r] == 1) queue.push_back(r);
    std::vector<uint64_t> st_key;
    std::vector<uint32_t> st_row;
    st_key.reserve(n);
    st_row.reserve(n);
    while (!queue.empty()) {
        const uint32_t r = queue.back();
        queue.pop_back();
        if (cnt[r] != 1) continue;
        const uint64_t key = xr[r];
        st_key.push_back(key);
        st_row.push_back(r);
        const taxor::ixf_probe p = taxor::ixf_probe_key_arith(key, seed, (uint32_t)seg_len, arith);
        for (int j = 0; j < 3; ++j) {
            const uint32_t rr = p.row[j];
            cnt[rr]--;
            xr[rr] ^= key;
            if (cnt[rr] == 1) queue.push_back(rr);
        }
    }
    for (uint32_t r : touched) { // leave the scratch clean for the next call
        cnt[r] = 0;
        xr[r] = 0;
    }
    if (st_key.size() != n) return 1; // not peelable under this seed (or duplicate keys)
    for (size_t i = st_key.size(); i-- > 0;) {
        const taxor::ixf_probe p = taxor::ixf_probe_key_arith(st_key[i], seed, (uint32_t)seg_len, arith);
        uint8_t v = (uint8_t)(p.fp4 & 0xFFu);
        for (int j = 0; j < 3; ++j)
            if (p.row[j] != st_row[i]) v ^= column[p.row[j]];
        column[st_row[i]] = v;
    }
    return 0;
}

int taxor_synth_reads(const char *genomes, const uint64_t *genome_off, uint64_t n_genomes, uint64_t n_reads,
                      uint32_t read_len, double error_rate, double frac_random, double frac_reverse,
                      uint64_t seed, int threads, char *bases, uint64_t cap, uint64_t *offsets, int32_t *origin)
{
    if ((uint64_t)read_len * n_reads > cap) return TAXOR_E_ARG;
    if (threads < 1) threads = 1;
    static const char ACGT[4] = {'A', 'C', 'G', 'T'};
    auto comp = [](char c) { return c == 'A' ? 'T' : c == 'C' ? 'G' : c == 'G' ? 'C' : 'A'; };
    auto work = [&](uint64_t lo, uint64_t hi) {
        for (uint64_t i = lo; i < hi; ++i) {
            // every read gets its own stream: the state is a hash of (seed, i).  (splitmix64 advances its state by a
            // constant, so seeding read i with seed + i * that constant made read i replay read 0's stream i draws
            // later -- error positions were then correlated across reads and the error rate varied along the read.)
            uint64_t s0 = seed ^ (i * 0xD1342543DE82EF95ull + 0x2545F4914F6CDD1Dull);
            uint64_t st = splitmix64(s0) ^ (splitmix64(s0) << 1);
            char *out = bases + i * read_len;
            offsets[i] = i * read_len;
            const double u0 = (double)(splitmix64(st) >> 11) * (1.0 / 9007199254740992.0);
            if (n_genomes == 0 || u0 < frac_random) {
                if (origin) origin[i] = -1;
                for (uint32_t j = 0; j < read_len; ++j) out[j] = ACGT[splitmix64(st) & 3];
                continue;
            }
            const uint64_t g = splitmix64(st) % n_genomes;
            if (origin) origin[i] = (int32_t)g;
            const char *G = genomes + genome_off[g];
            const uint64_t glen = genome_off[g + 1] - genome_off[g];
            const uint64_t span = glen > read_len ? glen - read_len : 0;
            const uint64_t start = span ? splitmix64(st) % span : 0;
            const bool rev = (double)(splitmix64(st) >> 11) * (1.0 / 9007199254740992.0) < frac_reverse;
            uint64_t src = 0; // offset within the sampled stretch
            uint32_t j = 0;
            while (j < read_len) {
                char c;
                if (!rev) {
                    const uint64_t pos = start + src;
                    c = pos < glen ? G[pos] : ACGT[splitmix64(st) & 3];
                } else { // walk the stretch [start, start+read_len) backwards, complemented
                    const int64_t pos = (int64_t)start + (int64_t)read_len - 1 - (int64_t)src;
                    c = (pos >= 0 && (uint64_t)pos < glen) ? comp(G[pos]) : ACGT[splitmix64(st) & 3];
                }
                ++src;
                const double x = (double)(splitmix64(st) >> 11) * (1.0 / 9007199254740992.0);
                if (x < error_rate * 0.4) out[j++] = ACGT[splitmix64(st) & 3];          // substitution
                else if (x < error_rate * 0.7) {                                           // insertion
                    out[j++] = c;
                    if (j < read_len) out[j++] = ACGT[splitmix64(st) & 3];
                } else if (x < error_rate) continue;                                       // deletion
                else out[j++] = c;
            }
        }
    };
    std::vector<std::thread> pool;
    const uint64_t per = (n_reads + (uint64_t)threads - 1) / (uint64_t)threads;
    for (int t = 0; t < threads; ++t) {
        const uint64_t lo = per * (uint64_t)t, hi = lo + per > n_reads ? n_reads : lo + per;
        if (lo < hi) pool.emplace_back(work, lo, hi);
    }
    for (auto &th : pool) th.join();
    offsets[n_reads] = n_reads * (uint64_t)read_len;
    return 0;
}

} // extern "C"

// ---- the IXF tree of `taxor build` (DESIGN.md "taxor build: the layout").  The reference asks chopper (HyperLogLog counts,
// hierarchical binning; taxor_build.cpp:428-492), which is not vendored; this is a simpler rule over EXACT counts:
//   n <= t_max user bins: one IXF of leaves.  It gets min(t_max, next multiple of 64 of n) bins -- bins up to the row's 64-byte
//     multiple cost a query nothing -- and a user bin larger than twice the mean is split (largest per part first) while bins are
//     left, so the IXF's seg_len, which follows its largest bin, shrinks.
//   n > t_max: user bins of at least total / t_max keys stay leaves (split into floor(count / (total / t_max)) parts), the rest,
//     in descending count order, are cut into the remaining bins as contiguous groups of about equal weight; a group of one is a
//     leaf, a larger group a merged bin whose child IXF is laid out the same way.
//   with a rank (taxor_build_layout_ranked, `taxor build --group-similar`): the rest is ordered by rank instead of by count before it
//     is cut, in every IXF of the tree; which bins stay leaves does not change.
// Deterministic: ties break on the user bin's index.
namespace {

struct LayIxf {
    std::vector<int64_t> next, fname;
    std::vector<uint64_t> part, parts;
    std::vector<uint64_t> weight;   // keys of each bin (merged: sum of the children's)
};

struct LayBuild {
    const uint64_t *cnt;
    const uint64_t *rank = nullptr;   // --group-similar: the order of the bins that are cut into groups (null: their count order)
    uint64_t T;
    std::vector<LayIxf> ixfs;
    std::vector<uint32_t> level;

    static uint64_t r64(uint64_t x) { return (x + 63) / 64 * 64; }

    // leaves (user bin, parts) and the greedy split of the largest per-part bins into `budget` bins, down to `thr`
    void split(std::vector<std::pair<uint32_t, uint64_t>> &lv, uint64_t budget, double thr)
    {
        uint64_t used = 0;
        for (auto &x : lv) used += x.second;
        auto per = [&](size_t i) { return (double)cnt[lv[i].first] / (double)lv[i].second; };
        auto less = [&](size_t a, size_t b) { return per(a) < per(b) || (per(a) == per(b) && lv[a].first > lv[b].first); };
        std::priority_queue<size_t, std::vector<size_t>, decltype(less)> pq(less);
        for (size_t i = 0; i < lv.size(); ++i) pq.push(i);
        while (used < budget && !pq.empty()) {
            const size_t i = pq.top();
            if (per(i) <= thr || lv[i].second + 1 > cnt[lv[i].first]) break;
            pq.pop();
            ++lv[i].second;
            ++used;
            pq.push(i);
        }
    }

    uint32_t make(std::vector<uint32_t> S, uint32_t lvl)
    {
        std::sort(S.begin(), S.end(), [&](uint32_t a, uint32_t b) { return cnt[a] > cnt[b] || (cnt[a] == cnt[b] && a < b); });
        const uint32_t id = (uint32_t)ixfs.size();
        ixfs.emplace_back();
        level.push_back(lvl);
        const uint64_t n = S.size();
        double total = 0;
        for (uint32_t u : S) total += (double)cnt[u];
        std::vector<std::pair<uint32_t, uint64_t>> lv;
        std::vector<std::vector<uint32_t>> groups;
        if (n <= T) {
            for (uint32_t u : S) lv.push_back({u, 1});
            split(lv, std::min(T, r64(n)), 2.0 * total / (double)n);
        } else {
            const double target = total / (double)T;
            uint64_t d = 0, sum_p = 0;
            while (d < n && (double)cnt[S[d]] >= target && target > 0) {
                const uint64_t p = std::max<uint64_t>(1, std::min<uint64_t>(cnt[S[d]], (uint64_t)((double)cnt[S[d]] / target)));
                lv.push_back({S[d], p});
                sum_p += p;
                ++d;
            }
            while (sum_p + 1 > T) {                       // keep at least one bin for the rest
                auto it = std::max_element(lv.begin(), lv.end(), [](const auto &a, const auto &b) { return a.second < b.second; });
                if (it->second > 1) { --it->second; --sum_p; }
                else { sum_p -= lv.back().second; lv.pop_back(); --d; }
            }
            const uint64_t M = T - sum_p;                  // bins for the S[d..n) (n - d > M: there are more of them than bins)
            if (rank)                                      // similar bins stand together; ties keep the count order
                std::stable_sort(S.begin() + (ptrdiff_t)d, S.end(), [&](uint32_t a, uint32_t b) { return rank[a] < rank[b]; });
            double rest = 0;
            for (uint64_t i = d; i < n; ++i) rest += (double)cnt[S[i]];
            uint64_t i = d;
            for (uint64_t g = 0; g < M; ++g) {
                const uint64_t left_groups = M - g;
                const double want = rest / (double)left_groups;
                std::vector<uint32_t> grp;
                double wsum = 0;
                // at least one member; more while the group is light and every later group still gets one
                while (i < n && (grp.empty() || g + 1 == M || (wsum < want && n - i > left_groups - 1))) {
                    grp.push_back(S[i]);
                    wsum += (double)cnt[S[i]];
                    ++i;
                }
                rest -= wsum;
                if (grp.size() == 1) lv.push_back({grp[0], 1});
                else groups.push_back(std::move(grp));
            }
        }
        for (const auto &x : lv)
            for (uint64_t j = 0; j < x.second; ++j) {
                LayIxf &f = ixfs[id];
                f.next.push_back(id);
                f.fname.push_back(x.first);
                f.part.push_back(j);
                f.parts.push_back(x.second);
                f.weight.push_back(cnt[x.first] * (j + 1) / x.second - cnt[x.first] * j / x.second);
            }
        for (const auto &grp : groups) {
            const size_t b = ixfs[id].next.size();
            uint64_t w = 0;
            for (uint32_t u : grp) w += cnt[u];
            ixfs[id].next.push_back(-1);
            ixfs[id].fname.push_back(-1);
            ixfs[id].part.push_back(0);
            ixfs[id].parts.push_back(0);
            ixfs[id].weight.push_back(w);
            const uint32_t child = make(grp, lvl + 1);
            ixfs[id].next[b] = child;
        }
        return id;
    }
};

struct LayoutOwned {
    taxor_layout pub{};
    std::vector<uint64_t> ixf_bins, bin_first, part, parts;
    std::vector<int64_t> next, fname;
};

LayoutOwned *layout_for(const uint64_t *counts, uint64_t n, uint64_t T, const uint64_t *rank)
{
    LayBuild lb;
    lb.cnt = counts;
    lb.rank = rank;
    lb.T = T;
    std::vector<uint32_t> all(n);
    for (uint64_t i = 0; i < n; ++i) all[i] = (uint32_t)i;
    lb.make(all, 0);
    auto *L = new LayoutOwned();
    const uint64_t m = lb.ixfs.size();
    L->bin_first.push_back(0);
    std::vector<double> stride3(m);
    double idx_bytes = 0, total = 0;
    uint32_t depth = 0;
    for (uint64_t i = 0; i < m; ++i) {
        const LayIxf &f = lb.ixfs[i];
        L->ixf_bins.push_back(f.next.size());
        L->bin_first.push_back(L->bin_first.back() + f.next.size());
        L->next.insert(L->next.end(), f.next.begin(), f.next.end());
        L->fname.insert(L->fname.end(), f.fname.begin(), f.fname.end());
        L->part.insert(L->part.end(), f.part.begin(), f.part.end());
        L->parts.insert(L->parts.end(), f.parts.begin(), f.parts.end());
        stride3[i] = 3.0 * (double)LayBuild::r64(f.next.size());
        const uint64_t mx = f.weight.empty() ? 1 : std::max<uint64_t>(1, *std::max_element(f.weight.begin(), f.weight.end()));
        idx_bytes += (double)taxor_ixf_seg_len(mx) * stride3[i];
        depth = std::max(depth, lb.level[i] + 1);
    }
    // expected bytes per query hash: a key of user bin u is looked up in every IXF on u's path (weight: u's keys)
    std::vector<double> path(m, 0.0);
    std::vector<int64_t> parent(m, -1);
    for (uint64_t i = 0; i < m; ++i)
        for (const int64_t c : lb.ixfs[i].next)
            if (c >= 0 && (uint64_t)c != i) parent[c] = (int64_t)i;
    for (uint64_t i = 0; i < m; ++i) path[i] = stride3[i] + (parent[i] >= 0 ? path[parent[i]] : 0.0);   // parents come first
    double cost = 0;
    for (uint64_t i = 0; i < m; ++i) {
        const LayIxf &f = lb.ixfs[i];
        for (size_t b = 0; b < f.fname.size(); ++b)
            if (f.fname[b] >= 0 && f.part[b] == 0) {
                cost += (double)counts[f.fname[b]] * path[i];
                total += (double)counts[f.fname[b]];
            }
    }
    L->pub.n_ixf = m;
    L->pub.n_bins_total = L->next.size();
    L->pub.t_max = T;
    L->pub.depth = depth;
    L->pub.bytes_per_hash = total > 0 ? cost / total : 0.0;
    L->pub.index_bytes = idx_bytes;
    L->pub.ixf_bins = L->ixf_bins.data();
    L->pub.bin_first = L->bin_first.data();
    L->pub.next_ixf = L->next.data();
    L->pub.fname_idx = L->fname.data();
    L->pub.part = L->part.data();
    L->pub.parts = L->parts.data();
    return L;
}

} // namespace

extern "C" {

int taxor_build_layout(const uint64_t *counts, uint64_t n, uint64_t t_max, taxor_layout **out)
{
    return taxor_build_layout_ranked(counts, n, t_max, nullptr, out);
}

int taxor_build_layout_ranked(const uint64_t *counts, uint64_t n, uint64_t t_max, const uint64_t *rank, taxor_layout **out)
{
    if (!out) return TAXOR_E_ARG;
    *out = nullptr;
    if (!counts || n == 0 || n >= (1ull << 31) || (t_max && t_max < 2)) return TAXOR_E_ARG;
    std::set<uint64_t> cand;
    if (t_max) cand.insert(t_max);
    else {
        for (uint64_t t = 64; t <= 4096; t *= 2) cand.insert(t);                    // taxor_build.cpp:177-178
        cand.insert(std::max<uint64_t>(64, (uint64_t)std::ceil(std::sqrt((double)n) / 64.0) * 64));   // :182-184
    }
    LayoutOwned *best = nullptr;
    for (const uint64_t T : cand) {                                              // ascending: ties keep the smaller t_max
        LayoutOwned *L = layout_for(counts, n, T, rank);
        if (!best || L->pub.bytes_per_hash < best->pub.bytes_per_hash ||
            (L->pub.bytes_per_hash == best->pub.bytes_per_hash && L->pub.index_bytes < best->pub.index_bytes)) {
            delete best;
            best = L;
        } else
            delete L;
    }
    *out = &best->pub;
    return TAXOR_OK;
}

void taxor_layout_free(taxor_layout *l)
{
    delete reinterpret_cast<LayoutOwned *>(l);   // pub is the first member
}

// ---- the similarity order of `taxor build --group-similar` ("Similarity-aware layout")
int taxor_cluster_order(const uint32_t *shared, const uint32_t *uni, uint64_t n, double jmin, uint64_t *order, uint64_t *cluster)
{
    if (!shared || !uni || !order || n == 0 || n >= (1ull << 31) || !(jmin > 0.0)) return TAXOR_E_ARG;
    std::vector<uint32_t> up(n);                          // union-find; a root is the smallest member of its set
    for (uint64_t i = 0; i < n; ++i) up[i] = (uint32_t)i;
    auto find = [&](uint32_t x) {
        while (up[x] != x) x = up[x] = up[up[x]];
        return x;
    };
    for (uint64_t i = 0; i < n; ++i)
        for (uint64_t j = i + 1; j < n; ++j) {
            const uint32_t s = shared[i * n + j], u = uni[i * n + j];
            if (u > 0 && (double)s >= jmin * (double)u) {
                const uint32_t a = find((uint32_t)i), b = find((uint32_t)j);
                if (a != b) up[std::max(a, b)] = std::min(a, b);
            }
        }
    // clusters in the order of their smallest member = of their roots; members ascending
    std::vector<uint64_t> ordinal(n, 0), size(n, 0), at(n, 0);
    uint64_t nc = 0;
    for (uint64_t i = 0; i < n; ++i) {
        const uint32_t r = find((uint32_t)i);
        if (r == i) ordinal[i] = nc++;
        ++size[ordinal[r]];                               // (a root comes before every other member)
    }
    uint64_t run = 0;
    for (uint64_t c = 0; c < nc; ++c) {
        at[c] = run;
        run += size[c];
    }
    for (uint64_t i = 0; i < n; ++i) {
        const uint64_t c = ordinal[find((uint32_t)i)];
        order[at[c]++] = i;
        if (cluster) cluster[i] = c;
    }
    return TAXOR_OK;
}

// ---- taxor_index_plan_passes: which IXFs a search of an index larger than the device holds together (DESIGN.md section 9,
// "Search beyond device memory").  Host only.
extern "C" __attribute__((visibility("hidden"))) void taxor_set_last_error(const char *msg);

namespace {

__attribute__((format(printf, 2, 3))) int plan_fail(int code, const char *fmt, ...)
{
    char buf[768];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    taxor_set_last_error(buf);
    return code;
}

inline uint64_t slab_round(uint64_t x) { return (x + 4095) / 4096 * 4096; }

} // namespace

int taxor_index_plan_passes(const taxor_hixf_view *v, uint64_t budget_bytes, taxor_pass_plan *plan, uint32_t *pass_of_ixf, uint64_t *pass_bytes)
{
    if (!v || !plan || v->n_ixf == 0 || !v->ixf || v->n_ixf >= (1u << 30)) return plan_fail(TAXOR_E_ARG, "plan_passes: empty view");
    const uint64_t n = v->n_ixf;
    std::vector<uint64_t> bytes(n);
    for (uint64_t i = 0; i < n; ++i) {
        const taxor_ixf_view &f = v->ixf[i];
        if (f.bins == 0 || f.stride < f.bins || f.stride % 64 != 0 || f.seg_len == 0 || !f.next_ixf || !f.fname_idx || 3 * f.seg_len >= (1ull << 32) ||
            f.stride > (1u << 20))
            return plan_fail(TAXOR_E_ARG, "plan_passes: IXF %llu malformed (bins=%llu stride=%llu seg_len=%llu)", (unsigned long long)i,
                             (unsigned long long)f.bins, (unsigned long long)f.stride, (unsigned long long)f.seg_len);
        bytes[i] = slab_round(3 * f.seg_len * f.stride);
    }
    // the subtrees: one per merged bin of the root, in root-bin order, each with everything below it
    struct Subtree { uint64_t root_bin, child, bytes; };
    std::vector<Subtree> sub;
    std::vector<uint32_t> owner(n, TAXOR_PASS_ROOT);      // subtree index first, pass number at the end
    std::vector<uint8_t> seen(n, 0);
    seen[0] = 1;
    struct Edge { uint64_t parent, bin; int64_t child; };
    std::vector<Edge> stack;
    for (uint64_t b = 0; b < v->ixf[0].bins; ++b) {
        if (v->ixf[0].fname_idx[b] >= 0) continue;
        Subtree st{b, (uint64_t)v->ixf[0].next_ixf[b], 0};
        stack.assign(1, Edge{0, b, v->ixf[0].next_ixf[b]});
        while (!stack.empty()) {
            const Edge e = stack.back();
            stack.pop_back();
            if (e.child <= 0 || (uint64_t)e.child >= n)
                return plan_fail(TAXOR_E_ARG, "plan_passes: IXF %llu bin %llu: bad child %lld", (unsigned long long)e.parent, (unsigned long long)e.bin, (long long)e.child);
            const uint64_t c = (uint64_t)e.child;
            if (seen[c]) return plan_fail(TAXOR_E_ARG, "plan_passes: IXF %llu is referenced twice (not a tree)", (unsigned long long)c);
            seen[c] = 1;
            owner[c] = (uint32_t)sub.size();
            st.bytes += bytes[c];
            const taxor_ixf_view &f = v->ixf[c];
            for (uint64_t x = 0; x < f.bins; ++x)
                if (f.fname_idx[x] < 0) stack.push_back(Edge{c, x, f.next_ixf[x]});
        }
        sub.push_back(st);
    }
    const uint64_t root_bytes = bytes[0] + 4096;       // the slab's tail pad is the root's: it is resident in every pass
    uint64_t total = 0;
    for (const Subtree &s : sub) total += s.bytes;
    std::vector<uint64_t> gbytes;
    std::vector<uint32_t> gof(sub.size(), 0);
    if (root_bytes > budget_bytes)
        return plan_fail(TAXOR_E_ARG, "search: the root IXF alone needs %llu bytes on the device, the index budget is %llu (root-exceeds-budget): it stays resident in every pass, "
                                      "so this index cannot be searched under this budget", (unsigned long long)root_bytes, (unsigned long long)budget_bytes);
    const uint64_t avail = budget_bytes - root_bytes;
    if (sub.empty() || total <= avail) gbytes.push_back(total);
    else {
        // greedy in root-bin order.  Two groups are on the device at a time -- one searched, the next one uploading -- so every pair of
        // neighbours has to fit beside the root; a group is closed when the next subtree would take it past half of what the root
        // leaves (a subtree larger than that is a group of its own) or past what the group before it leaves
        const uint64_t half = avail / 2;
        uint64_t cur = 0, prev = 0;
        bool open = false;
        for (size_t j = 0; j < sub.size(); ++j) {
            const Subtree &s = sub[j];
            if (s.bytes > avail)
                return plan_fail(TAXOR_E_ARG, "search: the subtree under root bin %llu (child IXF %llu) needs %llu bytes, the root leaves %llu of the index budget of %llu "
                                              "(subtree-exceeds-budget); a smaller --tmax at build time gives smaller subtrees",
                                 (unsigned long long)s.root_bin, (unsigned long long)s.child, (unsigned long long)s.bytes, (unsigned long long)avail, (unsigned long long)budget_bytes);
            if (open && (cur + s.bytes > half || prev + cur + s.bytes > avail)) {
                gbytes.push_back(cur);
                prev = cur;
                cur = 0;
                open = false;
            }
            if (prev + cur + s.bytes > avail)
                return plan_fail(TAXOR_E_ARG, "search: the subtree under root bin %llu (child IXF %llu) needs %llu bytes, the root and the group before it (%llu bytes, on the device "
                                              "while this one uploads) leave %llu of the index budget of %llu (subtree-exceeds-budget; this is the greedy packing's refusal, not proof that no grouping "
                                              "exists: a somewhat larger budget is searched); a smaller --tmax at build time gives smaller subtrees",
                                 (unsigned long long)s.root_bin, (unsigned long long)s.child, (unsigned long long)s.bytes, (unsigned long long)prev,
                                 (unsigned long long)(avail - prev), (unsigned long long)budget_bytes);
            cur += s.bytes;
            open = true;
            gof[j] = (uint32_t)gbytes.size();
        }
        gbytes.push_back(cur);
    }
    uint64_t pair = 0;
    for (size_t g = 0; g < gbytes.size(); ++g) pair = std::max(pair, gbytes[g] + (g + 1 < gbytes.size() ? gbytes[g + 1] : 0));
    plan->n_passes = (uint32_t)gbytes.size();
    plan->n_subtrees = (uint32_t)sub.size();
    plan->root_bytes = root_bytes;
    plan->slab_bytes = root_bytes + pair;
    plan->index_bytes = root_bytes + total;
    if (pass_of_ixf)
        for (uint64_t i = 0; i < n; ++i) pass_of_ixf[i] = owner[i] == TAXOR_PASS_ROOT ? TAXOR_PASS_ROOT : gof[owner[i]];   // (an IXF no bin leads to: never searched, never uploaded)
    if (pass_bytes)
        for (size_t g = 0; g < gbytes.size(); ++g) pass_bytes[g] = gbytes[g];
    return TAXOR_OK;
}

// ---- the saved hash lists' store of a paged search (saved_batch.h): its bound and the decision made from it, for `taxor search`
uint64_t taxor_saved_bytes_bound(uint64_t bases, int use_syncmer, uint32_t kmer_size, uint32_t syncmer_size, uint32_t t_syncmer)
{
    return taxor::saved_bytes_bound(bases, use_syncmer != 0, (int)kmer_size, (int)syncmer_size, (int)t_syncmer);
}

int taxor_saved_store_fits(uint64_t bound_bytes, uint64_t available_bytes) { return taxor::saved_store_fits(bound_bytes, available_bytes) ? 1 : 0; }

} // extern "C"

// ---- the lineage table of `taxor search --lca-file / --report-file` (lineage.h).  Host only.
struct taxor_lineage {
    taxor::Lineage l;
    std::vector<const char *> id_p, name_p;
};

extern "C" {

int taxor_lineage_create(const taxor_hixf_meta *meta, uint64_t n_user_bins, taxor_lineage **out)
{
    if (!out) return plan_fail(TAXOR_E_ARG, "lineage_create: null argument");
    *out = nullptr;
    if (!meta || (meta->n_species && !meta->species)) return plan_fail(TAXOR_E_ARG, "lineage_create: null argument");
    if (n_user_bins >= (1ull << 31)) return plan_fail(TAXOR_E_ARG, "lineage_create: user bins are numbered in 31 bits");
    auto *t = new taxor_lineage;
    const std::string err = taxor::lineage_build(*meta, n_user_bins, t->l);
    if (!err.empty()) {
        delete t;
        return plan_fail(TAXOR_E_ARG, "%s", err.c_str());
    }
    for (const auto &s : t->l.id) t->id_p.push_back(s.c_str());
    for (const auto &s : t->l.name) t->name_p.push_back(s.c_str());
    *out = t;
    return TAXOR_OK;
}

int taxor_lineage_get_view(const taxor_lineage *t, taxor_lineage_view *v)
{
    if (!t || !v) return plan_fail(TAXOR_E_ARG, "lineage_get_view: null argument");
    v->n_user_bins = t->l.n_bins;
    v->n_nodes = t->l.id.size();
    v->max_depth = t->l.max_depth;
    v->reserved = 0;
    v->bin_species = t->l.bin_species.data();
    v->path_off = t->l.path_off.data();
    v->path = t->l.path.data();
    v->parent = t->l.parent.data();
    v->depth = t->l.depth.data();
    v->id = t->id_p.data();
    v->name = t->name_p.data();
    v->rank = t->l.rank.data();
    return TAXOR_OK;
}

void taxor_lineage_free(taxor_lineage *t) { delete t; }

} // extern "C"
