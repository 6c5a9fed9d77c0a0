// key_store_check.cpp -- the host side of a build beyond device memory (taxor_amd/csrc/key_store.h) under ASan + UBSan: waves appended
// to the store come back bin by bin, the parts of a split bin tile it exactly, waves respect the budget and cover every genome once,
// and the two refusals answer from numbers.  argv[1]: a file in /proc/meminfo's format.  Prints "ok <checks>" or the first failure.
#include "key_store.h"

#include <cinttypes>
#include <random>

#define CHECK(x)                                                        \
    do {                                                                \
        ++checks;                                                       \
        if (!(x)) { printf("FAILED line %d: %s\n", __LINE__, #x); return 1; } \
    } while (0)

int main(int argc, char **argv)
{
    using namespace taxor;
    uint64_t checks = 0;
    std::mt19937_64 rng(7);
    // ---- the store: waves of bins, some empty, the last one filling it to the last key
    {
        std::vector<std::vector<uint64_t>> bins;
        for (int b = 0; b < 300; ++b) {
            std::vector<uint64_t> v(b % 9 == 0 ? 0 : rng() % 2000);
            for (auto &x : v) x = rng();
            bins.push_back(v);
        }
        uint64_t total = 0;
        for (auto &v : bins) total += v.size();
        KeyStore st;
        CHECK(st.reserve(total));
        CHECK(st.size() == 0 && st.bins() == 0);
        for (size_t b0 = 0; b0 < bins.size();) {
            const size_t b1 = std::min(bins.size(), b0 + 1 + rng() % 40);
            std::vector<uint64_t> keys, off{1000};                     // (a wave's offsets need not start at 0)
            for (size_t b = b0; b < b1; ++b) {
                keys.insert(keys.end(), bins[b].begin(), bins[b].end());
                off.push_back(1000 + keys.size());
            }
            CHECK(st.append(keys.data(), off.data(), b1 - b0));
            b0 = b1;
        }
        CHECK(st.bins() == bins.size() && st.size() == total);
        for (size_t b = 0; b < bins.size(); ++b) {
            CHECK(st.bin_off()[b + 1] - st.bin_off()[b] == bins[b].size());
            CHECK(bins[b].empty() || memcmp(st.keys() + st.bin_off()[b], bins[b].data(), bins[b].size() * 8) == 0);
        }
        const uint64_t one = 1, off1[2] = {0, 1};
        CHECK(!st.append(&one, off1, 1));                              // full: refused, nothing written
        CHECK(st.size() == total && st.bins() == bins.size());
        const uint64_t off0[2] = {5, 5};
        CHECK(st.append(nullptr, off0, 1) && st.bins() == bins.size() + 1);
        KeyStore empty;
        CHECK(empty.reserve(0) && empty.size() == 0);
    }
    // ---- parts: they tile [first, first + m), in order, sizes within one of each other, for counts up to 2^32 and beyond
    for (uint64_t m : {0ull, 1ull, 2ull, 63ull, 64ull, 1000003ull, 0xFFFFFFFEull, 0xFFFFFFFFFFull, 0xFFFFFFFFFFFFFF00ull})
        for (uint64_t parts : {1ull, 2ull, 3ull, 64ull, 4096ull, 1048576ull}) {
            const uint64_t first = 0xFFull;
            uint64_t next = first, lo = ~0ull, hi = 0;
            for (uint64_t j = 0; j < parts; j += (parts > 4096 ? parts / 4096 : 1)) {
                uint64_t f = 0, c = 0;
                key_part_range(first, m, parts, j, &f, &c);
                if (parts <= 4096) { CHECK(f == next); next = f + c; }
                CHECK(f >= first && f + c <= first + m);
                lo = std::min(lo, c);
                hi = std::max(hi, c);
            }
            uint64_t f = 0, c = 0;
            key_part_range(first, m, parts, parts - 1, &f, &c);
            CHECK(f + c == first + m);
            CHECK(hi - lo <= 1);
        }
    // ---- waves
    for (int round = 0; round < 200; ++round) {
        std::vector<uint64_t> bound(1 + rng() % 100), first;
        for (auto &x : bound) x = 1 + rng() % 1000;
        const uint64_t budget = 1 + rng() % 3000;
        const int64_t big = cut_waves(bound, budget, first);
        uint64_t mx = 0;
        for (auto x : bound) mx = std::max(mx, x);
        if (mx > budget) {
            CHECK(big >= 0 && bound[big] > budget);
            for (int64_t g = 0; g < big; ++g) CHECK(bound[g] <= budget);
            continue;
        }
        CHECK(big == -1 && first.front() == 0 && first.back() == bound.size());
        for (size_t w = 0; w + 1 < first.size(); ++w) {
            CHECK(first[w] < first[w + 1]);
            uint64_t sum = 0;
            for (uint64_t g = first[w]; g < first[w + 1]; ++g) sum += bound[g];
            CHECK(sum <= budget);
            CHECK(w + 2 == first.size() || sum + bound[first[w + 1]] > budget);      // a wave ends only where the next genome does not fit
        }
    }
    {
        std::vector<uint64_t> none, first;
        CHECK(cut_waves(none, 10, first) == -1 && first.size() == 2 && first[1] == 0);
    }
    // ---- bounds and refusals
    CHECK(key_bound_of_file(1000, false, true, 22, 12, 5) == 201 && key_bound_of_file(1000, true, true, 22, 12, 5) == 801);
    CHECK(key_bound_of_file(1000, false, false, 20, 0, 5) == 1001 && key_bound_of_file(0, false, true, 2, 1, 1) == 1);
    CHECK(host_store_refusal(1 << 20, 8ull << 20).empty() && host_store_refusal(0, 1).empty());
    const std::string no = host_store_refusal((1 << 20) + 1, 8ull << 20);
    CHECK(no.find("8 MiB of host memory, 8 MiB are available") != std::string::npos);
    CHECK(!host_store_refusal(~0ull, ~0ull).empty());                  // 2^67 bytes: no overflow into "fits"
    CHECK(host_memory_available("/nonexistent/meminfo") == 0);
    if (argc > 1) CHECK(host_memory_available(argv[1]) == (123456ull << 10));
    printf("ok %" PRIu64 "\n", checks);
    return 0;
}
