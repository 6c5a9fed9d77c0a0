// hitmap_check.cpp -- the host side of `taxor search --hitmap-file` (taxor_amd/csrc/hitmap_format.h) under ASan + UBSan: the segment of a
// hash and the size of a segment over every S in [1, 64] and read sizes at and around the segment count, the piece length and 2^31 - 1
// (where i * S must not leave 64 bits), and the line formatter with null names, no hashes, one segment and sixty-four.  Prints
// "ok <checks>" or the first failure.
#include "hitmap_format.h"

#include <cstdio>
#include <vector>

#define CHECK(x)                                                        \
    do {                                                                \
        ++checks;                                                       \
        if (!(x)) { printf("FAILED line %d: %s\n", __LINE__, #x); return 1; } \
    } while (0)

int main()
{
    using namespace taxor;
    uint64_t checks = 0;
    const uint64_t sizes[] = {1, 2, 3, 15, 16, 17, 63, 64, 65, 127, 2047, 2048, 2049, 5245};
    for (uint32_t S = 1; S <= HITMAP_MAX_SEGMENTS; ++S)
        for (uint64_t n : sizes) {
            std::vector<uint64_t> cnt(S, 0);
            uint32_t last = 0;
            for (uint64_t i = 0; i < n; ++i) {
                const uint32_t s = hitmap_seg(i, S, n);
                if (s >= S || s < last) { printf("FAILED: seg(%llu, %u, %llu) = %u\n", (unsigned long long)i, S, (unsigned long long)n, s); return 1; }
                last = s;
                ++cnt[s];
            }
            uint64_t sum = 0;
            for (uint32_t j = 0; j < S; ++j) {
                CHECK(hitmap_seg_size(j, S, n) == cnt[j]);
                sum += cnt[j];
            }
            CHECK(sum == n);
            CHECK(hitmap_seg_first(0, S, n) == 0 && hitmap_seg_first(S, S, n) == n);
        }
    {   // the largest read the searcher takes: the products stay inside 64 bits, the last hash lies in the last segment
        const uint64_t n = (1ull << 31) - 1;
        for (uint32_t S : {1u, 2u, 16u, 63u, 64u}) {
            CHECK(hitmap_seg(n - 1, S, n) == S - 1 && hitmap_seg(0, S, n) == 0);
            uint64_t sum = 0;
            for (uint32_t j = 0; j < S; ++j) {
                const uint64_t f = hitmap_seg_first(j, S, n);
                CHECK(f == n || hitmap_seg(f, S, n) == j);
                CHECK(f == 0 || hitmap_seg(f - 1, S, n) < j);
                sum += hitmap_seg_size(j, S, n);
            }
            CHECK(sum == n);
        }
    }
    {   // the formatter
        std::string out;
        const uint32_t h4[4] = {1, 0, 2, 0};
        hitmap_line(out, "read 1", 6, "ACC", "562", 1200, 5, 4, h4, 4);
        CHECK(out == "read 1\tACC\t562\t1200\t5\t4\t3\t2,1,1,1\t1,0,2,0\n");
        out.clear();
        hitmap_line(out, "", 0, nullptr, nullptr, 0, 0, 0, h4, 1);
        CHECK(out == "\t-\t-\t0\t0\t0\t1\t0\t1\n");
        out.clear();
        std::vector<uint32_t> h64(64, 4294967295u);
        hitmap_line(out, "r", 1, "A", "1", 18446744073709551615ull, 4294967295u, 4294967295u, h64.data(), 64);
        CHECK(out.find("\t18446744073709551615\t4294967295\t4294967295\t274877906880\t") != std::string::npos);
        CHECK(out.back() == '\n');
        size_t commas = 0;
        for (char c : out) commas += c == ',';
        CHECK(commas == 2 * 63);
        CHECK(std::string(hitmap_header()).find("SEGMENT_HITS\n") != std::string::npos);
    }
    printf("ok %llu\n", (unsigned long long)checks);
    return 0;
}
