// breakpoint_check.cpp -- the host side of `taxor search --breakpoint-file` (taxor_amd/csrc/breakpoint_format.h) under ASan + UBSan: the
// approximate base position of a break over read sizes at and around the round and piece lengths and at the ends of 32 and 64 bits
// (against 128-bit arithmetic), and the line formatter with null names, an empty id and the largest numbers.  With arguments
// "p query_len n" ... it prints breakpoint_base of every triple, one per line, for the Python restatement to be compared with.
// Prints "ok <checks>" or the first failure.
#include "breakpoint_format.h"

#include <algorithm>
#include <cstdio>
#include <cstdlib>

#define CHECK(x)                                                        \
    do {                                                                \
        ++checks;                                                       \
        if (!(x)) { printf("FAILED line %d: %s\n", __LINE__, #x); return 1; } \
    } while (0)

int main(int argc, char **argv)
{
    using namespace taxor;
    if (argc > 1) {
        for (int i = 1; i + 2 < argc; i += 3)
            printf("%llu\n", (unsigned long long)breakpoint_base(strtoull(argv[i], nullptr, 10), strtoull(argv[i + 1], nullptr, 10), strtoull(argv[i + 2], nullptr, 10)));
        return 0;
    }
    uint64_t checks = 0;
    const uint64_t sizes[] = {1, 2, 3, 63, 64, 65, 127, 2047, 2048, 2049, 5245, (1ull << 31) - 1, (1ull << 32) - 1};
    const uint64_t lens[] = {0, 1, 21, 22, 1200, 10000, 1000003, (1ull << 31) - 1, 1ull << 32, (1ull << 40) + 7, ~0ull};
    for (uint64_t n : sizes)
        for (uint64_t len : lens) {
            uint64_t ps[] = {0, 1, n / 3, n / 2, n - 1};
            std::sort(ps, ps + 5);                      // the position ascends with p
            uint64_t last = 0;
            for (uint64_t p : ps) {
                if (p >= n) continue;
                const uint64_t got = breakpoint_base(p, len, n);
                CHECK(got == (uint64_t)((unsigned __int128)p * len / n));
                CHECK(got >= last && got <= len);
                last = got;
            }
        }
    CHECK(breakpoint_base(0, 1000, 0) == 0 && breakpoint_base(5, 1000, 0) == 0);      // a read without a hash has no break; no division by 0
    CHECK(breakpoint_base(1024, 12000, 2048) == 6000 && breakpoint_base(1, 10, 3) == 3 && breakpoint_base(2, 10, 3) == 6);
    {   // the formatter
        std::string out;
        breakpoint_line(out, "read 1", 6, 12000, 5245, 3, {"GCF_1", "562"}, 2700, 2622, {"GCF_1", "562"}, 2600, 12, {"GCF_3", "1280"}, 2590, 100, 2490);
        CHECK(out == "read 1\t12000\t5245\t3\tGCF_1\t562\t2700\t2622\t5998\tGCF_1\t562\t2600\t12\tGCF_3\t1280\t2590\t100\t2490\n");
        out.clear();
        breakpoint_line(out, "", 0, 18446744073709551615ull, 4294967295u, 4294967295u, {nullptr, nullptr}, 4294967295u, 4294967294u, {nullptr, "1"}, 4294967295u,
                        4294967295u, {"a", nullptr}, 4294967295u, 4294967295u, 4294967295u);
        CHECK(out == "\t18446744073709551615\t4294967295\t4294967295\t-\t-\t4294967295\t4294967294\t18446744069414584318\t-\t1\t4294967295\t4294967295\ta\t-\t4294967295\t4294967295\t"
                     "4294967295\n");
        size_t tabs = 0;
        for (char c : std::string(breakpoint_header())) tabs += c == '\t';
        CHECK(tabs == 17 && std::string(breakpoint_header()).find("\tBREAK_HASH\tBREAK_BASE_APPROX\t") != std::string::npos);
        out.clear();
        breakpoint_line(out, "r", 1, 10, 3, 2, {"x", "1"}, 2, 1, {"x", "1"}, 1, 0, {"y", "2"}, 2, 1, 1);
        tabs = 0;
        for (char c : out) tabs += c == '\t';
        CHECK(tabs == 17 && out.back() == '\n');
    }
    printf("ok %llu\n", (unsigned long long)checks);
    return 0;
}
