// confidence_check.cpp -- the host side of `taxor search --lca-confidence` (taxor_amd/csrc/confidence_format.h) under ASan + UBSan: which
// thresholds are accepted, whether a depth holds at and around the boundary and at the ends of 32 bits, and the line formatter for a
// called read, a read the threshold made unclassified, a read that was unclassified anyway, an empty id and the largest numbers.
// Prints "ok <checks>" or the first failure.
#include "confidence_format.h"

#include <cstdio>
#include <limits>

#define CHECK(x)                                                        \
    do {                                                                \
        ++checks;                                                       \
        if (!(x)) { printf("FAILED line %d: %s\n", __LINE__, #x); return 1; } \
    } while (0)

int main()
{
    using namespace taxor;
    uint64_t checks = 0;
    CHECK(confidence_valid(0.0) && confidence_valid(1.0) && confidence_valid(0.5) && confidence_valid(-0.0));
    CHECK(!confidence_valid(-1e-9) && !confidence_valid(1.0000001) && !confidence_valid(std::numeric_limits<double>::quiet_NaN()));
    CHECK(!confidence_valid(std::numeric_limits<double>::infinity()) && !confidence_valid(-std::numeric_limits<double>::infinity()));
    // the boundary: 5 of 10 holds at 0.5, 4 does not; at 0 everything holds, a read without a hash included; at 1 only all of them
    CHECK(confidence_holds(5, 0.5, 10) && !confidence_holds(4, 0.5, 10) && confidence_holds(6, 0.5, 10));
    CHECK(confidence_holds(0, 0.0, 10) && confidence_holds(0, 0.0, 0) && confidence_holds(0, 1.0, 0));
    CHECK(confidence_holds(10, 1.0, 10) && !confidence_holds(9, 1.0, 10));
    CHECK(confidence_holds(4294967295u, 1.0, 4294967295u) && !confidence_holds(4294967294u, 1.0, 4294967295u));
    for (uint32_t n = 0; n <= 300; ++n)
        for (uint32_t s = 0; s <= n; ++s) {
            CHECK(confidence_holds(s, 0.25, n) == (4ull * s >= n));           // 0.25 * n is exact in fp64
            CHECK(confidence_holds(s, 0.0, n));
        }
    {   // the formatter
        std::string out;
        confidence_line(out, "read 1", 6, "562", 1200, 100, 60, 2, 55, "562", 55);
        CHECK(out == "C\tread 1\t562\t1200\t100\t60\t2\t55\t562\t55\n");
        out.clear();
        confidence_line(out, "r", 1, "561", 1200, 100, 60, 2, 70, "562", 40);      // climbed
        CHECK(out == "C\tr\t561\t1200\t100\t60\t2\t70\t562\t40\n");
        out.clear();
        confidence_line(out, "r", 1, nullptr, 1200, 100, 12, 1, 14, "562", 12);    // the threshold made it unclassified: its real counts
        CHECK(out == "U\tr\t0\t1200\t100\t12\t1\t14\t562\t12\n");
        out.clear();
        confidence_line(out, "r", 1, nullptr, 8, 77, 66, 55, 44, nullptr, 33);     // unclassified anyway: zeros, whatever the words hold
        CHECK(out == "U\tr\t0\t8\t0\t0\t0\t0\t0\t0\n");
        out.clear();
        confidence_line(out, "", 0, "1", 18446744073709551615ull, 4294967295u, 4294967295u, 4294967295u, 4294967295u, "1", 4294967295u);
        CHECK(out == "C\t\t1\t18446744073709551615\t4294967295\t4294967295\t4294967295\t4294967295\t1\t4294967295\n");
        size_t tabs = 0;
        for (char c : std::string(confidence_header())) tabs += c == '\t';
        CHECK(tabs == 9 && std::string(confidence_header()).find("\tSUPPORT\tLCA_TAXID\tLCA_SUPPORT\n") != std::string::npos);
    }
    printf("ok %llu\n", (unsigned long long)checks);
    return 0;
}
