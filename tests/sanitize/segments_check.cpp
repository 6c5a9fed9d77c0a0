// segments_check.cpp -- the host side of `taxor search --segments-file` (taxor_amd/csrc/segments_format.h) under ASan + UBSan: the SHAPE
// of a reported read from the user bins of its segments, and the line formatter with null names, an empty id, the largest numbers and
// a segment that ends where the read does.  With arguments "bin bin ..." it prints segments_shape of the list, for the Python
// restatement to be compared with.  Prints "ok <checks>" or the first failure.
#include "segments_format.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#define CHECK(x)                                                        \
    do {                                                                \
        ++checks;                                                       \
        if (!(x)) { printf("FAILED line %d: %s\n", __LINE__, #x); return 1; } \
    } while (0)

int main(int argc, char **argv)
{
    using namespace taxor;
    if (argc > 1) {
        std::vector<int64_t> bins;
        for (int i = 1; i < argc; ++i) bins.push_back(strtoll(argv[i], nullptr, 10));
        printf("%s\n", segments_shape(bins.size(), bins.data()));
        return 0;
    }
    uint64_t checks = 0;
    auto shape = [](std::vector<int64_t> b) { return std::string(segments_shape(b.size(), b.data())); };
    CHECK(shape({1, 2}) == "split" && shape({7, 7}) == "split");                 // two candidates of one user bin are still two segments
    CHECK(shape({1, 2, 1}) == "insert" && shape({0, 9223372036854775807ll, 0}) == "insert");
    CHECK(shape({1, 2, 3}) == "mosaic" && shape({1, 1, 2}) == "mosaic" && shape({1, 2, 2}) == "mosaic");
    CHECK(shape({1, 2, 1, 2}) == "mosaic" && shape({1, 2, 1, 2, 1}) == "mosaic");
    CHECK(SEGMENTS_DEFAULT_SWITCH_COST == 16 && SEGMENTS_MAX_SWITCH_COST == 1048576);
    {   // the formatter
        std::string out;
        segments_line(out, "read 1", 6, 12000, 1200, 3, 3, "insert", 1100, 1000, 1, 400, 600, {"GCF_3", "1280"}, 180, {"GCF_1", "562"}, 4);
        CHECK(out == "read 1\t12000\t1200\t3\t3\tinsert\t1100\t1000\t1\t400\t600\t4000\t6000\tGCF_3\t1280\t180\tGCF_1\t562\t4\n");
        out.clear();
        segments_line(out, "r", 1, 10, 3, 2, 2, "split", 3, 2, 1, 2, 3, {"y", "2"}, 1, {"x", "1"}, 0);   // the last segment ends at the read's end
        CHECK(out == "r\t10\t3\t2\t2\tsplit\t3\t2\t1\t2\t3\t6\t10\ty\t2\t1\tx\t1\t0\n");
        out.clear();
        segments_line(out, "", 0, 18446744073709551615ull, 2147483647u, 4294967295u, 2147483647u, "mosaic", 4294967295u, 4294967295u, 2147483646u, 2147483646u,
                      2147483647u, {nullptr, "1"}, 4294967295u, {nullptr, nullptr}, 4294967295u);
        CHECK(out == "\t18446744073709551615\t2147483647\t4294967295\t2147483647\tmosaic\t4294967295\t4294967295\t2147483646\t2147483646\t2147483647\t"
                     "18446744065119617018\t18446744073709551615\t-\t1\t4294967295\t-\t-\t4294967295\n");
        CHECK(breakpoint_base(2147483646u, ~0ull, 2147483647u) == (uint64_t)((unsigned __int128)2147483646u * ~0ull / 2147483647u));
        CHECK(breakpoint_base(2147483647u, ~0ull, 2147483647u) == ~0ull);       // p == n: the read's length, for every length
        size_t tabs = 0;
        for (char c : std::string(segments_header())) tabs += c == '\t';
        CHECK(tabs == 18 && std::string(segments_header()).find("\tBASE_START_APPROX\tBASE_END_APPROX\t") != std::string::npos);
        tabs = 0;
        for (char c : out) tabs += c == '\t';
        CHECK(tabs == 18 && out.back() == '\n');
        out.clear();
        segments_line(out, "e", 1, 100, 0, 0, 2, "split", 0, 0, 0, 0, 0, {"a", "b"}, 0, {"a", "b"}, 0);    // no hash: no division by 0
        CHECK(out == "e\t100\t0\t0\t2\tsplit\t0\t0\t0\t0\t0\t0\t0\ta\tb\t0\ta\tb\t0\n");
    }
    printf("ok %llu\n", (unsigned long long)checks);
    return 0;
}
