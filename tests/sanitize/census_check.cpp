// census_check.cpp -- the host side of `taxor census` / `taxor search --coverage-breadth` (taxor_amd/csrc/census_format.h) under ASan +
// UBSan: the estimate's rounding, the capacity's bisection at its edges (segment lengths no bin fits, the largest ones), the sums per
// user bin and IXF with flagged bins, bins that name no user bin of the index, an empty index, and every line formatter with NA, null
// names and the largest numbers.  Prints "ok <checks>" or the first failure.
#include "census_format.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
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
    CHECK(census_keys_est(0) == 0 && census_keys_est(1) == 1 && census_keys_est(127) == 127 && census_keys_est(128) == 129 && census_keys_est(255) == 256);
    CHECK(census_keys_est(996) == 1000 && census_keys_est(1ull << 52) == (uint64_t)std::llround((double)(1ull << 52) * 256.0 / 255.0));
    for (uint64_t seg = 0; seg < 3000; ++seg) {      // the definition, by walking
        const uint64_t c = census_capacity(seg);
        if (seg < ixf_seg_len(0)) { CHECK(c == 0); continue; }
        CHECK(ixf_seg_len(c) <= seg && ixf_seg_len(c + 1) > seg);
    }
    for (uint64_t n : {0ull, 1ull, 2ull, 1000ull, 1000000ull, 4000000000ull}) CHECK(census_capacity(ixf_seg_len(n)) >= n);
    CHECK(census_capacity((1ull << 32) / 3) > 3000000000ull && census_capacity(~0ull) == census_capacity(1ull << 40));
    CHECK(census_peeled(0, 0) && !census_peeled(1, 0) && census_peeled(5, 5) && !census_peeled(6, 5));
    {   // two IXFs: a flagged leaf poisons its user bin and its IXF only; a merged bin counts for its IXF's maximum; a leaf that names a
        // user bin outside the index counts as a leaf of its IXF and for nobody
        const uint64_t seg = ixf_seg_len(100), cap = census_capacity(seg);
        const int64_t fn0[4] = {0, 0, -1, 1}, fn1[3] = {2, 7, 1};
        const census_ixf fs[2] = {{4, seg, 64, fn0}, {3, seg, 64, fn1}};
        const uint64_t nz[7] = {10, 20, 90, cap + 1, 0, 50, 40};
        census_tables t;
        census_sum(fs, 2, nz, 3, t);
        CHECK(t.index_hashes.size() == 3 && t.leaf_bins[0] == 2 && t.leaf_bins[1] == 2 && t.leaf_bins[2] == 1);
        CHECK(!t.index_hashes[0].flagged && t.index_hashes[0].value == 30 && t.index_hashes[1].flagged && !t.index_hashes[2].flagged && t.index_hashes[2].value == 0);
        CHECK(t.ixf[0].leaf_bins == 3 && t.ixf[0].max_bin_keys.flagged && t.ixf[1].leaf_bins == 3 && !t.ixf[1].max_bin_keys.flagged);
        CHECK(cap >= 90 && t.ixf[1].max_bin_keys.value == 50);
        CHECK(t.ixf[0].capacity == cap);
        census_sum(fs, 0, nullptr, 0, t);            // an empty index
        CHECK(t.index_hashes.empty() && t.ixf.empty());
        const census_ixf no_names[1] = {{2, seg, 64, nullptr}};
        census_sum(no_names, 1, nz, 1, t);
        CHECK(t.ixf[0].leaf_bins == 0 && t.leaf_bins[0] == 0 && t.ixf[0].max_bin_keys.value == 20);
    }
    {
        std::string s;
        census_ref_line(s, "acc", "name of it", "7", 15000, 2, census_count{2345, false});
        CHECK(s == "acc\tname of it\t7\t15000\t2\t2345\t156.33\n");
        s.clear();
        census_ref_line(s, nullptr, nullptr, nullptr, 0, 0, census_count{5, false});
        CHECK(s == "-\t-\t-\t0\t0\t5\tNA\n");
        s.clear();
        census_ref_line(s, "a", "b", "c", 9, 1, census_count{5, true});
        CHECK(s == "a\tb\tc\t9\t1\tNA\tNA\n");
        s.clear();
        census_ref_line(s, "a", "b", "c", 1, ~0ull, census_count{~0ull, false});
        CHECK(s == "a\tb\tc\t1\t18446744073709551615\t18446744073709551615\t18446744073709551616000.00\n");
        size_t tabs = 0;
        for (char c : std::string(census_ref_header())) tabs += c == '\t';
        CHECK(tabs == 6);
    }
    {
        std::string s;
        census_ixf_line(s, 1, 64, 60, 3, 64, census_count{0, false});
        CHECK(s == "1\t64\t60\t4\t9\t0\t0\tNA\t576\n");
        s.clear();
        const uint64_t seg = ixf_seg_len(1000), cap = census_capacity(seg);
        census_ixf_line(s, 0, 1025, 1000, seg, 1088, census_count{cap, false});
        char want[256];
        snprintf(want, sizeof want, "0\t1025\t1000\t25\t%llu\t%llu\t%llu\t1.000\t%llu\n", (unsigned long long)(3 * seg), (unsigned long long)cap, (unsigned long long)cap,
                 (unsigned long long)(3 * seg * 1088));
        CHECK(s == want);
        s.clear();
        census_ixf_line(s, ~0ull, 3, 5, seg, 64, census_count{1, true});       // more leaves than bins cannot underflow
        CHECK(s.find("\t3\t5\t0\t") != std::string::npos && s.find("\tNA\tNA\t") != std::string::npos);
        size_t tabs = 0;
        for (char c : std::string(census_ixf_header())) tabs += c == '\t';
        CHECK(tabs == 8);
    }
    {
        auto cols = [](uint64_t d, uint64_t hm, census_count ih) { std::string s; census_breadth_columns(s, d, hm, ih); return s; };
        CHECK(cols(7, 9, census_count{0, false}) == "\t0\tNA\tNA\tNA" && cols(7, 9, census_count{3, true}) == "\tNA\tNA\tNA\tNA");
        CHECK(cols(500, 700, census_count{1000, false}) == "\t1000\t0.5000\t0.5034\t0.99");
        CHECK(cols(1200, 5000, census_count{1000, false}) == "\t1000\t1.0000\t0.9933\t1.01");
        CHECK(cols(1, 1, census_count{1000000000, false}) == "\t1000000000\t0.0000\t0.0000\tNA");
        CHECK(cols(0, 0, census_count{10, false}) == "\t10\t0.0000\t0.0000\tNA");
        CHECK(cols(~0ull, ~0ull, census_count{1, false}) == "\t1\t1.0000\t1.0000\t1.00");
        CHECK(cols(1, ~0ull, census_count{~0ull, false}) == "\t18446744073709551615\t0.0000\t0.6321\t0.00");
        size_t tabs = 0;
        for (char c : std::string(census_breadth_header())) tabs += c == '\t';
        CHECK(tabs == 4);
    }
    printf("ok %llu\n", (unsigned long long)checks);
    return 0;
}
