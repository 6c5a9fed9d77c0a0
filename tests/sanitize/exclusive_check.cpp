// exclusive_check.cpp -- the host side of `taxor search --exclusive-file` / `--exclusive-reads-file` (taxor_amd/csrc/exclusive_format.h)
// under ASan + UBSan: the fraction's four decimals at its rounding edges, rows of zeros, null names, an empty id, the largest numbers,
// the rounded distinct count, and a batch without a row (the file is its header).  With arguments "exclusive_hits hits" it prints the
// fraction, for the Python restatement to be compared with.  Prints "ok <checks>" or the first failure.
#include "exclusive_format.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <vector>

#define CHECK(x)                                                        \
    do {                                                                \
        ++checks;                                                       \
        if (!(x)) { printf("FAILED line %d: %s\n", __LINE__, #x); return 1; } \
    } while (0)

struct Row {
    uint64_t cand_reads, hits, excl, excl_reads, distinct;
};

// what the CLI does with a run's table: the header, then one line per row
static std::string file_of(const std::vector<Row> &rows)
{
    std::string out = taxor::exclusive_header();
    for (const Row &r : rows) taxor::exclusive_bin_line(out, {"acc", "7"}, r.cand_reads, r.hits, r.excl, r.excl_reads, r.distinct);
    return out;
}

int main(int argc, char **argv)
{
    using namespace taxor;
    if (argc == 3) {
        std::string s;
        exclusive_put_fraction(s, strtoull(argv[1], nullptr, 10), strtoull(argv[2], nullptr, 10));
        printf("%s\n", s.c_str());
        return 0;
    }
    uint64_t checks = 0;
    auto frac = [](uint64_t e, uint64_t h) { std::string s; exclusive_put_fraction(s, e, h); return s; };
    CHECK(frac(0, 0) == "0.0000" && frac(0, 5) == "0.0000" && frac(5, 5) == "1.0000" && frac(1, 2) == "0.5000");
    CHECK(frac(1, 3) == "0.3333" && frac(2, 3) == "0.6667" && frac(1, 8) == "0.1250" && frac(1, 16) == "0.0625");
    CHECK(frac(1, 20000) == "0.0001" && frac(1, 20001) == "0.0000" && frac(1, 19999) == "0.0001");      // around half of the last digit
    CHECK(frac(19999, 20000) == "1.0000" && frac(19997, 20000) == "0.9999" && frac(9999, 10000) == "0.9999");
    CHECK(frac(~0ull - 1, ~0ull) == "1.0000" && frac(1, ~0ull) == "0.0000" && frac(~0ull, ~0ull) == "1.0000");
    CHECK(exclusive_distinct(0.0, 0) == 0 && exclusive_distinct(0.0, 3) == 1 && exclusive_distinct(0.4, 1) == 1 && exclusive_distinct(0.4, 0) == 0);
    CHECK(exclusive_distinct(2.5, 9) == 3 && exclusive_distinct(3.5, 9) == 4 && exclusive_distinct(2.49, 9) == 2);      // halves away from zero
    CHECK(exclusive_distinct(std::numeric_limits<double>::quiet_NaN(), 2) == 1 && exclusive_distinct(std::numeric_limits<double>::infinity(), 0) == 0);
    CHECK(exclusive_distinct(-3.0, 0) == 0 && exclusive_distinct(1e30, 1) == 1);
    {   // the per-user-bin file: no row, a row of zeros, the largest numbers, null names
        CHECK(file_of({}) == "#ACCESSION\tTAXID\tCANDIDATE_READS\tHITS\tEXCLUSIVE_HITS\tEXCLUSIVE_READS\tDISTINCT_EXCLUSIVE\tEXCLUSIVE_FRACTION\n");
        CHECK(file_of({{1, 0, 0, 0, 0}}) == std::string(exclusive_header()) + "acc\t7\t1\t0\t0\t0\t0\t0.0000\n");
        CHECK(file_of({{3, 40, 10, 2, 9}, {1, 7, 7, 1, 7}}) == std::string(exclusive_header()) + "acc\t7\t3\t40\t10\t2\t9\t0.2500\nacc\t7\t1\t7\t7\t1\t7\t1.0000\n");
        std::string out;
        exclusive_bin_line(out, {nullptr, nullptr}, ~0ull, ~0ull, ~0ull, ~0ull, ~0ull);
        CHECK(out == "-\t-\t18446744073709551615\t18446744073709551615\t18446744073709551615\t18446744073709551615\t18446744073709551615\t1.0000\n");
        size_t tabs = 0;
        for (char c : std::string(exclusive_header())) tabs += c == '\t';
        CHECK(tabs == 7);
    }
    {   // the per-read file
        std::string out;
        exclusive_read_line(out, "read 1", 6, {"GCF_3", "1280"}, 12000, 1200, 900, 910, 35, 3, 1000, 870);
        CHECK(out == "read 1\tGCF_3\t1280\t12000\t1200\t900\t910\t35\t3\t1000\t870\n");
        out.clear();
        exclusive_read_line(out, "", 0, {nullptr, "1"}, ~0ull, 4294967295u, 4294967295u, 4294967295u, 4294967295u, 4294967295u, 4294967295u, 4294967295u);
        CHECK(out == "\t-\t1\t18446744073709551615\t4294967295\t4294967295\t4294967295\t4294967295\t4294967295\t4294967295\t4294967295\n");
        out.clear();
        exclusive_read_line(out, "z", 1, {"a", nullptr}, 0, 0, 0, 0, 0, 0, 0, 0);
        CHECK(out == "z\ta\t-\t0\t0\t0\t0\t0\t0\t0\t0\n");
        size_t tabs = 0;
        for (char c : std::string(exclusive_reads_header())) tabs += c == '\t';
        CHECK(tabs == 10 && std::string(exclusive_reads_header()).find("\tQHASH_MATCH\tHITS\tEXCLUSIVE_HITS\tCANDIDATES\tMATCHED\tSHARED\n") != std::string::npos);
    }
    printf("ok %llu\n", (unsigned long long)checks);
    return 0;
}
