// exclusive_format.h -- the host side of `taxor search --exclusive-file` / `--exclusive-reads-file`: the
// rounded distinct count, the fraction's four decimals and the text of one line of either file.  exclusive.hip computes the words; the
// CLI formats them with exclusive_bin_line and exclusive_read_line.  No HIP in here: tests/sanitize/exclusive_check.cpp runs it under
// ASan + UBSan.
#pragma once
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <string>

namespace taxor {

inline void exclusive_put_u64(std::string &s, uint64_t v)
{
    char tmp[20];
    int n = 0;
    do { tmp[n++] = (char)('0' + v % 10); v /= 10; } while (v);
    while (n) s += tmp[--n];
}

// DISTINCT_EXCLUSIVE: the sketch's estimate rounded half away from zero, at least 1 where a hash was exclusive at all
inline uint64_t exclusive_distinct(double estimate, uint64_t exclusive_hits)
{
    long long d = std::isfinite(estimate) && estimate > 0.0 && estimate < 9.0e18 ? std::llround(estimate) : 0;
    if (exclusive_hits > 0 && d < 1) d = 1;
    return (uint64_t)d;
}

// EXCLUSIVE_FRACTION = exclusive_hits / hits with four decimals, 0.0000 where hits is 0.  Reported, not thresholded: 0.5 is no verdict
inline void exclusive_put_fraction(std::string &s, uint64_t exclusive_hits, uint64_t hits)
{
    char tmp[64];
    const int n = snprintf(tmp, sizeof tmp, "%.4f", hits ? (double)exclusive_hits / (double)hits : 0.0);
    if (n > 0) s.append(tmp, (size_t)(n < (int)sizeof tmp ? n : (int)sizeof tmp - 1));
}

// the files' first lines
inline const char *exclusive_header() { return "#ACCESSION\tTAXID\tCANDIDATE_READS\tHITS\tEXCLUSIVE_HITS\tEXCLUSIVE_READS\tDISTINCT_EXCLUSIVE\tEXCLUSIVE_FRACTION\n"; }
inline const char *exclusive_reads_header()
{
    return "#QUERY_NAME\tACCESSION\tTAXID\tQUERY_LEN\tQHASH_COUNT\tQHASH_MATCH\tHITS\tEXCLUSIVE_HITS\tCANDIDATES\tMATCHED\tSHARED\n";
}

// a reference as the TSV names it; either string may be null ("-")
struct exclusive_ref {
    const char *accession, *taxid;
};

// --exclusive-file: one user bin that was a candidate of an examined read, appended to `out`
inline void exclusive_bin_line(std::string &out, exclusive_ref ref, uint64_t cand_reads, uint64_t hits, uint64_t exclusive_hits, uint64_t exclusive_reads, uint64_t distinct)
{
    auto num = [&](uint64_t v) { out += '\t'; exclusive_put_u64(out, v); };
    out += ref.accession ? ref.accession : "-";
    out += '\t';
    out += ref.taxid ? ref.taxid : "-";
    num(cand_reads);
    num(hits);
    num(exclusive_hits);
    num(exclusive_reads);
    num(distinct);
    out += '\t';
    exclusive_put_fraction(out, exclusive_hits, hits);
    out += '\n';
}

// --exclusive-reads-file: one surviving tuple of an examined read with two candidates or more, appended to `out`
inline void exclusive_read_line(std::string &out, const char *id, uint64_t id_len, exclusive_ref ref, uint64_t query_len, uint32_t n_hashes, uint32_t count, uint32_t hits,
                                uint32_t exclusive_hits, uint32_t candidates, uint32_t matched, uint32_t shared)
{
    auto num = [&](uint64_t v) { out += '\t'; exclusive_put_u64(out, v); };
    out.append(id, id_len);
    out += '\t';
    out += ref.accession ? ref.accession : "-";
    out += '\t';
    out += ref.taxid ? ref.taxid : "-";
    num(query_len);
    num(n_hashes);
    num(count);
    num(hits);
    num(exclusive_hits);
    num(candidates);
    num(matched);
    num(shared);
    out += '\n';
}

}   // namespace taxor
