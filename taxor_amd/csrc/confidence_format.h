// confidence_format.h -- the host side of `taxor search --lca-confidence`: whether a depth of a call's
// lineage holds under the threshold, and the text of one line of the call file with its three further columns.  confidence.hip
// evaluates confidence_holds' expression on the device (that object is built with -ffp-contract=off); the CLI formats with
// confidence_line.  No HIP in here: tests/sanitize/confidence_check.cpp runs it under ASan + UBSan.
#pragma once
#include <cmath>
#include <cstdint>
#include <string>

namespace taxor {

// a confidence the library and the CLI accept: a number in [0, 1]
inline bool confidence_valid(double c) { return !std::isnan(c) && c >= 0.0 && c <= 1.0; }

// depth d holds when support[d] is not below C * n, fp64 as written (constexpr: the device's compiler takes it as it stands)
constexpr bool confidence_holds(uint32_t support, double c, uint32_t n_hashes) { return !((double)support < c * (double)n_hashes); }

inline void confidence_put_u64(std::string &s, uint64_t v)
{
    char tmp[20];
    int n = 0;
    do { tmp[n++] = (char)('0' + v % 10); v /= 10; } while (v);
    while (n) s += tmp[--n];
}

// the call file's first line when the option is given
inline const char *confidence_header() { return "#STATUS\tQUERY_NAME\tTAXID\tQUERY_LEN\tQHASH_COUNT\tBEST_QHASH_MATCH\tREFERENCES\tSUPPORT\tLCA_TAXID\tLCA_SUPPORT\n"; }

// One read: appended to `out`.  taxid: the confident call's id string, null for an unclassified read; lca_taxid: the id string of
// section 10.3's call, null for a read that was unclassified before the threshold was asked (it prints zeros: nothing matched).  A
// read the threshold made unclassified has taxid null and lca_taxid set: U, TAXID 0, its real counts, support[0], and the call it lost.
inline void confidence_line(std::string &out, const char *id, uint64_t id_len, const char *taxid, uint64_t query_len, uint32_t n_hashes, uint32_t best, uint32_t n_refs,
                            uint32_t support, const char *lca_taxid, uint32_t lca_support)
{
    const bool never = lca_taxid == nullptr;
    out += taxid ? "C\t" : "U\t";
    out.append(id, id_len);
    out += '\t';
    out += taxid ? taxid : "0";
    out += '\t';
    confidence_put_u64(out, query_len);
    const uint64_t num[5] = {never ? 0u : n_hashes, never ? 0u : best, never ? 0u : n_refs, never ? 0u : support, never ? 0u : lca_support};
    for (int i = 0; i < 4; ++i) {
        out += '\t';
        confidence_put_u64(out, num[i]);
    }
    out += '\t';
    out += never ? "0" : lca_taxid;
    out += '\t';
    confidence_put_u64(out, num[4]);
    out += '\n';
}

}   // namespace taxor
