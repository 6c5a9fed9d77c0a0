// census_format.h -- the host side of `taxor census` and `taxor search --coverage-breadth`: the key estimate of
// a bin from its column's nonzero bytes, an IXF's capacity, the test that says a column is a peeled filter at all, the sums per user
// bin and IXF, and the text of one line of refs.tsv, of ixfs.tsv and of the four columns the coverage file gains.  census.hip counts the
// bytes; the CLI formats with the functions below.  No HIP in here: tests/sanitize/census_check.cpp runs it under ASan + UBSan.
#pragma once
#include "ixf_arith.h"

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

namespace taxor {

// A bin's n keys each own one slot, and a slot's byte is uniform over 256 values: nonzero ~ Binomial(n, 255/256), so
// nonzero * 256 / 255 estimates n with standard deviation sqrt(n / 255); nonzero <= n always
inline uint64_t census_keys_est(uint64_t nonzero) { return (uint64_t)std::llround((double)nonzero * 256.0 / 255.0); }

// keys a bin of an IXF with this segment length is sized for: the largest n with ixf_seg_len(n) <= seg_len, by bisection (ixf_seg_len
// does not fall as n grows); 0 when not even an empty bin fits
inline uint64_t census_capacity(uint64_t seg_len)
{
    if (seg_len > (1ull << 40)) seg_len = 1ull << 40;          // 1.23 * n stays far inside a double's integers
    if (ixf_seg_len(0) > seg_len) return 0;
    uint64_t lo = 0, hi = 3 * seg_len + 3;                     // ixf_seg_len(lo) <= seg_len < ixf_seg_len(hi): 1.23 * hi / 3 > seg_len
    while (hi - lo > 1) {
        const uint64_t mid = lo + (hi - lo) / 2;
        if (ixf_seg_len(mid) <= seg_len) lo = mid;
        else hi = mid;
    }
    return lo;
}

// more nonzero bytes than the IXF has room for keys: the column is no peeled filter (random fill, a writer that leaves free slots as
// they were) and its estimate says nothing
inline bool census_peeled(uint64_t nonzero, uint64_t capacity) { return nonzero <= capacity; }

// a count that may be "NA"
struct census_count {
    uint64_t value;
    bool flagged;
};

inline void census_put_u64(std::string &s, uint64_t v)
{
    char tmp[20];
    int n = 0;
    do { tmp[n++] = (char)('0' + v % 10); v /= 10; } while (v);
    while (n) s += tmp[--n];
}

inline void census_put_count(std::string &s, census_count c)
{
    if (c.flagged) s += "NA";
    else census_put_u64(s, c.value);
}

inline void census_put_double(std::string &s, const char *fmt, double v)
{
    char tmp[400];
    const int n = snprintf(tmp, sizeof tmp, fmt, v);
    if (n > 0) s.append(tmp, (size_t)(n < (int)sizeof tmp ? n : (int)sizeof tmp - 1));
}

// what the census needs of one IXF
struct census_ixf {
    uint64_t bins, seg_len, stride;
    const int64_t *fname_idx;      // [bins], < 0 = merged bin
};

struct census_ixf_sum {
    uint64_t leaf_bins, capacity;
    census_count max_bin_keys;     // flagged when any bin of the IXF is not a peeled filter
};

struct census_tables {
    std::vector<census_count> index_hashes;    // [n_user_bins] keys_est summed over the user bin's leaf technical bins; flagged if any part is
    std::vector<uint64_t> leaf_bins;           // [n_user_bins]
    std::vector<census_ixf_sum> ixf;           // [n_ixf]
};

// nonzero: the census's words in index bin order (all bins of IXF 0, then IXF 1, ...).  A leaf bin that names a user bin outside
// [0, n_user_bins) counts for its IXF only
inline void census_sum(const census_ixf *ixf, uint64_t n_ixf, const uint64_t *nonzero, uint64_t n_user_bins, census_tables &out)
{
    out.index_hashes.assign(n_user_bins, census_count{0, false});
    out.leaf_bins.assign(n_user_bins, 0);
    out.ixf.assign(n_ixf, census_ixf_sum{0, 0, census_count{0, false}});
    uint64_t at = 0;
    for (uint64_t x = 0; x < n_ixf; ++x) {
        census_ixf_sum &s = out.ixf[x];
        s.capacity = census_capacity(ixf[x].seg_len);
        for (uint64_t j = 0; j < ixf[x].bins; ++j, ++at) {
            const bool peeled = census_peeled(nonzero[at], s.capacity);
            const uint64_t est = census_keys_est(nonzero[at]);
            if (!peeled) s.max_bin_keys.flagged = true;
            else if (est > s.max_bin_keys.value) s.max_bin_keys.value = est;
            const int64_t b = ixf[x].fname_idx ? ixf[x].fname_idx[j] : -1;
            if (b < 0) continue;
            ++s.leaf_bins;
            if ((uint64_t)b >= n_user_bins) continue;
            ++out.leaf_bins[(uint64_t)b];
            if (!peeled) out.index_hashes[(uint64_t)b].flagged = true;
            else out.index_hashes[(uint64_t)b].value += est;
        }
    }
}

inline const char *census_ref_header() { return "#ACCESSION\tREFERENCE_NAME\tTAXID\tREF_LEN\tLEAF_BINS\tINDEX_HASHES\tHASHES_PER_KB\n"; }
inline const char *census_ixf_header() { return "#IXF\tBINS\tLEAF_BINS\tMERGED_BINS\tROWS\tCAPACITY\tMAX_BIN_KEYS\tFILL\tBYTES\n"; }
inline const char *census_breadth_header() { return "\tINDEX_HASHES\tBREADTH\tEXPECTED_BREADTH\tBREADTH_RATIO"; }

// refs.tsv: one user bin.  HASHES_PER_KB = INDEX_HASHES * 1000 / REF_LEN with two decimals, NA when INDEX_HASHES is or REF_LEN is 0
inline void census_ref_line(std::string &out, const char *accession, const char *name, const char *taxid, uint64_t ref_len, uint64_t leaf_bins, census_count index_hashes)
{
    out += accession ? accession : "-";
    out += '\t';
    out += name ? name : "-";
    out += '\t';
    out += taxid ? taxid : "-";
    out += '\t';
    census_put_u64(out, ref_len);
    out += '\t';
    census_put_u64(out, leaf_bins);
    out += '\t';
    census_put_count(out, index_hashes);
    out += '\t';
    if (index_hashes.flagged || ref_len == 0) out += "NA";
    else census_put_double(out, "%.2f", (double)index_hashes.value * 1000.0 / (double)ref_len);
    out += '\n';
}

// ixfs.tsv: one IXF.  ROWS = 3 * seg_len, BYTES = ROWS * stride, FILL = MAX_BIN_KEYS / CAPACITY with three decimals (NA when
// MAX_BIN_KEYS is or CAPACITY is 0): a low fill means rows nobody needs
inline void census_ixf_line(std::string &out, uint64_t ixf, uint64_t bins, uint64_t leaf_bins, uint64_t seg_len, uint64_t stride, census_count max_bin_keys)
{
    const uint64_t capacity = census_capacity(seg_len);
    auto num = [&](uint64_t v) { census_put_u64(out, v); out += '\t'; };
    num(ixf);
    num(bins);
    num(leaf_bins);
    num(bins >= leaf_bins ? bins - leaf_bins : 0);
    num(3 * seg_len);
    num(capacity);
    census_put_count(out, max_bin_keys);
    out += '\t';
    if (max_bin_keys.flagged || capacity == 0) out += "NA";
    else census_put_double(out, "%.3f", (double)max_bin_keys.value / (double)capacity);
    out += '\t';
    census_put_u64(out, 3 * seg_len * stride);
    out += '\n';
}

// `--coverage-breadth`: the four columns behind a line of the coverage file, each led by its tab.  BREADTH = min(1, distinct /
// index_hashes), EXPECTED_BREADTH = 1 - exp(-hash_matches / index_hashes) (uniform sampling with replacement), BREADTH_RATIO their
// quotient; the three are NA where INDEX_HASHES is NA or 0, the ratio also where the expectation prints as 0.0000.  Reported, not
// thresholded
inline void census_breadth_columns(std::string &out, uint64_t distinct, uint64_t hash_matches, census_count index_hashes)
{
    out += '\t';
    census_put_count(out, index_hashes);
    if (index_hashes.flagged || index_hashes.value == 0) {
        out += "\tNA\tNA\tNA";
        return;
    }
    const double ih = (double)index_hashes.value;
    double breadth = (double)distinct / ih;
    if (breadth > 1.0) breadth = 1.0;
    const double expected = 1.0 - std::exp(-(double)hash_matches / ih);
    std::string e;
    census_put_double(e, "%.4f", expected);
    out += '\t';
    census_put_double(out, "%.4f", breadth);
    out += '\t';
    out += e;
    out += '\t';
    if (e == "0.0000") out += "NA";
    else census_put_double(out, "%.2f", breadth / expected);
}

}   // namespace taxor
