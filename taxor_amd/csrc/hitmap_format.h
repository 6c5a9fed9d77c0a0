// hitmap_format.h -- the host side of `taxor search --hitmap-file`: where a hash of a read lies among the
// S segments of the read's ordered hash list, how many hashes a segment holds, and the text of one line of the file.  hitmap.hip
// evaluates hitmap_seg's expression on the device; the CLI formats with hitmap_line.  No HIP in here:
// tests/sanitize/hitmap_check.cpp runs it under ASan + UBSan.
#pragma once
#include <cstdint>
#include <string>

namespace taxor {

constexpr uint32_t HITMAP_DEFAULT_SEGMENTS = 16, HITMAP_MAX_SEGMENTS = 64;

// segment of hash i (its rank in the read's saved list, from 0) of a read with n hashes, i < n: floor(i * S / n) in 64 bits
inline uint32_t hitmap_seg(uint64_t i, uint32_t S, uint64_t n) { return (uint32_t)(i * (uint64_t)S / n); }

// first hash of segment j, j <= S: the smallest i with floor(i * S / n) >= j, which is ceil(j * n / S)
inline uint64_t hitmap_seg_first(uint32_t j, uint32_t S, uint64_t n) { return ((uint64_t)j * n + S - 1) / S; }

// hashes of segment j; 0 for some segments when n < S
inline uint64_t hitmap_seg_size(uint32_t j, uint32_t S, uint64_t n) { return hitmap_seg_first(j + 1, S, n) - hitmap_seg_first(j, S, n); }

inline void hitmap_put_u64(std::string &s, uint64_t v)
{
    char tmp[20];
    int n = 0;
    do { tmp[n++] = (char)('0' + v % 10); v /= 10; } while (v);
    while (n) s += tmp[--n];
}

// the file's first line
inline const char *hitmap_header() { return "#QUERY_NAME\tACCESSION\tTAXID\tQUERY_LEN\tQHASH_COUNT\tQHASH_MATCH\tLOCATED\tSEGMENT_SIZES\tSEGMENT_HITS\n"; }

// one mapped tuple: appended to `out`.  hits: the tuple's S counters.  accession / taxid may be null ("-")
inline void hitmap_line(std::string &out, const char *id, uint64_t id_len, const char *accession, const char *taxid, uint64_t query_len, uint32_t n_hashes,
                        uint32_t count, const uint32_t *hits, uint32_t S)
{
    out.append(id, id_len);
    out += '\t';
    out += accession ? accession : "-";
    out += '\t';
    out += taxid ? taxid : "-";
    out += '\t';
    hitmap_put_u64(out, query_len);
    out += '\t';
    hitmap_put_u64(out, n_hashes);
    out += '\t';
    hitmap_put_u64(out, count);
    out += '\t';
    uint64_t located = 0;
    for (uint32_t j = 0; j < S; ++j) located += hits[j];
    hitmap_put_u64(out, located);
    out += '\t';
    for (uint32_t j = 0; j < S; ++j) {
        if (j) out += ',';
        hitmap_put_u64(out, n_hashes ? hitmap_seg_size(j, S, n_hashes) : 0);
    }
    out += '\t';
    for (uint32_t j = 0; j < S; ++j) {
        if (j) out += ',';
        hitmap_put_u64(out, hits[j]);
    }
    out += '\n';
}

}   // namespace taxor
