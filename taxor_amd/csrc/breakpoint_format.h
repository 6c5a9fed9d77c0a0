// breakpoint_format.h -- the host side of `taxor search --breakpoint-file`: the approximate base position of
// a break in the read's ordered hash list, and the text of one line of the file.  breakpoint.hip computes the words; the CLI formats
// them with breakpoint_line.  No HIP in here: tests/sanitize/breakpoint_check.cpp runs it under ASan + UBSan.
#pragma once
#include <cstdint>
#include <string>

namespace taxor {

constexpr uint32_t BREAKPOINT_DEFAULT_MIN_GAIN = 1;

// floor(p * query_len / n) for a break in front of hash p of n, p < n < 2^32, in 64 bits for every query_len: with query_len =
// q * n + rem the value is p * q + floor(p * rem / n), where p * q <= query_len and p * rem < 2^64.  0 for a read without a hash.
// APPROXIMATE: the hash list carries no positions, so this is the base only as far as the read's hashes are spread evenly.
inline uint64_t breakpoint_base(uint64_t p, uint64_t query_len, uint64_t n)
{
    if (n == 0) return 0;
    return p * (query_len / n) + p * (query_len % n) / n;
}

inline void breakpoint_put_u64(std::string &s, uint64_t v)
{
    char tmp[20];
    int n = 0;
    do { tmp[n++] = (char)('0' + v % 10); v /= 10; } while (v);
    while (n) s += tmp[--n];
}

// the file's first line
inline const char *breakpoint_header()
{
    return "#QUERY_NAME\tQUERY_LEN\tQHASH_COUNT\tCANDIDATES\tBEST_ACCESSION\tBEST_TAXID\tBEST_LOCATED\tBREAK_HASH\tBREAK_BASE_APPROX\tLEFT_ACCESSION\tLEFT_TAXID\t"
           "LEFT_HITS\tLEFT_HITS_OF_RIGHT\tRIGHT_ACCESSION\tRIGHT_TAXID\tRIGHT_HITS\tRIGHT_HITS_OF_LEFT\tGAIN\n";
}

// a reference as the TSV names it; either string may be null ("-")
struct breakpoint_ref {
    const char *accession, *taxid;
};

// one reported read: appended to `out`.  LEFT is A (the best reference in front of the break), RIGHT is B (the best from it on)
inline void breakpoint_line(std::string &out, const char *id, uint64_t id_len, uint64_t query_len, uint32_t n_hashes, uint32_t candidates, breakpoint_ref best,
                            uint32_t single, uint32_t break_hash, breakpoint_ref left, uint32_t pre_a, uint32_t pre_b, breakpoint_ref right, uint32_t suf_b,
                            uint32_t suf_a, uint32_t gain)
{
    auto num = [&](uint64_t v) { out += '\t'; breakpoint_put_u64(out, v); };
    auto ref = [&](const breakpoint_ref &r) { out += '\t'; out += r.accession ? r.accession : "-"; out += '\t'; out += r.taxid ? r.taxid : "-"; };
    out.append(id, id_len);
    num(query_len);
    num(n_hashes);
    num(candidates);
    ref(best);
    num(single);
    num(break_hash);
    num(breakpoint_base(break_hash, query_len, n_hashes));
    ref(left);
    num(pre_a);
    num(pre_b);
    ref(right);
    num(suf_b);
    num(suf_a);
    num(gain);
    out += '\n';
}

// ---- `--base-positions`: the same header and the same line, with two columns appended.  left_end_base =
// pos[break_hash - 1] + k, the base behind the last k-mer in front of the break; break_base = pos[break_hash], the first base of the
// k-mer the break stands in front of -- real bases, from the positions captured with the hash lists
inline std::string breakpoint_header_positions()
{
    std::string h = breakpoint_header();
    h.pop_back();
    return h + "\tLEFT_END_BASE\tBREAK_BASE\n";
}

inline void breakpoint_line_positions(std::string &out, const char *id, uint64_t id_len, uint64_t query_len, uint32_t n_hashes, uint32_t candidates, breakpoint_ref best,
                                      uint32_t single, uint32_t break_hash, breakpoint_ref left, uint32_t pre_a, uint32_t pre_b, breakpoint_ref right, uint32_t suf_b,
                                      uint32_t suf_a, uint32_t gain, uint64_t left_end_base, uint64_t break_base)
{
    breakpoint_line(out, id, id_len, query_len, n_hashes, candidates, best, single, break_hash, left, pre_a, pre_b, right, suf_b, suf_a, gain);
    out.pop_back();                                    // the line's '\n'
    out += '\t';
    breakpoint_put_u64(out, left_end_base);
    out += '\t';
    breakpoint_put_u64(out, break_base);
    out += '\n';
}

}   // namespace taxor
