// segments_format.h -- the host side of `taxor search --segments-file`: the SHAPE of a reported read, decided
// from the user bins of its segments alone, and the text of one line of the file (one line per segment).  segments.hip computes the
// segments; the CLI formats them with segments_line.  The two base columns are breakpoint_base of the segment's ends and keep the word
// APPROX in their names: the hash list carries no positions.  No HIP in here: tests/sanitize/segments_check.cpp runs it under
// ASan + UBSan.
#pragma once
#include "breakpoint_format.h"

#include <cstdint>
#include <string>

namespace taxor {

constexpr uint32_t SEGMENTS_DEFAULT_SWITCH_COST = 16;       // a choice, not a measurement
constexpr uint32_t SEGMENTS_MAX_SWITCH_COST = 1u << 20;

// the file's first line
inline const char *segments_header()
{
    return "#QUERY_NAME\tQUERY_LEN\tQHASH_COUNT\tCANDIDATES\tSEGMENTS\tSHAPE\tPATH_HITS\tSINGLE_HITS\tSEGMENT\tHASH_START\tHASH_END\tBASE_START_APPROX\tBASE_END_APPROX\t"
           "ACCESSION\tTAXID\tHITS\tBEST_ACCESSION\tBEST_TAXID\tHITS_OF_BEST\n";
}

// bins[0 .. k): the user bins of a reported read's segments in list order, k >= 2.  Neighbouring segments differ in CANDIDATE, not
// necessarily in user bin (a user bin may stand in several tuples); the shape looks at the user bins only
inline const char *segments_shape(uint64_t k, const int64_t *bins)
{
    if (k == 2) return "split";
    if (k == 3 && bins[0] == bins[2]) return "insert";
    return "mosaic";
}

// one segment of a reported read: appended to `out`.  `ref` is the segment's reference, `best` the best single reference of the read
inline void segments_line(std::string &out, const char *id, uint64_t id_len, uint64_t query_len, uint32_t n_hashes, uint32_t candidates, uint32_t n_segments,
                          const char *shape, uint32_t path_hits, uint32_t single, uint32_t segment, uint32_t start, uint32_t end, breakpoint_ref ref, uint32_t hits,
                          breakpoint_ref best, uint32_t best_hits)
{
    auto num = [&](uint64_t v) { out += '\t'; breakpoint_put_u64(out, v); };
    auto name = [&](const breakpoint_ref &r) { out += '\t'; out += r.accession ? r.accession : "-"; out += '\t'; out += r.taxid ? r.taxid : "-"; };
    out.append(id, id_len);
    num(query_len);
    num(n_hashes);
    num(candidates);
    num(n_segments);
    out += '\t';
    out += shape;
    num(path_hits);
    num(single);
    num(segment);
    num(start);
    num(end);
    num(breakpoint_base(start, query_len, n_hashes));
    num(breakpoint_base(end, query_len, n_hashes));        // end == n_hashes gives query_len
    name(ref);
    num(hits);
    name(best);
    num(best_hits);
    out += '\n';
}

// ---- `--base-positions`: the same header and the same line, with two columns appended.  base_start = pos of
// the segment's first hash; base_end = pos of its last hash + k, exclusive and at most query_len -- real bases
inline std::string segments_header_positions()
{
    std::string h = segments_header();
    h.pop_back();
    return h + "\tBASE_START\tBASE_END\n";
}

inline void segments_line_positions(std::string &out, const char *id, uint64_t id_len, uint64_t query_len, uint32_t n_hashes, uint32_t candidates, uint32_t n_segments,
                                    const char *shape, uint32_t path_hits, uint32_t single, uint32_t segment, uint32_t start, uint32_t end, breakpoint_ref ref, uint32_t hits,
                                    breakpoint_ref best, uint32_t best_hits, uint64_t base_start, uint64_t base_end)
{
    segments_line(out, id, id_len, query_len, n_hashes, candidates, n_segments, shape, path_hits, single, segment, start, end, ref, hits, best, best_hits);
    out.pop_back();                                    // the line's '\n'
    out += '\t';
    breakpoint_put_u64(out, base_start);
    out += '\t';
    breakpoint_put_u64(out, base_end);
    out += '\n';
}

}   // namespace taxor
