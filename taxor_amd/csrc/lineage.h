// lineage.h -- the taxonomy of an index as a tree (host only; `taxor search --lca-file / --report-file`, lca.hip).
//
// Every taxor_species carries taxid_string and taxnames_string, the ';'-separated path from superkingdom to species.  From them:
//   species of user bin b   the first species whose user_bin == b, species[0] if none (taxor_format_read's rule: the calls agree with
//                           the TSV's text)
//   fields                  ids = split(taxid_string, ';'), names = split(taxnames_string, ';'), no trailing empty field (profile_split);
//                           position d of ids pairs with position d of names
//   node                    a distinct non-empty id string; node numbers are dense, in byte-wise order of the id strings
//   name, rank              names[d] without its first three characters (empty if shorter than 3); names[d][0], '-' if the field is
//                           empty; the first occurrence in user-bin order decides
//   compacted path          b's non-empty ids as node numbers, root-down; a node's parent is its predecessor, the first node's is ROOT
//   ROOT                    a virtual node, id string "1", name "root", rank 'R'.  A compacted path whose first id is "1" starts AT
//                           ROOT: that id is ROOT itself and is not stored.  (The path's length below counts it.)
// Refused, with a message that names the ids and the accessions involved: an id with two different parents in two paths, an id twice in
// one path (a "1" anywhere but first is ROOT twice, or ROOT below a node), a compacted path longer than LINEAGE_MAX_DEPTH, names shorter
// than ids.  With single-parent paths the longest common prefix of two paths ends at their tree LCA; that is why.
#pragma once
#include "../../include/taxor_gpu.h"

#include <cstdint>
#include <map>
#include <string>
#include <vector>

namespace taxor {

constexpr uint32_t LINEAGE_MAX_DEPTH = 64;

struct Lineage {
    uint64_t n_bins = 0;
    uint32_t max_depth = 0;                 // the longest stored path
    std::vector<uint32_t> bin_species;      // [n_bins]
    std::vector<uint64_t> path_off;         // [n_bins + 1]
    std::vector<int32_t> path;              // node numbers, root-down
    std::vector<std::string> id, name;      // [n_nodes]
    std::vector<char> rank;                 // [n_nodes]
    std::vector<int32_t> parent;            // [n_nodes] node number, -1 = ROOT
    std::vector<uint32_t> depth;            // [n_nodes] 1 for ROOT's children
};

// profile_split's rule (profile_cmd.h): getline over ';' -- no trailing empty field
inline std::vector<std::string> lineage_split(const char *s)
{
    std::vector<std::string> out;
    if (!s) return out;
    const std::string str(s);
    size_t a = 0;
    while (a < str.size()) {
        const size_t e = str.find(';', a);
        if (e == std::string::npos) { out.push_back(str.substr(a)); break; }
        out.push_back(str.substr(a, e - a));
        a = e + 1;
    }
    return out;
}

// fills `out`; returns the refusal's message, empty if all went well
inline std::string lineage_build(const taxor_hixf_meta &m, uint64_t n_bins, Lineage &out)
{
    out = Lineage();
    out.n_bins = n_bins;
    out.bin_species.assign(n_bins, 0u);
    for (uint64_t i = m.n_species; i-- > 0;)
        if (m.species[i].user_bin < n_bins) out.bin_species[m.species[i].user_bin] = (uint32_t)i;
    struct Node { std::string name; char rank; std::string parent; const char *acc; };
    std::map<std::string, Node> nodes;                  // std::string orders bytes as unsigned: the project's byte-wise order
    std::vector<std::vector<std::string>> paths(n_bins);
    auto acc_of = [&](uint64_t b) { const char *a = m.species[out.bin_species[b]].accession_id; return a ? a : ""; };
    for (uint64_t b = 0; b < n_bins && m.n_species; ++b) {
        const taxor_species &sp = m.species[out.bin_species[b]];
        const std::vector<std::string> ids = lineage_split(sp.taxid_string), names = lineage_split(sp.taxnames_string);
        const std::string acc = acc_of(b);
        if (names.size() < ids.size())
            return "lineage: " + acc + " (user bin " + std::to_string(b) + ") has " + std::to_string(ids.size()) + " ids in \"" + (sp.taxid_string ? sp.taxid_string : "") +
                   "\" and only " + std::to_string(names.size()) + " names";
        std::vector<std::string> &p = paths[b];
        std::string prev;                               // the parent's id, empty = ROOT
        uint32_t len = 0;
        for (size_t d = 0; d < ids.size(); ++d) {
            if (ids[d].empty()) continue;
            if (++len > LINEAGE_MAX_DEPTH)
                return "lineage: the path of " + acc + " (user bin " + std::to_string(b) + ") has more than " + std::to_string(LINEAGE_MAX_DEPTH) + " ids (the " +
                       std::to_string(len) + "th is " + ids[d] + ")";
            if (ids[d] == "1") {
                if (len == 1) continue;                 // the path starts at ROOT itself
                return "lineage: id 1 is the root and stands below id " + prev + " in the path of " + acc + " (user bin " + std::to_string(b) + ")";
            }
            for (const std::string &q : p)
                if (q == ids[d]) return "lineage: id " + ids[d] + " occurs twice in the path of " + acc + " (user bin " + std::to_string(b) + ")";
            auto it = nodes.find(ids[d]);
            if (it == nodes.end())
                nodes.emplace(ids[d], Node{names[d].size() >= 3 ? names[d].substr(3) : std::string(), names[d].empty() ? '-' : names[d][0], prev, sp.accession_id});
            else if (it->second.parent != prev)
                return "lineage: id " + ids[d] + " has two parents: " + (it->second.parent.empty() ? "1" : it->second.parent) + " in the path of " +
                       (it->second.acc ? it->second.acc : "") + " and " + (prev.empty() ? "1" : prev) + " in the path of " + acc;
            p.push_back(ids[d]);
            prev = ids[d];
        }
    }
    std::map<std::string, int32_t> number;
    for (const auto &kv : nodes) {
        number.emplace(kv.first, (int32_t)out.id.size());
        out.id.push_back(kv.first);
        out.name.push_back(kv.second.name);
        out.rank.push_back(kv.second.rank);
    }
    out.parent.assign(out.id.size(), -1);
    out.depth.assign(out.id.size(), 0);
    out.path_off.assign(n_bins + 1, 0);
    for (uint64_t b = 0; b < n_bins; ++b) {
        int32_t prev = -1;
        for (size_t d = 0; d < paths[b].size(); ++d) {
            const int32_t x = number[paths[b][d]];
            out.path.push_back(x);
            out.parent[(size_t)x] = prev;
            out.depth[(size_t)x] = (uint32_t)d + 1;
            prev = x;
        }
        out.path_off[b + 1] = out.path.size();
        if (paths[b].size() > out.max_depth) out.max_depth = (uint32_t)paths[b].size();
    }
    return std::string();
}

} // namespace taxor
