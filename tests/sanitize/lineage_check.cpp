// lineage_check.cpp -- the lineage builder (taxor_amd/csrc/lineage.h) under ASan + UBSan over its edge inputs: empty fields in the middle
// and at the front of a path, paths of 1, 7 and 64 nodes, 65 refused, a path starting with "1", a user bin without a species, two
// species sharing a user bin, names shorter than 3, null strings, and every refusal.  Prints "ok <checks>" or the first failure.
#include "lineage.h"

#include <cstdio>
#include <cstring>

#define CHECK(x)                                                        \
    do {                                                                \
        ++checks;                                                       \
        if (!(x)) { printf("FAILED line %d: %s\n", __LINE__, #x); return 1; } \
    } while (0)

static taxor_species sp(uint64_t ub, const char *ids, const char *names, const char *acc)
{
    return taxor_species{"organism", acc, "0", names, ids, ub, 1000};
}

static std::string build(const std::vector<taxor_species> &v, uint64_t n_bins, taxor::Lineage &l)
{
    taxor_hixf_meta m{};
    m.n_species = v.size();
    m.species = v.data();
    return taxor::lineage_build(m, n_bins, l);
}

int main()
{
    using namespace taxor;
    uint64_t checks = 0;
    Lineage l;
    std::string ids64, names64;
    for (int i = 0; i < 64; ++i) {
        ids64 += (i ? ";" : "") + std::to_string(5000 + i);
        names64 += (i ? ";x__N" : "x__N") + std::to_string(i);
    }
    {
        std::vector<taxor_species> v{sp(0, "77", "s__Lonely", "A0"),
                                     sp(1, "2;1224;1236;91347;543;561;562", "k__B;p__P;c__G;o__E;f__E;g__E;s__E coli", "A1"),
                                     sp(2, ids64.c_str(), names64.c_str(), "A2"),
                                     sp(3, "2;;9236;;9543", "k__B;p__;c__G;;f__E", "A3"),
                                     sp(4, ";;1239;91061", "k__;p__;c__F;o__B", "A4"),
                                     sp(5, "", "", "A5"),
                                     sp(6, ";;", ";;", "A6"),
                                     sp(6, "2;4242", "k__B;s__never looked at", "A6b"),
                                     sp(9, "1;2;1224", "x__root;k__B;p__P", "A9"),
                                     sp(10, "9;9a", "k_;s", "A10"),
                                     sp(11, nullptr, nullptr, "A11")};
        CHECK(build(v, 13, l).empty());
        CHECK(l.n_bins == 13 && l.max_depth == 64 && l.path_off.size() == 14);
        CHECK(l.path_off[1] - l.path_off[0] == 1 && l.path_off[2] - l.path_off[1] == 7 && l.path_off[3] - l.path_off[2] == 64);
        CHECK(l.path_off[4] - l.path_off[3] == 3 && l.path_off[5] - l.path_off[4] == 2);
        CHECK(l.path_off[6] == l.path_off[5] && l.path_off[7] == l.path_off[6]);
        CHECK(l.bin_species[7] == 0 && l.bin_species[8] == 0 && l.bin_species[6] == 6);            // no species: species[0]; the first of two wins
        CHECK(l.path_off[8] - l.path_off[7] == 1);                                                  // bin 7 falls back to species 0's path
        CHECK(l.path_off[10] - l.path_off[9] == 2);                                                 // the leading "1" is ROOT itself
        CHECK(l.path_off[12] == l.path_off[11] + 0 && l.path_off[13] - l.path_off[12] == 1);
        for (size_t i = 1; i < l.id.size(); ++i) CHECK(l.id[i - 1] < l.id[i]);
        for (size_t i = 0; i < l.id.size(); ++i) {
            CHECK(l.id[i] != "1" && l.id[i] != "4242");
            CHECK(l.parent[i] >= -1 && l.parent[i] < (int32_t)l.id.size());
            CHECK(l.depth[i] == (l.parent[i] < 0 ? 1u : l.depth[(size_t)l.parent[i]] + 1));
            if (l.id[i] == "9") CHECK(l.name[i].empty() && l.rank[i] == 'k');
            if (l.id[i] == "9a") CHECK(l.name[i].empty() && l.rank[i] == 's');
            if (l.id[i] == "9236") CHECK(l.name[i] == "G" && l.rank[i] == 'c');
            if (l.id[i] == "1239") CHECK(l.parent[i] == -1);
        }
        for (int32_t x : l.path) CHECK(x >= 0 && x < (int32_t)l.id.size());
    }
    {   // no species at all, no bins at all
        CHECK(build({}, 4, l).empty() && l.id.empty() && l.path.empty() && l.path_off.size() == 5);
        CHECK(build({sp(0, "2", "k__B", "A")}, 0, l).empty() && l.path_off.size() == 1);
    }
    {   // the refusals
        std::string e = build({sp(0, (ids64 + ";6000").c_str(), (names64 + ";x__last").c_str(), "DEEP")}, 1, l);
        CHECK(e.find("more than 64 ids") != std::string::npos && e.find("DEEP") != std::string::npos && e.find("6000") != std::string::npos);
        e = build({sp(0, ("1;" + ids64).c_str(), ("x__r;" + names64).c_str(), "DEEP1")}, 1, l);
        CHECK(e.find("more than 64 ids") != std::string::npos);
        e = build({sp(0, "2;1224;1236", "k__B;p__P;c__G", "PA"), sp(1, "2;;1236", "k__B;p__;c__G", "PB")}, 2, l);
        CHECK(e.find("id 1236 has two parents") != std::string::npos && e.find("PA") != std::string::npos && e.find("PB") != std::string::npos && e.find("1224") != std::string::npos);
        e = build({sp(0, "2;1224", "k__B;p__P", "PA"), sp(1, "1224", "p__P", "PB")}, 2, l);
        CHECK(e.find("id 1224 has two parents: 2 in the path of PA and 1 in the path of PB") != std::string::npos);
        e = build({sp(0, "2;1224;2", "k__B;p__P;c__B", "TW")}, 1, l);
        CHECK(e.find("id 2 occurs twice") != std::string::npos && e.find("TW") != std::string::npos);
        e = build({sp(0, "2;1;1224", "k__B;x__r;p__P", "RT")}, 1, l);
        CHECK(e.find("id 1 is the root") != std::string::npos && e.find("RT") != std::string::npos);
        e = build({sp(0, "2;1224;1236", "k__B;p__P", "SH")}, 1, l);
        CHECK(e.find("3 ids") != std::string::npos && e.find("only 2 names") != std::string::npos && e.find("SH") != std::string::npos);
        e = build({sp(0, "2;1224", nullptr, "NN")}, 1, l);
        CHECK(e.find("only 0 names") != std::string::npos);
    }
    printf("ok %llu\n", (unsigned long long)checks);
    return 0;
}
