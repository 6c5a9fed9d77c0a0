#!/usr/bin/env python3
"""Writes tests/golden/profile/: seeded synthetic search TSVs and what the REFERENCE's `taxor profile` writes for them (CAMI profile,
sequence abundances, binning file), read by tests/test_gpu_profile.py.  The reference's src/main/taxor_profile.cpp is compiled
where it lies, into a scratch directory outside the repository, against small stand-in headers written by this script (an
argument-parser shell, ankerl::unordered_dense::set over std::unordered_set, empty seqan3/utility headers).  Nothing of the
reference's text is stored, only the inputs and its answers.

Every case is also run through a second build with libstdc++'s debug mode and the host sanitizers: the reference leaves three
situations undefined (erasing a default-constructed iterator when no match of a multi-match read has a prior; an explained-by
cycle, on which its chain resolution never ends; a "-" line among several matches), and a golden case must hold none of them.
The checked build aborts on the first, the time limit catches the second, the TSV itself is inspected for the third.

Run:  python tests/golden/make_profile_golden.py [reference checkout, default /root/reference]"""
import json
import os
import random
import shutil
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "profile")
HEADER = "#QUERY_NAME\tACCESSION\tREFERENCE_NAME\tTAXID\tREF_LEN\tQUERY_LEN\tQHASH_COUNT\tQHASH_MATCH\tTAX_STR\tTAX_ID_STR\n"

ARGPARSE = r"""
#pragma once
#include <algorithm>
#include <cstdint>
#include <fstream>
#include <functional>
#include <iostream>
#include <map>
#include <set>
#include <sstream>
#include <stdexcept>
#include <string>
#include <vector>
namespace seqan3 {
struct argument_parser_error : std::runtime_error { using std::runtime_error::runtime_error; };
enum class option_spec { standard, required, advanced, hidden };
template <class T> struct arithmetic_range_validator {
    T lo, hi;
    arithmetic_range_validator(T a, T b) : lo(a), hi(b) {}
};
struct no_validator {};
class argument_parser {
    struct opt { std::string name; bool flag, required, seen; std::function<void(const std::string &)> set; };
    std::vector<opt> opts_;
    std::vector<std::string> args_;
public:
    struct { std::string version, author, email, short_description; std::vector<std::string> description; } info;
    argument_parser(const std::string &, int argc, char **argv) { for (int i = 1; i < argc; ++i) args_.push_back(argv[i]); }
    void add_subsection(const std::string &) {}
    template <class T, class V = no_validator>
    void add_option(T &value, char, const std::string &name, const std::string &, option_spec spec = option_spec::standard, V v = V{})
    {
        opts_.push_back({name, false, spec == option_spec::required, false, [&value, v, name](const std::string &s) {
            if constexpr (std::is_same_v<T, std::string>) value = s;
            else {
                std::istringstream is(s);
                T x{};
                if (!(is >> x) || !is.eof()) throw argument_parser_error("Value parse failed for --" + name);
                if constexpr (!std::is_same_v<V, no_validator>)
                    if (x < (T)v.lo || x > (T)v.hi) throw argument_parser_error("Validation failed for option --" + name);
                value = x;
            }
        }});
    }
    void add_flag(bool &value, char, const std::string &name, const std::string &, option_spec = option_spec::standard)
    {
        opts_.push_back({name, true, false, false, [&value](const std::string &) { value = true; }});
    }
    void parse()
    {
        for (size_t i = 0; i < args_.size(); ++i) {
            auto it = std::find_if(opts_.begin(), opts_.end(), [&](const opt &o) { return "--" + o.name == args_[i]; });
            if (it == opts_.end()) throw argument_parser_error("Unknown option " + args_[i]);
            it->seen = true;
            if (it->flag) it->set("");
            else {
                if (i + 1 >= args_.size()) throw argument_parser_error("Missing value for option " + args_[i]);
                it->set(args_[++i]);
            }
        }
        for (const opt &o : opts_)
            if (o.required && !o.seen) throw argument_parser_error("Option --" + o.name + " is required but not set.");
    }
};
}   // namespace seqan3
"""

ANKERL = r"""
#pragma once
#include <unordered_set>
namespace ankerl::unordered_dense {
template <class K> class set : public std::unordered_set<K> {};
}
"""

DRIVER = r"""
#include <seqan3/argument_parser/all.hpp>
namespace taxor::profile { int execute(seqan3::argument_parser &parser); }
int main(int argc, char **argv)
{
    seqan3::argument_parser parser{"taxor-profile", argc, argv};
    return taxor::profile::execute(parser);
}
"""


def build_reference(ref, work):
    inc = os.path.join(work, "standin")
    for rel, text in (("seqan3/argument_parser/all.hpp", ARGPARSE), ("seqan3/utility/views/chunk.hpp", "#pragma once\n"),
                      ("seqan3/utility/range/to.hpp", "#pragma once\n"), ("ankerl/unordered_dense.h", ANKERL)):
        path = os.path.join(inc, rel)
        os.makedirs(os.path.dirname(path), exist_ok=True)
        open(path, "w").write(text)
    open(os.path.join(work, "driver.cpp"), "w").write(DRIVER)
    src = os.path.join(ref, "src", "main", "taxor_profile.cpp")
    base = ["g++", "-std=c++20", "-w", "-I", inc, "-I", os.path.join(ref, "src", "main"), "-I", os.path.join(ref, "src", "taxonomy"),
            src, os.path.join(work, "driver.cpp")]
    plain, checked = os.path.join(work, "ref_profile"), os.path.join(work, "ref_profile_checked")
    subprocess.check_call(base + ["-O2", "-o", plain])
    subprocess.check_call(base + ["-O1", "-g", "-D_GLIBCXX_DEBUG", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", checked])
    return plain, checked


# ---- synthetic search results ---------------------------------------------------------------------------------------------------
class Case:
    def __init__(self, name, seed, args=()):
        self.name, self.args, self.rng = name, list(args), random.Random(seed)
        self.lines, self.species, self.n = [], {}, 0

    def sp(self, acc, genus=1, ref_len=None, tax=None):
        """declare a species; tax = (TAX_STR, TAX_ID_STR) overrides the generated path"""
        i = len(self.species) + 1
        tax = tax or (f"k__B;f__F;g__G{genus};s__S{i}", f"2;6;7{genus};10{i}")
        self.species[acc] = (f"10{i}", ref_len or self.rng.randrange(2, 9) * 1000000, tax)
        return acc

    def read(self, hits, name=None, qlen=None, count=None, match=None):
        """one read; hits = accessions in file order (none: a '-' line); match = per-hit QHASH_MATCH"""
        self.n += 1
        name = name or f"r{self.n}"
        qlen = qlen or self.rng.randrange(900, 9000)
        count = count or qlen // 11
        if not hits:
            self.lines.append(f"{name}\t-\t-\t-\t-\t{qlen}\n")
        for j, acc in enumerate(hits):
            taxid, ref_len, tax = self.species[acc]
            m = match[j] if match else self.rng.randrange(count // 3, count) + 1
            self.lines.append(f"{name}\t{acc}\tn\t{taxid}\t{ref_len}\t{qlen}\t{count}\t{m}\t{tax[0]}\t{tax[1]}\n")

    def text(self):
        return HEADER + "".join(self.lines)


def case_unique(name="unique", args=()):
    c = Case(name, 1, args)
    accs = [c.sp(f"GCF_{i}", genus=i % 3) for i in (3, 12, 1, 100, 25, 7)]
    for i in range(120):
        c.read([accs[i % 6 if i % 5 else 0]])
    for i in range(9):
        c.read([])
    return c


def case_round1():
    c = Case("round1", 2)
    a, b, d = c.sp("A1"), c.sp("B1"), c.sp("D1", genus=2)
    u, v = c.sp("U1", genus=2), c.sp("V1", genus=3)               # never hit alone
    for i in range(20):
        c.read([(a, b, d)[i % 3]])
    for i in range(30):
        c.read([u, (a, b, d)[i % 3], v] if i % 2 else [(a, b)[i % 2], u, d])
    for i in range(8):
        c.read([u, v])                                            # no flagged reference: the read stays as it is
    c.read([])
    return c


def case_round2():
    c = Case("round2", 3)
    a, b = c.sp("A2"), c.sp("B2", genus=2)
    few, thin = c.sp("FEW2", genus=2), c.sp("THIN2", genus=3)     # 2 unique reads; 3 unique among > 300 mappings
    for i in range(40):
        c.read([(a, b)[i % 2]])
    c.read([few]), c.read([few])
    for i in range(3):
        c.read([thin])
    for i in range(150):
        c.read([thin, (a, b)[i % 2]] if i % 3 else [(a, b)[i % 2], thin, few])
    for i in range(150):
        c.read([thin, b, a])
    return c


def case_explained():
    """no read is unique here, so rounds 1 and 2 remove nothing; E4 and E4b each hold a few reads more than E4a and share all but
    two (one) of them with it: both are explained by E4a"""
    c = Case("explained", 4)
    e, x, e2, y = c.sp("E4"), c.sp("E4a", genus=2), c.sp("E4b", genus=2), c.sp("Y4", genus=3)
    for i in range(60):
        c.read([e, x, e2] if i % 2 else [e2, x, e])               # erased: the explaining reference is in the read
    c.read([e, y])                                                # renamed
    c.read([y, e2, e])                                            # both renamed: the same reference twice in one read
    return c


def case_chain():
    c = Case("chain", 5)
    a, b, d, z = c.sp("CH_A"), c.sp("CH_B", genus=2), c.sp("CH_C", genus=2), c.sp("CH_Z", genus=3)
    for i in range(40):
        c.read([a, b, d] if i % 2 else [d, a, b])
    c.read([a, b, z])                                             # a and b renamed, to the same end of the chain
    c.read([a, z])
    return c


def case_ties():
    c = Case("ties", 6)
    p, q, s = c.sp("T_P"), c.sp("T_Q", genus=2), c.sp("T_S", genus=3)
    for i in range(45):
        c.read([(p, q, s)[i % 3]])
    for i in range(25):
        qlen = 2000 + 10 * i
        c.read([p, q] if i % 2 else [q, s, p], qlen=qlen, count=180, match=[120, 120, 120][:2 + (i + 1) % 2])
    for i in range(10):
        c.read([q, p], qlen=3000, count=250, match=[200, 150])
    return c


def case_many(name="many", args=()):
    c = Case(name, 7, args)
    accs = [c.sp(f"M{i}", genus=i % 4) for i in range(40)]
    for i in range(120):
        c.read([accs[i % 40]])
    for i in range(12):
        order = accs[:]
        c.rng.shuffle(order)
        c.read(order, qlen=8000, count=700, match=c.rng.sample(range(200, 690), 40))
    for i in range(30):
        c.read(c.rng.sample(accs, 3))
    return c


def case_names():
    c = Case("names", 8)
    a = c.sp("N_A", tax=("k__Bacteria;p__;c__Gamma;o__;f__Entero;g__Esch;s__E coli", "2;;1236;;543;561;562"))
    b = c.sp("N_B", tax=("k__Bacteria;p__Proteo;c__Gamma;o__;f__Entero;g__Esch;s__E albertii", "2;1224;1236;;543;561;208962"))
    d = c.sp("N_C", tax=("k__Archaea;p__Eury;c__;o__;f__;g__;s__M smithii", "2157;28890;;;;;2173"))
    for i in range(30):
        c.read([(a, b, d)[i % 3]], name=f"read_{i} runid=ab{i} ch={i % 7}")
    c.read([a], name="pair_1 first", qlen=4000, count=300)
    c.read([b], name="pair_1 second", qlen=4000, count=300)                            # one read id once cut at the space: two matches
    for i in range(10):
        c.read([a, b], name=f"read_{100 + i} runid=x")
    c.read([], name="read_9 nothing here")
    return c


def cases():
    many = case_many()
    uni = case_unique()
    out = [uni, case_round1(), case_round2(), case_explained(), case_chain(), case_ties(), many, case_names()]
    out.append(case_many("many_em1", ["--em-steps", "1"]))
    out.append(case_unique("unique_min0", ["--min-abundance", "0"]))
    out.append(case_unique("unique_min05", ["--min-abundance", "0.5"]))
    out.append(case_many("many_min0", ["--min-abundance", "0"]))
    return out


def dash_among_matches(text):
    first = {}
    for line in text.splitlines()[1:]:
        f = line.split("\t")
        rid = f[0].split(" ")[0]
        if rid in first and first[rid] == "-" and f[1] != "-":
            return True
        first.setdefault(rid, f[1])
    return False


def main():
    ref = sys.argv[1] if len(sys.argv) > 1 else "/root/reference"
    work = tempfile.mkdtemp(prefix="profile_golden_")
    try:
        plain, checked = build_reference(ref, work)
        if os.path.isdir(OUT):
            shutil.rmtree(OUT)
        os.makedirs(OUT)
        index, written = [], {}
        for c in cases():
            text = c.text()
            assert not dash_among_matches(text), c.name
            tsv = [k for k, v in written.items() if v == text]
            if tsv:
                tsv = tsv[0]
            else:
                tsv = c.name + ".tsv"
                written[tsv] = text
                open(os.path.join(OUT, tsv), "w").write(text)
            outs = {}
            for tag, exe in (("ref", plain), ("chk", checked)):
                d = os.path.join(work, c.name + "_" + tag)
                os.makedirs(d)
                cmd = [exe, "--search-file", os.path.join(OUT, tsv), "--cami-report-file", os.path.join(d, "cami"), "--seq-abundance-file",
                       os.path.join(d, "seq"), "--binning-file", os.path.join(d, "bin"), "--sample-id", "S_" + c.name] + c.args
                cp = subprocess.run(cmd, capture_output=True, text=True, timeout=120)        # a cycle never ends: the limit is the check
                assert cp.returncode == 0, (c.name, tag, cp.returncode, cp.stderr[-2000:])
                outs[tag] = {k: open(os.path.join(d, k)).read() for k in ("cami", "seq", "bin")}
                steps = [ln for ln in cp.stdout.splitlines() if ln.startswith("Number of EM steps needed")]
                outs[tag]["steps"] = steps[-1]
            assert outs["ref"] == outs["chk"], c.name
            for k in ("cami", "seq", "bin"):
                open(os.path.join(OUT, f"{c.name}.{k}"), "w").write(outs["ref"][k])
            index.append(dict(name=c.name, tsv=tsv, args=c.args, sample_id="S_" + c.name, em_steps_line=outs["ref"]["steps"]))
            print(c.name, outs["ref"]["steps"], len(text), "bytes", file=sys.stderr)
        json.dump(index, open(os.path.join(OUT, "cases.json"), "w"), indent=1)
        total = sum(os.path.getsize(os.path.join(OUT, f)) for f in os.listdir(OUT))
        assert total < 200 * 1024, total
        print("total", total, "bytes", file=sys.stderr)
    finally:
        shutil.rmtree(work, ignore_errors=True)


if __name__ == "__main__":
    main()
