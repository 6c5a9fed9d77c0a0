"""What `taxor search --lca-file / --report-file` must give, restated in Python from the definitions in include/taxor_gpu_tools.h
(the lineage, the per-read lowest common ancestor, the tallies, the clade roll-up and both file formats).  Nothing here is taken from
taxor_amd/csrc/lca.hip or lineage.h: nodes are id STRINGS, paths are lists of strings, and the node numbers are derived last."""

ROOT, UNCLASSIFIED = -1, -2
MAX_DEPTH = 64
CALL_HEADER = "#STATUS\tQUERY_NAME\tTAXID\tQUERY_LEN\tQHASH_COUNT\tBEST_QHASH_MATCH\tREFERENCES\n"
RANK_CODE = {"k": "D", "p": "P", "c": "C", "o": "O", "f": "F", "g": "G", "s": "S"}


class Refused(Exception):
    pass


def split(s):
    """profile_split: fields between ';', no trailing empty field"""
    parts = s.split(";")
    if parts and parts[-1] == "":
        parts.pop()
    return parts


def compact(taxid_string):
    """the non-empty ids, root-down, without a leading "1" (that id is ROOT itself)"""
    p = [x for x in split(taxid_string) if x != ""]
    return p[1:] if p and p[0] == "1" else p


class Lineage:
    def __init__(self, species, n_user_bins):
        by_bin = {}
        for i, s in enumerate(species):
            by_bin.setdefault(s["user_bin"], i)
        self.bin_species = [by_bin.get(b, 0) for b in range(n_user_bins)]
        self.paths, self.parent, self.name, self.rank = [], {}, {}, {}
        first_acc = {}
        for b in range(n_user_bins):
            if not species:
                self.paths.append([])
                continue
            sp = species[self.bin_species[b]]
            ids, names = split(sp["taxid_string"]), split(sp["taxnames_string"])
            if len(names) < len(ids):
                raise Refused(f"{sp['accession_id']}: {len(ids)} ids, only {len(names)} names")
            kept = [(x, names[d]) for d, x in enumerate(ids) if x != ""]
            if len(kept) > MAX_DEPTH:
                raise Refused(f"{sp['accession_id']}: more than {MAX_DEPTH} ids")
            if kept and kept[0][0] == "1":
                kept = kept[1:]
            path, prev = [], ""
            for x, nm in kept:
                if x == "1":
                    raise Refused(f"{sp['accession_id']}: id 1 is the root and stands below id {prev}")
                if x in path:
                    raise Refused(f"{sp['accession_id']}: id {x} occurs twice")
                if x not in self.parent:
                    self.parent[x], self.name[x], self.rank[x] = prev, nm[3:] if len(nm) >= 3 else "", nm[0] if nm else "-"
                    first_acc[x] = sp["accession_id"]
                elif self.parent[x] != prev:
                    raise Refused(f"id {x} has two parents: {self.parent[x] or '1'} ({first_acc[x]}) and {prev or '1'} ({sp['accession_id']})")
                path.append(x)
                prev = x
            self.paths.append(path)
        self.ids = sorted(self.parent, key=lambda x: x.encode())           # byte-wise
        self.number = {x: i for i, x in enumerate(self.ids)}

    def node_number(self, x):
        """an id string, "1" (ROOT) or "0" (unclassified) as the library numbers it"""
        return ROOT if x == "1" else UNCLASSIFIED if x == "0" else self.number[x]

    def depth(self, x):
        d = 0
        while x != "":
            x = self.parent[x]
            d += 1
        return d


def keeps(c, mx):
    return not (float(c) < float(mx) * 0.8)


def call_paths(paths_and_counts):
    """[(path as id strings, count)] of one read -> (taxid string, best, n_refs); "1" is ROOT, "0" unclassified"""
    if not paths_and_counts:
        return "0", 0, 0
    mx = max(c for _, c in paths_and_counts)
    if mx == 0:
        return "0", 0, 0
    surv = [p for p, c in paths_and_counts if keeps(c, mx)]
    common = list(surv[0])
    for p in surv[1:]:
        k = 0
        while k < len(common) and k < len(p) and common[k] == p[k]:
            k += 1
        common = common[:k]
    return (common[-1] if common else "1"), mx, len(surv)


class Expect:
    """reads added one by one; the per-read calls and the two tallies by id string"""

    def __init__(self, lineage):
        self.lin = lineage
        self.calls = []                    # (taxid string, best, n_refs)
        self.reads, self.bases = {}, {}

    def add(self, tuples, read_len):
        """tuples: [(user bin, count)]"""
        t = call_paths([(self.lin.paths[b], c) for b, c in tuples])
        self.calls.append(t)
        self.reads[t[0]] = self.reads.get(t[0], 0) + 1
        self.bases[t[0]] = self.bases.get(t[0], 0) + int(read_len)
        return t

    def add_csr(self, read_off, user_bin, count, query_len):
        out = []
        for r in range(len(read_off) - 1):
            lo, hi = int(read_off[r]), int(read_off[r + 1])
            out.append(self.add([(int(user_bin[i]), int(count[i])) for i in range(lo, hi)], int(query_len[r])))
        return out

    def tally_arrays(self):
        """(direct_reads, direct_bases) as lists of n_nodes + 2: the nodes, ROOT, UNCLASSIFIED"""
        n = len(self.lin.ids)
        out = []
        for d in (self.reads, self.bases):
            a = [0] * (n + 2)
            for x, v in d.items():
                a[n if x == "1" else n + 1 if x == "0" else self.lin.number[x]] += v
            out.append(a)
        return out


def call_line(status_id, name, read_len, n_hashes, best, n_refs):
    if status_id == "0":
        return f"U\t{name}\t0\t{read_len}\t0\t0\t0\n"
    return f"C\t{name}\t{status_id}\t{read_len}\t{n_hashes}\t{best}\t{n_refs}\n"


def report(lineage, direct):
    """Kraken-style report from {id string: direct count} ("1" ROOT, "0" unclassified)"""
    total = sum(direct.values())
    if total == 0:
        return ""
    children = {}
    for x, p in lineage.parent.items():
        children.setdefault(p, []).append(x)
    clade = {}

    def roll(x):
        c = direct.get(x if x != "" else "1", 0)
        for ch in children.get(x, []):
            c += roll(ch)
        clade[x] = c
        return c

    import sys
    sys.setrecursionlimit(10000)
    roll("")
    out = ""
    u = direct.get("0", 0)
    if u:
        out += "%6.2f\t%d\t%d\tU\t0\tunclassified\n" % (100.0 * u / total, u, u)

    def emit(x, depth):
        nonlocal out
        if clade[x] == 0:
            return
        if x == "":
            out += "%6.2f\t%d\t%d\tR\t1\troot\n" % (100.0 * clade[x] / total, clade[x], direct.get("1", 0))
        else:
            out += "%6.2f\t%d\t%d\t%s\t%s\t%s%s\n" % (100.0 * clade[x] / total, clade[x], direct.get(x, 0), RANK_CODE.get(lineage.rank[x], "-"), x,
                                                      "  " * depth, lineage.name[x])
        for ch in sorted(children.get(x, []), key=lambda y: (-clade[y], y.encode())):
            emit(ch, depth + 1)

    emit("", 0)
    return out


def from_tsv(tsv_text):
    """the TSV of a run -> per read, in the TSV's order: (name, read_len, n_hashes, [(path as id strings, count)]).  The lines of a
    read are the survivors of the 0.8 * max filter; their TAX_ID_STR gives the path."""
    reads, index = [], {}
    prev = None
    for line in tsv_text.splitlines():
        if line.startswith("#") or not line:
            continue
        f = line.split("\t")
        name = f[0]
        if name != prev or name not in index:
            reads.append([name, int(f[5]), 0, []])
            index[name] = len(reads) - 1
            prev = name
        r = reads[-1]
        if f[1] != "-":
            r[2] = int(f[6])
            r[3].append((compact(f[9]), int(f[7])))
    return reads


def files_from_tsv(lineage, tsv_text, unit="reads"):
    """(call file text, report text) a run must write, from its own TSV"""
    calls = CALL_HEADER
    direct = {}
    for name, read_len, n_hashes, pc in from_tsv(tsv_text):
        x, best, n_refs = call_paths(pc)
        calls += call_line(x, name, read_len, n_hashes, best, n_refs)
        direct[x] = direct.get(x, 0) + (1 if unit == "reads" else read_len)
    return calls, report(lineage, direct)
