"""What `taxor search --lca-confidence` must give, restated in Python from the definitions in include/taxor_gpu_tools.h alone: paths are
lists of id strings (tests/lca_expect.py), "hash h matches user bin b" is tests/coverage_expect.Expect.matches (the oracle's rows and
fingerprint), and support, the climb and the file's text are Python ints and floats.  Nothing is taken from confidence.hip."""
import numpy as np

from tests import lca_expect as le

CALL_HEADER = "#STATUS\tQUERY_NAME\tTAXID\tQUERY_LEN\tQHASH_COUNT\tBEST_QHASH_MATCH\tREFERENCES\tSUPPORT\tLCA_TAXID\tLCA_SUPPORT\n"


def common_prefix(p, q):
    k = 0
    while k < len(p) and k < len(q) and p[k] == q[k]:
        k += 1
    return k


def holds(support, C, n):
    return not (float(support) < float(C) * float(n))


def call(lineage, cov, C, tuples, hashes):
    """one read: tuples [(user bin, count)] -- ALL of them -- and its ordered hash list -> a dict of everything the library hands back,
    nodes as id strings ("1" ROOT, "0" unclassified)"""
    n = len(hashes)
    out = dict(node="0", depth=0, lca_node="0", lca_depth=0, support=0, lca_support=0, any_support=0, best=0, n_refs=0, n_hashes=n)
    mx = max([c for _, c in tuples], default=0)
    if mx == 0:
        return out
    surv = [lineage.paths[b] for b, c in tuples if le.keeps(c, mx)]
    P = list(surv[0])
    for p in surv[1:]:
        P = P[:common_prefix(P, p)]
    D = len(P)
    a = [None] * n
    h = np.asarray(hashes, np.uint64)
    agree = {}
    for b, _ in tuples:
        agree[b] = common_prefix(lineage.paths[b], P)
    for b, ag in agree.items():
        if n:
            for i in np.flatnonzero(cov.matches(b, h)):
                a[i] = ag if a[i] is None else max(a[i], ag)
    support = [sum(1 for x in a if x is not None and x >= d) for d in range(D + 1)]
    assert all(support[d] >= support[d + 1] for d in range(D))
    out.update(lca_node=P[-1] if P else "1", lca_depth=D, lca_support=support[D], any_support=support[0], best=mx, n_refs=len(surv))
    for d in range(D, -1, -1):
        if holds(support[d], C, n):
            out.update(node=P[d - 1] if d else "1", depth=d, support=support[d])
            return out
    out.update(support=support[0])                     # the threshold made it unclassified
    return out


def outcome(c):
    """never | stays | climbs <levels> | root | dropped"""
    if c["lca_node"] == "0":
        return "never"
    if c["node"] == "0":
        return "dropped"
    if c["depth"] == c["lca_depth"]:
        return "stays"
    return "root" if c["depth"] == 0 else "climbs %d" % (c["lca_depth"] - c["depth"])


class Expect:
    """reads added one by one; the per-read calls and the two tallies at the confident nodes by id string"""

    def __init__(self, lineage, cov, C):
        self.lin, self.cov, self.C = lineage, cov, C
        self.calls = []
        self.reads, self.bases = {}, {}

    def add(self, tuples, hashes, read_len):
        c = call(self.lin, self.cov, self.C, tuples, hashes)
        self.calls.append(c)
        self.reads[c["node"]] = self.reads.get(c["node"], 0) + 1
        self.bases[c["node"]] = self.bases.get(c["node"], 0) + int(read_len)
        return c

    def add_bases(self, reads, **kw):
        """reads as dna4-normalised bytes: the oracle's search gives all tuples, its syncmers the ordered hash lists"""
        from oracle import oracle as orc
        B = np.frombuffer(b"".join(reads), np.uint8)
        O = np.cumsum([0] + [len(r) for r in reads]).astype(np.uint64)
        nh, off, ub, cnt, _ = self.cov.oracle.search_batch(B, O, threads=4, **kw)
        out = []
        for i, r in enumerate(reads):
            lo, hi = int(off[i]), int(off[i + 1])
            hashes = orc.seq_to_syncmers(r) if len(r) else np.zeros(0, np.uint64)
            assert hashes.size == int(nh[i])
            out.append(self.add([(int(b), int(c)) for b, c in zip(ub[lo:hi], cnt[lo:hi])], hashes, len(r)))
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

    def arrays(self):
        """the words as the library numbers them"""
        num = self.lin.node_number
        f = lambda k: [c[k] for c in self.calls]
        return dict(node=[num(x) for x in f("node")], depth=f("depth"), lca_node=[num(x) for x in f("lca_node")], lca_depth=f("lca_depth"), support=f("support"),
                    lca_support=f("lca_support"), any_support=f("any_support"), best=f("best"), n_refs=f("n_refs"), n_hashes=f("n_hashes"))


def same(got, exp, lo=0, hi=None):
    """a Confidence.add_* result equals the expectation's calls [lo, hi), array for array"""
    want = exp.arrays()
    for k, w in want.items():
        g = [int(x) for x in getattr(got, k)]
        assert g == w[lo:hi], (k, [(i, a, b) for i, (a, b) in enumerate(zip(g, w[lo:hi])) if a != b][:8])


def same_tallies(t, exp):
    dr, db = exp.tally_arrays()
    assert [int(x) for x in t.direct_reads] == dr
    assert [int(x) for x in t.direct_bases] == db
    assert t.n_reads == len(exp.calls)


def call_line(c, name, read_len):
    if c["lca_node"] == "0":
        return f"U\t{name}\t0\t{read_len}\t0\t0\t0\t0\t0\t0\n"
    status = "U" if c["node"] == "0" else "C"
    return f"{status}\t{name}\t{c['node']}\t{read_len}\t{c['n_hashes']}\t{c['best']}\t{c['n_refs']}\t{c['support']}\t{c['lca_node']}\t{c['lca_support']}\n"


def files(exp, names, read_lens, unit="reads"):
    """(call file text, report text) of the reads added"""
    text = CALL_HEADER + "".join(call_line(c, nm, ln) for c, nm, ln in zip(exp.calls, names, read_lens))
    return text, le.report(exp.lin, exp.reads if unit == "reads" else exp.bases)
