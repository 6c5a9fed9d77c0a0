"""The restatement of the segments (taxor_amd/csrc/segments.hip, include/taxor_gpu_tools.h), from the oracle and tests/coverage_expect.py
alone: a read's tuples, its ordered hash list and the lookup of a hash in a user bin's leaf bins are tests/breakpoint_expect.py's
sources.  Everything else is Python ints: the recurrence as the header writes it, with its tie rules, and -- independently -- a brute
force over all M^n paths that returns the greatest value.  Shared by the segments tests."""
import itertools

import numpy as np

from oracle import oracle as orc
from tests.coverage_expect import Expect as CovExpect

COLUMNS = ("#QUERY_NAME\tQUERY_LEN\tQHASH_COUNT\tCANDIDATES\tSEGMENTS\tSHAPE\tPATH_HITS\tSINGLE_HITS\tSEGMENT\tHASH_START\tHASH_END\tBASE_START_APPROX\tBASE_END_APPROX\t"
           "ACCESSION\tTAXID\tHITS\tBEST_ACCESSION\tBEST_TAXID\tHITS_OF_BEST\n")
WORDS = ("n_candidates", "n", "n_segments", "path_hits", "path_switches", "single", "tuple_best", "bin_best")
ZERO = dict(examined=False, segs=[], **{f: 0 for f in WORDS})
W = 1 << 32


def base(p, query_len, n):
    """the approximate base position of hash p of n"""
    return (int(p) * int(query_len)) // int(n) if n else 0


def score(x, s, L):
    """value(s) from the definition: x[c][i] in {0, 1}, s a path"""
    hits = sum(x[s[i]][i] for i in range(len(s)))
    switches = sum(1 for i in range(1, len(s)) if s[i] != s[i - 1])
    return (hits - L * switches) * W - switches


def brute(x, L):
    """the greatest value over all M^n paths"""
    M, n = len(x), len(x[0])
    return max(score(x, s, L) for s in itertools.product(range(M), repeat=n))


def step(V, col, L):
    """one position of the recurrence: V_c(i-1) and x_c(i) -> V_c(i), sw_c(i), a(i-1)"""
    B = max(V)
    a = V.index(B)                                       # the lowest c attaining it
    J = B - (L * W + 1)
    return [xc * W + (v if v > J else J) for xc, v in zip(col, V)], [v < J for v in V], a


def all_values(M, n, L):
    """value of the recurrence for EVERY M x n matrix, by walking the tree of column prefixes with step(): out[m] for the matrix whose
    column i is the M bits of m from bit M * i on (bit c: x_c(i))"""
    cols = [[(code >> c) & 1 for c in range(M)] for code in range(1 << M)]
    out = np.zeros(1 << (M * n), np.int64)
    stack = [(1, code, [xc * W for xc in cols[code]]) for code in range(1 << M)]
    while stack:
        d, m, V = stack.pop()
        if d == n:
            out[m] = max(V)
            continue
        for code in range(1 << M):
            stack.append((d + 1, m | (code << (M * d)), step(V, cols[code], L)[0]))
    return out


def brute_all(M, n):
    """the brute force over all M^n paths for EVERY M x n matrix at once (numbered as in all_values): best[s][m] = the most hits a path
    with exactly s switches has on matrix m.  Every path is walked; numpy only carries the 2^(M n) matrices side by side"""
    m = np.arange(1 << (M * n), dtype=np.int64)
    bit = [[((m >> (M * i + c)) & 1).astype(np.int8) for c in range(M)] for i in range(n)]
    best = [np.full(m.size, -1, np.int8) for _ in range(n)]

    def walk(i, prev, s, hits):
        for c in range(M):
            h = hits + bit[i][c]
            k = s + (i > 0 and c != prev)
            if i == n - 1:
                np.maximum(best[k], h, out=best[k])
            else:
                walk(i + 1, c, k, h)

    walk(0, 0, 0, np.zeros(m.size, np.int8))
    return best


def brute_values(best, L):
    """the greatest value of every matrix from brute_all's table"""
    out = None
    for s, h in enumerate(best):
        v = np.where(h >= 0, (h.astype(np.int64) - L * s) * W - s, np.iinfo(np.int64).min)
        out = v if out is None else np.maximum(out, v)
    return out


def matrix(M, n, m):
    """matrix number m of all_values / brute_all as x[c][i]"""
    return [[(m >> (M * i + c)) & 1 for i in range(n)] for c in range(M)]


def viterbi(x, L):
    """the recurrence and its backtrace -> (value, path); a tie stays, equal candidates go to the lowest index"""
    M, n = len(x), len(x[0])
    V = [x[c][0] * W for c in range(M)]
    sw, a = [None], []                                   # sw[i][c] for i >= 1; a[i] for i = 0 .. n-1
    for i in range(1, n):
        nV, s, ai = step(V, [x[c][i] for c in range(M)], L)
        sw.append(s)
        a.append(ai)
        assert not sw[i][a[i - 1]]
        assert all(nV[c] >= V[c] >= 0 for c in range(M))
        V = nV
    B = max(V)
    a.append(V.index(B))
    s = [0] * n
    s[n - 1] = a[n - 1]
    for i in range(n - 1, 0, -1):
        s[i - 1] = a[i - 1] if sw[i][s[i]] else s[i]
        assert not sw[i][s[i]] or s[i - 1] != s[i]       # every switch changes the candidate
    return B, s


def segment(x, L):
    """x[c][i] for M >= 2 candidates and n > 0 hashes -> the words of the read and its segments (start, end, c, hits, best_hits)"""
    M, n = len(x), len(x[0])
    total = [sum(row) for row in x]
    single = max(total)
    best = total.index(single)
    value, s = viterbi(x, L)
    assert value == score(x, s, L)
    segs, start = [], 0
    for i in range(1, n + 1):
        if i == n or s[i] != s[i - 1]:
            c = s[start]
            segs.append((start, i, c, sum(x[c][start:i]), sum(x[best][start:i])))
            start = i
    K = len(segs)
    hits = sum(g[3] for g in segs)
    assert value == (hits - L * (K - 1)) * W - (K - 1) and hits - L * (K - 1) >= single
    return dict(M=M, n=n, single=single, best=best, K=K, hits=hits, segs=segs, value=value, path=s)


def shape(bins):
    if len(bins) == 2:
        return "split"
    if len(bins) == 3 and bins[0] == bins[2]:
        return "insert"
    return "mosaic"


class SgExpect:
    """reads are added in batch order; same() compares what Segments.add_batch / add_csr return for the batch"""

    def __init__(self, host=None, cov=None, L=16):
        self.cov = cov if cov is not None else CovExpect(host)
        self.oracle = self.cov.oracle
        self.L = int(L)
        self.clear()

    def clear(self):
        self.reads, self.n_hashes, self.n_tuples = [], [], 0

    def add_read(self, hashes, user_bin, count):
        """one read: its ordered hash list and ALL its tuples, in CSR order"""
        h = np.asarray(hashes, np.uint64)
        cand = [(self.n_tuples + t, int(b)) for t, (b, c) in enumerate(zip(user_bin, count)) if int(c) > 0]
        self.n_tuples += len(count)
        self.n_hashes.append(int(h.size))
        if h.size == 0 or len(cand) < 2:
            self.reads.append(dict(ZERO))
            return self.reads[-1]
        masks = {}
        for _, b in cand:
            if b not in masks:
                masks[b] = [int(v) for v in self.cov.matches(b, h)]
        g = segment([masks[b] for _, b in cand], self.L)
        best = cand[g["best"]]
        segs = [dict(start=st, end=en, tuple=cand[c][0], bin=cand[c][1], hits=hi, best_hits=bh, c=c) for st, en, c, hi, bh in g["segs"]]
        self.reads.append(dict(examined=True, n_candidates=g["M"], n=g["n"], n_segments=g["K"], path_hits=g["hits"], path_switches=g["K"] - 1, single=g["single"],
                               tuple_best=best[0], bin_best=best[1], segs=segs, bins=[b for _, b in cand], path=g["path"]))
        return self.reads[-1]

    def add_bases(self, reads, **kw):
        """reads as dna4-normalised bytes (orc_search_batch, orc_seq_to_syncmers)"""
        B = np.frombuffer(b"".join(reads), np.uint8)
        O = np.cumsum([0] + [len(r) for r in reads]).astype(np.uint64)
        nh, off, ub, cnt, _ = self.oracle.search_batch(B, O, threads=4, **kw)
        for i, r in enumerate(reads):
            lo, hi = int(off[i]), int(off[i + 1])
            hashes = orc.seq_to_syncmers(r) if len(r) else np.zeros(0, np.uint64)
            assert hashes.size == int(nh[i])
            self.add_read(hashes, ub[lo:hi], cnt[lo:hi])

    def reported(self, r):
        return self.reads[r]["examined"] and self.reads[r]["n_segments"] >= 2

    def shape(self, r):
        return shape([g["bin"] for g in self.reads[r]["segs"]])

    def text(self, sp, ids, read_lens):
        """the lines of `taxor search --segments-file` for the reads added (no header): sp the species dicts, ids as str"""
        by_bin = {}
        for s in sp:
            by_bin.setdefault(s["user_bin"], s)
        ref = lambda b: [by_bin.get(b, sp[0])["accession_id"], by_bin.get(b, sp[0])["taxid"]]
        out = []
        for r, rid in enumerate(ids):
            if not self.reported(r):
                continue
            x, n = self.reads[r], self.n_hashes[r]
            head = [rid, read_lens[r], n, x["n_candidates"], x["n_segments"], self.shape(r), x["path_hits"], x["single"]]
            for j, g in enumerate(x["segs"]):
                f = head + [j, g["start"], g["end"], base(g["start"], read_lens[r], n), base(g["end"], read_lens[r], n)] + ref(g["bin"]) + [g["hits"]]
                f += ref(x["bin_best"]) + [g["best_hits"]]
                out.append("\t".join(str(v) for v in f) + "\n")
        return "".join(out)


def same(got, exp, lo=0, hi=None, tuple_shift=0):
    """a SegmentsBatch equals reads [lo, hi) of the expectation, word for word; tuple_shift: the tuples of the batches before.  The
    invariants of the definition are asserted on what the device returned, read by read"""
    reads = exp.reads[lo:hi]
    assert got.examined.size == len(reads)
    assert [bool(v) for v in got.examined] == [x["examined"] for x in reads]
    assert [int(v) for v in got.n_hashes] == exp.n_hashes[lo:hi]
    assert got.switch_cost == exp.L
    for f in WORDS:
        shift = tuple_shift if f.startswith("tuple_") else 0
        want = [x[f] - (shift if x["examined"] else 0) for x in reads]
        have = [int(v) for v in getattr(got, f)]
        assert have == want, (f, [(i, h, w) for i, (h, w) in enumerate(zip(have, want)) if h != w][:8])
    off = [0]
    for x in reads:
        off.append(off[-1] + (len(x["segs"]) if x["examined"] and x["n_segments"] >= 2 else 0))
    assert [int(v) for v in got.seg_off] == off
    flat = [g for x in reads if x["examined"] and x["n_segments"] >= 2 for g in x["segs"]]
    for f, key in (("seg_start", "start"), ("seg_end", "end"), ("seg_tuple", "tuple"), ("seg_bin", "bin"), ("seg_hits", "hits"), ("seg_best_hits", "best_hits")):
        want = [g[key] - (tuple_shift if key == "tuple" else 0) for g in flat]
        have = [int(v) for v in getattr(got, f)]
        assert have == want, (f, [(i, h, w) for i, (h, w) in enumerate(zip(have, want)) if h != w][:8])
    assert [bool(v) for v in got.reported] == [bool(x["examined"] and x["n_segments"] >= 2) for x in reads]
    assert got.n_examined == sum(x["examined"] for x in reads) and got.n_reported == int(got.reported.sum())
    L = got.switch_cost
    for r in range(len(reads)):
        if not got.examined[r]:
            assert int(got.n_segments[r]) == 0
            continue
        assert int(got.path_hits[r]) - L * int(got.path_switches[r]) >= int(got.single[r]) and int(got.n_segments[r]) == int(got.path_switches[r]) + 1
        a, b = int(got.seg_off[r]), int(got.seg_off[r + 1])
        if not got.reported[r]:
            assert a == b and int(got.path_hits[r]) == int(got.single[r])
            continue
        assert b - a == int(got.n_segments[r])
        assert int(got.seg_start[a]) == 0 and int(got.seg_end[b - 1]) == int(got.n[r])                 # the segments tile [0, n)
        assert all(int(got.seg_end[j]) == int(got.seg_start[j + 1]) for j in range(a, b - 1)) and all(int(got.seg_start[j]) < int(got.seg_end[j]) for j in range(a, b))
        assert all(int(got.seg_tuple[j]) != int(got.seg_tuple[j + 1]) for j in range(a, b - 1))       # neighbours differ in candidate
        assert sum(int(got.seg_hits[j]) for j in range(a, b)) == int(got.path_hits[r])
