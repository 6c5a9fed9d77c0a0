"""The restatement of the breakpoint words (taxor_amd/csrc/breakpoint.hip, include/taxor_gpu_tools.h), from the oracle alone:
orc_search_batch / orc_bulk_contains give a read's tuples, orc_seq_to_syncmers its ordered hash list, orc_ixf_probe a hash's rows and
fingerprint; the leaf bins of a user bin and the lookup in them are tests/coverage_expect.py's.  Everything else is Python ints: a plain
double loop over p and c, with the tie rules as the header writes them.  Shared by the breakpoint tests."""
import numpy as np

from oracle import oracle as orc
from tests.coverage_expect import Expect as CovExpect

COLUMNS = ("#QUERY_NAME\tQUERY_LEN\tQHASH_COUNT\tCANDIDATES\tBEST_ACCESSION\tBEST_TAXID\tBEST_LOCATED\tBREAK_HASH\tBREAK_BASE_APPROX\tLEFT_ACCESSION\tLEFT_TAXID\t"
           "LEFT_HITS\tLEFT_HITS_OF_RIGHT\tRIGHT_ACCESSION\tRIGHT_TAXID\tRIGHT_HITS\tRIGHT_HITS_OF_LEFT\tGAIN\n")
WORDS = ("gain", "break_hash", "tuple_a", "tuple_b", "tuple_best", "pre_a", "suf_b", "pre_b", "suf_a", "single", "n_candidates", "n")
ZERO = dict(examined=False, bin_a=0, bin_b=0, bin_best=0, **{f: 0 for f in WORDS})


def base(p, query_len, n):
    """the approximate base position of a break in front of hash p of n"""
    return (int(p) * int(query_len)) // int(n) if n else 0


def best_split(x):
    """x[c][i] in {0, 1} for M >= 2 candidates and n > 0 hashes -> gain, p*, A, B, best and the four counts around the break"""
    M, n = len(x), len(x[0])
    total = [sum(row) for row in x]
    single = max(total)
    best = total.index(single)                           # the lowest c that attains it
    pre = [0] * M                                        # pre_c(p)
    top = None
    for p in range(n):
        P = S = -1
        A = B = None
        for c in range(M):
            suf = total[c] - pre[c]
            if pre[c] > P:                               # strictly: the lowest c keeps a tie
                P, A = pre[c], c
            if suf > S:
                S, B = suf, c
        if top is None or P + S > top["split"]:          # strictly: the smallest p keeps a tie
            top = dict(split=P + S, p=p, A=A, B=B, pre_a=pre[A], suf_b=total[B] - pre[B], pre_b=pre[B], suf_a=total[A] - pre[A])
        for c in range(M):
            pre[c] += x[c][p]
    assert top["split"] >= single and (top["split"] == single or top["A"] != top["B"])
    return dict(top, gain=top["split"] - single, single=single, best=best, M=M, n=n)


class BpExpect:
    """reads are added in batch order; arrays() gives what Breakpoints.add_batch / add_csr return for the batch"""

    def __init__(self, host=None, cov=None):
        self.cov = cov if cov is not None else CovExpect(host)
        self.oracle = self.cov.oracle
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
        s = best_split([masks[b] for _, b in cand])
        A, B, best = cand[s["A"]], cand[s["B"]], cand[s["best"]]
        self.reads.append(dict(examined=True, gain=s["gain"], break_hash=s["p"], tuple_a=A[0], tuple_b=B[0], tuple_best=best[0], pre_a=s["pre_a"], suf_b=s["suf_b"],
                               pre_b=s["pre_b"], suf_a=s["suf_a"], single=s["single"], n_candidates=s["M"], n=s["n"], bin_a=A[1], bin_b=B[1], bin_best=best[1],
                               bins=[b for _, b in cand]))
        return self.reads[-1]

    def add_hash_list(self, hashes, thr):
        """a read given as a hash list and a threshold (orc_bulk_contains)"""
        ub, cnt, _ = self.oracle.bulk_contains(np.asarray(hashes, np.uint64), int(thr))
        return self.add_read(hashes, ub, cnt)

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

    def reported(self, r, G):
        return self.reads[r]["examined"] and self.reads[r]["gain"] >= G

    def text(self, sp, ids, read_lens, G=1):
        """the lines of `taxor search --breakpoint-file` for the reads added (no header): sp the species dicts, ids as str"""
        by_bin = {}
        for s in sp:
            by_bin.setdefault(s["user_bin"], s)
        ref = lambda b: [by_bin.get(b, sp[0])["accession_id"], by_bin.get(b, sp[0])["taxid"]]
        out = []
        for r, rid in enumerate(ids):
            if not self.reported(r, G):
                continue
            x, n = self.reads[r], self.n_hashes[r]
            f = [rid, read_lens[r], n, x["n_candidates"]] + ref(x["bin_best"]) + [x["single"], x["break_hash"], base(x["break_hash"], read_lens[r], n)]
            f += ref(x["bin_a"]) + [x["pre_a"], x["pre_b"]] + ref(x["bin_b"]) + [x["suf_b"], x["suf_a"], x["gain"]]
            out.append("\t".join(str(v) for v in f) + "\n")
        return "".join(out)


def same(got, exp, lo=0, hi=None, tuple_shift=0, G=None):
    """a BreakpointBatch equals reads [lo, hi) of the expectation, word for word; tuple_shift: the tuples of the batches before"""
    reads = exp.reads[lo:hi]
    assert got.examined.size == len(reads)
    assert [bool(v) for v in got.examined] == [x["examined"] for x in reads]
    assert [int(v) for v in got.n_hashes] == exp.n_hashes[lo:hi]
    for f in WORDS + ("bin_a", "bin_b", "bin_best"):
        shift = tuple_shift if f.startswith("tuple_") else 0
        want = [x[f] - (shift if x["examined"] else 0) for x in reads]
        have = [int(v) for v in getattr(got, f)]
        assert have == want, (f, [(i, h, w) for i, (h, w) in enumerate(zip(have, want)) if h != w][:8])
    G = got.min_gain if G is None else G
    assert [bool(v) for v in got.reported] == [bool(x["examined"] and x["gain"] >= G) for x in reads]
    assert got.n_examined == sum(x["examined"] for x in reads) and got.n_reported == int(got.reported.sum())
