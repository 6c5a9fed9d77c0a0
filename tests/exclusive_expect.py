"""The restatement of the exclusive-hash words (taxor_amd/csrc/exclusive.hip, include/taxor_gpu_tools.h), from the oracle alone:
orc_search_batch / orc_bulk_contains give a read's tuples, orc_seq_to_syncmers its ordered hash list, orc_ixf_probe a hash's rows and
fingerprint; the leaf bins of a user bin and the lookup in them are tests/coverage_expect.py's (CovExpect.matches(b, h) is x).
Everything else is Python ints and sets; the registers come from tests/test_hll_cpu.py's slot restatement.  Shared by the exclusive
tests."""
import numpy as np

from oracle import oracle as orc
from tests.coverage_expect import Expect as CovExpect
from tests.test_hll_cpu import slots

BIN_COLUMNS = "#ACCESSION\tTAXID\tCANDIDATE_READS\tHITS\tEXCLUSIVE_HITS\tEXCLUSIVE_READS\tDISTINCT_EXCLUSIVE\tEXCLUSIVE_FRACTION\n"
READ_COLUMNS = "#QUERY_NAME\tACCESSION\tTAXID\tQUERY_LEN\tQHASH_COUNT\tQHASH_MATCH\tHITS\tEXCLUSIVE_HITS\tCANDIDATES\tMATCHED\tSHARED\n"
READ_WORDS = ("n_candidates", "n", "matched", "shared")
CAND_WORDS = ("cand_tuple", "cand_bin", "cand_count", "cand_hits", "cand_excl")


def exclusive(x):
    """x[c][i] in {0, 1} for M >= 1 candidates and n > 0 hashes -> hits[c], excl[c], shared, matched, and per candidate the i exclusive to it"""
    M, n = len(x), len(x[0])
    hits, excl, own = [sum(row) for row in x], [0] * M, [[] for _ in range(M)]
    shared = matched = 0
    for i in range(n):
        who = [c for c in range(M) if x[c][i]]
        matched += len(who) >= 1
        shared += len(who) >= 2
        if len(who) == 1:
            excl[who[0]] += 1
            own[who[0]].append(i)
    # the identities of the header, on every read
    assert sum(excl) + shared == matched <= n and all(e <= h for e, h in zip(excl, hits)) and sum(hits) >= matched
    assert M != 1 or excl[0] == hits[0]
    return hits, excl, shared, matched, own


class ExExpect:
    """reads are added in batch order; clear_batch() starts the next batch and keeps the run's per-user-bin sums and sets"""

    def __init__(self, host=None, cov=None):
        self.cov = cov if cov is not None else CovExpect(host)
        self.oracle = self.cov.oracle
        nb = self.cov.n_bins
        self.cand_reads, self.hits, self.exclusive_hits, self.exclusive_reads = ([0] * nb for _ in range(4))
        self.owned = [set() for _ in range(nb)]           # the hashes that were exclusive to the user bin, over the run
        self.clear_batch()

    def clear_batch(self):
        self.reads, self.n_hashes, self.n_tuples = [], [], 0

    def add_read(self, hashes, user_bin, count, times=1):
        """one read: its ordered hash list and ALL its tuples, in CSR order"""
        h = np.asarray(hashes, np.uint64)
        cand = [(self.n_tuples + t, int(b), int(c)) for t, (b, c) in enumerate(zip(user_bin, count)) if int(c) > 0]
        self.n_tuples += len(count)
        self.n_hashes.append(int(h.size))
        if h.size == 0 or len(cand) < 1:
            self.reads.append(dict(examined=False, n_candidates=0 if h.size == 0 else len(cand), n=0, matched=0, shared=0, cands=[]))
            return self.reads[-1]
        masks = {}
        for _, b, _ in cand:
            if b not in masks:
                masks[b] = [int(v) for v in self.cov.matches(b, h)]
        hits, excl, shared, matched, own = exclusive([masks[b] for _, b, _ in cand])
        for (t, b, c), hc, ec, ow in zip(cand, hits, excl, own):
            self.cand_reads[b] += times
            self.hits[b] += times * hc
            self.exclusive_hits[b] += times * ec
            self.exclusive_reads[b] += times * (ec > 0)
            self.owned[b].update(int(h[i]) for i in ow)
        self.reads.append(dict(examined=True, n_candidates=len(cand), n=int(h.size), matched=matched, shared=shared,
                               cands=[dict(cand_tuple=t, cand_bin=b, cand_count=c, cand_hits=hc, cand_excl=ec) for (t, b, c), hc, ec in zip(cand, hits, excl)]))
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

    def registers(self, p):
        reg = np.zeros((self.cov.n_bins, 1 << p), np.uint8)
        for b, s in enumerate(self.owned):
            if s:
                idx, rho = slots(np.fromiter(s, np.uint64, len(s)), p)
                np.maximum.at(reg[b], idx, rho)
        return reg

    # ---- the two files (no header)
    @staticmethod
    def _refs(sp):
        by_bin = {}
        for s in sp:
            by_bin.setdefault(s["user_bin"], s)
        return lambda b: [by_bin.get(b, sp[0])["accession_id"], by_bin.get(b, sp[0])["taxid"]]

    def bin_text(self, sp, distinct):
        """`--exclusive-file`: distinct(b) gives DISTINCT_EXCLUSIVE"""
        ref, out = self._refs(sp), []
        for b in range(self.cov.n_bins):
            if self.cand_reads[b] == 0:
                continue
            h, e = self.hits[b], self.exclusive_hits[b]
            f = ref(b) + [self.cand_reads[b], h, e, self.exclusive_reads[b], distinct(b), "%.4f" % (e / h if h else 0.0)]
            out.append("\t".join(str(v) for v in f) + "\n")
        return "".join(out)

    def read_text(self, sp, ids, read_lens):
        """`--exclusive-reads-file` for the reads of the current batch: ids as str"""
        ref, out = self._refs(sp), []
        for r, rid in enumerate(ids):
            x = self.reads[r]
            if not x["examined"] or x["n_candidates"] < 2:
                continue
            keep = orc.classify_filter(np.array([c["cand_count"] for c in x["cands"]], np.uint32))
            for c, k in zip(x["cands"], keep):
                if k:
                    f = [rid] + ref(c["cand_bin"]) + [read_lens[r], self.n_hashes[r], c["cand_count"], c["cand_hits"], c["cand_excl"], x["n_candidates"], x["matched"],
                                                      x["shared"]]
                    out.append("\t".join(str(v) for v in f) + "\n")
        return "".join(out)


def same(got, exp, lo=0, hi=None, tuple_shift=0):
    """an ExclusiveBatch equals reads [lo, hi) of the expectation's current batch, word for word; tuple_shift: the tuples of the batches before"""
    reads = exp.reads[lo:hi]
    assert got.examined.size == len(reads)
    assert [bool(v) for v in got.examined] == [x["examined"] for x in reads]
    assert [int(v) for v in got.n_hashes] == exp.n_hashes[lo:hi]
    for f in READ_WORDS:
        have, want = [int(v) for v in getattr(got, f)], [x[f] for x in reads]
        assert have == want, (f, [(i, h, w) for i, (h, w) in enumerate(zip(have, want)) if h != w][:8])
    assert [int(v) for v in got.cand_off] == [int(v) for v in np.cumsum([0] + [len(x["cands"]) for x in reads])]
    for f in CAND_WORDS:
        shift = tuple_shift if f == "cand_tuple" else 0
        have, want = [int(v) for v in getattr(got, f)], [c[f] - shift for x in reads for c in x["cands"]]
        assert have == want, (f, [(i, h, w) for i, (h, w) in enumerate(zip(have, want)) if h != w][:8])
    assert got.n_examined == sum(x["examined"] for x in reads)
    # the identities, on what the device returned
    for r in range(len(reads)):
        a, b = int(got.cand_off[r]), int(got.cand_off[r + 1])
        ex, hi_ = got.cand_excl[a:b].astype(np.int64), got.cand_hits[a:b].astype(np.int64)
        assert int(ex.sum()) + int(got.shared[r]) == int(got.matched[r]) <= int(got.n[r]) and (ex <= hi_).all() and int(hi_.sum()) >= int(got.matched[r])
        assert b - a != 1 or ex[0] == hi_[0]


def same_table(table, exp, p=12):
    """an Exclusive.results() table equals the expectation's sums and registers, array for array"""
    assert table.precision == p
    for f in ("cand_reads", "hits", "exclusive_hits", "exclusive_reads"):
        have, want = [int(v) for v in getattr(table, f)], getattr(exp, f)
        assert have == want, (f, [(i, h, w) for i, (h, w) in enumerate(zip(have, want)) if h != w][:8])
    want = exp.registers(p)
    assert np.array_equal(table.registers, want), np.argwhere(table.registers != want)[:8]
