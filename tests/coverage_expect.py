"""The CPU expectation of the coverage accumulator (taxor_amd/csrc/coverage.hip), from the oracle alone: orc_ixf_probe gives a hash's
rows and fingerprint, orc_bulk_contains / orc_search_batch the tuples, orc_classify_filter the survivors; the slot function is the
numpy restatement tests/test_hll_cpu.py pins to the library's.  Shared by the coverage tests."""
import numpy as np

from oracle import oracle as orc
from tests.test_hll_cpu import slots


class Expect:
    def __init__(self, host):
        """host: the IXF dicts of synth.materialize_host (with data)"""
        self.oracle = orc.Hixf(host, [f["next_ixf"] for f in host], [f["fname_idx"] for f in host])
        self.data = [np.asarray(f["data"], np.uint8).reshape(3 * f["seg_len"], f["stride"]) for f in host]
        self.n_bins = 1 + max(int(np.max(f["fname_idx"])) for f in host)
        self.leaves = {}                                  # user bin -> [(ixf, bin)] in index order
        for x, f in enumerate(host):
            for j, b in enumerate(f["fname_idx"]):
                if b >= 0:
                    self.leaves.setdefault(int(b), []).append((x, j))
        self._probe = {}
        self.clear()

    def clear(self):
        self.reads = np.zeros(self.n_bins, np.uint64)
        self.hash_matches = np.zeros(self.n_bins, np.uint64)
        self.matched = [set() for _ in range(self.n_bins)]

    def _probes(self, x, hashes):
        rows = np.empty((len(hashes), 3), np.int64)
        fp = np.empty(len(hashes), np.uint8)
        for i, h in enumerate(hashes):
            key = (x, int(h))
            if key not in self._probe:
                self._probe[key] = self.oracle.ixf_probe(x, int(h))
            r, f = self._probe[key]
            rows[i] = r
            fp[i] = f
        return rows, fp

    def matches(self, b, hashes):
        """mask over `hashes`: matched in at least one leaf technical bin of user bin b"""
        m = np.zeros(len(hashes), bool)
        for x, j in self.leaves.get(b, []):
            rows, fp = self._probes(x, hashes)
            d = self.data[x]
            m |= (d[rows[:, 0], j] ^ d[rows[:, 1], j] ^ d[rows[:, 2], j]) == fp
        return m

    def lookups(self, b, hashes, stop_at_first):
        """leaf-bin lookups the device makes for `hashes` against user bin b (read_probe.h's leaf_lookup): per hash the number of b's
        leaf bins, or with stop_at_first the index of the first matching leaf bin plus one (all of them when none matches)"""
        leaves = self.leaves.get(b, [])
        n = len(hashes)
        if not stop_at_first or n == 0:
            return n * len(leaves)
        made = np.full(n, len(leaves), np.int64)
        open_ = np.ones(n, bool)
        for at, (x, j) in enumerate(leaves):
            rows, fp = self._probes(x, hashes)
            d = self.data[x]
            hit = open_ & ((d[rows[:, 0], j] ^ d[rows[:, 1], j] ^ d[rows[:, 2], j]) == fp)
            made[hit] = at + 1
            open_ &= ~hit
        return int(made.sum())

    def add_read(self, hashes, user_bin, count, times=1):
        """one read: its hash list and its tuples before the 0.8 * max filter.  Returns the surviving (user bin, count) pairs"""
        if len(count) == 0:
            return []
        keep = orc.classify_filter(np.asarray(count, np.uint32))
        out = []
        for b, c, k in zip(user_bin, count, keep):
            if not k:
                continue
            b, c = int(b), int(c)
            out.append((b, c))
            self.reads[b] += np.uint64(times)
            self.hash_matches[b] += np.uint64(times * c)
            if len(hashes):
                h = np.asarray(hashes, np.uint64)
                self.matched[b].update(int(v) for v in h[self.matches(b, h)])
        return out

    def add_hash_list(self, hashes, thr):
        """a read given as a hash list and a threshold (orc_bulk_contains)"""
        ub, cnt, _ = self.oracle.bulk_contains(np.asarray(hashes, np.uint64), int(thr))
        return self.add_read(hashes, ub, cnt)

    def add_bases(self, reads, times=1, **kw):
        """reads as dna4-normalised bytes (orc_search_batch, orc_seq_to_syncmers).  Returns per read the surviving pairs"""
        B = np.frombuffer(b"".join(reads), np.uint8)
        O = np.cumsum([0] + [len(r) for r in reads]).astype(np.uint64)
        nh, off, ub, cnt, _ = self.oracle.search_batch(B, O, threads=4, **kw)
        out = []
        for i, r in enumerate(reads):
            lo, hi = int(off[i]), int(off[i + 1])
            hashes = orc.seq_to_syncmers(r) if len(r) else np.zeros(0, np.uint64)
            assert hashes.size == int(nh[i])
            out.append(self.add_read(hashes, ub[lo:hi], cnt[lo:hi], times))
        return out

    def registers(self, p):
        reg = np.zeros((self.n_bins, 1 << p), np.uint8)
        for b, s in enumerate(self.matched):
            if s:
                idx, rho = slots(np.fromiter(s, np.uint64, len(s)), p)
                np.maximum.at(reg[b], idx, rho)
        return reg


def same(table, exp, p=12):
    """a Coverage.results() table equals the expectation, array for array"""
    assert table.precision == p
    assert np.array_equal(table.reads, exp.reads), np.flatnonzero(table.reads != exp.reads)
    assert np.array_equal(table.hash_matches, exp.hash_matches)
    want = exp.registers(p)
    assert np.array_equal(table.registers, want), np.argwhere(table.registers != want)[:8]


def candidate_lookups(cov, reads, min_candidates):
    """the leaf-bin lookups breakpoint.hip, segments.hip and exclusive.hip count for hand-made (what, tuples, hashes) reads: a read is
    examined when it has a hash and at least min_candidates candidates (tuples with count > 0); every candidate of an examined read is
    looked up for every hash of the read, and a lookup stops at the candidate's first matching leaf bin"""
    total, memo = 0, {}
    for _, tuples, hashes in reads:
        cand = [int(b) for b, c in tuples if c > 0]
        if len(hashes) == 0 or len(cand) < min_candidates:
            continue
        h = np.asarray(hashes, np.uint64)
        for b in cand:
            key = (b, h.tobytes())
            if key not in memo:
                memo[key] = cov.lookups(b, h, True)
            total += memo[key]
    return total


STAGE_CUT = {"TAXOR_TUNING": "1", "TAXOR_STAGE_HASHES": "4096", "TAXOR_STAGE_PIECES": "3"}


def same_results(a, b):
    """two result objects of one class hold equal arrays and equal counters; the seconds are left out"""
    for k, v in vars(a).items():
        if isinstance(v, np.ndarray):
            assert np.array_equal(v, getattr(b, k)), k
        elif not k.startswith("seconds"):
            assert v == getattr(b, k), k
