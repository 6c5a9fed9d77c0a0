"""The CPU expectation of the hit map (taxor_amd/csrc/hitmap.hip), from the oracle alone: orc_search_batch / orc_bulk_contains give the
tuples, orc_classify_filter the survivors, orc_seq_to_syncmers a read's ordered hash list, orc_ixf_probe a hash's rows and fingerprint;
the leaf bins of a user bin and the lookup in them are tests/coverage_expect.py's (the two features share that definition).  seg and
size are restated here in Python integers.  Shared by the hit map tests."""
import numpy as np

from oracle import oracle as orc
from tests.coverage_expect import Expect

COLUMNS = "#QUERY_NAME\tACCESSION\tTAXID\tQUERY_LEN\tQHASH_COUNT\tQHASH_MATCH\tLOCATED\tSEGMENT_SIZES\tSEGMENT_HITS\n"


def seg(i, S, n):
    """segment of hash i of n"""
    return (int(i) * int(S)) // int(n)


def size(j, S, n):
    """hashes of segment j: ceil((j + 1) * n / S) - ceil(j * n / S)"""
    ceil = lambda a, b: -((-a) // b)
    return ceil((int(j) + 1) * int(n), int(S)) - ceil(int(j) * int(n), int(S))


class HitExpect:
    """reads are added in batch order; arrays(S) gives what Hitmap.add_batch returns for the batch"""

    def __init__(self, host):
        self.cov = Expect(host)
        self.oracle = self.cov.oracle
        self.leaves = self.cov.leaves
        self.clear()

    def clear(self):
        self.n_hashes, self.n_tuples = [], 0
        self.map_off = [0]
        self.rows = []                                   # per mapped tuple: (index in the batch CSR, user bin, count, read, mask over the read's hashes)

    def add_read(self, hashes, user_bin, count):
        """one read: its ordered hash list and its tuples before the 0.8 * max filter, in CSR order"""
        h = np.asarray(hashes, np.uint64)
        r = len(self.n_hashes)
        if h.size and len(count):                        # a survivor is mapped when the read has a hash
            keep = orc.classify_filter(np.asarray(count, np.uint32))
            for t, (b, c, k) in enumerate(zip(user_bin, count, keep)):
                if k:
                    self.rows.append((self.n_tuples + t, int(b), int(c), r, self.cov.matches(int(b), h)))
        self.n_hashes.append(int(h.size))
        self.n_tuples += len(count)
        self.map_off.append(len(self.rows))

    def add_hash_list(self, hashes, thr):
        """a read given as a hash list and a threshold (orc_bulk_contains)"""
        ub, cnt, _ = self.oracle.bulk_contains(np.asarray(hashes, np.uint64), int(thr))
        self.add_read(hashes, ub, cnt)

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

    def hits(self, row, S):
        _, _, _, r, mask = row
        n = self.n_hashes[r]
        out = np.zeros(S, np.uint32)
        for i in np.flatnonzero(mask):
            out[seg(i, S, n)] += 1
        return out

    def arrays(self, S):
        m = len(self.rows)
        return dict(map_off=np.array(self.map_off, np.uint64), tuple=np.array([x[0] for x in self.rows], np.uint64),
                    user_bin=np.array([x[1] for x in self.rows], np.int64), count=np.array([x[2] for x in self.rows], np.uint32),
                    hits=np.array([self.hits(x, S) for x in self.rows], np.uint32).reshape(m, S), n_hashes=np.array(self.n_hashes, np.uint32))

    def text(self, sp, ids, read_lens, S):
        """the lines of `taxor search --hitmap-file` for the reads added (no header): sp the species dicts, ids as str"""
        by_bin = {}
        for s in sp:
            by_bin.setdefault(s["user_bin"], s)
        out = []
        for r, rid in enumerate(ids):
            n = self.n_hashes[r]
            for row in self.rows[self.map_off[r]:self.map_off[r + 1]]:
                s = by_bin.get(row[1], sp[0])
                h = self.hits(row, S)
                out.append("\t".join([rid, s["accession_id"], s["taxid"], str(read_lens[r]), str(n), str(row[2]), str(int(h.sum())),
                                      ",".join(str(size(j, S, n)) for j in range(S)), ",".join(str(int(x)) for x in h)]) + "\n")
        return "".join(out)


def same(got, exp, S):
    """a Hitmap.add_batch result equals the expectation, array for array"""
    want = exp.arrays(S)
    assert got.segments == S
    for f in ("n_hashes", "map_off", "tuple", "user_bin", "count"):
        assert np.array_equal(getattr(got, f), want[f]), (f, getattr(got, f)[:12], want[f][:12])
    assert got.hits.shape == want["hits"].shape
    assert np.array_equal(got.hits, want["hits"]), np.argwhere(got.hits != want["hits"])[:8]
