"""The result assembly of `taxor search` at its size edges: hit records -> per-read CSR in the reference's DFS order, by
k_finalize_small (one block, calls that go through the four lanes) and by launch_finalize (scan / scatter / k_sort_small /
k_sort_big, the pipeline of large batches).  Every comparison is exact -- n_hashes, read_off, user_bin, count against
oracle.Hixf.search_batch -- and every case that is meant to run on the lanes says so through `small_pieces_rerun`.

The indexes are tiny and hand-made: L leaf runs, flat or two-level with the merged bins in the MIDDLE of the root, so the DFS
order of a read's tuples (root leaves, a child's leaves where its merged bin stands, root leaves) differs from the order of
the bins and from the order in which the hit records arrive (a child's after all of the root's).  A read's tuples are left in
arrival order by a sorter that skips it, so a skipped read shows.  Thresholds are (size_t)(hashes * 1.0): an error-free read
of a planted genome reports exactly the leaf runs the genome was planted in, a random read of several hashes nothing, and a
read without a hash -- shorter than k, or empty -- has threshold 0 and reports every leaf run (L tuples: a "wide" read when
L > 64).

What fits a lane.  k_query_level (kernels.hip, the tally at the end of an item) appends ONE hit record per reported tuple: a
record is made where a leaf run's sum reaches the threshold (split bins fold into their run's last bin), nowhere else.  So a
piece stays on its lane iff its tuple total, known from the oracle alone, is within the lane's hit buffer, the lane's tuple
scratch and the 65 536-tuple result area, and its queue entries are within the lane's queue.  ensure_scratch (api.hip) sizes
these from the LARGEST piece the lane has held, n: hits max(16 n, L + 64), tuples max(12 n + 1024, L + 64), queue
max(8 n, IXFs + 64); they never shrink, and a rerun through the pipeline doubles whichever overflowed (check_flags).  `Lanes`
below keeps that book from the piece sizes alone -- recomputed here from small_begin's rule and pinned -- and asserts BEFORE
the GPU call that each piece fits or, where the case wants a rerun, that it does not.  A threshold-0 read enters every merged
bin's child, any other read at most those: at most two queue entries per read here, within 8 n.

Mutants the cases are meant to catch (k_finalize_small unless said otherwise).  Only the one marked * was run on the GPU, once: it
is the parent commit's kernel, and cases a (W >= 65), b and f failed against it (docs/EXPERIMENTS.md section 15); the others are
argued from the code:
  a  W in {63, 64, 65, 66}: `bi < 63` / `k < 63` off-by-one at the list's end; W = 0, 1: an unconditional first big sort
  b* the old second sweep (first 64 ARRIVALS in a list + read-order positions 64 and up): a wide read in neither set
  c  `m >= 64` for `m > 64` in the wave sort (L = 64 goes to no sorter); `N <= m` for `N < m` at a power of two (L = 128);
     k_sort_small's `n > 64` the same way (small_path=False)
  d  `tbase` not advanced over a reused lane's piece (small_harvest_one); `sRoff[n]` not written at n = 4096; thread 1023's
     reads dropped (`r + 1 < n`); counters not cleared at the end of a 4096-read piece
  e  a rerun piece's tuples appended at the wrong base, or the pieces after it shifted; `small_pieces_rerun` stuck after it
  f  `total >= tuple_cap` for `total > tuple_cap`; a result area one tuple short
  g  `r < 4095` for `base + j < n_reads` in the scans; k_scan_offsets without the carried base; k_sort_small without its
     grid stride (reads past 16 384 unsorted); k_sort_big without its grid stride (big reads past 256 unsorted)
"""
import os

import numpy as np
import pytest

from oracle import oracle as orc
from taxor_amd import GpuIndex, Searcher, synth

pytestmark = pytest.mark.gpu

K, S, T = 16, 8, 4
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)


# ------------------------------------------------------------------------------------------------ small_begin's rule, restated
def _round_up(x, m):
    return (x + m - 1) // m * m


def piece_sizes(n):
    """the pieces small_begin (api.hip) cuts a call of n reads into; piece p runs on lane p % 4"""
    if n <= 512:
        return [n]
    if n <= 1280:
        a = min(_round_up(n * 5 // 8, 64), n)
        return [a] + ([n - a] if a < n else [])
    if n <= 2048:
        per = _round_up((n + 3) // 4, 64)
        return [min(per, n - f) for f in range(0, n, per)]
    first = max(256, _round_up(n // 8, 64))
    rest = n - first
    k = max(3, (rest + 4095) // 4096)
    per = min(4096, _round_up((rest + k - 1) // k, 64))
    return [first] + [min(per, n - f) for f in range(first, n, per)]


def test_piece_rule_is_pinned():
    """a later change of small_begin's rule, or of the constants beside it, shows up here before it silently moves the cases below
    off their edges"""
    assert piece_sizes(1) == [1] and piece_sizes(512) == [512]
    assert piece_sizes(513) == [320, 193] and piece_sizes(1280) == [832, 448]
    assert piece_sizes(2048) == [512] * 4 and piece_sizes(1281) == [384, 384, 384, 129]
    assert piece_sizes(3000) == [384, 896, 896, 824]
    assert piece_sizes(14080) == [1792, 4096, 4096, 4096]
    assert piece_sizes(14081) == [1792, 3136, 3136, 3136, 2881]
    assert piece_sizes(16384) == [2048, 3584, 3584, 3584, 3584]
    api = open(os.path.join(ROOT, "taxor_amd", "csrc", "api.hip")).read()
    hdr = open(os.path.join(ROOT, "taxor_amd", "csrc", "kernels.h")).read()
    assert "SMALL_MAX_READS = 16384, SMALL_MAX_BASES = 1ull << 28, SMALL_PIECE_MIN = 256, SMALL_TUPLES = 1u << 16;" in api
    assert "constexpr uint32_t SMALL_LANES = 4;" in api and "SMALL_FIN_MAX = 4096;" in hdr
    assert "const uint64_t hmin = std::max<uint64_t>(16ull * R, idx->leaf_runs + 64);" in api
    assert "const uint64_t tmin = std::max<uint64_t>(12 * s->n_reads + 1024, idx->leaf_runs + 64);" in api
    assert "const uint64_t qmin = std::max<uint64_t>(8ull * R, idx->h_ixf.size() + 64);" in api


# ------------------------------------------------------------------------------------------------ indexes and reads
class Index:
    """L leaf runs: flat (n_merged = 0), or a root whose n_merged merged bins stand at 1/3 and 2/3 of it over children of
    their own leaves.  plant = [(keys, leaf runs)]: the keys go into the columns of those leaf runs (positions in DFS order)
    and of the merged bins above them; every other column is random fill."""

    def __init__(self, L, n_merged=2, plant=(), seed=1):
        rng = np.random.default_rng(seed)
        if L < 5:
            n_merged = 0
        child = [L // 4 + i for i in range(n_merged)]
        R = L - sum(child) + n_merged
        at = [R * (i + 1) // (n_merged + 1) for i in range(n_merged)]
        ub = rng.permutation(L).astype(np.int64)                      # user bins in no order of any kind
        nx, fn = np.zeros(R, np.int64), np.full(R, -1, np.int64)
        leaves = []                                                   # (ixf, bin) in DFS order
        for b in range(R):
            if b in at:
                c = at.index(b)
                nx[b] = c + 1
                leaves += [(c + 1, j) for j in range(child[c])]
            else:
                leaves.append((0, b))
        assert len(leaves) == L
        fns = [fn] + [np.zeros(c, np.int64) for c in child]
        for i, (f, b) in enumerate(leaves):
            fns[f][b] = ub[i]
        keys = [dict() for _ in range(1 + n_merged)]
        for ks, where in plant:
            for i in where:
                f, b = leaves[i]
                keys[f].setdefault(b, []).append(ks)
                if f:
                    keys[0].setdefault(at[f - 1], []).append(ks)
        self.ixfs = []
        for f, bins in enumerate([R] + child):
            mine = {b: np.unique(np.concatenate(v)) for b, v in keys[f].items()}
            seg = synth.seg_len_for(max([len(v) for v in mine.values()] + [64]))
            stride = _round_up(bins, 64)
            sd, cols = synth.build_columns(mine, seg, 11 + f + seed) if mine else (11 + f + seed, {})
            data = rng.integers(0, 256, size=(3 * seg, stride), dtype=np.uint8)
            for b, col in cols.items():
                data[:, b] = col
            self.ixfs.append(dict(bins=bins, stride=stride, seg_len=seg, seed=sd, fname_idx=fns[f], data=data.reshape(-1),
                                  next_ixf=nx if f == 0 else np.full(bins, f, np.int64)))
        self.L, self.n_merged, self.ub = L, n_merged, ub
        self.oracle = orc.Hixf(self.ixfs, [f["next_ixf"] for f in self.ixfs], [f["fname_idx"] for f in self.ixfs])
        self._gpu = None

    @property
    def gpu(self):
        if self._gpu is None:
            self._gpu = GpuIndex(self.ixfs, self.L, K, S, T)
            assert self._gpu.leaf_runs == self.L
        return self._gpu

    def want(self, B, O):
        return self.oracle.search_batch(B, O, k=K, s=S, t=T, percentage=1.0, threads=8)

    def searcher(self, **kw):
        return Searcher(self.gpu, percentage=1.0, **kw)

    def close(self):
        if self._gpu is not None:
            self._gpu.close()


def genome(seed, n=4000):
    return ACGT[np.random.default_rng(seed).integers(0, 4, size=n)]


def keys_of(g):
    return orc.seq_to_syncmers(g.tobytes(), K, S, T)


def cat(reads):
    O = np.zeros(len(reads) + 1, dtype=np.uint64)
    O[1:] = np.cumsum([len(r) for r in reads])
    return np.frombuffer(b"".join(reads), dtype=np.uint8), O


def random_read(rng, lo=60, hi=100):
    return ACGT[rng.integers(0, 4, size=int(rng.integers(lo, hi + 1)))].tobytes()


def read_of(rng, g, lo=60, hi=100):
    n = int(rng.integers(lo, hi + 1))
    a = int(rng.integers(0, g.size - n))
    return g[a:a + n].tobytes()


def wide_read(rng):
    """no hash, threshold 0: empty, or shorter than k"""
    return ACGT[rng.integers(0, 4, size=int(rng.integers(0, K)))].tobytes()


def per_read(want):
    return np.diff(want[1].astype(np.int64))


def same(res, want):
    nh, off, ub, cnt, _ = want
    assert np.array_equal(res.n_hashes, nh)
    assert np.array_equal(res.read_off, off)
    bad = [r for r in range(nh.size) if not (np.array_equal(res.user_bin[int(off[r]):int(off[r + 1])], ub[int(off[r]):int(off[r + 1])])
                                             and np.array_equal(res.count[int(off[r]):int(off[r + 1])], cnt[int(off[r]):int(off[r + 1])]))] \
        if not (np.array_equal(res.user_bin, ub) and np.array_equal(res.count, cnt)) else []
    assert not bad, f"{len(bad)} reads differ from the oracle, the first at {bad[:24]}"
    assert np.array_equal(res.user_bin, ub) and np.array_equal(res.count, cnt)


class Lanes:
    """a searcher with its lanes' capacities kept as the docstring above derives them, from the piece sizes alone"""

    def __init__(self, index, **kw):
        self.ix, self.sr = index, index.searcher(**kw)
        self.n_max = [0] * 4
        self.hits, self.tuples = [0] * 4, [0] * 4            # lower bounds of each lane's capacities

    def search(self, reads, want, rerun=()):
        """the call; `rerun`: the pieces that must NOT fit.  Asserted from the oracle's output before the GPU sees the reads."""
        B, O = cat(reads)
        m, sizes = per_read(want), piece_sizes(len(reads))
        assert sum(sizes) == len(reads) and max(sizes) <= 4096
        assert self.ix.n_merged <= 8                                    # queue entries <= n_merged per read <= 8 n
        first = 0
        for p, n in enumerate(sizes):
            li, tot = p % 4, int(m[first:first + n].sum())
            self.n_max[li] = max(self.n_max[li], n)
            self.hits[li] = max(self.hits[li], 16 * self.n_max[li], self.ix.L + 64)
            self.tuples[li] = max(self.tuples[li], 12 * self.n_max[li] + 1024, self.ix.L + 64)
            fits = tot <= self.hits[li] and tot <= min(self.tuples[li], 65536)
            assert fits == (p not in rerun), (p, n, tot, self.hits[li], self.tuples[li])
            if not fits:          # check_flags: max(2 x capacity, need + 1024) for whichever overflowed
                if tot > self.hits[li]:
                    self.hits[li] = max(2 * self.hits[li], tot + 1024)
                if tot > self.tuples[li]:
                    self.tuples[li] = max(2 * self.tuples[li], tot + 1024)
            first += n
        res = self.sr.search_batch(B, O)
        same(res, want)
        st = self.sr.stats()
        assert st["small_pieces_rerun"] == len(rerun), (st["small_pieces_rerun"], rerun)
        assert st["tree_stalls_recovered"] == 0
        assert st["n_tuples"] == res.user_bin.size == int(want[1][-1]) and st["n_hashes"] == int(want[0].sum())
        return res

    def warm_up(self, rng):
        """a call of 16 384 short random reads: five pieces, so every lane has held 3584 reads and keeps the buffers of that size"""
        reads = [random_read(rng, 40, 48) for _ in range(16384)]
        B, O = cat(reads)
        self.search(reads, self.ix.want(B, O))
        assert self.n_max == [3584] * 4

    def close(self):
        self.sr.close()


# ------------------------------------------------------------------------------------------------ shared, made once
_cache = {}


def shared(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def planted_index(L, runs, seed=1):
    """L leaf runs, genome `seed` planted in `runs` of them, evenly spread over the DFS order"""
    def make():
        g = genome(seed)
        where = sorted({(2 * j + 1) * L // (2 * runs) for j in range(runs)})
        return Index(L, plant=[(keys_of(g), where)], seed=seed), g, len(where)
    return shared(("index", L, runs, seed), make)


def warm_lanes(L):
    """one searcher per index whose four lanes have each held a 3584-read piece; shared by the one-piece cases, which need
    more than the 12 x 512 + 1024 tuples a fresh lane has for 512 reads"""
    def make():
        ix, _, _ = planted_index(L, 24)
        lanes = Lanes(ix)
        lanes.warm_up(np.random.default_rng(L))
        return lanes
    return shared(("lanes", L), make)


def mixed_piece(rng, g, n, wide_at):
    """n reads: wide ones at the given positions, elsewhere random reads (nothing reported) and error-free reads of g in turn"""
    return [wide_read(rng) if i in wide_at else (random_read(rng) if i & 1 else read_of(rng, g)) for i in range(n)]


# ------------------------------------------------------------------------------------------------ a. count of wide reads in one piece
@pytest.mark.parametrize("W", [0, 1, 63, 64, 65, 66, 80, 110])
@pytest.mark.parametrize("L", [65, 70])
def test_count_of_wide_reads_in_one_piece(L, W):
    lanes = warm_lanes(L)
    ix, g, runs = planted_index(L, 24)
    rng = np.random.default_rng(1000 * L + W)
    n = 509                                                             # one piece, the last wave iteration not full
    reads = mixed_piece(rng, g, n, set(rng.choice(n, size=W, replace=False).tolist()))
    want = ix.want(*cat(reads))
    m = per_read(want)
    assert int((m > 64).sum()) == W and int((m == L).sum()) == W and int((m == runs).sum()) > 150
    assert piece_sizes(n) == [n]
    lanes.search(reads, want)


# ------------------------------------------------------------------------------------------------ b. wide reads the old second sweep missed
def test_wide_reads_logged_out_of_read_order():
    """One 512-read piece is 32 iterations of 16 waves; read i is wave i % 16's, iteration i // 16.  Waves 0-7 spend their first 24
    iterations on reads of 24 tuples each (a 24-step shuffle loop per read) and meet wide reads in iterations 24-31: 64 of them.
    Waves 8-15 have reads without a tuple until their wide reads of iterations 30 and 31: 16.  In read order the 49th to 56th wide
    reads are waves 0-7's of iteration 30, the 57th to 64th waves 8-15's, the last 16 iteration 31's.  Waves 8-15 arrive at theirs
    long before waves 0-7 arrive at any: a list of the first 64 arrivals holds those 16 and waves 0-7's first 48, a sweep over
    read-order positions 64 and up adds iteration 31's, and waves 0-7's of iteration 30 -- reads 480 to 487 -- are in neither.
    Against the parent commit's kernel this test failed on an MI355X with eight reads in arrival order: 468, 480 and 482 to 487
    (docs/EXPERIMENTS.md section 15) -- the predicted ones but for 481, which made the list, and 468, which did not."""
    L = 65
    lanes = warm_lanes(L)
    ix, g, runs = planted_index(L, 24)
    rng = np.random.default_rng(7)
    reads = []
    for i in range(512):
        w, it = i % 16, i // 16
        if w < 8:
            reads.append(wide_read(rng) if it >= 24 else read_of(rng, g))
        else:
            reads.append(wide_read(rng) if it >= 30 else random_read(rng))
    want = ix.want(*cat(reads))
    m = per_read(want).reshape(32, 16)
    assert runs == 24 and np.all(m[:24, :8] == 24) and np.all(m[24:, :8] == L)
    assert np.all(m[:30, 8:] == 0) and np.all(m[30:, 8:] == L)
    wide = np.flatnonzero(m.reshape(-1) > 64)
    assert wide.size == 80 and wide[48:56].tolist() == list(range(480, 488)) and wide[56:64].tolist() == list(range(488, 496))
    # a wide read left unsorted would show: its tuples' arrival order (the root's, then the children's) is not the DFS order
    assert not np.array_equal(want[2][int(want[1][480]):int(want[1][481])], np.sort(want[2][int(want[1][480]):int(want[1][481])]))
    lanes.search(reads, want)


# ------------------------------------------------------------------------------------------------ c. tuples per read around the sorters' boundaries
@pytest.mark.parametrize("L", [2, 63, 64, 65, 127, 128, 129, 200])
def test_tuples_per_read_around_the_sorter_boundaries(L):
    """threshold-0 reads of exactly L tuples: the wave rank sort up to 64, the block's sorting network from 65, N at and beside a
    power of two -- on a lane (k_finalize_small) and through the pipeline (k_sort_small / k_sort_big)"""
    ix, g, runs = planted_index(L, min(8, L))
    rng = np.random.default_rng(L)
    n = 305
    reads = mixed_piece(rng, g, n, {0, 17, 150, 151, 304})
    want = ix.want(*cat(reads))
    m = per_read(want)
    assert int((m == L).sum()) >= 5 and m[0] == m[304] == L and int((m == runs).sum()) > 100
    lanes = Lanes(ix)
    lanes.search(reads, want)
    plain = ix.searcher(small_path=False)
    same(plain.search_batch(*cat(reads)), want)
    assert plain.stats()["small_pieces_rerun"] == 0
    plain.close(); lanes.close()


# ------------------------------------------------------------------------------------------------ d. largest pieces and lane reuse
def _many_reads(n, wide_at):
    def make():
        gs = [genome(40 + i) for i in range(6)]
        L = 12
        ix = Index(L, plant=[(keys_of(gs[i]), [(2 * i + j * 5) % L for j in range(1 + i % 3)]) for i in range(6)], seed=3)
        return ix, gs
    ix, gs = shared("index d", make)
    rng = np.random.default_rng(n)
    reads = [wide_read(rng) if i in wide_at else (random_read(rng, 40, 120) if i % 3 == 0 else read_of(rng, gs[i % 6], 40, 120)) for i in range(n)]
    want = ix.want(*cat(reads))
    m = per_read(want)
    assert np.all(m[sorted(wide_at)] == 12) and int(((m >= 1) & (m <= 3)).sum()) > n // 2
    return ix, reads, want


def test_three_pieces_of_exactly_4096_reads():
    """sRoff[n] at n = 4096, thread 1023's four reads, all 16 words of every wave's ballots"""
    n = 14080
    assert piece_sizes(n) == [1792, 4096, 4096, 4096]
    ix, reads, want = _many_reads(n, {0, 5, 1791, 1792, 5887, 5888, 9000, 9983, 9984, 14076, 14077, 14078, 14079})
    lanes = Lanes(ix)
    lanes.search(reads, want)
    lanes.close()


def test_five_pieces_reuse_a_lane():
    """piece 4 runs on lane 0 after piece 0 has been harvested; the call again: every lane's counters came back cleared"""
    n = 16384
    assert piece_sizes(n) == [2048, 3584, 3584, 3584, 3584]
    ix, reads, want = _many_reads(n, {0, 2047, 2048, 9000, 9215, 9216, 12800, 16000, 16383})
    lanes = Lanes(ix)
    for _ in range(2):
        lanes.search(reads, want)
    lanes.close()


def test_one_read_past_the_small_calls():
    """16 385 reads are past SMALL_MAX_READS: the pipeline of large batches, same tuples, nothing counted as a rerun"""
    ix, reads, want = _many_reads(16385, {0, 8000, 16384})
    sr = ix.searcher()
    same(sr.search_batch(*cat(reads)), want)
    assert sr.stats()["small_pieces_rerun"] == 0
    sr.close()


# ------------------------------------------------------------------------------------------------ e. one piece of several overflows
def test_one_piece_of_four_overflows():
    L = 200
    ix, g, runs = planted_index(L, 8)
    rng = np.random.default_rng(5)
    n = 2048
    assert piece_sizes(n) == [512] * 4
    wide_at = set((1024 + rng.choice(512, size=330, replace=False)).tolist()) | {3, 700, 2047}
    reads = mixed_piece(rng, g, n, wide_at)
    want = ix.want(*cat(reads))
    assert int(want[1][1536] - want[1][1024]) > 65536
    lanes = Lanes(ix)
    lanes.search(reads, want, rerun=(2,))
    ordinary = mixed_piece(rng, g, n, {9, 1030, 2000})
    lanes.search(ordinary, ix.want(*cat(ordinary)))
    lanes.close()


# ------------------------------------------------------------------------------------------------ f. the result area's edge
def test_result_area_holds_65536_tuples_and_not_one_more():
    """A lane's tuple scratch is 12 n + 1024 for the largest piece it has held, 50 176 at most on the public route, so the 65 536 of
    the result area are reached only after a rerun has grown the scratch: the first call here overflows on purpose (65 792 tuples),
    and check_flags leaves the lane with 66 816 hits and tuples.  Then 65 536 tuples fit and 65 537 do not."""
    L = 256
    ix, g, runs = planted_index(L, 1)
    rng = np.random.default_rng(6)
    lanes = Lanes(ix)
    prime = [wide_read(rng) for _ in range(257)] + [random_read(rng) for _ in range(255)]
    want = ix.want(*cat(prime))
    assert int(want[1][-1]) == 257 * 256
    lanes.search(prime, want, rerun=(0,))
    assert lanes.hits[0] == lanes.tuples[0] == 66816
    full = mixed_piece(rng, g, 512, set(range(1, 512, 2)))
    full = [random_read(rng) if i % 2 == 0 else r for i, r in enumerate(full)]       # 256 wide reads, 256 that report nothing
    want_full = ix.want(*cat(full))
    assert int(want_full[1][-1]) == 65536
    lanes.search(full, want_full)
    over = list(full)
    over[300] = read_of(rng, g)                                                      # one tuple: the genome's one leaf run
    want_over = ix.want(*cat(over))
    assert runs == 1 and int(want_over[1][-1]) == 65537
    lanes.search(over, want_over, rerun=(0,))
    lanes.search(full, want_full)
    lanes.close()


# ------------------------------------------------------------------------------------------------ g. launch_finalize's block and grid edges
def _wide_batch(L, n, n_random=0):
    def make():
        rng = np.random.default_rng(L * 100000 + n)
        reads = [wide_read(rng) for _ in range(n)] + [random_read(rng) for _ in range(n_random)]
        reads = [reads[i] for i in rng.permutation(len(reads))]
        ix = shared(("index g", L), lambda: Index(L, seed=L))
        want = ix.want(*cat(reads))
        assert int((per_read(want) == L).sum()) == n and int(want[1][-1]) == n * L
        return ix, reads, want
    return shared(("batch g", L, n), make)


@pytest.mark.parametrize("sub_batch_reads", [0, 4096, 4097])
def test_pipeline_finalize_at_its_block_and_grid_edges(sub_batch_reads):
    """small_path=False.  Every read of these batches has 5 tuples and needs sorting: 4095 / 4096 / 4097 / 8193 reads stand at and
    beside the scans' 4096 reads per block, 16 385 are one read past k_sort_small's one grid pass (4096 blocks x 4 waves), and
    sub-batches of 4096 and 4097 reads carry the tuple base from one sub-batch to the next at a block's edge.  300 reads of 70 tuples
    are more than k_sort_big's 256 blocks."""
    for n in (4095, 4096, 4097, 8193, 16385):
        ix, reads, want = _wide_batch(5, n)
        sr = ix.searcher(small_path=False, sub_batch_reads=sub_batch_reads)
        same(sr.search_batch(*cat(reads)), want)
        assert sr.stats()["small_pieces_rerun"] == 0
        sr.close()
    ix, reads, want = _wide_batch(70, 300, n_random=100)
    sr = ix.searcher(small_path=False, sub_batch_reads=sub_batch_reads)
    same(sr.search_batch(*cat(reads)), want)
    sr.close()
