"""Where along a read each reference matched (taxor_gpu_hitmap_*, taxor_amd/csrc/hitmap.hip): map_off, tuple, user_bin, count and hits
equal the CPU expectation (tests/hitmap_expect.py, from the oracle alone) array for array -- they are integers."""
import numpy as np
import pytest

from oracle import oracle as orc
from taxor_amd import GpuIndex, Searcher, _lib, synth
from taxor_amd.search import Hitmap
from tests.coverage_expect import STAGE_CUT, same_results
from tests.hitmap_expect import HitExpect, same, seg, size
from tests.test_gpu_coverage import _cat, _layout

pytestmark = pytest.mark.gpu

COUNTS = [0, 0, 1, 63, 64, 65, 2048, 2049, 5245]


def _prefix_with(g, c):
    """the shortest prefix of g with exactly c distinct hashes: the count ascends with the length, by at most one per base"""
    lo, hi = 22, len(g)
    assert orc.seq_to_syncmers(g).size >= c
    while lo < hi:
        mid = (lo + hi) // 2
        if orc.seq_to_syncmers(g[:mid]).size >= c:
            hi = mid
        else:
            lo = mid + 1
    assert orc.seq_to_syncmers(g[:lo]).size == c
    return g[:lo]


@pytest.fixture(scope="module")
def world():
    g, go = synth.random_genomes(5, 65000, seed=41)
    G = [bytes(g[int(go[i]):int(go[i + 1])]) for i in range(5)]
    planted = [np.unique(orc.seq_to_syncmers(x)) for x in G]
    # keys of genome 0 that genomes 2 and 3 share, for the hash lists made by hand: the first five are in 0 (5 of 5), 2 (4) and 3 (3)
    k0 = planted[0]
    planted[2] = np.unique(np.concatenate([planted[2], k0[:4], k0[10:11]]))
    planted[3] = np.unique(np.concatenate([planted[3], k0[:3]]))
    lay, ub = _layout(planted, seed=42)                  # IXFs of 65, 1, 63 and 64 bins; genome 0 split over two root bins
    host = synth.materialize_host(lay)
    assert sorted(f["bins"] for f in host) == [1, 63, 64, 65]
    # reads of 0, 0, 1, 63, 64, 65 hashes (wave rounds), 2048, 2049 (the piece boundary) and 5245 (three pieces): from the split user
    # bin, from leaves in the root and in every child
    src = {1: G[4][1000:], 63: G[4][3000:], 64: G[1][500:], 65: G[2][700:], 2048: G[0][100:], 2049: G[3][2000:], 5245: G[2][1000:]}
    edge = [b"", b"ACGTACGTAC"] + [_prefix_with(src[c], c) for c in COUNTS[2:]]
    chimera = G[1][20000:26000] + G[3][30000:36000]
    bases, offs, origin = synth.synth_reads(g, go, 40, 1400, error_rate=0.02, frac_random=0.2, seed=43)
    ordinary = [bytes(bases[int(offs[i]):int(offs[i + 1])]) for i in range(40)]
    assert set(int(o) for o in origin) >= {0, 1, 2, 3, 4, -1}
    ordinary.insert(20, b"ACGTTGCA")                      # a read without a hash among ordinary reads
    idx = GpuIndex(host, lay["n_user_bins"])
    reads = edge + [chimera] + ordinary
    e = HitExpect(host)
    e.add_bases(reads)
    w = dict(G=G, planted=planted, lay=lay, ub=ub, host=host, idx=idx, reads=reads, n_edge=len(edge), i_chimera=len(edge), i_empty=len(edge) + 1 + 20,
             expect=e)
    yield w
    idx.close()


def _run(w, hm, reads, sub_batch_reads=0, sr=None, **kw):
    """one batch from bases with capture on, located by hm"""
    own = sr is None
    if own:
        sr = Searcher(w["idx"], sub_batch_reads=sub_batch_reads, **kw)
    sr.capture(True)
    res = sr.search_batch(*_cat(reads))
    sv = sr.take_saved()
    got = hm.add_batch(sr, sv)
    lists = [np.array(sv.hashes[int(sv.hash_off[r]):int(sv.hash_off[r + 1])]) for r in range(len(reads))]
    n_sub = sv.n_sub_batches
    sv.close()
    if own:
        sr.close()
    return got, res, lists, n_sub


@pytest.mark.parametrize("S", [1, 2, 16, 64])
def test_one_batch_equals_the_expectation(world, S):
    w = world
    e = w["expect"]
    with Hitmap(w["idx"], w["host"], segments=S) as hm:
        got, res, lists, _ = _run(w, hm, w["reads"])
    assert [int(x) for x in got.n_hashes[:w["n_edge"]]] == COUNTS
    same(got, e, S)
    assert got.probes > 0 and got.seconds_kernels > 0
    ub = w["ub"]
    # what the reads were chosen for: the split user bin, leaves in the root and in children of 1, 63 and 64 bins, reads of one, two
    # and three pieces, and -- for S above the count -- empty segments
    assert set(int(b) for b in got.user_bin) >= {ub[k] for k in (0, 1, 2, 3, 4, "1 again")}
    if S == 16:
        # the saved list is the oracle's ordered syncmer list of the same read (k22/s12): the feature rests on this
        for r, read in enumerate(w["reads"]):
            want = orc.seq_to_syncmers(read) if len(read) else np.zeros(0, np.uint64)
            assert np.array_equal(lists[r], want), r
        # invariants: a user bin with exactly one leaf technical bin locates every hash the search counted
        one_leaf = [t for t in range(got.count.size) if len(e.leaves[int(got.user_bin[t])]) == 1]
        assert len(one_leaf) > 10 and any(len(e.leaves[int(b)]) == 2 for b in got.user_bin)
        for t in one_leaf:
            assert int(got.hits[t].sum()) == int(got.count[t]), t
        # the tuple indices point at the mapped tuples of the batch CSR
        assert np.array_equal(res.user_bin[got.tuple.astype(np.int64)], got.user_bin) and np.array_equal(res.count[got.tuple.astype(np.int64)], got.count)
    for r in (2, 3):                                     # 1 and 63 hashes
        n = int(got.n_hashes[r])
        for t in range(int(got.map_off[r]), int(got.map_off[r + 1])):
            for j in range(S):
                assert got.hits[t, j] <= size(j, S, n)
            if n < S:
                assert sum(size(j, S, n) == 0 for j in range(S)) == S - n


def test_segment_sizes_sum_to_the_count():
    for S in (1, 2, 3, 16, 63, 64):
        for n in (1, 2, 15, 16, 17, 63, 64, 65, 2048, 2049, 5245, 2**31 - 1):
            sizes = [size(j, S, n) for j in range(S)]
            assert sum(sizes) == n and min(sizes) >= 0
            if n <= 5245:
                cnt = [0] * S
                for i in range(n):
                    cnt[seg(i, S, n)] += 1
                assert cnt == sizes, (S, n)


def test_a_read_without_a_hash_maps_nothing_and_shifts_nothing(world):
    w = world
    with Hitmap(w["idx"], w["host"]) as hm:
        got, res, _, _ = _run(w, hm, w["reads"])
    for r in (0, 1, w["i_empty"]):
        assert got.n_hashes[r] == 0 and got.map_off[r + 1] == got.map_off[r]
        assert res.read_off[r + 1] - res.read_off[r] > 5  # the TSV's zero-count lines are there: every leaf reports
    # the reads behind it are where the expectation puts them, and their tuples are their own
    r = w["i_empty"]
    after = [q for q in range(r + 1, len(w["reads"])) if got.map_off[q + 1] > got.map_off[q]]
    assert len(after) >= 5
    for q in after:
        for t in range(int(got.map_off[q]), int(got.map_off[q + 1])):
            assert res.read_off[q] <= got.tuple[t] < res.read_off[q + 1]


def test_a_chimera_shows_its_halves(world):
    """what a user sees: the first half of the read from genome 1, the second from genome 3.  Searched at --percentage 0.3: under the
    syncmer model's threshold, about half of a read's hashes, only the larger half of such a read is reported at all"""
    w = world
    S = 16
    ub, read = w["ub"], w["reads"][w["i_chimera"]]
    e = HitExpect(w["host"])
    e.add_bases([read], percentage=0.3)
    with Hitmap(w["idx"], w["host"], segments=S) as hm:
        got, _, _, _ = _run(w, hm, [read], percentage=0.3)
    same(got, e, S)
    rows = {int(got.user_bin[t]): (int(got.count[t]), got.hits[t].astype(np.int64)) for t in range(got.count.size)}
    assert {ub[1], ub[3]} <= set(rows)                   # each has at least 0.8 * max: both survive
    (ca, ha), (cb, hb) = rows[ub[1]], rows[ub[3]]
    assert min(ca, cb) >= 0.8 * max(ca, cb) and ha.sum() == ca and hb.sum() == cb
    n = int(got.n_hashes[0])
    sizes = np.array([size(j, S, n) for j in range(S)])
    assert (ha[:7] >= 0.9 * sizes[:7]).all() and ha[9:].sum() <= 0.05 * ca
    assert (hb[9:] >= 0.9 * sizes[9:]).all() and hb[:7].sum() <= 0.05 * cb


def test_the_cut_into_batches_and_sub_batches_does_not_matter(world):
    w = world
    reads, e = w["reads"], w["expect"]
    want = e.arrays(16)
    k = 21
    with Hitmap(w["idx"], w["host"]) as hm:
        sr = Searcher(w["idx"], sub_batch_reads=8)
        whole, _, _, n_sub = _run(w, hm, reads, sr=sr)
        assert n_sub >= 3                                 # one batch spans several sub-batches
        a, ra, _, _ = _run(w, hm, reads[:k], sr=sr)
        b, _, _, _ = _run(w, hm, reads[k:], sr=sr)
        sr.close()
    same(whole, e, 16)
    assert np.array_equal(np.concatenate([a.hits, b.hits]), want["hits"])
    assert np.array_equal(np.concatenate([a.map_off, b.map_off[1:] + a.map_off[-1]]), want["map_off"])
    assert np.array_equal(np.concatenate([a.tuple, b.tuple + np.uint64(ra.user_bin.size)]), want["tuple"])
    assert np.array_equal(np.concatenate([a.user_bin, b.user_bin]), want["user_bin"]) and np.array_equal(np.concatenate([a.count, b.count]), want["count"])


def _replay(idx, seed_read, lists, thr):
    """a captured batch of len(lists) reads of len(lists[0]) hashes each, its hashes and thresholds rewritten, searched again"""
    sr = Searcher(idx)
    sr.capture(True)
    sr.search_batch(*_cat([seed_read] * len(lists)))
    sv = sr.take_saved()
    assert [int(x) for x in sv.n_hashes] == [len(l) for l in lists]
    sv.hashes[:] = np.concatenate(lists)
    sv.threshold[:] = thr
    sr.capture(False)
    res = sr.search_saved(sv)
    return sr, sv, res


def test_the_filter_boundary_through_lists_made_by_hand(world):
    """counts 5, 4 and 3 against a maximum of 5: 4 is exactly 0.8 * 5 and survives, 3 does not; a read with no tuple"""
    w = world
    k0, ub = w["planted"][0], w["ub"]
    five = _prefix_with(w["G"][4][1000:], 5)
    rng = np.random.default_rng(7)
    lists = [k0[:5], k0[10:15], rng.integers(1, 2**63, size=5, dtype=np.uint64), k0[20:25]]
    thr = [1, 1, 5, 5]
    sr, sv, res = _replay(w["idx"], five, lists, thr)
    e = HitExpect(w["host"])
    for h, t in zip(lists, thr):
        e.add_hash_list(h, t)
    tup = dict(zip(*[x.tolist() for x in e.oracle.bulk_contains(lists[0], 1)[:2]]))
    assert (tup[ub[0]], tup[ub[2]], tup[ub[3]]) == (5, 4, 3)
    with Hitmap(w["idx"], w["host"], segments=2) as hm:
        got = hm.add_batch(sr, sv)
    same(got, e, 2)
    first = {int(got.user_bin[t]): int(got.count[t]) for t in range(int(got.map_off[0]), int(got.map_off[1]))}
    assert first == {ub[0]: 5, ub[2]: 4}                  # 4 against 5 kept, 3 dropped
    assert got.map_off[3] == got.map_off[2]               # no tuple
    t2 = [t for t in range(int(got.map_off[0]), int(got.map_off[1])) if got.user_bin[t] == ub[2]][0]
    assert got.hits[t2].tolist() == [3, 1]                # five hashes: ranks 0, 1, 2 | 3, 4; genome 2 holds the first four
    # every mapped tuple, every hash of its read, every leaf bin of its user bin
    assert got.probes == sum(e.cov.lookups(int(got.user_bin[t]), lists[r], False) for r in range(4) for t in range(int(got.map_off[r]), int(got.map_off[r + 1])))
    sv.close()
    sr.close()


def test_a_thousand_tuples_keep_csr_order():
    """one read, 1000 reporting bins, 70 of them at the maximum and the rest at half of it: the 70 come out in CSR order"""
    rng = np.random.default_rng(5)
    bins, n_leaf, n_full, nk = 1030, 1000, 70, 20
    keys = np.unique(rng.integers(1, 2**63, size=nk + 8, dtype=np.uint64))[:nk]
    rng.shuffle(keys)
    full = set(int(x) for x in rng.choice(n_leaf, size=n_full, replace=False))
    nub = [0]

    def new_ub():
        nub[0] += 1
        return nub[0] - 1

    f = dict(bins=bins, stride=(bins + 63) // 64 * 64, keys={}, fname_idx=np.full(bins, -2, dtype=np.int64), child_of={}, max_elems=None)
    for b in range(n_leaf):
        f["keys"][b] = np.sort(keys if b in full else keys[(b % 2)::2])
        f["fname_idx"][b] = new_ub()
    lay = dict(ixfs=synth._finalize_layout([f], new_ub, rng, "host"), n_user_bins=None)
    lay["n_user_bins"] = nub[0]
    host = synth.materialize_host(lay)
    idx = GpuIndex(host, lay["n_user_bins"])
    g, _ = synth.random_genomes(1, 2000, seed=3)
    sr, sv, res = _replay(idx, _prefix_with(bytes(g), nk), [keys], [1])
    e = HitExpect(host)
    e.add_hash_list(keys, 1)
    assert res.user_bin.size >= n_leaf and np.array_equal(res.user_bin, e.oracle.bulk_contains(keys, 1)[0])
    with Hitmap(idx, host, segments=4) as hm:
        got = hm.add_batch(sr, sv)
    same(got, e, 4)
    assert got.count.size == n_full and sorted(int(b) for b in got.user_bin) == sorted(full)
    assert (np.diff(got.tuple.astype(np.int64)) > 0).all() and (got.hits == 5).all()
    sv.close()
    sr.close()
    idx.close()


def test_index_from_the_gpu_builder(world):
    """an IXF built on the device from known key lists: a read made only of bin 9's keys, in order, fills every segment"""
    w = world
    bins, n, S = 64, 6000, 16
    rng = np.random.default_rng(11)
    keys = {b: np.unique(rng.integers(1, 2**63, size=n + 64, dtype=np.uint64))[:n] for b in (2, 9, 40)}
    ixfs = [dict(bins=bins, stride=64, seg_len=synth.seg_len_for(n), seed=1, next_ixf=np.zeros(bins, np.int64), fname_idx=np.arange(bins), data=None)]
    idx = GpuIndex(ixfs, bins)
    idx.fill_random(0, 5)
    idx.build_ixf(0, keys, seed0=3)
    cap = Searcher(w["idx"])
    cap.capture(True)
    cap.search_batch(*_cat([w["reads"][8]]))                                  # the 5245-hash read: as many hashes as wanted
    sv = cap.take_saved()
    m = int(sv.n_hashes[0])
    assert m == 5245
    sv.hashes[:] = keys[9][:m]
    sv.threshold[:] = m
    sr = Searcher(idx)
    res = sr.search_saved(sv)
    assert (9, m) in res.tuples(0)
    with Hitmap(idx, ixfs, segments=S) as hm:
        got = hm.add_batch(sr, sv)
    t = [t for t in range(got.count.size) if got.user_bin[t] == 9]
    assert len(t) == 1 and got.count[t[0]] == m
    assert got.hits[t[0]].tolist() == [size(j, S, m) for j in range(S)]
    sv.close()
    sr.close()
    cap.close()
    idx.close()


def test_refusals_come_before_any_launch(world):
    w = world
    idx = w["idx"]
    for S in (0, 65):
        with pytest.raises(_lib.TaxorError) as ei:
            Hitmap(idx, w["host"], segments=S)
        assert ei.value.code == -1 and "segments" in str(ei.value)
    total = sum(3 * f["seg_len"] * f["stride"] + 8192 for f in w["host"])
    paged = GpuIndex.paged(w["host"], w["lay"]["n_user_bins"], 4 * total)
    with pytest.raises(_lib.TaxorError) as ei:
        Hitmap(paged, w["host"])
    assert ei.value.code == -1 and "paged index" in str(ei.value)
    paged.close()
    reads = w["reads"][w["n_edge"] + 1:]
    sr = Searcher(idx)
    with Hitmap(idx, w["host"]) as hm:
        with pytest.raises(_lib.TaxorError) as ei:
            hm.add_batch(sr, None)
        assert ei.value.code == -1 and "saved" in str(ei.value)
        sr.capture(True)
        sr.search_batch(*_cat(reads[:10]))
        sv10 = sr.take_saved()
        sr.search_batch(*_cat(reads[:12]))
        with pytest.raises(_lib.TaxorError) as ei:                             # a saved batch from another batch
            hm.add_batch(sr, sv10)
        assert ei.value.code == -1 and "n_reads" in str(ei.value)
        sr.search_batch(*_cat(reads[2:12]))                                    # as many reads, other hash counts
        with pytest.raises(_lib.TaxorError) as ei:
            hm.add_batch(sr, sv10)
        assert ei.value.code == -1 and "n_hashes" in str(ei.value)
        other = GpuIndex(w["host"], w["lay"]["n_user_bins"])
        so = Searcher(other)
        so.capture(True)
        so.search_batch(*_cat(reads[:10]))
        with pytest.raises(_lib.TaxorError) as ei:                             # a searcher of another index
            hm.add_batch(so, sv10)
        assert ei.value.code == -1 and "index" in str(ei.value)
        so.close()
        other.close()
        sr.search_batch(*_cat(reads[:10]))                                     # and the batch it belongs to is taken
        got = hm.add_batch(sr, sv10)
        assert got.map_off.size == 11 and got.count.size > 0
        sv10.close()
    sr.close()


def test_the_stage_cut_does_not_matter(world, monkeypatch):
    """staging buffers of 4096 hashes and 3 pieces: the pieces of the reads of 2048, 2049 and 5245 hashes fall into different sets, for
    the lists made by hand as for the reads; a buffer that cannot hold one piece is refused"""
    w = world
    k0 = w["planted"][0]
    lists = [k0[:5], k0[10:15], k0[20:25]]
    sr, sv, _ = _replay(w["idx"], _prefix_with(w["G"][4][1000:], 5), lists, [1, 1, 5])
    by_hand = HitExpect(w["host"])
    for h, t in zip(lists, [1, 1, 5]):
        by_hand.add_hash_list(h, t)
    with Hitmap(w["idx"], w["host"], segments=2) as hm:
        plain_hand = hm.add_batch(sr, sv)
    with Hitmap(w["idx"], w["host"]) as hm:
        plain, _, _, _ = _run(w, hm, w["reads"])
    for k, v in STAGE_CUT.items():
        monkeypatch.setenv(k, v)
    with Hitmap(w["idx"], w["host"], segments=2) as hm:
        cut_hand = hm.add_batch(sr, sv)
    with Hitmap(w["idx"], w["host"]) as hm:
        cut, _, _, _ = _run(w, hm, w["reads"])
    sv.close()
    sr.close()
    same(cut_hand, by_hand, 2)
    same(cut, w["expect"], 16)
    same_results(cut_hand, plain_hand)
    same_results(cut, plain)
    monkeypatch.setenv("TAXOR_STAGE_HASHES", "2047")
    with pytest.raises(_lib.TaxorError) as ei:
        Hitmap(w["idx"], w["host"])
    assert ei.value.code == -1 and "TAXOR_STAGE_HASHES" in str(ei.value)
