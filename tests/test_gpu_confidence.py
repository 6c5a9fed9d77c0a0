"""Hash support behind each LCA call (taxor_gpu_confidence_*, taxor_amd/csrc/confidence.hip): every returned array and both tallies
EQUAL the Python restatement (tests/confidence_expect.py, from the definitions alone) -- they are integers."""
import numpy as np
import pytest

from oracle import oracle as orc
from taxor_amd import GpuIndex, Searcher, _lib, synth
from taxor_amd.search import Confidence, Lca, Lineage
from tests import confidence_expect as ce
from tests import lca_expect as le
from tests.coverage_expect import STAGE_CUT, same_results
from tests.coverage_expect import Expect as CovExpect
from tests.test_gpu_coverage import _cat, _layout
from tests.test_gpu_lca import species

pytestmark = pytest.mark.gpu

DEEP = ";".join(str(5000 + i) for i in range(64))
DEEP_NAMES = ";".join(f"x__D{i}" for i in range(64))
HASH_COUNTS = [0, 1, 63, 64, 65, 2048, 2049, 5245]
TUPLE_COUNTS = [0, 1, 63, 64, 65, 1000]


def world_species(ub, n_user_bins):
    """genome 0 and genome 2 are two species of one genus, genome 3 a genus of their family; genome 1 stands alone, its copy under
    another user bin has the EMPTY path; genome 4 has a path of 64 nodes; every other user bin is a decoy under another root child"""
    named = {ub[0]: ("2;10;100;1000", "k__K;f__F;g__G;s__Sa"), ub[2]: ("2;10;100;1001", "k__K;f__F;g__G;s__Sb"), ub[3]: ("2;10;101;1002", "k__K;f__F;g__H;s__Sc"),
             ub[1]: ("2;20;200;2000", "k__K;f__E;g__I;s__Sd"), ub["1 again"]: ("", ""), ub[4]: (DEEP, DEEP_NAMES)}
    return [species(b, *named[b]) if b in named else species(b, f"3;{9000 + b}", f"k__Decoys;s__Decoy {b}") for b in range(n_user_bins)]


def make_world():
    """host only: test_gpu_hitmap.py's world (five 65-kb genomes; IXFs of 65, 1, 63 and 64 bins; genome 0 split over two root bins)"""
    g, go = synth.random_genomes(5, 65000, seed=41)
    G = [bytes(g[int(go[i]):int(go[i + 1])]) for i in range(5)]
    planted = [np.unique(orc.seq_to_syncmers(x)) for x in G]
    own = [p.copy() for p in planted]
    k0 = planted[0]
    planted[2] = np.unique(np.concatenate([planted[2], k0[:4], k0[10:11]]))      # the first five keys of genome 0: in 0 (5), 2 (4) and 3 (3)
    planted[3] = np.unique(np.concatenate([planted[3], k0[:3]]))
    lay, ub = _layout(planted, seed=42)
    host = synth.materialize_host(lay)
    assert sorted(f["bins"] for f in host) == [1, 63, 64, 65]
    sp = world_species(ub, lay["n_user_bins"])
    return dict(g=g, go=go, G=G, planted=planted, own=own, lay=lay, ub=ub, host=host, sp=sp, cov=CovExpect(host), lin=le.Lineage(sp, lay["n_user_bins"]))


def hand_reads(w):
    """[(what, tuples, hashes)]: tuples and hash lists made by hand -- a count need not be what a search would report"""
    ub, cov, own = w["ub"], w["cov"], w["own"]
    k0 = w["planted"][0]
    rng = np.random.default_rng(17)
    reported = [ub[k] for k in (0, 1, 2, 3, 4, "1 again")]

    def pick(keys, inside, n):
        """the first n of `keys` that match exactly the user bins `inside` among the reported ones"""
        keys = np.asarray(keys[:4 * n + 400], np.uint64)
        m = {b: cov.matches(b, keys) for b in reported}
        ok = np.ones(keys.size, bool)
        for b in reported:
            ok &= m[b] == (b in inside)
        assert ok.sum() >= n, (inside, int(ok.sum()), n)
        return keys[ok][:n]

    none = lambda n: pick(rng.integers(1, 2**63, size=4 * n + 400, dtype=np.uint64), set(), n)
    only0 = lambda n: pick(own[0][20:], {ub[0]}, n)
    only1 = lambda n: pick(own[1], {ub[1], ub["1 again"]}, n)
    only2 = lambda n: pick(own[2], {ub[2]}, n)
    only4 = lambda n: pick(own[4], {ub[4]}, n)
    # a hash found in BOTH parts of the split user bin (one a fingerprint collision): looked up leaf by leaf
    some = np.asarray(k0[:6000], np.uint64)
    parts = []
    for x, j in cov.leaves[ub[0]]:
        rows, fp = cov._probes(x, some)
        d = cov.data[x]
        parts.append((d[rows[:, 0], j] ^ d[rows[:, 1], j] ^ d[rows[:, 2], j]) == fp)
    assert len(parts) == 2
    both = some[parts[0] & parts[1]]
    assert both.size >= 1
    cat = lambda *a: np.concatenate([np.asarray(x, np.uint64) for x in a])
    sib = [(ub[0], 10), (ub[2], 5)]                                              # 5 against 10: the sibling species is no survivor
    reads = [("no tuple", [], k0[:7]), ("all counts zero", [(ub[0], 0), (ub[2], 0)], k0[:7]),
             ("the maximum wins", [(ub[3], 3), (ub[2], 3), (ub[0], 5)], k0[:5]),
             ("both parts of the split bin", [(ub[0], 3)], cat(both[:1], only0(2))),
             ("the empty path: D = 0", [(ub[1], 5), (ub["1 again"], 5)], cat(only1(5), none(3))),
             ("depth 64", [(ub[4], 7)], cat(only4(7), none(2))),
             ("depth 64 beside another", [(ub[4], 7), (ub[1], 2)], cat(only4(3), only1(4), none(3))),
             ("boundary: 5 of 10", [(ub[1], 5)], cat(only1(5), none(5))),
             ("boundary: 4 of 10, a sibling has the fifth", sib, cat(only0(4), only2(1), none(5))),
             ("to the root", [(ub[0], 10), (ub[4], 5)], cat(only0(4), only4(2), none(4))),
             ("dropped", [(ub[0], 10)], cat(only0(2), none(8))),
             ("stays", [(ub[0], 10), (ub[2], 9)], cat(k0[:4], none(2))),
             ("tuples without hashes", sib, [])]
    for n in HASH_COUNTS:                                                         # wave rounds, the piece boundary, three pieces
        hs = cat(k0[:n // 2], none(n - n // 2)) if n else []
        reads.append((f"{n} hashes", [(ub[3], 9), (ub[0], 20), (ub[2], 12)], hs))
    for n in TUPLE_COUNTS:                                                        # tuples repeat user bins: the definitions do not mind
        bins = rng.choice(reported, size=n)
        cnt = rng.integers(0, 30, size=n)
        reads.append((f"{n} tuples", [(int(b), int(c)) for b, c in zip(bins, cnt)], cat(k0[:40], only1(20), only4(10), none(30))))
    return reads


def csr(reads):
    """[(what, tuples, hashes)] -> read_off, user_bin, count, query_len, hash_off, hashes"""
    off = np.cumsum([0] + [len(t) for _, t, _ in reads]).astype(np.uint64)
    hoff = np.cumsum([0] + [len(h) for _, _, h in reads]).astype(np.uint64)
    flat = [x for _, t, _ in reads for x in t]
    hashes = np.concatenate([np.asarray(h, np.uint64) for _, _, h in reads] + [np.zeros(0, np.uint64)])
    return off, np.array([b for b, _ in flat], np.int64), np.array([c for _, c in flat], np.uint32), lens_of(reads), hoff, hashes


def lens_of(reads):
    return [1000 + 7 * i + len(h) for i, (_, _, h) in enumerate(reads)]


@pytest.fixture(scope="module")
def world():
    w = make_world()
    w["idx"] = GpuIndex(w["host"], w["lay"]["n_user_bins"])
    w["glin"] = Lineage(w["sp"], w["lay"]["n_user_bins"])
    w["hand"] = hand_reads(w)
    w["expect"] = {}
    for C in (0.0, 0.5, 1.0):                          # computed once, shared, never changed
        e = ce.Expect(w["lin"], w["cov"], C)
        for (_, t, h), ln in zip(w["hand"], lens_of(w["hand"])):
            e.add(t, h, ln)
        w["expect"][C] = e
    yield w
    w["idx"].close()


def test_the_expectation_holds_every_outcome(world):
    e, what = world["expect"][0.5], [x for x, _, _ in world["hand"]]
    got = {w: ce.outcome(c) for w, c in zip(what, e.calls)}
    assert got["no tuple"] == got["all counts zero"] == "never"
    assert got["boundary: 5 of 10"] == "stays" and got["boundary: 4 of 10, a sibling has the fifth"] == "climbs 1"
    assert got["to the root"] == "root" and got["dropped"] == "dropped" and got["stays"] == "stays"
    c = dict(zip(what, e.calls))
    assert c["the maximum wins"]["lca_depth"] == 4 and c["the maximum wins"]["lca_support"] == 5           # in 0 (4), 2 (3) and 3 (2): every hash at 4
    assert c["both parts of the split bin"]["any_support"] == 3                                             # once, not twice
    assert c["the empty path: D = 0"]["lca_node"] == "1" and c["the empty path: D = 0"]["lca_depth"] == 0
    assert c["depth 64"]["lca_depth"] == 64 and c["depth 64"]["lca_node"] == "5063"
    assert c["boundary: 5 of 10"]["support"] == 5 and c["boundary: 4 of 10, a sibling has the fifth"]["lca_support"] == 4
    assert c["boundary: 4 of 10, a sibling has the fifth"]["node"] == "100" and c["boundary: 4 of 10, a sibling has the fifth"]["support"] == 5
    assert c["dropped"]["support"] == 2 and c["dropped"]["lca_node"] == "1000"
    assert [c[f"{n} hashes"]["n_hashes"] for n in HASH_COUNTS] == HASH_COUNTS
    assert {"never", "stays", "climbs 1", "root", "dropped"} <= set(got.values())


@pytest.mark.parametrize("C", [0.0, 0.5, 1.0])
def test_hand_made_reads_equal_the_expectation(world, C):
    w = world
    e = w["expect"][C]
    with Confidence(w["idx"], w["host"], w["glin"], C) as cf:
        got = cf.add_csr(*csr(w["hand"]))
        t = cf.results()
    ce.same(got, e)
    ce.same_tallies(t, e)
    assert got.probes > 0 and got.seconds_kernels > 0 and 0 < got.tuple_steps <= got.tuple_steps_full


def test_confidence_zero_is_the_plain_lca_and_raising_it_never_deepens(world):
    w = world
    off, ub, cnt, ql, hoff, hashes = csr(w["hand"])
    with Lca(w["idx"], w["glin"]) as lca:
        plain = lca.add_csr(off, ub, cnt, ql)
        pt = lca.results()
    res = {}
    for C in (0.0, 0.5, 1.0):
        with Confidence(w["idx"], w["host"], w["glin"], C) as cf:
            res[C] = (cf.add_csr(off, ub, cnt, ql, hoff, hashes), cf.results())
    zero, zt = res[0.0]
    assert np.array_equal(zero.node, plain.node) and np.array_equal(zero.best, plain.best) and np.array_equal(zero.n_refs, plain.n_refs)
    assert np.array_equal(zt.direct_reads, pt.direct_reads) and np.array_equal(zt.direct_bases, pt.direct_bases)
    for C in (0.0, 0.5, 1.0):
        assert np.array_equal(res[C][0].lca_node, plain.node) and np.array_equal(res[C][0].lca_depth, zero.depth)
    rank = lambda c: np.where(c.node == _lib.LCA_UNCLASSIFIED, -1, c.depth.astype(np.int64))
    assert (rank(res[0.5][0]) <= rank(zero)).all() and (rank(res[1.0][0]) <= rank(res[0.5][0])).all()
    assert (rank(res[1.0][0]) < rank(zero)).any()


def test_two_adds_equal_one_in_either_order(world):
    w = world
    e, hand = w["expect"][0.5], w["hand"]
    k = 14
    for order in ((0, 1), (1, 0)):
        parts = [(0, k), (k, len(hand))]
        with Confidence(w["idx"], w["host"], w["glin"], 0.5) as cf:
            for i in order:
                lo, hi = parts[i]
                off, ub, cnt, _, hoff, hashes = csr(hand[lo:hi])
                ce.same(cf.add_csr(off, ub, cnt, lens_of(hand)[lo:hi], hoff, hashes), e, lo, hi)
            ce.same_tallies(cf.results(), e)


def _search_and_add(w, cf, sr, reads, first=0):
    sr.capture(True)
    res = sr.search_batch(*_cat(reads))
    sv = sr.take_saved()
    got = cf.add_batch(sr, sv, first)
    n_sub = sv.n_sub_batches
    sv.close()
    return got, res, n_sub


def test_add_batch_after_a_real_search(world):
    """the 0.02-error reads and random reads of test_gpu_hitmap.py's world, in one batch of several sub-batches and in two batches"""
    w = world
    bases, offs, origin = synth.synth_reads(w["g"], w["go"], 40, 1400, error_rate=0.02, frac_random=0.2, seed=43)
    reads = [bytes(bases[int(offs[i]):int(offs[i + 1])]) for i in range(40)]
    reads.insert(20, b"ACGTTGCA")                                                 # a read without a hash
    reads.append(w["G"][1][20000:26000] + w["G"][3][30000:36000])                 # a chimera: more than one piece
    e = ce.Expect(w["lin"], w["cov"], 0.5)
    exp = e.add_bases(reads)
    assert {"stays", "never"} <= {ce.outcome(c) for c in exp}
    sr = Searcher(w["idx"], sub_batch_reads=8)
    with Confidence(w["idx"], w["host"], w["glin"], 0.5) as cf:
        got, res, n_sub = _search_and_add(w, cf, sr, reads, first=5)
        assert n_sub >= 3 and got.first_read == 5 and np.array_equal(got.n_hashes, res.n_hashes)
        ce.same(got, e)
        ce.same_tallies(cf.results(), e)
    with Confidence(w["idx"], w["host"], w["glin"], 0.5) as cf:                   # two batches on one searcher
        a, _, _ = _search_and_add(w, cf, sr, reads[:21])
        b, _, _ = _search_and_add(w, cf, sr, reads[21:], first=21)
        ce.same(a, e, 0, 21)
        ce.same(b, e, 21, None)
        ce.same_tallies(cf.results(), e)
    sr.close()


def test_index_from_the_gpu_builder(world):
    """an IXF built on the device from known key lists: a read made of bin 9's keys and bin 40's, a species and another genus"""
    w = world
    bins, n = 64, 3000
    rng = np.random.default_rng(11)
    keys = {b: np.unique(rng.integers(1, 2**63, size=n + 64, dtype=np.uint64))[:n] for b in (2, 9, 40)}
    ixfs = [dict(bins=bins, stride=64, seg_len=synth.seg_len_for(n), seed=1, next_ixf=np.zeros(bins, np.int64), fname_idx=np.arange(bins), data=None)]
    idx = GpuIndex(ixfs, bins)
    idx.fill_random(0, 5)
    idx.build_ixf(0, keys, seed0=3)
    sp = [species(2, "2;10;100;1000", "k__K;f__F;g__G;s__Sa"), species(9, "2;10;100;1001", "k__K;f__F;g__G;s__Sb"), species(40, "2;20;200;2000", "k__K;f__E;g__I;s__Sd")]
    lin = Lineage(sp, bins)
    cap = Searcher(w["idx"])
    cap.capture(True)
    cap.search_batch(*_cat([w["G"][2][1000:30000]]))
    sv = cap.take_saved()
    m = int(sv.n_hashes[0])
    assert m >= 2000
    sv.hashes[:] = np.concatenate([keys[9][:m // 2], keys[40][:m // 4], keys[2][:m - m // 2 - m // 4]])
    sv.threshold[:] = m // 8
    sr = Searcher(idx)
    res = sr.search_saved(sv)
    cnt = dict(res.tuples(0))
    assert cnt[9] >= m // 2 and cnt[40] >= m // 4 and 2 in cnt
    # the restatement over what the builder made: the IXF's bytes and its current seed, downloaded
    built = [dict(ixfs[0], seed=idx.ixf_seed(0), data=idx.download_ixf(0))]
    e = ce.Expect(le.Lineage(sp, bins), CovExpect(built), 0.6)
    c = e.add([(int(b), int(k)) for b, k in res.tuples(0)], np.array(sv.hashes), int(sv.read_len[0]))
    # bin 9 alone survives (m / 2 against m / 4): D = 4 with about half of the hashes, the genus with three quarters, everything at the root
    assert c["lca_depth"] == 4 and c["lca_support"] == cnt[9] and ce.outcome(c) == "climbs 1" and c["node"] == "100" and c["any_support"] >= m - 2
    with Confidence(idx, ixfs, lin, 0.6) as cf:
        got = cf.add_batch(sr, sv)
        t = cf.results()
    ce.same(got, e)
    ce.same_tallies(t, e)
    sv.close()
    sr.close()
    cap.close()
    idx.close()


def test_refusals_come_before_any_launch(world):
    w = world
    idx, nb = w["idx"], w["lay"]["n_user_bins"]
    for C in (-0.01, 1.01, float("nan")):
        with pytest.raises(_lib.TaxorError) as ei:
            Confidence(idx, w["host"], w["glin"], C)
        assert ei.value.code == -1 and "confidence" in str(ei.value)
    other_lin = Lineage(w["sp"][:3], 3)
    with pytest.raises(_lib.TaxorError) as ei:
        Confidence(idx, w["host"], other_lin, 0.5)
    assert ei.value.code == -1 and "n_user_bins" in str(ei.value)
    total = sum(3 * f["seg_len"] * f["stride"] + 8192 for f in w["host"])
    paged = GpuIndex.paged(w["host"], nb, 4 * total)
    with pytest.raises(_lib.TaxorError) as ei:
        Confidence(paged, w["host"], w["glin"], 0.5)
    assert ei.value.code == -1 and "paged index" in str(ei.value)
    paged.close()
    bases, offs, _ = synth.synth_reads(w["g"], w["go"], 12, 1400, error_rate=0.02, seed=44)
    reads = [bytes(bases[int(offs[i]):int(offs[i + 1])]) for i in range(12)]
    sr = Searcher(idx)
    with Confidence(idx, w["host"], w["glin"], 0.5) as cf:
        with pytest.raises(_lib.TaxorError) as ei:                                 # a user bin outside the lineage
            cf.add_csr([0, 1], [nb], [3], [10], [0, 0], [])
        assert ei.value.code == -1 and "user_bin" in str(ei.value) and str(nb) in str(ei.value)
        with pytest.raises(_lib.TaxorError) as ei:
            cf.add_batch(sr, None)
        assert ei.value.code == -1 and "saved" in str(ei.value)
        sr.capture(True)
        sr.search_batch(*_cat(reads[:10]))
        sv10 = sr.take_saved()
        sr.search_batch(*_cat(reads[:12]))
        with pytest.raises(_lib.TaxorError) as ei:                                 # a saved batch from another batch
            cf.add_batch(sr, sv10)
        assert ei.value.code == -1 and "n_reads" in str(ei.value)
        sr.search_batch(*_cat(reads[2:12]))                                        # as many reads, other hash counts
        with pytest.raises(_lib.TaxorError) as ei:
            cf.add_batch(sr, sv10)
        assert ei.value.code == -1 and "n_hashes" in str(ei.value)
        other = GpuIndex(w["host"], nb)
        so = Searcher(other)
        so.capture(True)
        so.search_batch(*_cat(reads[:10]))
        with pytest.raises(_lib.TaxorError) as ei:                                 # a searcher of another index
            cf.add_batch(so, sv10)
        assert ei.value.code == -1 and "index" in str(ei.value)
        so.close()
        other.close()
        t = cf.results()
        assert not t.direct_reads.any() and t.n_reads == 0 and t.seconds_kernel == 0     # nothing was launched
        sr.search_batch(*_cat(reads[:10]))                                         # and the batch it belongs to is taken
        got = cf.add_batch(sr, sv10)
        assert got.node.size == 10 and (got.node != _lib.LCA_UNCLASSIFIED).any()
        sv10.close()
    sr.close()


def test_the_stage_cut_does_not_matter(world, monkeypatch):
    """staging buffers of 4096 hashes and 3 pieces: the pieces of the reads of 2048, 2049 and 5245 hashes fall into different sets.  The
    three counters are printed: the skip schedule is not derived, they are compared between versions of the library"""
    w = world
    e = w["expect"][0.5]
    with Confidence(w["idx"], w["host"], w["glin"], 0.5) as cf:
        plain, plain_t = cf.add_csr(*csr(w["hand"])), cf.results()
    for k, v in STAGE_CUT.items():
        monkeypatch.setenv(k, v)
    with Confidence(w["idx"], w["host"], w["glin"], 0.5) as cf:
        cut, cut_t = cf.add_csr(*csr(w["hand"])), cf.results()
    print("confidence counters (probes, tuple_steps, tuple_steps_full):", plain.probes, plain.tuple_steps, plain.tuple_steps_full)
    ce.same(cut, e)
    ce.same_tallies(cut_t, e)
    same_results(cut, plain)
    same_results(cut_t, plain_t)
