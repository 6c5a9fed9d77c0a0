"""Paint a read with its references (taxor_gpu_segments_*, taxor_amd/csrc/segments.hip): every word and every segment of a batch EQUALS
the Python restatement (tests/segments_expect.py, from the oracle and the definitions alone) -- they are integers."""
import numpy as np
import pytest

from oracle import oracle as orc
from taxor_amd import GpuIndex, Searcher, _lib, synth
from taxor_amd.search import Segments
from tests import segments_expect as se
from tests.coverage_expect import candidate_lookups
from tests.coverage_expect import Expect as CovExpect
from tests.test_gpu_coverage import _cat
from tests.test_gpu_hitmap import COUNTS, _run, world  # noqa: F401  (the hit map tests' world, reused)

pytestmark = pytest.mark.gpu

SIZES = [0, 1, 63, 64, 65, 128, 2047, 2048, 2049, 5245]
TUPLE_COUNTS = [0, 1, 2, 3, 63, 64, 65, 130]
COSTS = [1, 2, 16, 2**20]
LOW = 0.003                                              # a threshold a fingerprint collision passes: every read has many candidates


@pytest.fixture(scope="module")
def hand(world):
    """[(what, tuples, hashes)] made by hand from the planted keys, and their expectation under every cost -- computed once, shared,
    never changed"""
    w = world
    ub, cov = w["ub"], w["expect"].cov
    rng = np.random.default_rng(29)
    a, b, c, a2, d, f = ub[1], ub[3], ub[2], ub["1 again"], ub[4], ub[0]
    own = {x: np.unique(orc.seq_to_syncmers(w["G"][g])) for x, g in ((a, 1), (b, 3), (c, 2))}

    def pick(keys, inside, n):
        keys = np.asarray(keys[:n + n // 8 + 200], np.uint64)
        ok = np.ones(keys.size, bool)
        for x in (a, b, c, d, f):
            ok &= cov.matches(x, keys) == (x in inside)
        assert ok.sum() >= n
        return keys[ok][:n]

    A, B, C = pick(own[a], {a}, 2700), pick(own[b], {b}, 2700), pick(own[c], {c}, 200)
    none = pick(rng.integers(1, 2**63, size=600, dtype=np.uint64), set(), 200)
    cat = lambda *x: np.concatenate([np.asarray(v, np.uint64) for v in x] + [np.zeros(0, np.uint64)])
    two = [(a, 5), (b, 5)]
    reads = [(f"A|B of {n}", two, cat(A[:n - n // 2], B[:n // 2])) for n in SIZES]
    alt = np.empty(128, np.uint64)
    alt[0::2], alt[1::2] = A[:64], B[:64]
    reads += [("A|B|A", two, cat(A[:300], B[:100], A[300:600])),
              ("A|B|A across pieces", two, cat(A[:1000], B[:49], A[1000:2000])),
              ("A|B|C", [(a, 5), (b, 5), (c, 5)], cat(A[:100], B[:100], C[:100])),
              ("A|B|A|B|C", [(a, 5), (b, 5), (c, 5)], cat(A[:40], B[:40], A[40:80], B[40:80], C[:40])),
              ("a short insert", two, cat(A[:200], B[:20], A[200:400])),
              ("alternation", two, alt),
              ("an empty stretch between", two, cat(A[:50], none[:30], B[:50])),
              ("nothing but ties", [(a, 5), (a2, 5)], A[:70]),
              ("twins and a partner", [(a, 5), (a2, 5), (b, 5)], cat(A[:30], B[:30])),
              ("twins the other way", [(a2, 5), (a, 5), (b, 5)], cat(A[:30], B[:30])),
              ("a zero count between", [(a, 5), (c, 0), (b, 5)], cat(A[:20], B[:20])),
              ("one candidate", [(a, 5), (b, 0)], cat(A[:20], B[:20])),
              ("no hash", two, [])]
    bins = [a, b, c, d, f, a2]
    for m in TUPLE_COUNTS:                                # tuples repeat user bins: the definitions do not mind
        reads.append((f"{m} tuples", [(int(x), int(k)) for x, k in zip(rng.choice(bins, size=m), rng.integers(1, 30, size=m))], cat(A[:40], none[:9], B[:40], C[:30])))
    # 130 candidates, the partners on either side of the chunk edge at 64; then twins on either side of it
    def wide(at):
        t = [(d, 1)] * 130
        for i, x in at.items():
            t[i] = (x, 5)
        return t
    reads += [("across the chunk edge, downwards", wide({70: a, 3: b}), cat(A[:60], B[:60])),
              ("across the chunk edge, upwards", wide({5: a, 100: b}), cat(A[:60], B[:60])),
              ("twins across the chunk edge", wide({10: a, 80: a2, 129: b}), cat(A[:60], B[:60])),
              ("twins across the chunk edge, the other way", wide({10: a2, 80: a, 64: b}), cat(B[:60], A[:60]))]
    cnt = np.zeros(1000, np.int64)
    cnt[rng.choice(1000, size=70, replace=False)] = rng.integers(1, 30, size=70)
    reads.append(("1000 tuples", [(int(x), int(k)) for x, k in zip(rng.choice(bins, size=1000), cnt)], cat(B[:70], none[:9], A[:70])))
    exp = {}
    for L in COSTS:
        exp[L] = se.SgExpect(cov=cov, L=L)
        for _, t, h in reads:
            exp[L].add_read(h, [x for x, _ in t], [k for _, k in t])
    return dict(reads=reads, e=exp, a=a, b=b, c=c, a2=a2)


def csr(reads):
    off = np.cumsum([0] + [len(t) for _, t, _ in reads]).astype(np.uint64)
    hoff = np.cumsum([0] + [len(h) for _, _, h in reads]).astype(np.uint64)
    flat = [x for _, t, _ in reads for x in t]
    hashes = np.concatenate([np.asarray(h, np.uint64) for _, _, h in reads] + [np.zeros(0, np.uint64)])
    return off, np.array([x for x, _ in flat], np.int64), np.array([k for _, k in flat], np.uint32), hoff, hashes


def test_the_expectation_holds_every_outcome(hand):
    """no case below passes vacuously: what each hand-made read was made for is there in the restatement"""
    what = [w for w, _, _ in hand["reads"]]
    a, b, c, a2 = hand["a"], hand["b"], hand["c"], hand["a2"]
    x = dict(zip(what, hand["e"][16].reads))
    e16 = hand["e"][16]
    bins = lambda r: [g["bin"] for g in r["segs"]]
    for n in SIZES:
        r = x[f"A|B of {n}"]
        assert r["examined"] == (n > 0) and r["n"] == n
        if n >= 63:                                       # the boundary stands where the keys change
            assert r["n_segments"] == 2 and bins(r) == [a, b] and r["segs"][0]["end"] == n - n // 2 and r["path_hits"] == n
    assert x["A|B of 1"]["n_segments"] == 1
    assert bins(x["A|B|A"]) == [a, b, a] and bins(x["A|B|A across pieces"]) == [a, b, a] and x["A|B|A across pieces"]["segs"][1]["start"] == 1000
    assert bins(x["A|B|C"]) == [a, b, c] and bins(x["A|B|A|B|C"]) == [a, b, a, b, c]
    assert x["a short insert"]["n_segments"] == 1 and x["a short insert"]["path_hits"] == 400                # 20 hits do not pay 2 * 16
    assert bins(dict(zip(what, hand["e"][2].reads))["a short insert"]) == [a, b, a]
    assert x["alternation"]["n_segments"] == 1 and dict(zip(what, hand["e"][1].reads))["alternation"]["n_segments"] == 1      # a switch that only ties is not taken
    assert x["nothing but ties"]["n_segments"] == 1 and x["nothing but ties"]["bin_best"] == a
    assert bins(x["twins and a partner"]) == [a, b] and bins(x["twins the other way"]) == [a2, b]
    assert x["a zero count between"]["n_candidates"] == 2 and x["a zero count between"]["segs"][1]["tuple"] - x["a zero count between"]["segs"][0]["tuple"] == 2
    assert not x["one candidate"]["examined"] and not x["no hash"]["examined"]
    assert [x[f"{m} tuples"]["examined"] for m in TUPLE_COUNTS] == [False, False] + [True] * 6
    assert [x[f"{m} tuples"]["n_candidates"] for m in TUPLE_COUNTS[2:]] == TUPLE_COUNTS[2:]
    # the partners of a read with more than 64 candidates stand on either side of the chunk edge; twins: the lower index
    dn, up = x["across the chunk edge, downwards"], x["across the chunk edge, upwards"]
    assert [g["c"] for g in dn["segs"]] == [70, 3] and [g["c"] for g in up["segs"]] == [5, 100] and dn["n_candidates"] == 130
    assert [g["c"] for g in x["twins across the chunk edge"]["segs"]] == [10, 129] and [g["c"] for g in x["twins across the chunk edge, the other way"]["segs"]] == [64, 10]
    assert x["1000 tuples"]["n_candidates"] == 70
    ks = {r["n_segments"] for r in e16.reads}
    assert {0, 1, 2, 3} <= ks and max(ks) > 3
    assert {e16.shape(r) for r in range(len(what)) if e16.reported(r)} == {"split", "insert", "mosaic"}
    assert all(r["n_segments"] <= 1 for r in hand["e"][2**20].reads) and any(r["n_segments"] == 1 for r in hand["e"][2**20].reads)
    sw = lambda r: r["n_segments"]
    assert sum(map(sw, hand["e"][1].reads)) >= sum(map(sw, hand["e"][2].reads)) >= sum(map(sw, e16.reads)) > sum(map(sw, hand["e"][2**20].reads))
    # an empty stretch between A and B: every boundary in it scores the same.  Through the stretch V_b rides on J, which stands still, so
    # sw_b is a tie there and stays unset; its last set bit is at the stretch's first hash, and that is where the recurrence puts the boundary
    assert [(g["start"], g["end"]) for g in x["an empty stretch between"]["segs"]] == [(0, 50), (50, 130)]


@pytest.mark.parametrize("L", COSTS)
def test_hand_made_reads_equal_the_expectation(world, hand, L):
    w, e = world, hand["e"][L]
    with Segments(w["idx"], w["host"], switch_cost=L) as sg:
        got = sg.add_csr(*csr(hand["reads"]))
    se.same(got, e)
    assert got.lookups > 0 and got.seconds_kernels > 0
    assert got.lookups == candidate_lookups(w["expect"].cov, hand["reads"], 2)               # every candidate of an examined read, every hash
    if L == 2**20:
        assert got.n_reported == 0 and got.seg_off[-1] == 0


def test_two_adds_and_small_scratch_equal_one(world, hand, monkeypatch):
    """the same CSR in two calls (tuple indices stay those of the arrays given), and under a scratch budget of 64 mask words, which
    cuts the batch into many groups and leaves the reads above it alone in scratch grown to fit"""
    w, e, reads = world, hand["e"][16], hand["reads"]
    off, ub, cnt, hoff, hashes = csr(reads)
    k = 12
    with Segments(w["idx"], w["host"]) as sg:
        assert sg.switch_cost == 16
        se.same(sg.add_csr(off[:k + 1], ub, cnt, hoff[:k + 1], hashes), e, 0, k)
        se.same(sg.add_csr(off[k:], ub, cnt, hoff[k:], hashes), e, k, None)
        se.same(sg.add_csr(off[:1], ub, cnt, hoff[:1], hashes), e, 0, 0)               # an empty batch
        assert sg.add_csr(off, ub, cnt, hoff, hashes).n_groups == 1 and sg.add_csr(off[:1], ub, cnt, hoff[:1], hashes).n_groups == 0
    # the cut the budget makes, restated: a read joins the group while the group's mask words stay within the budget; else it opens one
    words = [x["n_candidates"] * ((x["n"] + 63) // 64) for x in e.reads if x["examined"]]
    groups, cur = 0, None
    for mw in words:
        if cur is None or cur + mw > 64:
            groups, cur = groups + 1, 0
        cur += mw
    assert 10 < groups < len(words) and max(words) > 64 * 4            # many groups, several reads in some, and reads far above the budget alone
    monkeypatch.setenv("TAXOR_TUNING", "1")
    monkeypatch.setenv("TAXOR_SEGMENTS_BUDGET_WORDS", "64")
    with Segments(w["idx"], w["host"]) as sg:
        got = sg.add_csr(off, ub, cnt, hoff, hashes)
    se.same(got, e)
    assert got.n_groups == groups                                       # the knob was heard: it moved the cut, and no result


@pytest.fixture(scope="module")
def searched(world):
    """the hit map world's reads (0 .. 5245 hashes, a chimera, ordinary reads, one without a hash) under a threshold a fingerprint
    collision passes: most reads have dozens of candidates.  Cost 2: collisions then pay for a switch now and then"""
    e = se.SgExpect(cov=world["expect"].cov, L=2)
    e.add_bases(world["reads"], percentage=LOW)
    return e


def test_a_real_search_equals_the_expectation(world, searched):
    w, e = world, searched
    with Segments(w["idx"], w["host"], switch_cost=2) as sg:
        got, res, lists, _ = _run(w, sg, w["reads"], percentage=LOW)
    assert [int(x) for x in got.n_hashes[:w["n_edge"]]] == COUNTS
    assert sorted(f["bins"] for f in w["host"]) == [1, 63, 64, 65]
    se.same(got, e)
    ex = [r for r in e.reads if r["examined"]]
    assert {r["n"] for r in ex} >= set(COUNTS[3:]) and not e.reads[0]["examined"] and not e.reads[w["i_empty"]]["examined"]
    assert any(w["ub"][0] in r["bins"] for r in ex) and max(r["n_candidates"] for r in ex) > 30       # the split user bin; dozens of candidates
    assert any(r["n_segments"] >= 2 for r in ex) and any(r["n_segments"] == 1 for r in ex) and got.lookups > 0
    t = got.seg_tuple.astype(np.int64)
    assert np.array_equal(res.user_bin[t], got.seg_bin) and (res.count[t] > 0).all()                  # the indices point into the batch CSR


def test_planted_reads_come_out_as_split_and_insert(world):
    """6 kb of genome 4 followed by 6 kb of genome 2, and 6 kb of genome 4 with 3 kb of genome 3 in the middle, under the default cost"""
    w = world
    ub, G = w["ub"], w["G"]
    reads = [G[4][10000:16000] + G[2][30000:36000], G[4][20000:26000] + G[3][30000:33000] + G[4][26000:32000]]
    e = se.SgExpect(cov=w["expect"].cov)
    e.add_bases(reads, percentage=0.1)
    bins = lambda r: [g["bin"] for g in e.reads[r]["segs"]]
    assert (bins(0), e.shape(0)) == ([ub[4], ub[2]], "split") and (bins(1), e.shape(1)) == ([ub[4], ub[3], ub[4]], "insert")
    # the 21 k-mers across a junction are in neither genome: a boundary lies within a dozen hashes of it
    assert abs(e.reads[0]["segs"][0]["end"] - orc.seq_to_syncmers(reads[0][:6000]).size) <= 14
    assert abs(e.reads[1]["segs"][1]["start"] - orc.seq_to_syncmers(reads[1][:6000]).size) <= 14
    with Segments(w["idx"], w["host"]) as sg:
        got, _, _, _ = _run(w, sg, reads, percentage=0.1)
    se.same(got, e)
    assert [int(k) for k in got.n_segments] == [2, 3] and [int(x) for x in got.seg_bin] == [ub[4], ub[2], ub[4], ub[3], ub[4]]


def test_the_cut_into_batches_and_sub_batches_does_not_matter(world, searched):
    w, e, reads = world, searched, world["reads"]
    k = 21
    with Segments(w["idx"], w["host"], switch_cost=2) as sg:
        sr = Searcher(w["idx"], sub_batch_reads=8, percentage=LOW)
        whole, _, _, n_sub = _run(w, sg, reads, sr=sr)
        assert n_sub >= 3                                 # one batch spans several sub-batches
        a, ra, _, _ = _run(w, sg, reads[:k], sr=sr)
        b, _, _, _ = _run(w, sg, reads[k:], sr=sr)
        sr.close()
    se.same(whole, e)
    se.same(a, e, 0, k)
    se.same(b, e, k, None, tuple_shift=int(ra.user_bin.size))


def test_index_from_the_gpu_builder(world):
    """an IXF built on the device from known key lists: a read of bin 9's keys with bin 40's in the middle is an insert"""
    w = world
    bins, n = 64, 3000
    rng = np.random.default_rng(11)
    keys = {b: np.unique(rng.integers(1, 2**63, size=n + 64, dtype=np.uint64))[:n] for b in (2, 9, 40)}
    ixfs = [dict(bins=bins, stride=64, seg_len=synth.seg_len_for(n), seed=1, next_ixf=np.zeros(bins, np.int64), fname_idx=np.arange(bins), data=None)]
    idx = GpuIndex(ixfs, bins)
    idx.fill_random(0, 5)
    idx.build_ixf(0, keys, seed0=3)
    cap, sr, sv = Searcher(w["idx"]), Searcher(idx), None
    try:                                                                         # whatever fails below, nothing of the device is left to the interpreter's exit
        cap.capture(True)
        cap.search_batch(*_cat([w["reads"][6]]))                                 # the 2048-hash read
        sv = cap.take_saved()
        m = int(sv.n_hashes[0])
        assert m == 2048
        sv.hashes[:] = np.concatenate([keys[9][:900], keys[40][:500], keys[9][900:1548]])
        sv.threshold[:] = m // 5
        res = sr.search_saved(sv)
        cnt = dict(res.tuples(0))
        assert cnt[9] >= 1548 and cnt[40] >= 500
        built = [dict(ixfs[0], seed=idx.ixf_seed(0), data=idx.download_ixf(0))]  # the restatement over what the builder made
        e = se.SgExpect(cov=CovExpect(built))
        x = e.add_read(np.array(sv.hashes), [b for b, _ in res.tuples(0)], [c for _, c in res.tuples(0)])
        assert [(g["bin"], g["start"], g["end"]) for g in x["segs"]] == [(9, 0, 900), (40, 900, 1400), (9, 1400, 2048)] and e.shape(0) == "insert"
        with Segments(idx, ixfs) as sg:
            got = sg.add_batch(sr, sv)
        se.same(got, e)
    finally:
        if sv is not None:
            sv.close()
        sr.close()
        cap.close()
        idx.close()


def test_refusals_come_before_any_launch(world):
    w = world
    idx, nb = w["idx"], w["lay"]["n_user_bins"]
    for cost in (0, 2**20 + 1):
        with pytest.raises(_lib.TaxorError) as ei:
            Segments(idx, w["host"], switch_cost=cost)
        assert ei.value.code == -1 and "switch_cost" in str(ei.value)
    total = sum(3 * f["seg_len"] * f["stride"] + 8192 for f in w["host"])
    paged = GpuIndex.paged(w["host"], nb, 4 * total)
    with pytest.raises(_lib.TaxorError) as ei:
        Segments(paged, w["host"])
    assert ei.value.code == -1 and "paged index" in str(ei.value)
    paged.close()
    reads = w["reads"][w["n_edge"] + 1:]
    sr = Searcher(idx)
    with Segments(idx, w["host"]) as sg:
        with pytest.raises(_lib.TaxorError) as ei:                                 # a user bin outside the index
            sg.add_csr([0, 1], [nb], [3], [0, 0], [])
        assert ei.value.code == -1 and "user_bin" in str(ei.value) and str(nb) in str(ei.value)
        with pytest.raises(_lib.TaxorError) as ei:
            sg.add_batch(sr, None)
        assert ei.value.code == -1 and "saved" in str(ei.value)
        sr.capture(True)
        sr.search_batch(*_cat(reads[:10]))
        sv10 = sr.take_saved()
        sr.search_batch(*_cat(reads[:12]))
        with pytest.raises(_lib.TaxorError) as ei:                                 # a saved batch from another batch
            sg.add_batch(sr, sv10)
        assert ei.value.code == -1 and "n_reads" in str(ei.value)
        sr.search_batch(*_cat(reads[2:12]))                                        # as many reads, other hash counts
        with pytest.raises(_lib.TaxorError) as ei:
            sg.add_batch(sr, sv10)
        assert ei.value.code == -1 and "n_hashes" in str(ei.value)
        other = GpuIndex(w["host"], nb)
        so = Searcher(other)
        so.capture(True)
        so.search_batch(*_cat(reads[:10]))
        with pytest.raises(_lib.TaxorError) as ei:                                 # a searcher of another index
            sg.add_batch(so, sv10)
        assert ei.value.code == -1 and "index" in str(ei.value)
        so.close()
        other.close()
        sr.search_batch(*_cat(reads[:10]))                                         # and the batch it belongs to is taken
        got = sg.add_batch(sr, sv10)
        assert got.examined.size == 10
        sv10.close()
    sr.close()
