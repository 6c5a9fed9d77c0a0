"""Hashes only one reference explains (taxor_gpu_exclusive_*, taxor_amd/csrc/exclusive.hip): every word of a batch, the four sums per user
bin and every register byte EQUAL the Python restatement (tests/exclusive_expect.py, from the oracle and the definitions alone) -- they
are integers."""
import numpy as np
import pytest

from oracle import oracle as orc
from taxor_amd import GpuIndex, Searcher, _lib, synth
from taxor_amd.search import Exclusive
from tests import exclusive_expect as xe
from tests.coverage_expect import STAGE_CUT, candidate_lookups, same_results
from tests.coverage_expect import Expect as CovExpect
from tests.test_gpu_coverage import _cat
from tests.test_gpu_hitmap import COUNTS, _run, world  # noqa: F401  (the hit map tests' world, reused)

pytestmark = pytest.mark.gpu

LENGTHS = [0, 1, 63, 64, 65, 2048, 2049]                 # wave rounds and the piece edge
CANDIDATES = [0, 1, 2, 64, 65]
LOW = 0.003                                              # a threshold a fingerprint collision passes: every read has many candidates


def hand_reads(w):
    """[(what, tuples, hashes)] made by hand from the planted keys; needs the world's host arrays and oracle only, no device"""
    ub, cov, nb = w["ub"], w["expect"].cov, w["lay"]["n_user_bins"]
    rng = np.random.default_rng(29)
    own1 = np.unique(orc.seq_to_syncmers(w["G"][1]))
    own3 = np.unique(orc.seq_to_syncmers(w["G"][3]))
    a, b, a2 = ub[1], ub[3], ub["1 again"]
    named = [ub[0], a, ub[2], b, ub[4], a2]

    def pick(keys, inside, n):
        """the first n of `keys` that exactly the user bins `inside`, of the six named ones, hold"""
        keys = np.asarray(keys[:n + n // 8 + 200], np.uint64)
        ok = np.ones(keys.size, bool)
        for x in named:
            ok &= cov.matches(x, keys) == (x in inside)
        assert ok.sum() >= n, (inside, int(ok.sum()), n)
        return keys[ok][:n]

    A = pick(own1, {a, a2}, 2100)                         # genome 1 lies under two user bins: held by one candidate, or by two
    B = pick(own3, {b}, 200)
    none = pick(rng.integers(1, 2**63, size=400, dtype=np.uint64), set(), 60)
    every = pick(w["planted"][0][:3], {ub[0], ub[2], b}, 2)     # the world planted genome 0's first keys in genomes 2 and 3 as well
    cat = lambda *x: np.concatenate([np.asarray(v, np.uint64) for v in x])

    def mix(n):
        nb_, nn = min(n // 4, 150), min(n // 8, 40)
        h = cat(A[:n - nb_ - nn], B[:nb_], none[:nn])
        assert h.size == n
        return h[rng.permutation(n)]                      # every round holds lanes of every kind

    two = [(a, 5), (b, 5)]
    reads = [(f"{n} hashes", two, mix(n)) for n in LENGTHS]
    reads += [("held by one", two, cat(A[:40], B[:30], none[:10])),
              ("held by two", [(a, 5), (a2, 4), (b, 5)], cat(A[:40], B[:30], none[:10])),
              ("held by all", [(ub[0], 5), (ub[2], 5), (b, 5)], cat(every, B[:30], none[:10])),
              ("a zero count between", [(a, 5), (a2, 0), (b, 5)], cat(A[:20], B[:20])),
              ("a user bin twice", [(b, 5), (a, 3), (b, 2)], cat(A[:20], B[:20], none[:5])),
              ("one candidate", [(b, 7)], cat(B[:70], A[:9], none[:9])),
              ("only zero counts", [(a, 0), (b, 0)], cat(A[:5], B[:5])),
              ("the split user bin", [(ub[0], 9), (b, 3)], cat(w["planted"][0][100:180], B[:20]))]
    for m in CANDIDATES:                                  # distinct user bins, the two planted ones among them from 2 on; one with count 0 beside
        bins = [int(x) for x in rng.permutation([x for x in range(nb) if x not in (a, b)])[:max(m - 2, 0)]]
        t = ([(b, 4)] if m == 1 else [(a, 4), (b, 4)] if m >= 2 else []) + [(x, int(rng.integers(1, 30))) for x in bins]
        t = [t[i] for i in rng.permutation(len(t))]
        reads.append((f"{m} candidates", t[:len(t) // 2] + [(ub[4], 0)] + t[len(t) // 2:], cat(A[:60], none[:9], B[:61])[rng.permutation(130)]))
    return dict(reads=reads, a=a, b=b, a2=a2)


@pytest.fixture(scope="module")
def hand(world):
    """the hand-made reads and their expectation -- computed once, shared, never changed"""
    out = hand_reads(world)
    e = xe.ExExpect(cov=world["expect"].cov)
    for _, t, h in out["reads"]:
        e.add_read(h, [x for x, _ in t], [c for _, c in t])
    return dict(out, e=e)


def csr(reads):
    off = np.cumsum([0] + [len(t) for _, t, _ in reads]).astype(np.uint64)
    hoff = np.cumsum([0] + [len(h) for _, _, h in reads]).astype(np.uint64)
    flat = [x for _, t, _ in reads for x in t]
    hashes = np.concatenate([np.asarray(h, np.uint64) for _, _, h in reads] + [np.zeros(0, np.uint64)])
    return off, np.array([x for x, _ in flat], np.int64), np.array([c for _, c in flat], np.uint32), hoff, hashes


def check_outcomes(hand):
    """no case passes vacuously: what each hand-made read was made for is there in the restatement"""
    x = dict(zip([w for w, _, _ in hand["reads"]], hand["e"].reads))
    a, b = hand["a"], hand["b"]
    of = lambda r, bin_: [c for c in r["cands"] if c["cand_bin"] == bin_]
    assert not x["0 hashes"]["examined"] and [x[f"{n} hashes"]["n"] for n in LENGTHS[1:]] == LENGTHS[1:]
    r = x["2049 hashes"]
    assert of(r, a)[0]["cand_excl"] == 2049 - 150 - 40 and of(r, b)[0]["cand_excl"] == 150 and r["shared"] == 0 and r["matched"] == 2049 - 40
    r = x["held by one"]
    assert (of(r, a)[0]["cand_excl"], of(r, b)[0]["cand_excl"], r["shared"], r["matched"]) == (40, 30, 0, 70)
    r = x["held by two"]
    assert (of(r, a)[0]["cand_excl"], of(r, hand["a2"])[0]["cand_excl"], of(r, b)[0]["cand_excl"], r["shared"], r["matched"]) == (0, 0, 30, 40, 70)
    r = x["held by all"]
    assert r["shared"] == 2 and r["matched"] == 32 and of(r, b)[0]["cand_excl"] == 30 and of(r, b)[0]["cand_hits"] == 32
    r = x["a zero count between"]
    assert r["n_candidates"] == 2 and r["cands"][1]["cand_tuple"] - r["cands"][0]["cand_tuple"] == 2 and r["shared"] == 0
    r = x["a user bin twice"]
    assert [c["cand_excl"] for c in r["cands"]] == [0, 20, 0] and r["shared"] == 20 and [c["cand_hits"] for c in r["cands"]] == [20, 20, 20]
    r = x["one candidate"]
    assert r["examined"] and r["n_candidates"] == 1 and r["cands"][0]["cand_excl"] == r["cands"][0]["cand_hits"] == 70 == r["matched"] and r["shared"] == 0
    assert not x["only zero counts"]["examined"] and x["only zero counts"]["n_candidates"] == 0
    assert x["the split user bin"]["cands"][0]["cand_excl"] >= 78                 # both parts of the split bin are looked up
    assert [x[f"{m} candidates"]["examined"] for m in CANDIDATES] == [False] + [True] * 4
    assert [x[f"{m} candidates"]["n_candidates"] for m in CANDIDATES] == CANDIDATES
    r = x["65 candidates"]                                                        # 63 foreign bins answer yes at 1/256 each: some hash is shared
    assert r["shared"] > 0 and of(r, a)[0]["cand_excl"] < 60 and sum(c["cand_hits"] for c in r["cands"] if c["cand_bin"] not in (a, b)) > 0


def test_the_expectation_holds_every_outcome(hand):
    check_outcomes(hand)


@pytest.mark.parametrize("P", [4, 12, 16])
def test_hand_made_reads_equal_the_expectation(world, hand, P):
    w, e = world, hand["e"]
    with Exclusive(w["idx"], w["host"], precision=P) as ex:
        got = ex.add_csr(*csr(hand["reads"]))
        table = ex.results()
    xe.same(got, e)
    xe.same_table(table, e, P)
    assert got.probes > 0 and got.seconds_kernels > 0 and table.probes == got.probes
    assert got.probes == candidate_lookups(w["expect"].cov, hand["reads"], 1)                # every candidate of an examined read, every hash
    b = hand["b"]
    assert table.exclusive_hits[b] > 150 and table.exclusive_reads[b] >= 10 and table.registers[b].any()
    est = table.distinct(b)                               # 200 distinct keys of genome 3 were ever exclusive to it, and a few collisions
    assert 1 <= est and (P < 12 or abs(est - len(e.owned[b])) <= 0.1 * len(e.owned[b]))


def test_precision_zero_is_twelve_and_others_are_refused(world):
    w = world
    with Exclusive(w["idx"], w["host"]) as ex:
        assert ex.results().precision == 12
    for p in (3, 17):
        with pytest.raises(_lib.TaxorError) as ei:
            Exclusive(w["idx"], w["host"], precision=p)
        assert ei.value.code == -1 and "precision" in str(ei.value)


def test_one_read_fifty_times(world, hand):
    """fifty waves raise the same registers and add to the same four sums"""
    w = world
    read = dict(zip([x for x, _, _ in hand["reads"]], hand["reads"]))["held by two"]
    e = xe.ExExpect(cov=w["expect"].cov)
    for _ in range(50):
        e.add_read(read[2], [x for x, _ in read[1]], [c for _, c in read[1]])
    with Exclusive(w["idx"], w["host"]) as ex:
        got = ex.add_csr(*csr([read] * 50))
        table = ex.results()
    xe.same(got, e)
    xe.same_table(table, e)
    assert table.cand_reads[hand["b"]] == 50 and table.exclusive_hits[hand["b"]] == 50 * 30 and table.exclusive_reads[hand["a"]] == 0


def test_two_adds_in_either_order_equal_one(world, hand):
    """the same CSR in two calls (tuple indices stay those of the arrays given); the run's table does not depend on the order"""
    w, e, reads = world, hand["e"], hand["reads"]
    off, ub, cnt, hoff, hashes = csr(reads)
    k = 9
    tables = []
    for first in (True, False):
        with Exclusive(w["idx"], w["host"]) as ex:
            parts = [(off[:k + 1], hoff[:k + 1], 0, k), (off[k:], hoff[k:], k, None)]
            for o, ho, lo, hi in parts if first else parts[::-1]:
                xe.same(ex.add_csr(o, ub, cnt, ho, hashes), e, lo, hi)
            tables.append(ex.results())
    for t in tables:
        xe.same_table(t, e)


@pytest.fixture(scope="module")
def searched(world):
    """the hit map world's reads (0 .. 5245 hashes, a chimera, ordinary reads, one without a hash) under a threshold a fingerprint
    collision passes: most reads have dozens of candidates"""
    e = xe.ExExpect(cov=world["expect"].cov)
    e.add_bases(world["reads"], percentage=LOW)
    return e


def test_a_real_search_equals_the_expectation(world, searched):
    w, e = world, searched
    with Exclusive(w["idx"], w["host"]) as ex:
        got, res, lists, _ = _run(w, ex, w["reads"], percentage=LOW)
        table = ex.results()
    assert [int(x) for x in got.n_hashes[:w["n_edge"]]] == COUNTS
    assert sorted(f["bins"] for f in w["host"]) == [1, 63, 64, 65]
    xe.same(got, e)
    xe.same_table(table, e)
    exd = [r for r in e.reads if r["examined"]]
    assert {r["n"] for r in exd} >= set(COUNTS[3:]) and not e.reads[0]["examined"] and not e.reads[w["i_empty"]]["examined"]
    assert any(c["cand_bin"] == w["ub"][0] for r in exd for c in r["cands"]) and max(r["n_candidates"] for r in exd) > 30     # the split user bin; dozens of candidates
    assert any(r["shared"] > 0 for r in exd) and any(c["cand_excl"] > 0 for r in exd for c in r["cands"]) and got.probes > 0
    t = got.cand_tuple.astype(np.int64)
    assert np.array_equal(res.user_bin[t], got.cand_bin) and np.array_equal(res.count[t], got.cand_count) and (got.cand_count > 0).all()


def test_the_cut_into_batches_and_sub_batches_does_not_matter(world, searched):
    w, e, reads = world, searched, world["reads"]
    k = 21
    with Exclusive(w["idx"], w["host"]) as ex:
        sr = Searcher(w["idx"], sub_batch_reads=8, percentage=LOW)
        whole, _, _, n_sub = _run(w, ex, reads, sr=sr)
        assert n_sub >= 3                                 # one batch spans several sub-batches
        one = ex.results()
    with Exclusive(w["idx"], w["host"]) as ex:
        b, _, _, _ = _run(w, ex, reads[k:], sr=sr)        # the later reads first
        a, ra, _, _ = _run(w, ex, reads[:k], sr=sr)
        two = ex.results()
        sr.close()
    xe.same(whole, e)
    xe.same(a, e, 0, k)
    xe.same(b, e, k, None, tuple_shift=int(ra.user_bin.size))
    xe.same_table(one, e)
    xe.same_table(two, e)


def test_index_from_the_gpu_builder(world):
    """an IXF built on the device from known key lists: bin 9's keys, 200 of which bin 2 holds as well, followed by bin 40's"""
    w = world
    bins, n = 64, 3000
    rng = np.random.default_rng(13)
    keys = {b: np.unique(rng.integers(1, 2**63, size=n + 64, dtype=np.uint64))[:n] for b in (2, 9, 40)}
    keys[2] = np.unique(np.concatenate([keys[2][:n - 200], keys[9][:200]]))
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
        cut = 1300
        sv.hashes[:] = np.concatenate([keys[9][:cut], keys[40][:m - cut]])
        sv.threshold[:] = 100
        res = sr.search_saved(sv)
        cnt = dict(res.tuples(0))
        assert cnt[9] >= cut and cnt[40] >= m - cut and cnt[2] >= 200
        built = [dict(ixfs[0], seed=idx.ixf_seed(0), data=idx.download_ixf(0))]  # the restatement over what the builder made
        e = xe.ExExpect(cov=CovExpect(built))
        x = e.add_read(np.array(sv.hashes), [b for b, _ in res.tuples(0)], [c for _, c in res.tuples(0)])
        by = {c["cand_bin"]: c for c in x["cands"]}
        # bin 9 keeps its 1100 keys that bin 2 lacks, less the fingerprint collisions with bins 2 and 40 (one in 256 each: 50 is out of reach)
        assert x["n_candidates"] == 3 and 200 <= x["shared"] <= 250 and 1050 <= by[9]["cand_excl"] <= 1100 and m - cut - 30 <= by[40]["cand_excl"] <= m - cut
        with Exclusive(idx, ixfs) as ex:
            got = ex.add_batch(sr, sv)
            table = ex.results()
        xe.same(got, e)
        xe.same_table(table, e)
    finally:
        if sv is not None:
            sv.close()
        sr.close()
        cap.close()
        idx.close()


def test_refusals_come_before_any_launch(world):
    w = world
    idx, nb = w["idx"], w["lay"]["n_user_bins"]
    total = sum(3 * f["seg_len"] * f["stride"] + 8192 for f in w["host"])
    paged = GpuIndex.paged(w["host"], nb, 4 * total)
    with pytest.raises(_lib.TaxorError) as ei:
        Exclusive(paged, w["host"])
    assert ei.value.code == -1 and "paged index" in str(ei.value)
    paged.close()
    reads = w["reads"][w["n_edge"] + 1:]
    sr = Searcher(idx)
    with Exclusive(idx, w["host"]) as ex:
        with pytest.raises(_lib.TaxorError) as ei:                                 # a user bin outside the index
            ex.add_csr([0, 1], [nb], [3], [0, 0], [])
        assert ei.value.code == -1 and "user_bin" in str(ei.value) and str(nb) in str(ei.value)
        with pytest.raises(_lib.TaxorError) as ei:
            ex.add_batch(sr, None)
        assert ei.value.code == -1 and "saved" in str(ei.value)
        sr.capture(True)
        sr.search_batch(*_cat(reads[:10]))
        sv10 = sr.take_saved()
        sr.search_batch(*_cat(reads[:12]))
        with pytest.raises(_lib.TaxorError) as ei:                                 # a saved batch from another batch
            ex.add_batch(sr, sv10)
        assert ei.value.code == -1 and "n_reads" in str(ei.value)
        sr.search_batch(*_cat(reads[2:12]))                                        # as many reads, other hash counts
        with pytest.raises(_lib.TaxorError) as ei:
            ex.add_batch(sr, sv10)
        assert ei.value.code == -1 and "n_hashes" in str(ei.value)
        other = GpuIndex(w["host"], nb)
        so = Searcher(other)
        so.capture(True)
        so.search_batch(*_cat(reads[:10]))
        with pytest.raises(_lib.TaxorError) as ei:                                 # a searcher of another index
            ex.add_batch(so, sv10)
        assert ei.value.code == -1 and "index" in str(ei.value)
        so.close()
        other.close()
        assert not ex.results().cand_reads.any()                                   # nothing of the refused calls was counted
        sr.search_batch(*_cat(reads[:10]))                                         # and the batch it belongs to is taken
        got = ex.add_batch(sr, sv10)
        assert got.examined.size == 10
        empty = ex.add_csr([0], [], [], [0], [])                                   # a batch without a read
        assert empty.examined.size == 0 and [int(v) for v in empty.cand_off] == [0]
        sv10.close()
    sr.close()


def test_the_stage_cut_does_not_matter(world, hand, monkeypatch):
    """staging buffers of 4096 hashes and 3 pieces: the pieces of the reads of 2047, 2048 and 2049 hashes fall into different sets"""
    w, e = world, hand["e"]
    with Exclusive(w["idx"], w["host"]) as ex:
        plain, plain_table = ex.add_csr(*csr(hand["reads"])), ex.results()
    for k, v in STAGE_CUT.items():
        monkeypatch.setenv(k, v)
    with Exclusive(w["idx"], w["host"]) as ex:
        cut, cut_table = ex.add_csr(*csr(hand["reads"])), ex.results()
    xe.same(cut, e)
    xe.same_table(cut_table, e)
    same_results(cut, plain)
    same_results(cut_table, plain_table)
