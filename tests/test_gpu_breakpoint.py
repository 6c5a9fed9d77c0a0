"""Where a read switches reference (taxor_gpu_breakpoint_*, taxor_amd/csrc/breakpoint.hip): every word of a batch EQUALS the Python
restatement (tests/breakpoint_expect.py, from the oracle and the definitions alone) -- they are integers."""
import numpy as np
import pytest

from oracle import oracle as orc
from taxor_amd import GpuIndex, Searcher, _lib, synth
from taxor_amd.search import Breakpoints
from tests import breakpoint_expect as be
from tests.coverage_expect import STAGE_CUT, candidate_lookups, same_results
from tests.coverage_expect import Expect as CovExpect
from tests.test_gpu_coverage import _cat
from tests.test_gpu_hitmap import COUNTS, _run, world  # noqa: F401  (the hit map tests' world, reused)

pytestmark = pytest.mark.gpu

BREAKS = [1, 63, 64, 65, 2047, 2048, 2049]
TUPLE_COUNTS = [0, 1, 2, 63, 64, 65]
LOW = 0.003                                              # a threshold a fingerprint collision passes: every read has many candidates


@pytest.fixture(scope="module")
def hand(world):
    """[(what, tuples, hashes)] made by hand from the planted keys, and their expectation -- computed once, shared, never changed"""
    w = world
    ub, cov = w["ub"], w["expect"].cov
    rng = np.random.default_rng(23)
    own1 = np.unique(orc.seq_to_syncmers(w["G"][1]))
    own3 = np.unique(orc.seq_to_syncmers(w["G"][3]))
    a, b, a2 = ub[1], ub[3], ub["1 again"]

    def pick(keys, inside, n):
        keys = np.asarray(keys[:n + n // 8 + 200], np.uint64)
        ok = np.ones(keys.size, bool)
        for x in (a, b, ub[2]):
            ok &= cov.matches(x, keys) == (x in inside)
        assert ok.sum() >= n
        return keys[ok][:n]

    A = pick(own1, {a}, 2200)
    B = pick(own3, {b}, 200)
    none = pick(rng.integers(1, 2**63, size=400, dtype=np.uint64), set(), 60)
    cat = lambda *x: np.concatenate([np.asarray(v, np.uint64) for v in x])
    two = [(a, 5), (b, 5)]
    reads = [(f"break at {p}", two, cat(A[:p], B[:40])) for p in BREAKS]
    reads += [("break at n-1", two, cat(A[:99], B[:1])),
              ("equal splits", two, cat(A[:3], none[:2], B[:3])),
              ("equal prefixes", [(a, 5), (a2, 5), (b, 5)], cat(A[:30], B[:30])),
              ("equal prefixes, the other first", [(a2, 5), (a, 5), (b, 5)], cat(A[:30], B[:30])),
              ("one dominates", [(a, 9), (b, 1)], cat(A[:50], none[:10])),
              ("a zero count between", [(a, 5), (ub[2], 0), (b, 5)], cat(A[:20], B[:20])),
              ("no hash", two, []),
              ("gain 1", two, cat(A[:1], B[:50])), ("gain 4", two, cat(A[:4], B[:50])), ("gain 5", two, cat(A[:5], B[:50]))]
    bins = [a, b, ub[2], ub[4], ub[0], a2]
    for m in TUPLE_COUNTS:                                # tuples repeat user bins: the definitions do not mind
        reads.append((f"{m} tuples", [(int(x), int(c)) for x, c in zip(rng.choice(bins, size=m), rng.integers(1, 30, size=m))], cat(A[:40], none[:9], B[:40])))
    cnt = np.zeros(1000, np.int64)
    cnt[rng.choice(1000, size=70, replace=False)] = rng.integers(1, 30, size=70)
    reads.append(("1000 tuples", [(int(x), int(c)) for x, c in zip(rng.choice(bins, size=1000), cnt)], cat(B[:70], none[:9], A[:70])))
    e = be.BpExpect(cov=cov)
    for _, t, h in reads:
        e.add_read(h, [x for x, _ in t], [c for _, c in t])
    return dict(reads=reads, e=e, a=a, b=b, a2=a2)


def csr(reads):
    off = np.cumsum([0] + [len(t) for _, t, _ in reads]).astype(np.uint64)
    hoff = np.cumsum([0] + [len(h) for _, _, h in reads]).astype(np.uint64)
    flat = [x for _, t, _ in reads for x in t]
    hashes = np.concatenate([np.asarray(h, np.uint64) for _, _, h in reads] + [np.zeros(0, np.uint64)])
    return off, np.array([x for x, _ in flat], np.int64), np.array([c for _, c in flat], np.uint32), hoff, hashes


def test_the_expectation_holds_every_outcome(hand):
    """no case below passes vacuously: what each hand-made read was made for is there in the restatement"""
    x = dict(zip([w for w, _, _ in hand["reads"]], hand["e"].reads))
    a, b, a2 = hand["a"], hand["b"], hand["a2"]
    for p in BREAKS:
        r = x[f"break at {p}"]
        assert r["examined"] and (r["break_hash"], r["bin_a"], r["bin_b"], r["pre_a"], r["suf_b"], r["gain"]) == (p, a, b, p, 40, min(p, 40))
    assert (x["break at n-1"]["break_hash"], x["break at n-1"]["n"], x["break at n-1"]["gain"]) == (99, 100, 1)
    assert (x["equal splits"]["break_hash"], x["equal splits"]["gain"]) == (3, 3)            # split(3) = split(4) = split(5) = 6
    assert (x["equal prefixes"]["bin_a"], x["equal prefixes"]["tuple_a"] - x["equal prefixes"]["tuple_best"]) == (a, 0)
    assert x["equal prefixes, the other first"]["bin_a"] == a2 and x["equal prefixes, the other first"]["n_candidates"] == 3
    assert x["one dominates"]["examined"] and x["one dominates"]["gain"] == 0 and x["one dominates"]["break_hash"] == 0
    assert x["a zero count between"]["n_candidates"] == 2 and x["a zero count between"]["tuple_b"] - x["a zero count between"]["tuple_a"] == 2
    assert not x["no hash"]["examined"]
    assert [x[f"gain {g}"]["gain"] for g in (1, 4, 5)] == [1, 4, 5]
    assert [x[f"{m} tuples"]["examined"] for m in TUPLE_COUNTS] == [False, False] + [True] * 4
    assert [x[f"{m} tuples"]["n_candidates"] for m in TUPLE_COUNTS[2:]] == TUPLE_COUNTS[2:]
    assert x["1000 tuples"]["n_candidates"] == 70 and x["1000 tuples"]["gain"] > 0 and x["1000 tuples"]["bin_a"] == b
    for r in hand["e"].reads:
        assert not r["examined"] or r["gain"] == 0 or r["tuple_a"] != r["tuple_b"]


@pytest.mark.parametrize("G", [1, 5])
def test_hand_made_reads_equal_the_expectation(world, hand, G):
    w, e = world, hand["e"]
    with Breakpoints(w["idx"], w["host"], min_gain=G) as bp:
        got = bp.add_csr(*csr(hand["reads"]))
    be.same(got, e)
    what = [x for x, _, _ in hand["reads"]]
    rep = dict(zip(what, got.reported))
    assert not rep["one dominates"] and not rep["no hash"] and rep["gain 5"] and rep["break at 2048"]
    assert rep["gain 4"] == (G == 1) and rep["gain 1"] == (G == 1)                           # the boundary G - 1 / G
    assert got.lookups > 0 and got.seconds_kernels > 0
    assert got.lookups == candidate_lookups(w["expect"].cov, hand["reads"], 2)               # every candidate of an examined read, every hash
    assert (got.tuple_a[got.gain > 0] != got.tuple_b[got.gain > 0]).all()                    # A != B wherever the split gains


def test_two_adds_and_small_scratch_equal_one(world, hand, monkeypatch):
    """the same CSR in two calls (tuple indices stay those of the arrays given), and under a scratch budget of 64 mask words, which
    cuts the batch into many groups and leaves the reads above it alone in scratch grown to fit"""
    w, e, reads = world, hand["e"], hand["reads"]
    off, ub, cnt, hoff, hashes = csr(reads)
    k = 9
    with Breakpoints(w["idx"], w["host"]) as bp:
        be.same(bp.add_csr(off[:k + 1], ub, cnt, hoff[:k + 1], hashes), e, 0, k)
        be.same(bp.add_csr(off[k:], ub, cnt, hoff[k:], hashes), e, k, None)
    monkeypatch.setenv("TAXOR_TUNING", "1")
    monkeypatch.setenv("TAXOR_BREAKPOINT_BUDGET_WORDS", "64")
    with Breakpoints(w["idx"], w["host"]) as bp:
        be.same(bp.add_csr(off, ub, cnt, hoff, hashes), e)


def test_the_stage_cut_does_not_matter(world, hand, monkeypatch):
    """staging buffers of 4096 hashes and 3 pieces: the pieces of the reads of 2047, 2048 and 2049 + 40 hashes fall into different sets"""
    w, e = world, hand["e"]
    with Breakpoints(w["idx"], w["host"]) as bp:
        plain = bp.add_csr(*csr(hand["reads"]))
    for k, v in STAGE_CUT.items():
        monkeypatch.setenv(k, v)
    with Breakpoints(w["idx"], w["host"]) as bp:
        cut = bp.add_csr(*csr(hand["reads"]))
    be.same(cut, e)
    same_results(cut, plain)


@pytest.fixture(scope="module")
def searched(world):
    """the hit map world's reads (0 .. 5245 hashes, a chimera, ordinary reads, one without a hash) under a threshold a fingerprint
    collision passes: most reads have dozens of candidates"""
    e = be.BpExpect(cov=world["expect"].cov)
    e.add_bases(world["reads"], percentage=LOW)
    return e


def test_a_real_search_equals_the_expectation(world, searched):
    w, e = world, searched
    with Breakpoints(w["idx"], w["host"]) as bp:
        got, res, lists, _ = _run(w, bp, w["reads"], percentage=LOW)
    assert [int(x) for x in got.n_hashes[:w["n_edge"]]] == COUNTS
    assert sorted(f["bins"] for f in w["host"]) == [1, 63, 64, 65]
    be.same(got, e)
    ex = [r for r in e.reads if r["examined"]]
    assert {r["n"] for r in ex} >= set(COUNTS[3:]) and not e.reads[0]["examined"] and not e.reads[w["i_empty"]]["examined"]
    assert any(w["ub"][0] in r["bins"] for r in ex) and max(r["n_candidates"] for r in ex) > 30       # the split user bin; dozens of candidates
    assert any(r["gain"] > 0 for r in ex) and got.lookups > 0
    t = got.tuple_a[got.examined].astype(np.int64)
    assert np.array_equal(res.user_bin[t], got.bin_a[got.examined]) and (res.count[t] > 0).all()        # the indices point into the batch CSR


def test_the_chimera_is_reported_at_its_junction(world):
    """6 kb of genome 1 followed by 6 kb of genome 3, searched at --percentage 0.3 as the hit map test does"""
    w = world
    ub, read = w["ub"], w["reads"][w["i_chimera"]]
    e = be.BpExpect(cov=w["expect"].cov)
    e.add_bases([read], percentage=0.3)
    with Breakpoints(w["idx"], w["host"]) as bp:
        got, _, _, _ = _run(w, bp, [read], percentage=0.3)
    be.same(got, e)
    junction = orc.seq_to_syncmers(read[:6000]).size
    assert got.reported[0] and got.gain[0] > 0 and got.bin_a[0] != got.bin_b[0]
    assert int(got.bin_a[0]) in (ub[1], ub["1 again"]) and int(got.bin_b[0]) == ub[3]      # genome 1 lies under two user bins: the first in CSR order
    # the hashes of the first 6 kb all match genome 1 (the read is error-free), so the break is not in front of `junction`; the 21 k-mers
    # across the junction are in neither genome, and p* is the SMALLEST p at the maximum: it moves past `junction` only over hashes that
    # collide with genome 1's fingerprints, one in 256 each -- three in a row is out of reach
    assert 0 <= int(got.break_hash[0]) - junction <= 3, (int(got.break_hash[0]), junction)
    assert got.pre_a[0] >= 0.95 * junction and got.suf_b[0] >= 0.95 * (int(got.n[0]) - junction - 12)     # 21 k-mers across the junction hold at most some 12 hashes


def test_the_cut_into_batches_and_sub_batches_does_not_matter(world, searched):
    w, e, reads = world, searched, world["reads"]
    k = 21
    with Breakpoints(w["idx"], w["host"]) as bp:
        sr = Searcher(w["idx"], sub_batch_reads=8, percentage=LOW)
        whole, _, _, n_sub = _run(w, bp, reads, sr=sr)
        assert n_sub >= 3                                 # one batch spans several sub-batches
        a, ra, _, _ = _run(w, bp, reads[:k], sr=sr)
        b, _, _, _ = _run(w, bp, reads[k:], sr=sr)
        sr.close()
    be.same(whole, e)
    be.same(a, e, 0, k)
    be.same(b, e, k, None, tuple_shift=int(ra.user_bin.size))


def test_index_from_the_gpu_builder(world):
    """an IXF built on the device from known key lists: a read of bin 9's keys followed by bin 40's breaks where they meet"""
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
        cut = 1300
        sv.hashes[:] = np.concatenate([keys[9][:cut], keys[40][:m - cut]])
        sv.threshold[:] = m // 4
        res = sr.search_saved(sv)
        cnt = dict(res.tuples(0))
        assert cnt[9] >= cut and cnt[40] >= m - cut
        built = [dict(ixfs[0], seed=idx.ixf_seed(0), data=idx.download_ixf(0))]  # the restatement over what the builder made
        e = be.BpExpect(cov=CovExpect(built))
        x = e.add_read(np.array(sv.hashes), [b for b, _ in res.tuples(0)], [c for _, c in res.tuples(0)])
        # single = bin 9's 1300 keys and its fingerprint collisions among bin 40's 748 (one in 256 each, 3 expected: 20 is out of reach)
        assert (x["bin_a"], x["bin_b"], x["break_hash"]) == (9, 40, cut) and m - cut - 20 <= x["gain"] <= m - cut
        with Breakpoints(idx, ixfs) as bp:
            got = bp.add_batch(sr, sv)
        be.same(got, e)
    finally:
        if sv is not None:
            sv.close()
        sr.close()
        cap.close()
        idx.close()


def test_refusals_come_before_any_launch(world):
    w = world
    idx, nb = w["idx"], w["lay"]["n_user_bins"]
    with pytest.raises(_lib.TaxorError) as ei:
        Breakpoints(idx, w["host"], min_gain=0)
    assert ei.value.code == -1 and "min_gain" in str(ei.value)
    total = sum(3 * f["seg_len"] * f["stride"] + 8192 for f in w["host"])
    paged = GpuIndex.paged(w["host"], nb, 4 * total)
    with pytest.raises(_lib.TaxorError) as ei:
        Breakpoints(paged, w["host"])
    assert ei.value.code == -1 and "paged index" in str(ei.value)
    paged.close()
    reads = w["reads"][w["n_edge"] + 1:]
    sr = Searcher(idx)
    with Breakpoints(idx, w["host"]) as bp:
        with pytest.raises(_lib.TaxorError) as ei:                                 # a user bin outside the index
            bp.add_csr([0, 1], [nb], [3], [0, 0], [])
        assert ei.value.code == -1 and "user_bin" in str(ei.value) and str(nb) in str(ei.value)
        with pytest.raises(_lib.TaxorError) as ei:
            bp.add_batch(sr, None)
        assert ei.value.code == -1 and "saved" in str(ei.value)
        sr.capture(True)
        sr.search_batch(*_cat(reads[:10]))
        sv10 = sr.take_saved()
        sr.search_batch(*_cat(reads[:12]))
        with pytest.raises(_lib.TaxorError) as ei:                                 # a saved batch from another batch
            bp.add_batch(sr, sv10)
        assert ei.value.code == -1 and "n_reads" in str(ei.value)
        sr.search_batch(*_cat(reads[2:12]))                                        # as many reads, other hash counts
        with pytest.raises(_lib.TaxorError) as ei:
            bp.add_batch(sr, sv10)
        assert ei.value.code == -1 and "n_hashes" in str(ei.value)
        other = GpuIndex(w["host"], nb)
        so = Searcher(other)
        so.capture(True)
        so.search_batch(*_cat(reads[:10]))
        with pytest.raises(_lib.TaxorError) as ei:                                 # a searcher of another index
            bp.add_batch(so, sv10)
        assert ei.value.code == -1 and "index" in str(ei.value)
        so.close()
        other.close()
        sr.search_batch(*_cat(reads[:10]))                                         # and the batch it belongs to is taken
        got = bp.add_batch(sr, sv10)
        assert got.examined.size == 10
        sv10.close()
    sr.close()
