"""Distinct matched hashes per user bin (taxor_gpu_coverage_*, taxor_amd/csrc/coverage.hip): reads, hash_matches and the sketches'
registers equal the CPU expectation (tests/coverage_expect.py, from the oracle alone) array for array -- they are integers."""
import math

import numpy as np
import pytest

from oracle import oracle as orc
from taxor_amd import GpuIndex, Searcher, _lib, synth
from taxor_amd.search import Coverage
from tests.coverage_expect import STAGE_CUT, Expect, same, same_results

pytestmark = pytest.mark.gpu


def _cat(reads):
    off = np.zeros(len(reads) + 1, np.uint64)
    off[1:] = np.cumsum([len(r) for r in reads])
    return np.frombuffer(b"".join(reads), np.uint8), off


def _layout(planted, seed):
    """root of 65 bins: genome 0 split over bins 0 and 1 (one user bin), genome 1 a leaf at bin 3, merged bins 10, 11, 12 ->
      A (1 bin): genome 2      B (63 bins): genome 3 at its last bin      C (64 bins): genome 4, and a copy of genome 1 under a user
      bin of its own (one hash list, two references)"""
    rng = np.random.default_rng(seed)
    nub = [0]

    def new_ub():
        nub[0] += 1
        return nub[0] - 1

    ixfs = []

    def new_ixf(bins):
        ixfs.append(dict(bins=bins, stride=(bins + 63) // 64 * 64, keys={}, fname_idx=np.full(bins, -2, dtype=np.int64), child_of={}, max_elems=None))
        return len(ixfs) - 1

    def leaf(i, bins_, keys):
        ub = new_ub()
        for j, b in enumerate(bins_):
            ixfs[i]["keys"][b] = keys[j::len(bins_)]
            ixfs[i]["fname_idx"][b] = ub
        return ub

    def child(i, b, bins):
        c = new_ixf(bins)
        ixfs[i]["fname_idx"][b] = -1
        ixfs[i]["child_of"][b] = c
        return c

    root = new_ixf(65)
    ub = {0: leaf(root, [0, 1], planted[0]), 1: leaf(root, [3], planted[1])}
    A, B, Cc = child(root, 10, 1), child(root, 11, 63), child(root, 12, 64)
    ub[2] = leaf(A, [0], planted[2])
    ub[3] = leaf(B, [62], planted[3])
    ub[4] = leaf(Cc, [63], planted[4])
    ub["1 again"] = leaf(Cc, [5], planted[1])
    out = synth._finalize_layout(ixfs, new_ub, rng, "host")
    return dict(ixfs=out, n_user_bins=nub[0]), ub


def _prefix_with(g, counts):
    """prefix lengths of g whose reads have exactly the given numbers of distinct hashes (a prefix gains at most one per base)"""
    want, found = set(counts), {}
    for n in range(22, len(g)):
        c = orc.seq_to_syncmers(g[:n]).size
        if c in want and c not in found:
            found[c] = n
            if len(found) == len(want):
                break
    assert set(found) == want, (want, found)
    return found


@pytest.fixture(scope="module")
def world():
    g, go = synth.random_genomes(5, 65000, seed=41)
    G = [bytes(g[int(go[i]):int(go[i + 1])]) for i in range(5)]
    planted = [np.unique(orc.seq_to_syncmers(x)) for x in G]
    # keys of genome 0 that genomes 2 and 3 share, for the hash lists made by hand: the first five are in 0 (5 of 5), 2 (4) and 3 (3);
    # of the next five one is in 2
    k0 = planted[0]
    planted[2] = np.unique(np.concatenate([planted[2], k0[:4], k0[10:11]]))
    planted[3] = np.unique(np.concatenate([planted[3], k0[:3]]))
    lay, ub = _layout(planted, seed=42)
    host = synth.materialize_host(lay)
    assert sorted(f["bins"] for f in host) == [1, 63, 64, 65]
    pre = _prefix_with(G[4][1000:], (1, 5, 63, 64, 65))
    edge = [b"", b"ACGTACGTAC"] + [G[4][1000:1000 + pre[c]] for c in (1, 5, 63, 64, 65)] + [G[3][2000:62000]]
    bases, offs, origin = synth.synth_reads(g, go, 60, 1400, error_rate=0.02, frac_random=0.2, seed=43)
    ordinary = [bytes(bases[int(offs[i]):int(offs[i + 1])]) for i in range(60)]
    assert set(int(o) for o in origin) >= {0, 1, 2, 3, 4, -1}
    idx = GpuIndex(host, lay["n_user_bins"])
    w = dict(G=G, planted=planted, lay=lay, ub=ub, host=host, idx=idx, reads=edge + ordinary, pre=pre, n_edge=len(edge), origin=origin)
    yield w
    idx.close()


def _run(w, cov, reads, sub_batch_reads=0, sr=None):
    """one batch from bases with capture on, added to cov"""
    own = sr is None
    if own:
        sr = Searcher(w["idx"], sub_batch_reads=sub_batch_reads)
    sr.capture(True)
    res = sr.search_batch(*_cat(reads))
    sv = sr.take_saved()
    cov.add_batch(sr, sv)
    out = (res, [int(x) for x in sv.n_hashes], sv.n_sub_batches)
    sv.close()
    if own:
        sr.close()
    return out


@pytest.fixture(scope="module")
def expect_all(world):
    """the expectation of the whole read set, once; the per-read survivors beside it"""
    e = Expect(world["host"])
    surv = e.add_bases(world["reads"])
    return e, surv


def test_one_batch_equals_the_expectation(world, expect_all):
    w = world
    e, surv = expect_all
    with Coverage(w["idx"], w["host"]) as cov:
        res, nh, _ = _run(w, cov, w["reads"])
        t = cov.results()
    assert nh[:7] == [0, 0, 1, 5, 63, 64, 65] and nh[7] > 4500              # past the 2048-hash split of a read, twice
    same(t, e)
    ub = w["ub"]
    # what the reads were chosen for: a split user bin, leaves in the root and in children of 1, 63 and 64 bins, a read with no
    # tuple, and one hash list that raises two sketches
    for k in (0, 1, 2, 3, 4, "1 again"):
        assert t.reads[ub[k]] > 0 and t.registers[ub[k]].any(), k
    assert any(len(s) == 0 for s in surv[w["n_edge"]:]) and any(len(s) >= 2 for s in surv)
    both = [s for s in surv if {ub[1], ub["1 again"]} <= {b for b, _ in s}]
    assert both
    assert t.probes > 0 and t.seconds_kernels > 0
    # every surviving tuple of every read, every hash of the read, every leaf bin of the tuple's user bin
    assert t.probes == sum(e.lookups(b, range(nh[r]), False) for r, s in enumerate(surv) for b, _ in s)
    # genome 3's bin (the long read's ~5000 hashes among them): the estimate stands within four standard errors of the exact count
    d = t.distinct(ub[3])
    n = len(e.matched[ub[3]])
    assert abs(d - n) <= 4 * 1.04 / 64 * n + 1, (d, n)


def test_the_same_read_fifty_times(world):
    w = world
    read = w["reads"][w["n_edge"] + int(np.argmax(w["origin"] == 2))]
    one, fifty = Expect(w["host"]), Expect(w["host"])
    s1 = one.add_bases([read])
    fifty.add_bases([read], times=50)
    assert s1[0], "the read matches nothing"
    with Coverage(w["idx"], w["host"]) as a, Coverage(w["idx"], w["host"]) as b:
        _run(w, a, [read])
        _run(w, b, [read] * 50, sub_batch_reads=16)
        ta, tb = a.results(), b.results()
    same(ta, one)
    same(tb, fifty)
    bsel, c = s1[0][0]
    assert tb.reads[bsel] == 50 and tb.hash_matches[bsel] == 50 * c and ta.reads[bsel] == 1
    assert np.array_equal(ta.registers, tb.registers) and ta.distinct(bsel) == tb.distinct(bsel)


def test_two_adds_equal_one_in_either_order(world, expect_all):
    w = world
    e, _ = expect_all
    X, Y = w["reads"][:31], w["reads"][31:]
    sr = Searcher(w["idx"], sub_batch_reads=8)
    tabs = []
    for order in ((X, Y), (Y, X), (X + Y,)):
        with Coverage(w["idx"], w["host"]) as cov:
            for part in order:
                _, _, n_sub = _run(w, cov, part, sr=sr)
                assert n_sub >= 3                         # one batch spans several sub-batches: several staged groups
            tabs.append(cov.results())
    sr.close()
    for t in tabs:
        same(t, e)


@pytest.mark.parametrize("p", [4, 16])
def test_other_precisions(world, expect_all, p):
    w = world
    with Coverage(w["idx"], w["host"], precision=p) as cov:
        _run(w, cov, w["reads"])
        same(cov.results(), expect_all[0], p)


def test_hash_lists_made_by_hand(world):
    """the filter's boundary through replayed lists: a captured batch of four 5-hash reads has its hashes and thresholds rewritten --
    counts 5, 4 and 3 against a max of 5 (4 kept, 3 dropped), a read whose filter drops all but one tuple, a read with no tuple"""
    w = world
    k0, ub = w["planted"][0], w["ub"]
    five = w["reads"][3]
    rng = np.random.default_rng(7)
    lists = [k0[:5], k0[10:15], rng.integers(1, 2**63, size=5, dtype=np.uint64), k0[20:25]]
    thr = [1, 1, 5, 5]
    sr = Searcher(w["idx"])
    sr.capture(True)
    sr.search_batch(*_cat([five] * 4))
    sv = sr.take_saved()
    assert [int(x) for x in sv.n_hashes] == [5, 5, 5, 5]
    sv.hashes[:] = np.concatenate(lists)
    sv.threshold[:] = thr
    sr.capture(False)
    sr.search_saved(sv)
    e = Expect(w["host"])
    surv = [e.add_hash_list(h, t) for h, t in zip(lists, thr)]
    tup = dict(zip(*[x.tolist() for x in e.oracle.bulk_contains(lists[0], 1)[:2]]))
    assert (tup[ub[0]], tup[ub[2]], tup[ub[3]]) == (5, 4, 3)
    assert sorted(surv[0]) == sorted([(ub[0], 5), (ub[2], 4)])                # 4 against 5 kept, 3 dropped
    assert surv[1] == [(ub[0], 5)] and len(e.oracle.bulk_contains(lists[1], 1)[0]) >= 2      # all but one dropped
    assert surv[2] == []                                                        # no tuple
    with Coverage(w["idx"], w["host"]) as cov:
        cov.add_batch(sr, sv)
        t = cov.results()
    same(t, e)
    assert t.reads[ub[0]] == 3 and t.reads[ub[2]] == 1 and t.reads[ub[3]] == 0 and t.hash_matches[ub[2]] == 4
    sv.close()
    sr.close()


def test_refusals_come_before_any_launch(world):
    w = world
    idx = w["idx"]
    for p in (3, 17):
        with pytest.raises(_lib.TaxorError) as ei:
            Coverage(idx, w["host"], precision=p)
        assert ei.value.code == -1 and "precision" in str(ei.value)
    total = sum(3 * f["seg_len"] * f["stride"] + 8192 for f in w["host"])
    paged = GpuIndex.paged(w["host"], w["lay"]["n_user_bins"], 4 * total)
    with pytest.raises(_lib.TaxorError) as ei:
        Coverage(paged, w["host"])
    assert ei.value.code == -1 and "paged index" in str(ei.value)
    paged.close()
    sr = Searcher(idx)
    with Coverage(idx, w["host"]) as cov:
        sr.search_batch(*_cat(w["reads"][:10]))                                # capture off: there is no saved batch to give
        with pytest.raises(_lib.TaxorError) as ei:
            sr.take_saved()
        assert "capture is off" in str(ei.value)
        with pytest.raises(_lib.TaxorError) as ei:
            cov.add_batch(sr, None)
        assert ei.value.code == -1 and "saved" in str(ei.value)
        sr.capture(True)
        sr.search_batch(*_cat(w["reads"][:10]))
        sv10 = sr.take_saved()
        sr.search_batch(*_cat(w["reads"][:12]))
        with pytest.raises(_lib.TaxorError) as ei:                             # a saved batch from another batch
            cov.add_batch(sr, sv10)
        assert ei.value.code == -1 and "n_reads" in str(ei.value)
        sr.search_batch(*_cat(w["reads"][2:12]))                               # as many reads, other hash counts
        with pytest.raises(_lib.TaxorError) as ei:
            cov.add_batch(sr, sv10)
        assert ei.value.code == -1 and "n_hashes" in str(ei.value)
        other = GpuIndex(w["host"], w["lay"]["n_user_bins"])
        so = Searcher(other)
        so.capture(True)
        so.search_batch(*_cat(w["reads"][:10]))
        with pytest.raises(_lib.TaxorError) as ei:                             # a searcher of another index
            cov.add_batch(so, sv10)
        assert ei.value.code == -1 and "index" in str(ei.value)
        so.close()
        other.close()
        t = cov.results()
        assert not t.reads.any() and not t.registers.any() and t.probes == 0  # nothing was launched
        sv10.close()
    sr.close()


def test_index_from_the_gpu_builder(world):
    """an IXF built on the device from known key lists: a read made only of bin 9's keys -- all of them -- gives the list's length"""
    w = world
    bins, n = 64, 6000
    rng = np.random.default_rng(11)
    keys = {b: np.unique(rng.integers(1, 2**63, size=n + 64, dtype=np.uint64))[:n] for b in (2, 9, 40)}
    ixfs = [dict(bins=bins, stride=64, seg_len=synth.seg_len_for(n), seed=1, next_ixf=np.zeros(bins, np.int64), fname_idx=np.arange(bins), data=None)]
    idx = GpuIndex(ixfs, bins)
    idx.fill_random(0, 5)
    idx.build_ixf(0, keys, seed0=3)
    cap = Searcher(w["idx"])
    cap.capture(True)
    cap.search_batch(*_cat([w["reads"][7]]))                                  # the long read: as many hashes as wanted
    sv = cap.take_saved()
    m = int(sv.n_hashes[0])
    assert 4500 < m <= n
    sv.hashes[:] = keys[9][:m]
    sv.threshold[:] = m
    sr = Searcher(idx)
    res = sr.search_saved(sv)
    assert (9, m) in res.tuples(0)
    with Coverage(idx, ixfs) as cov:
        cov.add_batch(sr, sv)
        t = cov.results()
    assert t.reads[9] == 1 and t.hash_matches[9] == m and int(t.reads.sum()) == 1
    d = t.distinct(9)
    print(f"list of {m} keys: estimate {d}")
    assert abs(d - m) <= 4 * 1.04 / math.sqrt(4096) * m
    sv.close()
    sr.close()
    cap.close()
    idx.close()


def test_the_stage_cut_does_not_matter(world, expect_all, monkeypatch):
    """staging buffers of 4096 hashes and 3 pieces: the pieces of the long read fall into different sets"""
    w = world
    e, _ = expect_all
    with Coverage(w["idx"], w["host"]) as cov:
        _run(w, cov, w["reads"])
        plain = cov.results()
    for k, v in STAGE_CUT.items():
        monkeypatch.setenv(k, v)
    with Coverage(w["idx"], w["host"]) as cov:
        _run(w, cov, w["reads"])
        cut = cov.results()
    same(cut, e)
    same_results(cut, plain)
