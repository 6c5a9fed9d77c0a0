"""Syncmer indexes with s-mer sizes 17 to 31: the wide (64-bit s-mer value) instantiation of k_syncmers against the CPU oracle
and, where oracle/_ref/ holds the reference's own selector and k <= 31, against wyhash of the reference's selection.

Selector: all 120 (k, s) with 17 <= s < k <= 32 at t in {1, w//2, w}, on reads at the edges of the kernel's tiles, candidate
buffers and dedup passes (lengths from the kernel's own constants, read out of taxor_amd/csrc as tests/test_gpu_selector_domain.py
does) and on the "high-bit" reads of tests/golden/ref_syncmers_wide.npz, whose s-mers agree in their low 32 bits and differ only
above them (and, reverse-complemented, only below).  No index of this range takes the wave-per-read kernel (a w = 11, s <= 13
fast path with 32-bit values): the short reads below its cut, which it would take at s <= 13, come out right only through the
block kernel, at w = 11 (k = s + 10) too.
Whole path: search of a planted hierarchy, tuples identical to the oracle, as a small call and as a batch above SMALL_MAX_READS,
with FracMinHash scaling, and through a paged index in three passes.
Strand symmetry: the reference's selection is not strand-symmetric on tie-heavy reads (tests/test_syncmer_wide_ref_cpu.py);
the GPU is held to the oracle on both strands, and to equal hash sets wherever the oracle's are equal."""
import os

import numpy as np
import pytest

from oracle import oracle as orc
from taxor_amd import GpuIndex, Searcher, _lib, synth
from taxor_amd.search import plan_passes
from tests.test_gpu_paged_search import K4, _hash_genomes, _layout, _nbytes, _paged, _same
from tests.test_gpu_selector_domain import (BLK, POOL, REF, SMALL_MAX_READS, SY_LDS_CAND, SY_PASS, SY_T, SYNC_WAVE_CAND, _Reads, _dummy_index,
                                            _first_diff, _gpu_select, _wyhash)

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
_G = np.load(os.path.join(HERE, "golden", "ref_syncmers_wide.npz"))
_B, _O = _G["bases"].tobytes(), _G["offsets"].astype(np.int64)
HIGH_BIT = [_B[_O[i]:_O[i + 1]] for i in range(_O.size - 1)][-int(_G["n_high_bit"]):]       # (read, reverse complement) pairs


def _domain():
    return [(k, s) for k in range(18, 33) for s in range(17, 32) if s < k]


def _cfgs(k):
    return [(k, s, t) for k_, s in _domain() if k_ == k for t in sorted({1, (k - s + 1) // 2, k - s + 1} - {0})]


def _prefix_with(read, k, s, t, want):
    """shortest prefix of `read` with `want` selected syncmers: a window's selection depends on the windows before it only, so
    the count grows by at most one per base"""
    lo, hi = k - 1, len(read)
    assert orc.seq_to_syncmers(read, k, s, t).size >= want
    while lo < hi:
        mid = (lo + hi) // 2
        if orc.seq_to_syncmers(read[:mid], k, s, t).size >= want:
            hi = mid
        else:
            lo = mid + 1
    return read[:lo]


def _wide_reads(k, s, t):
    w = k - s + 1
    R = _Reads(k * 10007 + s * 101 + t)
    L = lambda nwin: nwin + k - 1
    out = [(f"nwin={n}", R.rnd(L(n))) for n in (0, 1, 2, SY_T - 1, SY_T, SY_T + 1, 2 * SY_T + 1)]
    out += [("nwin=2*SY_T tie-heavy", R.lowc(L(2 * SY_T))), ("nwin=SY_T+1 tie-heavy", R.lowc(L(SY_T + 1)))]
    out += [("shorter than s", R.rnd(s - 1)), ("length k-1", R.rnd(k - 1))]
    # below the short-read cut of the wave kernel (at most SYNC_WAVE_CAND candidate slots): block kernel here
    out += [(f"short {n}", R.rnd(n)) for n in (k, 150, 400, SYNC_WAVE_CAND)]
    out += [("short tie-heavy", R.lowc(300)), ("homopolymer", b"A" * L(SY_T + 37)), ("(AT)n", b"AT" * 1200), ("unit*n", R.rnd(97) * 30)]
    # candidate edges: SY_LDS_CAND -1/0/+1 selected (LDS buffer <-> spill to global), SY_PASS -1/0/+1 (one <-> two dedup passes),
    # BLK / BLK+1 (all-pairs <-> hash-table dedup); random reads at k >= 18 select no k-mer twice, so selected = distinct
    long = R.rnd(int((SY_LDS_CAND + 40) * (w + 2) * 1.6) + k)
    full = orc.seq_to_syncmers(long, k, s, t).size
    for name, n in (("BLK", BLK), ("SY_PASS", SY_PASS), ("SY_LDS_CAND", SY_LDS_CAND)):
        for d in (-1, 0, 1):
            assert full >= n + d, (k, s, t, full)
            out.append((f"n_sel={name}{d:+d}", _prefix_with(long, k, s, t, n + d)))
    out += [(f"high-bit {i}", r) for i, r in enumerate(HIGH_BIT)]
    return out


@pytest.mark.parametrize("k", range(18, 33))
def test_wide_syncmer_domain(k):
    for k_, s, t in _cfgs(k):
        named = _wide_reads(k, s, t)
        reads = [r for _, r in named]
        want = list(POOL.map(lambda r: orc.seq_to_syncmers(r, k, s, t), reads))
        for name, wv in zip([n for n, _ in named], want):
            if name.startswith("n_sel="):
                edge, d = name[6:-2], int(name[-2:])
                assert wv.size == dict(BLK=BLK, SY_PASS=SY_PASS, SY_LDS_CAND=SY_LDS_CAND)[edge] + d, (k, s, t, name, wv.size)
        if REF is not None and k <= 31:
            ref = list(POOL.map(lambda r: orc.ref_seq_to_syncmers(r, k, s, t), reads))
            for (name, r), a, b in zip(named, want, ref):
                assert a.tolist() == _wyhash(b).tolist(), f"oracle vs reference k={k} s={s} t={t} {name} (len {len(r)})"
        idx = _dummy_index(k, s, t)
        try:
            for sub in (0, 5):
                got = _gpu_select(idx, reads, sub)
                for (name, r), g, wv in zip(named, got, want):
                    if g.size != wv.size or not np.array_equal(g, wv):
                        j = _first_diff(g, wv)
                        raise AssertionError(f"k={k} s={s} t={t} sub_batch_reads={sub} read '{name}' (len {len(r)}): "
                                             f"GPU {g.size} vs oracle {wv.size} hashes, first difference at selection {j}")
                hb = got[-len(HIGH_BIT):]
                hw = want[-len(HIGH_BIT):]
                for i in range(0, len(HIGH_BIT), 2):          # a read and its reverse complement
                    if set(hw[i].tolist()) == set(hw[i + 1].tolist()):
                        assert set(hb[i].tolist()) == set(hb[i + 1].tolist()), (k, s, t, i)
        finally:
            idx.close()


@pytest.mark.parametrize("s", [17, 24, 31])
def test_high_bit_reads(s):
    """34-, 48- and 62-bit s-mer values at every k above s: the periodic reads with sparse substitutions, both strands, in one
    call; the selection is not empty, so the comparison is not vacuous"""
    for k in range(s + 1, 33):
        w = k - s + 1
        for t in sorted({1, (w + 1) // 2, w}):
            want = [orc.seq_to_syncmers(r, k, s, t) for r in HIGH_BIT]
            assert sum(x.size for x in want) > 0
            idx = _dummy_index(k, s, t)
            try:
                got = _gpu_select(idx, HIGH_BIT, 0)
            finally:
                idx.close()
            for i, (g, wv) in enumerate(zip(got, want)):
                assert np.array_equal(g, wv), (k, s, t, i, g.size, wv.size, _first_diff(g, wv))


def test_index_create_limits():
    for k, s, t in ((32, 31, 1), (18, 17, 1), (32, 17, 16), (31, 30, 2)):
        _dummy_index(k, s, t).close()
    for k, s, t in ((20, 20, 1), (17, 17, 1), (28, 20, 0), (33, 17, 1), (32, 32, 1), (40, 31, 1)):
        with pytest.raises(_lib.TaxorError) as e:
            _dummy_index(k, s, t).close()
        assert e.value.code == -1, (k, s, t, e.value)          # TAXOR_E_ARG
        assert "s<=16" not in str(e.value) and "1<=s<=31" in str(e.value)


# ------------------------------------------------------------------------------------------------ whole path
WHOLE = [(28, 20, 4, 1), (30, 26, 2, 1), (32, 31, 1, 1), (24, 17, 4, 1), (18, 17, 1, 1), (28, 20, 4, 10)]


@pytest.mark.parametrize("kst", WHOLE, ids=[f"k{k}s{s}t{t}" + (f"scaling{sc}" if sc > 1 else "") for k, s, t, sc in WHOLE])
def test_wide_whole_path(kst):
    k, s, t, scaling = kst
    err = 0.04
    pct = -1.0 if orc.syncmer_match_ratio(k, err) >= 0 else 0.3     # no syncmer-model row (odd k, k outside 12..30): percentage
    g, go = synth.random_genomes(5, 6000, seed=k * 100 + s)
    planted = [orc.seq_to_syncmers(bytes(g[int(go[i]):int(go[i + 1])]), k, s, t) for i in range(5)]
    if scaling > 1:                                                  # the keys a scaled build keeps (taxor_build.cpp: hash <= max / scaling)
        lim = float(2**64 - 1) / scaling
        planted = [p[np.array([float(orc.wyhash(int(x))) <= lim for x in p], dtype=bool)] for p in planted]
        assert all(p.size > 20 for p in planted)
    lay = synth.make_layout(planted, root_bins=66, child_bins=24, n_children=2, seed=k + 7 * s + 31 * t)
    host = synth.materialize_host(lay)
    idx = GpuIndex(host, lay["n_user_bins"], k, s, t, scaling=scaling)
    h = orc.Hixf(host, [f["next_ixf"] for f in host], [f["fname_idx"] for f in host])
    try:
        # a small call (the lanes) and a batch above SMALL_MAX_READS (the sub-batch pipeline), whole and in sub-batches
        for n, rl, subs in ((300, 900, (0,)), (SMALL_MAX_READS + 1, 150, (0, 4096))):
            bases, offs, _ = synth.synth_reads(g, go, n, rl, error_rate=0.03, frac_random=0.1, seed=n + k)
            nh, off, ub, cnt, _ = h.search_batch(bases, offs, k=k, s=s, t=t, err=err, percentage=pct, threads=8, scaling=scaling)
            assert ub.size > 0 and nh.max() > 0, (kst, n)
            for sub in subs:
                sr = Searcher(idx, error_rate=err, percentage=pct, sub_batch_reads=sub)
                try:
                    res = sr.search_batch(bases, offs)
                finally:
                    sr.close()
                assert np.array_equal(res.n_hashes, nh), (kst, n, sub)
                assert np.array_equal(res.read_off, off) and np.array_equal(res.user_bin, ub) and np.array_equal(res.count, cnt), (kst, n, sub)
    finally:
        idx.close()


def test_wide_paged_search_three_passes():
    """(28, 20, 4) through an index paged in three resident passes: the merged CSR equals the ordinary searcher's and the oracle's"""
    kw = dict(k=28, s=20, t=4)
    g, go = synth.random_genomes(9, 6000, seed=31)
    planted = _hash_genomes(g, go, **kw)
    for i in range(9):
        assert np.array_equal(planted[i], np.unique(orc.seq_to_syncmers(bytes(g[int(go[i]):int(go[i + 1])]), 28, 20, 4)))
    lay, ids = _layout(planted, seed=32)
    host = synth.materialize_host(lay)
    n_ub = lay["n_user_bins"]
    bases, offs, _ = synth.synth_reads(g, go, 200, 1500, error_rate=0.02, frac_random=0.15, seed=33)
    sub = [[ids["A"]], [ids["B"], ids["B1"], ids["B2"]], [ids["C"]], [ids["D"]], [ids["E"]]]
    sizes = [sum(_nbytes(host[i]) for i in ids_) for ids_ in sub]
    root = _nbytes(host[0]) + K4
    three = None
    for budget in range(root + max(sizes), root + sum(sizes), K4):
        try:
            plan, _, _ = plan_passes(host, n_ub, budget, **kw)
        except _lib.TaxorError:
            continue
        if plan["n_passes"] == 3:
            three = budget
            break
    assert three is not None, sizes
    w = dict(kw=kw, host=host, n_ub=n_ub, bases=bases, offs=offs, use_syncmer=True, ref={})
    n_passes, got = _paged(w, three, {})
    assert n_passes == 3
    idx = GpuIndex(host, n_ub, **kw)
    sr = Searcher(idx)
    try:
        ref = sr.search_batch(bases, offs)
    finally:
        sr.close()
        idx.close()
    _same(got, ref)
    h = orc.Hixf(host, [f["next_ixf"] for f in host], [f["fname_idx"] for f in host])
    nh, off, ub, cnt, _ = h.search_batch(bases, offs, k=28, s=20, t=4, threads=8)
    assert np.array_equal(ref.n_hashes, nh) and np.array_equal(ref.read_off, off)
    assert np.array_equal(ref.user_bin, ub) and np.array_equal(ref.count, cnt) and ub.size > 0
