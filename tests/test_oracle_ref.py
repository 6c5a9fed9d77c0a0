"""The oracle AND the product's host functions against the REAL reference wherever the reference compiles on its own:
oracle/_ref/libtaxor_ref.so is built by `make -C oracle ref` straight from a checkout of the reference (syncmer threshold table,
k-mer / FracMinHash threshold models, adjust_seed, the in-repo XOR-filter prototype, the chunk loop's scheduler
do_parallel.hpp and the result stream sync_out.hpp; see oracle/ref_driver.cpp).
What that library returns for these tests' inputs is stored in tests/golden/ref_vectors.npz (tests/golden/make_ref_golden.py), so
the tests hold the oracle against the reference's answers everywhere; where the library is at hand they also hold the stored answers
against it.  Only sync_out, which is the reference's own code running, needs the library itself."""
import ctypes as C
import os

import numpy as np
import pytest

from oracle import oracle as orc
from taxor_amd import _lib
from taxor_amd import search as ts

REF = orc.ref_lib()
G = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_vectors.npz"))


def _digest(*arrays):
    import hashlib
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def _canonical_nan(a):
    a = np.array(a, dtype=np.float64)
    a[np.isnan(a)] = np.nan
    return a


def test_syncmer_match_ratio_is_the_references_table():
    """get_min_syncmer_match_ratio (syncmer_model.hpp:38-50): every (k, error rate) the reference accepts"""
    assert G["smr_k"].tolist() == list(range(12, 31, 2)) and G["smr_e100"].tolist() == list(range(0, 2001))
    for i, k in enumerate(range(12, 31, 2)):
        for e100 in range(0, 2001):
            err = e100 / 10000.0
            want = float(G["smr_table"][i, e100])
            if REF is not None:
                assert REF.ref_syncmer_match_ratio(k, err) == want, (k, err)
            assert orc.syncmer_match_ratio(k, err) == want, (k, err)
            assert ts.threshold_ratio(k, err) == want, (k, err)
    extra = (0.15, 0.05, 0.04, 0.1, 0.2, 0.0, 0.07, 0.29 / 2)          # fp-rounding-sensitive row indices
    assert G["smr_extra_err"].tolist() == list(extra)
    for err, want in zip(extra, G["smr_extra"].tolist()):
        if REF is not None:
            assert REF.ref_syncmer_match_ratio(22, err) == want, err
        assert orc.syncmer_match_ratio(22, err) == want
    ratio = float(G["smr_table"][list(range(12, 31, 2)).index(22), 400])     # k = 22, error 0.04
    for n in (0, 1, 98, 435, 871, 10**6):
        assert orc.threshold(n, 22, 0.04) == int(n * ratio)


def test_threshold_model_components_are_the_references():
    """calculate_nmut_kmer_CI(...).second and calculate_containment_index_CI(...).first from the reference's own
    translation units, incl. the NaN / negative casts of very short reads (compiled as the reference compiles them)"""
    rng = np.random.default_rng(3)
    ns = [0, 1, 2, 3, 5, 7, 10, 20, 50, 99, 100, 435, 871, 4981, 9979, 99979, 10**6] + [int(x) for x in rng.integers(0, 300000, 400)]
    ks, errs, sfs = (16, 20, 22, 31, 32), (0.001, 0.01, 0.04, 0.1, 0.2, 0.5), (1e-3, 0.05, 1 / 7, 0.5, 0.999)
    assert G["thr_n"].tolist() == ns and G["thr_k"].tolist() == list(ks) and G["thr_err"].tolist() == list(errs) and G["thr_sf"].tolist() == list(sfs)
    lows = np.zeros((len(ks), len(errs), len(ns), len(sfs)))
    for a, k in enumerate(ks):
        for b, err in enumerate(errs):
            for c, n in enumerate(ns):
                high = int(G["nmut_kmer_ci_high"][a, b, c])
                if REF is not None:
                    assert REF.ref_nmut_kmer_ci_high(err, k, n, 0.95) == high, (k, err, n)
                assert orc.lib().orc_nmut_kmer_ci_high(err, k, n, 0.95) == high, (k, err, n)
                fp = int(n * 0.0039)
                want_kmer = (n - high - fp) % 2**64                                           # threshold.hpp:62-66
                assert orc.threshold_model(orc.THR_KMER, n, k, err) == want_kmer
                assert ts.threshold_model(_lib.THR_KMER, n, k, err) == want_kmer
                for d, sf in enumerate(sfs):
                    mine = orc.lib().orc_containment_index_ci_low(err, k, n, sf, 0.95)
                    if REF is not None:
                        low = REF.ref_containment_index_ci_low(err, k, n, sf, 0.95)
                        assert (low == mine) or (low != low and mine != mine), (k, err, n, sf)     # NaN == NaN
                    lows[a, b, c, d] = mine
    # every value of the table, NaN == NaN, against the reference's table (stored as its digest)
    assert _digest(_canonical_nan(lows)) == str(G["containment_index_ci_low_sha256"])
    want = float(G["normal_cdf_inverse_0975"])
    if REF is not None:
        assert REF.ref_normal_cdf_inverse(0.975) == want
    assert orc.lib().orc_normal_cdf_inverse(0.975) == want
    for k in range(1, 33):
        want = int(G["adjust_seed"][k - 1])
        if REF is not None:
            assert REF.ref_adjust_seed(k) == want
        assert orc.adjust_seed(k) == want


def test_ixf_arithmetic_is_the_in_repo_prototypes():
    """src/main/xorfilter.hpp (the evidence for the un-vendored IXF): same rows, same fingerprint, same sizing; a
    filter the prototype builds answers identically through the oracle's lookup and through the product's builder"""
    rng = np.random.default_rng(5)
    for n in (1, 2, 10, 1000, 50000):
        keys = np.unique(rng.integers(0, 2**63, size=n, dtype=np.uint64))
        probe = np.concatenate([keys[:200], rng.integers(0, 2**64, size=200, dtype=np.uint64)])
        others = rng.integers(0, 2**64, size=20000, dtype=np.uint64)
        assert _digest(keys, probe, others[:3000]) == str(G[f"xor{n}_inputs_sha256"]), "not the inputs the stored answers are for"
        seed, blk, fps = int(G[f"xor{n}_seed"]), int(G[f"xor{n}_blk"]), G[f"xor{n}_fingerprints"]
        h = None
        if REF is not None:
            s_, b_, a_ = C.c_uint64(), C.c_uint64(), C.c_uint64()
            h = REF.ref_xor_build(keys.ctypes.data, keys.size, C.byref(s_), C.byref(b_), C.byref(a_))
            assert h, "prototype construction failed"
            assert s_.value == seed and b_.value == blk
            assert np.array_equal(np.ctypeslib.as_array(REF.ref_xor_fingerprints(h), shape=(int(a_.value),))[:3 * blk], fps)
        assert orc.ixf_seg_len(keys.size) == blk == ts_seg_len(keys.size)           # (32 + 1.23 n) / 3
        data = np.zeros(3 * blk, dtype=np.uint8)
        data[:] = fps
        ixf = dict(bins=1, stride=1, seg_len=blk, seed=seed, data=data)
        hx = orc.Hixf([ixf], [np.zeros(1, np.int64)], [np.zeros(1, np.int64)])
        rows, fp = (C.c_uint64 * 3)(), C.c_uint8()
        mine_rows, mine_fp = np.zeros(3, np.uint64), np.zeros(1, np.uint8)
        for i, key in enumerate(probe):
            want_rows, want_fp = G[f"xor{n}_probe_rows"][i].tolist(), int(G[f"xor{n}_probe_fp"][i])
            if h is not None:
                REF.ref_xor_probe(h, int(key), rows, C.byref(fp))
                assert list(rows) == want_rows and fp.value == want_fp, key
            orc.lib().orc_ixf_probe(C.byref(hx._ixf[0]), C.c_uint64(int(key)), mine_rows.ctypes.data, mine_fp.ctypes.data)
            assert mine_rows.tolist() == want_rows and int(mine_fp[0]) == want_fp, key
        # membership through the oracle's bulk_count == the prototype's Contain
        assert int(hx.ixf_bulk_count(0, keys)[0]) == keys.size
        want = int(G[f"xor{n}_others_contained"])
        if h is not None:
            assert sum(REF.ref_xor_contain(h, int(x)) for x in others[:3000]) == want
        assert int(hx.ixf_bulk_count(0, others[:3000])[0]) == want
        # the product's own host builder under the prototype's seed produces a filter the prototype's lookup rule accepts
        col = np.zeros(3 * blk, dtype=np.uint8)
        rc = _lib.lib().taxor_ixf_build_bin(keys.ctypes.data, keys.size, seed, blk, col.ctypes.data)
        if rc == 0:
            ixf2 = dict(ixf, data=col)
            hx2 = orc.Hixf([ixf2], [np.zeros(1, np.int64)], [np.zeros(1, np.int64)])
            assert int(hx2.ixf_bulk_count(0, keys)[0]) == keys.size
        if h is not None:
            REF.ref_xor_free(h)


def ts_seg_len(n):
    return int(_lib.lib().taxor_ixf_seg_len(int(n)))


def test_do_parallel_slices_are_the_references():
    """hixf::do_parallel (do_parallel.hpp:22-29): `threads` tasks, floor(n / threads) records each, the remainder on the LAST task
    -- observed from the reference's own object code -- and the oracle's worker driven by it over 1024-record chunks
    (taxor_search.cpp:315-326) gives the same CSR as the oracle's OpenMP slices.  (The slices are the reference's stored answers where
    its library is absent; the chunked run needs the library itself.)"""
    for n, th in ((1024, 32), (1000, 32), (31, 32), (5, 3), (1, 1), (0, 4), (1024, 7)):
        # the tasks report their slices as they finish: the pairs come in any order, so they are compared as sorted sets
        out = G[f"slices_{n}_{th}"]
        got = sorted((int(out[2 * i]), int(out[2 * i + 1])) for i in range(th))
        if REF is not None:
            live = np.zeros(2 * th, dtype=np.uint64)
            REF.ref_do_parallel_slices(n, th, live.ctypes.data_as(C.c_void_p))
            assert sorted((int(live[2 * i]), int(live[2 * i + 1])) for i in range(th)) == got, (n, th)
        per = n // th
        want = sorted((per * i, n if i == th - 1 else per * (i + 1)) for i in range(th))
        assert got == want, (n, th)
    if REF is None:
        return
    from taxor_amd import synth
    rng = np.random.default_rng(11)
    g, go = synth.random_genomes(5, 8000, seed=11)
    planted = [np.unique(orc.seq_to_syncmers(bytes(g[int(go[i]):int(go[i + 1])]))) for i in range(5)]
    lay = synth.make_layout(planted, root_bins=64, child_bins=32, n_children=3, seed=11)
    host = synth.materialize_host(lay)
    h = orc.Hixf(host, [f["next_ixf"] for f in host], [f["fname_idx"] for f in host])
    bases, offs, _ = synth.synth_reads(g, go, 2500, 900, error_rate=0.02, frac_random=0.2, seed=12)
    want = h.search_batch(bases, offs, threads=4)
    for th, chunk in ((32, 1024), (3, 1024), (5, 700), (1, 1024)):
        tm = {}
        got = h.search_batch(bases, offs, threads=th, scheduler="reference", chunk=chunk, timing=tm)
        for a, b in zip(got[:4], want[:4]):
            assert np.array_equal(a, b), (th, chunk)
        assert got[4] == want[4] and tm["compute_time"] > 0
    assert want[2].size > 1000


@pytest.mark.skipif(REF is None, reason="runs the reference's own sync_out: needs oracle/_ref/libtaxor_ref.so, built where the reference's sources are")
def test_sync_out_serialises_whole_writes(tmp_path):
    """hixf::sync_out (sync_out.hpp:24-36): every operator<< is one mutexed write -- lines of concurrent writers never interleave"""
    p = tmp_path / "out.txt"
    REF.ref_sync_out_lines(str(p).encode(), 8, 500)
    lines = open(p).read().split("\n")
    assert lines[-1] == "" and len(lines) == 8 * 500 + 1
    assert sorted(lines[:-1]) == sorted(f"t{t}:{i}" for t in range(8) for i in range(500))
    for t in range(8):                        # each writer's own lines stay in its order
        assert [l for l in lines if l.startswith(f"t{t}:")] == [f"t{t}:{i}" for i in range(500)]
