"""A batch's saved hash lists (taxor_gpu_search_capture / _take_saved / _saved_begin):
1. the captured lists are the hash lists taxor_gpu_syncmers returns (that entry is pinned to the oracle), counts and thresholds with them,
   on a batch that crosses the capture's edges;
2. a replay gives exactly the arrays the run from bases gave -- same searcher after an unrelated batch, a second searcher, a syncmer, a
   minimiser and a wide (s >= 17) index, a batch that came in as 4-bit sequences;
3. a paged index: pass 0 from bases with capture, the later passes by replay, merged: the resident index's CSR;
4. the refusals name the field;
5. the profile feed reads a replayed batch's device results (the read lengths are back on the device)."""
import numpy as np
import pytest

from oracle import oracle as orc
from taxor_amd import GpuIndex, Searcher, _lib, synth, threshold
from tests.test_gpu_paged_search import _paged, _resident, _same, _world

pytestmark = pytest.mark.gpu

FIELDS = ("read_off", "user_bin", "count", "n_hashes")


def _cat(reads):
    off = np.zeros(len(reads) + 1, np.uint64)
    off[1:] = np.cumsum([len(r) for r in reads])
    return np.frombuffer(b"".join(reads), np.uint8), off


def _equal(a, b):
    """PassResults a == b, array by array"""
    for f in FIELDS:
        assert np.array_equal(getattr(a.results, f), getattr(b.results, f)), f
    assert np.array_equal(a.key, b.key)


def _captured(sr, bases, offs, nibbles=None):
    """one batch from bases (or 4-bit sequences) with capture on -> (PassResults, SavedBatch)"""
    from taxor_amd.search import PassResults
    sr.capture(True)
    r = sr.search_nibbles(nibbles) if nibbles is not None else sr.search_batch(bases, offs)
    out = PassResults(r, sr.result_keys(r.user_bin.size))
    return out, sr.take_saved()


@pytest.fixture(scope="module")
def world():
    return _world(True)


@pytest.fixture(scope="module")
def edge_batch(world):
    """reads that cross the capture's edges: no base at all, fewer than k, all N, exactly 63 / 64 / 65 / 129 hashes (the gather takes 64
    entries per round), both sides of the wave-per-read / block-per-read hashing split (512 candidate slots: ~2.5 kb), and ordinary reads"""
    w = world
    idx = GpuIndex(w["host"], w["n_ub"], **w["kw"])
    hs = Searcher(idx)
    gen, go = synth.random_genomes(3, 6000, seed=77)
    g = bytes(gen[:6000])
    # the number of distinct hashes of a prefix grows by at most one per base: every count up to the whole read's is some prefix's
    L = np.arange(22, 1700)
    hoff, _ = hs.seq_to_syncmers(*_cat([g[:int(l)] for l in L]))
    nh = np.diff(hoff.astype(np.int64))
    pick = {}
    for c in (63, 64, 65, 129):
        assert (nh == c).any(), c
        pick[c] = int(L[int(np.argmax(nh == c))])
    ordinary, oo, _ = synth.synth_reads(gen, go, 22, 1500, error_rate=0.02, frac_random=0.2, seed=78)
    reads = [b"", b"ACGTACGTAC", b"N" * 300] + [g[:pick[c]] for c in (63, 64, 65, 129)]
    reads += [bytes(gen[6000:8400]), bytes(gen[6000:8700]), bytes(gen[12100:18000])]           # 2400: one wave; 2700, 5900: a block
    reads += [bytes(ordinary[int(oo[i]):int(oo[i + 1])]) for i in range(22)]
    hs.close()
    yield dict(idx=idx, reads=reads, pick=pick)
    idx.close()


def test_captured_lists_are_the_hash_lists(edge_batch):
    e = edge_batch
    B, O = _cat(e["reads"])
    sr = Searcher(e["idx"], sub_batch_reads=8)                        # 32 reads: four sub-batches, both hash buffers used twice
    got, sv = _captured(sr, B, O)
    hoff, hashes = sr.seq_to_syncmers(B, O)
    assert sv.n_reads == len(e["reads"]) and sv.n_sub_batches >= 3
    assert np.array_equal(sv.hash_off, hoff) and np.array_equal(sv.hashes, hashes) and sv.total_hashes == hashes.size
    assert np.array_equal(sv.n_hashes, got.results.n_hashes) and np.array_equal(sv.n_hashes, np.diff(hoff))
    assert [int(x) for x in sv.threshold] == [threshold(int(n), sr.ratio) for n in sv.n_hashes]
    assert np.array_equal(sv.read_len, np.diff(O))
    assert [int(x) for x in sv.n_hashes[:2]] == [0, 0] and [int(x) for x in sv.n_hashes[3:7]] == [63, 64, 65, 129]
    assert int(sv.read_len[7]) // 5 + 2 <= 512 < int(sv.read_len[8]) // 5 and sv.n_hashes[9] > 400           # the hashing split's two sides
    assert sv.params["kmer_size"] == 22 and sv.params["syncmer_size"] == 12 and sv.params["t_syncmer"] == 5 and sv.params["use_syncmer"] == 1
    assert sv.nbytes >= hashes.size * 8
    # the sub-batch plan and the processing order a replay repeats
    assert sv.sub_first[0] == 0 and sv.sub_first[-1] == sv.n_reads and (np.diff(sv.sub_first.astype(np.int64)) > 0).all()
    for i in range(sv.n_sub_batches):
        a, b = int(sv.sub_first[i]), int(sv.sub_first[i + 1])
        assert sorted(int(x) for x in sv.order[a:b]) == list(range(b - a))
    sv.close()
    # a batch of one read
    one, sv1 = _captured(sr, *_cat([e["reads"][9]]))
    h1off, h1 = sr.seq_to_syncmers(*_cat([e["reads"][9]]))
    assert sv1.n_reads == 1 and sv1.n_sub_batches == 1 and np.array_equal(sv1.hashes, h1) and np.array_equal(sv1.hash_off, h1off)
    assert np.array_equal(sv1.n_hashes, one.results.n_hashes)
    sv1.close()
    sr.close()


def _kind(kind, world, tmp_path):
    """(index, searcher arguments, bases, offsets, nibble segments or None)"""
    if kind in ("syncmer", "nibbles"):
        idx = GpuIndex(world["host"], world["n_ub"], **world["kw"])
        if kind == "syncmer":
            return idx, {}, world["bases"], world["offs"], None
        from taxor_amd.search import read_bam
        from tests import bam_writer as bw
        from tests.test_gpu_bam import _bam_reads
        g, go = synth.random_genomes(9, 6000, seed=11)                # the world's genomes
        reads = _bam_reads(g, go, 60, seed=5)
        bw.write_bam(tmp_path / "r.bam", reads, block=5000, spare=0xF)
        _, seq4, boff, rlen, rev = read_bam(tmp_path / "r.bam")
        B, O = _cat([s for _, s in bw.selected(reads)])
        return idx, {}, B, O, [(seq4, boff, rlen, rev)]
    if kind == "minimiser":                                           # window 28 over k 20: the FracMinHash model, thresholds from the host
        from tests.test_gpu_minimiser import _planted
        g, go, lay, host = _planted(20, 28, seed=49)
        idx = GpuIndex(host, lay["n_user_bins"], k=20, s=0, t=0, use_syncmer=False, window_size=28)
    else:                                                             # wide: s-mers of 20 bases
        g, go = synth.random_genomes(5, 6000, seed=2820)
        planted = [orc.seq_to_syncmers(bytes(g[int(go[i]):int(go[i + 1])]), 28, 20, 4) for i in range(5)]
        lay = synth.make_layout(planted, root_bins=66, child_bins=24, n_children=2, seed=5)
        idx = GpuIndex(synth.materialize_host(lay), lay["n_user_bins"], 28, 20, 4)
    bases, offs, _ = synth.synth_reads(g, go, 120, 1200, error_rate=0.02, frac_random=0.15, seed=6)
    return idx, {}, bases, offs, None


@pytest.mark.parametrize("kind", ["syncmer", "minimiser", "wide", "nibbles"])
def test_replay_equals_the_run_from_bases(world, tmp_path, kind):
    idx, kw, bases, offs, nib = _kind(kind, world, tmp_path)
    sr = Searcher(idx, sub_batch_reads=48, **kw)                      # several sub-batches
    ref, sv = _captured(sr, bases, offs, nib)
    assert ref.results.user_bin.size > 0 and sv.n_sub_batches >= 2
    if nib is not None:                                               # the 4-bit route hashed what the restored reads hash
        plain, sv2 = _captured(sr, bases, offs)
        _equal(plain, ref)
        assert np.array_equal(sv2.hashes, sv.hashes) and np.array_equal(sv2.hash_off, sv.hash_off) and np.array_equal(sv2.threshold, sv.threshold)
        sv2.close()
    if kind == "minimiser":
        assert sr.model == _lib.THR_FRACMINHASH and sv.params["window_size"] == 28 and sv.params["use_syncmer"] == 0
    # the same searcher, after an unrelated batch ran in between (with and without capture)
    other = synth.synth_reads(*synth.random_genomes(2, 3000, seed=9), 70, 700, error_rate=0.0, frac_random=0.5, seed=10)[:2]
    sr.search_batch(*other)
    _equal(sr.search_saved_pass(sv), ref)
    sr.capture(False)
    sr.search_batch(*other)
    _equal(sr.search_saved_pass(sv), ref)
    st = sr.stats()
    assert st["n_reads"] == sv.n_reads and st["n_hashes"] == sv.total_hashes and st["n_tuples"] == ref.results.user_bin.size
    with pytest.raises(_lib.TaxorError) as e:                         # no packed bases to run again
        sr.run()
    assert e.value.code == -1 and "saved hash lists" in str(e.value)
    sr.close()
    # a second searcher with equal parameters (its own sub-batch size: the saved plan is what runs)
    s2 = Searcher(idx, **kw)
    _equal(s2.search_saved_pass(sv), ref)
    # ... whose run from bases (the lanes, where they apply) gives the same CSR
    if nib is None:
        r = s2.search_batch(bases, offs)
        for f in FIELDS:
            assert np.array_equal(getattr(r, f), getattr(ref.results, f)), f
    s2.close()
    sv.close()
    idx.close()


def test_capture_on_the_route_from_file_bytes(world):
    """taxor_gpu_search_fastx_begin with capture on: the device finds the records, and the lists saved are those of the same reads from bases"""
    from taxor_amd.search import PassResults
    w = world
    offs, n = w["offs"], 150
    raw = b"".join(b"@r%d x\n" % r + bytes(w["bases"][int(offs[r]):int(offs[r + 1])]) + b"\n+\n" + b"I" * int(offs[r + 1] - offs[r]) + b"\n" for r in range(n))
    idx = GpuIndex(w["host"], w["n_ub"], **w["kw"])
    sr = Searcher(idx, sub_batch_reads=40)
    ref, sv = _captured(sr, w["bases"], offs[:n + 1])
    fx = sr.search_fastx(raw, "@")
    assert fx.status == 0 and len(fx.ids) == n
    got = PassResults(fx.results, sr.result_keys(fx.results.user_bin.size))
    svx = sr.take_saved()
    _equal(got, ref)
    for f in ("hashes", "hash_off", "n_hashes", "threshold", "read_len"):       # (the sub-batch plan is the route's own: a resident batch does not ramp)
        assert np.array_equal(getattr(svx, f), getattr(sv, f)), f
    _equal(sr.search_saved_pass(svx), ref)
    sv.close()
    svx.close()
    sr.close()
    idx.close()


def test_paged_pass_zero_from_bases_later_passes_by_replay(world):
    w = world
    idx = GpuIndex.paged(w["host"], w["n_ub"], w["budget3"], **w["kw"])
    sr = Searcher(idx)
    assert idx.passes == 3
    idx.load_pass(0)
    p0, sv = _captured(sr, w["bases"], w["offs"])
    sr.capture(False)
    idx.load_pass(1)
    p1 = sr.search_saved_pass(sv)
    idx.load_pass(2)
    sr.search_saved(sv)
    got = sr.merge_prior([p0, p1])
    assert max(p0.key.size, p1.key.size) < got.user_bin.size          # no single pass saw the whole hierarchy
    _same(got, _resident(w, {}))
    _same(got, _paged(w, w["budget3"], {})[1])                        # ... and the run that hashes the reads in every pass
    sv.close()
    sr.close()
    idx.close()


def test_refusals_name_the_field(world):
    w = world
    idx = GpuIndex(w["host"], w["n_ub"], **w["kw"])
    sr = Searcher(idx, sub_batch_reads=64)
    sr.search_batch(w["bases"], w["offs"])
    with pytest.raises(_lib.TaxorError) as e:                         # take without capture
        sr.take_saved()
    assert e.value.code == -1 and "capture is off" in str(e.value)
    ref, sv = _captured(sr, w["bases"], w["offs"])
    with pytest.raises(_lib.TaxorError) as e:                         # taken already
        sr.take_saved()
    assert e.value.code == -1 and "taken already" in str(e.value)
    # another k
    bins = 64
    other = GpuIndex([dict(bins=bins, stride=64, seg_len=16, seed=1, next_ixf=np.zeros(bins, np.int64), fname_idx=np.arange(bins),
                           data=np.zeros(3 * 16 * 64, np.uint8))], bins, k=20, s=12, t=5)
    so = Searcher(other, ratio=sr.ratio)
    with pytest.raises(_lib.TaxorError) as e:
        so.search_saved(sv)
    assert e.value.code == -1 and "kmer_size" in str(e.value)
    so.close()
    other.close()
    # another error rate
    se = Searcher(idx, error_rate=0.02)
    with pytest.raises(_lib.TaxorError) as e:
        se.search_saved(sv)
    assert e.value.code == -1 and "error_rate" in str(e.value)
    se.close()
    # the saved arrays tampered with on the host: offsets that do not ascend, a count that contradicts them, an offset outside the array
    r = int(np.argmax(sv.n_hashes > 2))
    keep = (int(sv.hash_off[r + 1]), int(sv.n_hashes[r]))
    sv.hash_off[r + 1] = sv.hash_off[r] - 1 if sv.hash_off[r] else sv.hash_off[r + 2] + 1
    with pytest.raises(_lib.TaxorError) as e:
        sr.search_saved(sv)
    assert e.value.code == -1 and "hash_off" in str(e.value) and "ascend" in str(e.value)
    sv.hash_off[r + 1] = keep[0]
    sv.n_hashes[r] = keep[1] - 1
    with pytest.raises(_lib.TaxorError) as e:
        sr.search_saved(sv)
    assert e.value.code == -1 and "n_hashes" in str(e.value)
    sv.n_hashes[r] = keep[1]
    last = int(sv.hash_off[-1])
    sv.hash_off[-1] = last + 5
    with pytest.raises(_lib.TaxorError) as e:
        sr.search_saved(sv)
    assert e.value.code == -1 and "hash_off" in str(e.value) and "outside" in str(e.value)
    sv.hash_off[-1] = last
    _equal(sr.search_saved_pass(sv), ref)                             # mended: it runs, and the refusals left the searcher usable
    sv.close()
    sr.close()
    idx.close()


def test_profile_feed_after_a_replayed_batch(world):
    from taxor_amd.profile import ProfileFeed
    w = world
    idx = GpuIndex(w["host"], w["n_ub"], **w["kw"])
    sr = Searcher(idx, sub_batch_reads=64)
    nb = int(w["n_ub"])
    ref_of_bin = (np.arange(nb) % max(2, nb // 2)).astype(np.int32)
    ref_len = (1000 + 10 * np.arange(nb)).astype(np.uint64)
    n = w["offs"].size - 1
    rank = np.random.default_rng(3).permutation(n).astype(np.uint64)
    with ProfileFeed(ref_of_bin, ref_len, max(2, nb // 2)) as a, ProfileFeed(ref_of_bin, ref_len, max(2, nb // 2)) as b:
        _, sv = _captured(sr, w["bases"], w["offs"])
        a.add_batch(sr, 0)
        sr.search_batch(*synth.synth_reads(*synth.random_genomes(2, 3000, seed=9), 50, 900, error_rate=0.0, frac_random=0.5, seed=10)[:2])
        sr.search_saved(sv)                                           # other read lengths were on the device in between
        b.add_batch(sr, 0)
        fa, fb = a.finish(rank, run=False), b.finish(rank, run=False)
    for k in fa:
        assert np.array_equal(fa[k], fb[k]), k
    assert np.array_equal(np.sort(fa["query_len"]), np.sort(np.diff(w["offs"]).astype(np.uint64))) and (fa["csr_ref"] >= 0).sum() > 50
    sv.close()
    sr.close()
    idx.close()
