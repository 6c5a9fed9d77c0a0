"""Search of an index in resident passes (taxor_gpu_index_create_paged / _load_pass / taxor_gpu_search_merge_prior): the merged CSR of a
paged run is bit-identical to the CSR of an ordinary searcher on the same view, and to the CPU oracle."""
import numpy as np
import pytest

from oracle import oracle as orc
from taxor_amd import GpuIndex, Searcher, _lib, synth
from taxor_amd.search import PassResults, SearchResults, plan_passes

pytestmark = pytest.mark.gpu

K4 = 4096


def _hash_genomes(g, go, **idx_kw):
    bins = 64
    dummy = GpuIndex([dict(bins=bins, stride=64, seg_len=16, seed=1, next_ixf=np.zeros(bins, np.int64), fname_idx=np.arange(bins),
                           data=np.zeros(3 * 16 * 64, np.uint8))], bins, **idx_kw)
    hs = Searcher(dummy, ratio=0.5)
    hoff, hashes = hs.seq_to_syncmers(g, go)
    hs.close()
    dummy.close()
    return [np.unique(hashes[int(hoff[i]):int(hoff[i + 1])]) for i in range(go.size - 1)]


def _layout(planted, seed):
    """root of 64 bins: genome 0 split over bins 0..2, genome 1 at bin 3, merged bins 10, 11, 30, 31, 63 ->
      A (64 bins): genome 2, genome 3 split over two bins, a copy of genome 6 (its reads match two subtrees)
      B (100 bins) -> B1 (64) -> B2 (70): a chain three IXFs deep; genome 5 in B, genome 4 in B2
      C (192 bins): genome 6     D (130 bins): genome 7     E (64 bins): genome 8"""
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

    root = new_ixf(64)
    leaf(root, [0, 1, 2], planted[0])
    leaf(root, [3], planted[1])
    A = child(root, 10, 64)
    B = child(root, 11, 100)
    B1 = child(B, 99, 64)
    B2 = child(B1, 0, 70)
    Cc = child(root, 30, 192)
    D = child(root, 31, 130)
    E = child(root, 63, 64)
    leaf(A, [5], planted[2])
    leaf(A, [20, 21], planted[3])
    leaf(A, [63], planted[6])
    leaf(B, [17], planted[5])
    leaf(B2, [69], planted[4])
    leaf(Cc, [100], planted[6])
    leaf(D, [129], planted[7])
    leaf(E, [0], planted[8])
    out = synth._finalize_layout(ixfs, new_ub, rng, "host")
    return dict(ixfs=out, n_user_bins=nub[0]), dict(A=A, B=B, B1=B1, B2=B2, C=Cc, D=D, E=E)


def _nbytes(f):
    return (3 * f["seg_len"] * f["stride"] + K4 - 1) // K4 * K4


def _world(use_syncmer):
    kw = dict(k=22, s=12, t=5) if use_syncmer else dict(k=20, s=12, t=5, use_syncmer=False, window_size=24)
    g, go = synth.random_genomes(9, 6000, seed=11)
    planted = _hash_genomes(g, go, **kw)
    lay, ids = _layout(planted, seed=12)
    host = synth.materialize_host(lay)
    n_ub = lay["n_user_bins"]
    # reads: from every genome (so every subtree, the root's leaves, and genome 6 in two subtrees), random ones that match nothing,
    # a read of length 0 and one below k (no hashes: threshold 0, EVERY leaf run is reported -- several hundred tuples, the merge's
    # 64-at-a-time loop and the finalize's wide-read path)
    bases, offs, origin = synth.synth_reads(g, go, 198, 1500, error_rate=0.02, frac_random=0.15, seed=13)
    bases = np.concatenate([bases, np.frombuffer(b"ACGTACGTAC", np.uint8)])
    offs = np.concatenate([offs, [offs[-1], offs[-1] + 10]]).astype(np.uint64)      # read 198: length 0, read 199: length 10
    assert set(int(o) for o in origin) >= set(range(9)) | {-1}
    # budgets: subtrees A, B (chain), C, D, E in root-bin order
    sub = [[ids["A"]], [ids["B"], ids["B1"], ids["B2"]], [ids["C"]], [ids["D"]], [ids["E"]]]
    sizes = [sum(_nbytes(host[i]) for i in ids_) for ids_ in sub]
    root = _nbytes(host[0]) + K4
    three = None
    for budget in range(root + max(sizes), root + sum(sizes), K4):
        try:
            plan, of, by = plan_passes(host, n_ub, budget, **kw)
        except _lib.TaxorError:
            continue
        if plan["n_passes"] == 3 and 2 in [[int(of[s[0]]) for s in sub].count(g) for g in range(3)]:
            three = budget
            break
    assert three is not None, f"no budget gives 3 passes with two subtrees in one: subtree bytes {sizes}"
    assert of[ids["A"]] != of[ids["C"]]           # genome 6 lies in A and in C: its reads match two subtrees of different groups
    return dict(kw=kw, host=host, n_ub=n_ub, bases=bases, offs=offs, budget3=three, budget1=root + sum(sizes), sizes=sizes, root=root,
                use_syncmer=use_syncmer, ref={})


@pytest.fixture(scope="module")
def world():
    return _world(True)


@pytest.fixture(scope="module")
def world_minimiser():
    return _world(False)


def _searcher(idx, w, **flags):
    return Searcher(idx, **flags) if w["use_syncmer"] else Searcher(idx, percentage=0.3, **flags)


def _resident(w, flags):
    """the ordinary searcher's CSR under these flags, computed once"""
    key = tuple(sorted(flags.items()))
    if key not in w["ref"]:
        idx = GpuIndex(w["host"], w["n_ub"], **w["kw"])
        sr = _searcher(idx, w, **flags)
        w["ref"][key] = sr.search_batch(w["bases"], w["offs"])
        sr.close()
        idx.close()
    return w["ref"][key]


def _paged(w, budget, flags, batches=1):
    idx = GpuIndex.paged(w["host"], w["n_ub"], budget, **w["kw"])
    sr = _searcher(idx, w, **flags)
    n = w["offs"].size - 1
    cuts = [n * j // batches for j in range(batches + 1)]
    prior = [[] for _ in range(batches)]
    out = []
    w["pass_tuples"] = []                         # tuples of every pass but the last, summed over the batches
    n_passes = idx.passes
    for p in range(n_passes):
        idx.load_pass(p)
        assert idx.data_bytes <= budget
        for j in range(batches):
            o = w["offs"][cuts[j]:cuts[j + 1] + 1]
            if p + 1 < n_passes:
                prior[j].append(sr.search_pass(w["bases"], o))
                if j == 0:
                    w["pass_tuples"].append(0)
                w["pass_tuples"][p] += prior[j][-1].key.size
            else:
                sr.search_batch(w["bases"], o)
                out.append(sr.merge_prior(prior[j]))
    sr.close()
    idx.close()
    ro = np.concatenate([[0]] + [r.read_off[1:] + sum(int(q.read_off[-1]) for q in out[:i]) for i, r in enumerate(out)]).astype(np.uint64)
    return n_passes, SearchResults(ro, np.concatenate([r.user_bin for r in out]), np.concatenate([r.count for r in out]),
                                   np.concatenate([r.n_hashes for r in out]))


def _same(a, b):
    assert np.array_equal(a.n_hashes, b.n_hashes)
    assert np.array_equal(a.read_off, b.read_off)
    assert np.array_equal(a.user_bin, b.user_bin)
    assert np.array_equal(a.count, b.count)


FLAGS = {
    "default": {},                                                     # 200 reads: the lanes, the one-launch tree traversal
    "no_prune": dict(prune=False),
    "tree_stall": dict(force_tree_stall=True),                         # ... and its level-by-level recovery
    "levels_grouped": dict(small_path=False, group_always=True),       # level launches with the grouped queue
    "split_always": dict(split_always=True),
}


@pytest.mark.parametrize("name", list(FLAGS))
def test_three_passes_equal_the_resident_search(world, name):
    w = world
    ref = _resident(w, FLAGS[name])
    n_passes, got = _paged(w, w["budget3"], FLAGS[name])
    assert n_passes == 3
    _same(got, ref)
    assert len(w["pass_tuples"]) == 2 and max(w["pass_tuples"]) < ref.user_bin.size     # no single pass saw the whole hierarchy
    wide = np.diff(ref.read_off.astype(np.int64))
    assert wide[198] > 64 and wide[199] > 64 and (wide == 0).any() and ((wide > 0) & (wide <= 64)).any()


def test_one_pass_budget_equals_the_resident_search(world):
    w = world
    n_passes, got = _paged(w, w["budget1"], {})
    assert n_passes == 1
    _same(got, _resident(w, {}))


def test_several_batches_per_pass(world):
    w = world
    n_passes, got = _paged(w, w["budget3"], {}, batches=3)
    assert n_passes == 3
    _same(got, _resident(w, {}))


def test_minimiser_mode_index(world_minimiser):
    w = world_minimiser
    ref = _resident(w, {})
    n_passes, got = _paged(w, w["budget3"], {})
    assert n_passes == 3
    _same(got, ref)
    assert ref.user_bin.size > 0


@pytest.mark.parametrize("which", ["syncmer", "minimiser"])
def test_paged_search_equals_the_cpu_oracle(world, world_minimiser, which):
    w = world if which == "syncmer" else world_minimiser
    _, got = _paged(w, w["budget3"], {})
    sel = np.r_[0:40, 196:200]                    # a sample: planted and random reads, the two short reads
    offs, bases = w["offs"], w["bases"]
    sb = np.concatenate([bases[int(offs[r]):int(offs[r + 1])] for r in sel]) if sel.size else bases[:0]
    so = np.concatenate([[0], np.cumsum([int(offs[r + 1] - offs[r]) for r in sel])]).astype(np.uint64)
    h = orc.Hixf(w["host"], [f["next_ixf"] for f in w["host"]], [f["fname_idx"] for f in w["host"]])
    kw = dict(threads=2) if which == "syncmer" else dict(k=20, percentage=0.3, window=24, threads=2)
    nh, off, ub, cnt, _ = h.search_batch(sb, so, **kw)
    for j, r in enumerate(sel):
        lo, hi = int(got.read_off[r]), int(got.read_off[r + 1])
        a, b = int(off[j]), int(off[j + 1])
        assert got.n_hashes[r] == nh[j]
        assert np.array_equal(got.user_bin[lo:hi], ub[a:b]) and np.array_equal(got.count[lo:hi], cnt[a:b]), f"read {r}"


# ---- the merge alone ---------------------------------------------------------------------------------------------------------------
def _tiny_searcher():
    bins = 64
    idx = GpuIndex.paged([dict(bins=bins, stride=64, seg_len=16, seed=1, next_ixf=np.zeros(bins, np.int64), fname_idx=np.arange(bins),
                               data=np.zeros(3 * 16 * 64, np.uint8))], bins, 1 << 20)
    idx.load_pass(0)
    return idx, Searcher(idx, ratio=1.0)


def _prior(lists):
    """lists: per read [(key, user_bin, count), ...]"""
    ro = np.concatenate([[0], np.cumsum([len(x) for x in lists])]).astype(np.uint64)
    flat = [t for x in lists for t in x]
    res = SearchResults(ro, np.array([t[1] for t in flat], np.int64), np.array([t[2] for t in flat], np.uint32), np.zeros(len(lists), np.uint32))
    return PassResults(res, np.array([t[0] for t in flat], np.uint32))


def _three_random_reads():
    rng = np.random.default_rng(5)
    bases = rng.choice(np.frombuffer(b"ACGT", np.uint8), 3 * 300)
    return bases, np.array([0, 300, 600, 900], np.uint64)


def test_merge_three_lists_with_overlapping_keys_and_an_empty_one():
    """the searcher's own lists are empty here (random reads against an all-zero filter at ratio 1 match nothing), so the result is the
    merge of the priors: read 0 has 150 distinct keys over three overlapping lists (more than two rounds of 64), read 1 nothing,
    read 2 one key that all three hold"""
    idx, sr = _tiny_searcher()
    bases, offs = _three_random_reads()
    own = sr.search_batch(bases, offs)
    assert own.user_bin.size == 0
    t = lambda k: (k, 1000 + k, 7 * k + 1)
    p0 = _prior([[t(k) for k in range(0, 200, 2)], [], [t(9)]])                # even keys 0..198
    p1 = _prior([[t(k) for k in range(0, 300, 3)], [], [t(9)]])                # multiples of 3 below 300
    p2 = _prior([[], [], [t(9)]])
    p3 = _prior([[t(k) for k in range(100, 110)], [], []])
    got = sr.merge_prior([p0, p1, p2, p3])
    keys0 = sorted(set(range(0, 200, 2)) | set(range(0, 300, 3)) | set(range(100, 110)))
    assert list(got.read_off) == [0, len(keys0), len(keys0), len(keys0) + 1]
    assert list(got.user_bin) == [1000 + k for k in keys0] + [1009]
    assert list(got.count) == [7 * k + 1 for k in keys0] + [7 * 9 + 1]
    assert list(sr.result_keys(got.user_bin.size)) == keys0 + [9]
    assert np.array_equal(got.n_hashes, own.n_hashes)
    sr.close()
    idx.close()


def test_merge_refuses_one_key_with_two_counts():
    idx, sr = _tiny_searcher()
    bases, offs = _three_random_reads()
    sr.search_batch(bases, offs)
    a = _prior([[(4, 40, 10), (8, 80, 11)], [], []])
    b = _prior([[(8, 80, 12)], [], []])
    with pytest.raises(_lib.TaxorError) as e:
        sr.merge_prior([a, b])
    assert e.value.code == -4                     # TAXOR_E_INTERNAL
    with pytest.raises(_lib.TaxorError) as e:     # keys that do not ascend are refused on the host, before any launch
        sr.merge_prior([_prior([[(8, 80, 1), (4, 40, 1)], [], []])])
    assert e.value.code == -1
    sr.close()
    idx.close()


def test_load_pass_out_of_order_or_during_a_search_is_an_error(world):
    w = world
    idx = GpuIndex.paged(w["host"], w["n_ub"], w["budget3"], **w["kw"])
    sr = Searcher(idx)
    with pytest.raises(_lib.TaxorError) as e:
        idx.load_pass(1)                          # before pass 0
    assert e.value.code == -1 and "out of order" in str(e.value)
    idx.load_pass(0)
    with pytest.raises(_lib.TaxorError) as e:
        idx.load_pass(2)
    assert e.value.code == -1 and "out of order" in str(e.value)
    with pytest.raises(_lib.TaxorError) as e:
        idx.load_pass(3)
    assert e.value.code == -1
    sr.search_batch_begin(w["bases"], w["offs"])
    with pytest.raises(_lib.TaxorError) as e:     # the status check alone: nothing is launched, the batch in flight is then ended
        idx.load_pass(1)
    assert e.value.code == -1 and "has not ended" in str(e.value)
    sr.search_batch_end()
    idx.load_pass(1)
    idx.load_pass(2)
    idx.load_pass(0)                              # start over
    ordinary = GpuIndex(w["host"], w["n_ub"], **w["kw"])
    assert ordinary.passes == 0 and idx.passes == 3
    with pytest.raises(_lib.TaxorError) as e:
        ordinary.load_pass(0)
    assert e.value.code == -1 and "not a paged index" in str(e.value)
    ordinary.close()
    sr.close()
    idx.close()
