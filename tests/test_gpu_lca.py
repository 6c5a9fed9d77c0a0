"""Per-read lowest common ancestor and per-taxon tallies (taxor_gpu_lca_*, taxor_amd/csrc/lca.hip): node, best, n_refs, direct_reads
and direct_bases EQUAL the Python restatement (tests/lca_expect.py) -- they are integers."""
import numpy as np
import pytest

from taxor_amd import GpuIndex, Searcher, _lib, synth
from taxor_amd.search import Lca, Lineage
from tests import lca_expect as le

pytestmark = pytest.mark.gpu

ECOLI = ("2;1224;1236;91347;543;561;562", "k__Bacteria;p__Proteobacteria;c__Gammaproteobacteria;o__Enterobacterales;f__Enterobacteriaceae;g__Escherichia;s__Escherichia coli")
EFERG = ("2;1224;1236;91347;543;561;564", "k__Bacteria;p__Proteobacteria;c__Gammaproteobacteria;o__Enterobacterales;f__Enterobacteriaceae;g__Escherichia;s__Escherichia fergusonii")
SENT = ("2;1224;1236;91347;543;590;28901", "k__Bacteria;p__Proteobacteria;c__Gammaproteobacteria;o__Enterobacterales;f__Enterobacteriaceae;g__Salmonella;s__Salmonella enterica")
BSUB = ("2;1239;91061;1385;186817;1386;1423", "k__Bacteria;p__Firmicutes;c__Bacilli;o__Bacillales;f__Bacillaceae;g__Bacillus;s__Bacillus subtilis")
SAUR = ("2;1239;91061;1385;90964;1279;1280", "k__Bacteria;p__Firmicutes;c__Bacilli;o__Bacillales;f__Staphylococcaceae;g__Staphylococcus;s__Staphylococcus aureus")
MJAN = ("2157;28890;183939;2182;2183;2184;2190", "k__Archaea;p__Euryarchaeota;c__Methanococci;o__Methanococcales;f__Methanocaldococcaceae;g__Methanocaldococcus;s__Methanocaldococcus jannaschii")
SEVEN = [ECOLI, ECOLI, EFERG, SENT, BSUB, SAUR, MJAN]       # two strains of one species, a second species of their genus


def species(ub, ids, names, acc=None):
    return dict(organism_name=names.split(";")[-1][3:] or f"Organism {ub}", accession_id=acc or f"GCF_{ub:09d}.1", taxid=([x for x in ids.split(";") if x] or ["0"])[-1],
                taxnames_string=names, taxid_string=ids, user_bin=ub, seq_len=1000000 + ub)


DEEP = [str(5000 + i) for i in range(64)]
# hand-made lineage over 64 user bins; bins 8.. have no species and fall back to species[0]
HAND = [species(0, *ECOLI), species(1, *ECOLI, acc="GCF_STRAIN2"), species(2, *EFERG), species(3, "2;1224;1236", "k__Bacteria;p__Proteobacteria;c__Gammaproteobacteria"),
        species(4, "2157;28890", "k__Archaea;p__Euryarchaeota"), species(5, "", ""),
        species(6, ";".join(DEEP), ";".join(f"x__D{i}" for i in range(64))), species(7, ";".join(DEEP[:63] + ["7777"]), ";".join(f"x__D{i}" for i in range(64)))]
N_BINS = 64


def dummy_index(n_bins=N_BINS):
    return GpuIndex([dict(bins=64, stride=64, seg_len=16, seed=1, next_ixf=np.zeros(64, np.int64), fname_idx=np.arange(64), data=np.zeros(3 * 16 * 64, np.uint8))], n_bins)


@pytest.fixture(scope="module")
def hand():
    idx = dummy_index()
    lin, want = Lineage(HAND, N_BINS), le.Lineage(HAND, N_BINS)
    yield dict(idx=idx, lin=lin, want=want)
    idx.close()


def csr(reads):
    """[[(bin, count), ...], ...] -> read_off, user_bin, count"""
    off = np.zeros(len(reads) + 1, np.uint64)
    off[1:] = np.cumsum([len(r) for r in reads])
    flat = [t for r in reads for t in r]
    return off, np.array([b for b, _ in flat], np.int64), np.array([c for _, c in flat], np.uint32)


def check_calls(h, calls, expected):
    want = h["want"]
    assert [int(x) for x in calls.node] == [want.node_number(x) for x, _, _ in expected]
    assert [int(x) for x in calls.best] == [b for _, b, _ in expected]
    assert [int(x) for x in calls.n_refs] == [n for _, _, n in expected]


def check_tallies(t, e):
    dr, db = e.tally_arrays()
    assert [int(x) for x in t.direct_reads] == dr
    assert [int(x) for x in t.direct_bases] == db
    assert t.n_reads == len(e.calls)


def run(h, reads, lens=None, pieces=None):
    """add the reads (in `pieces`, lists of indices, or at once) -> (calls in read order, tallies)"""
    lens = lens if lens is not None else [100 + 3 * i for i in range(len(reads))]
    pieces = pieces or [list(range(len(reads)))]
    node, best, refs = {}, {}, {}
    with Lca(h["idx"], h["lin"]) as lca:
        for pc in pieces:
            c = lca.add_csr(*csr([reads[i] for i in pc]), [lens[i] for i in pc])
            assert c.n_hashes is None
            for j, i in enumerate(pc):
                node[i], best[i], refs[i] = int(c.node[j]), int(c.best[j]), int(c.n_refs[j])
        t = lca.results()
    return node, best, refs, t


def test_path_shapes_and_filter_edges(hand):
    h = hand
    reads = [[],                                            # no tuple: U
             [(0, 7)],                                      # one reference: its leaf
             [(0, 9), (1, 9)],                              # identical full paths in two user bins: the leaf node
             [(0, 9), (2, 8)],                              # sibling species: the genus
             [(0, 9), (3, 9)],                              # one path a prefix of the other: the shorter path's end
             [(3, 9), (0, 9)],                              # ... whichever comes first
             [(0, 9), (4, 9)],                              # disagreement at the first node: ROOT
             [(5, 3)],                                      # the empty path alone: ROOT
             [(0, 9), (5, 9)],                              # ... and beside another
             [(6, 4)], [(6, 4), (7, 4)],                    # depth 64: the 64th node, the 63rd
             [(0, 10), (4, 8)],                             # 8 against 10: both kept -> ROOT
             [(0, 10), (4, 7)],                             # 7 against 10: dropped -> the leaf
             [(0, 5), (4, 4)],                              # 4 against 5: both kept
             [(0, 0), (4, 0), (2, 0)],                      # all-zero counts: U
             [(40, 6), (0, 6)],                             # a user bin without a species: species[0]'s path
             [(4, 2), (0, 1), (2, 1)]]                      # the first survivor is not the first tuple's successor: 2157 alone
    e = le.Expect(h["want"])
    exp = [e.add(r, 100 + 3 * i) for i, r in enumerate(reads)]
    got = [x for x, _, _ in exp]
    assert got == ["0", "562", "562", "561", "1236", "1236", "1", "1", "1", "5063", "5062", "1", "562", "1", "0", "562", "28890"]
    assert exp[0] == ("0", 0, 0) and exp[14] == ("0", 0, 0) and exp[11][2] == 2 and exp[12][2] == 1
    node, best, refs, t = run(h, reads)
    want = h["want"]
    assert [node[i] for i in range(len(reads))] == [want.node_number(x) for x in got]
    assert [(best[i], refs[i]) for i in range(len(reads))] == [(b, n) for _, b, n in exp]
    check_tallies(t, e)
    assert t.seconds_kernel > 0


@pytest.mark.parametrize("n", [0, 1, 2, 63, 64, 65, 129, 1000])
def test_tuples_per_read_at_the_wave_round_edges(hand, n):
    """n tuples in a read among others; random counts, the bins of one genus and a far one"""
    h = hand
    rng = np.random.default_rng(100 + n)
    reads = []
    for v in range(6):
        bins = rng.choice([0, 1, 2, 3] if v % 2 else [0, 1, 2, 4, 6], size=n)
        cnt = rng.integers(0, 30, size=n) if v < 4 else rng.integers(28, 30, size=n)
        reads += [[(int(b), int(c)) for b, c in zip(bins, cnt)], [(2, 5)]]
    e = le.Expect(h["want"])
    exp = [e.add(r, 100 + 3 * i) for i, r in enumerate(reads)]
    node, best, refs, t = run(h, reads)
    assert [(node[i], best[i], refs[i]) for i in range(len(reads))] == [(h["want"].node_number(x), b, k) for x, b, k in exp]
    check_tallies(t, e)


def test_the_only_survivor_sits_in_the_third_round(hand):
    h = hand
    read = [(4, 1)] * 140 + [(2, 100)] + [(0, 79)] * 30
    e = le.Expect(h["want"])
    assert e.add(read, 500) == ("564", 100, 1)
    also = [(4, 1)] * 130 + [(2, 100), (0, 80)]              # two survivors, both in the third round: the genus
    assert e.add(also, 600) == ("561", 100, 2)
    node, best, refs, t = run(h, [read, also], [500, 600])
    assert (node[0], best[0], refs[0]) == (h["want"].number["564"], 100, 1) and (node[1], refs[1]) == (h["want"].number["561"], 2)
    check_tallies(t, e)


def test_more_reads_than_one_grid_pass_and_lengths_past_2_32(hand):
    h = hand
    n = 70000
    rng = np.random.default_rng(3)
    bins = rng.integers(0, 8, size=n)
    cnt = rng.integers(0, 3, size=n)                         # a third of the reads: count 0, unclassified
    lens = [(1 << 31) + i for i in range(n)]                 # four reads pass 2^32 already
    off = np.arange(n + 1, dtype=np.uint64)
    e = le.Expect(h["want"])
    exp = e.add_csr(off, bins, cnt, lens)
    with Lca(h["idx"], h["lin"]) as lca:
        c = lca.add_csr(off, bins, cnt, lens)
        t = lca.results()
    check_calls(h, c, exp)
    check_tallies(t, e)
    assert int(t.direct_bases.max()) > (1 << 44)


def test_two_adds_equal_one_in_either_order(hand):
    h = hand
    rng = np.random.default_rng(5)
    reads = [[(int(b), int(c)) for b, c in zip(rng.integers(0, 8, size=k), rng.integers(0, 12, size=k))] for k in rng.integers(0, 9, size=900)]
    e = le.Expect(h["want"])
    exp = [e.add(r, 100 + 3 * i) for i, r in enumerate(reads)]
    X, Y = list(range(0, 400)), list(range(400, 900))
    for pieces in ([X, Y], [Y, X], [X + Y], [Y[::-1], X[::-1]]):
        node, best, refs, t = run(h, reads, pieces=pieces)
        assert [(node[i], best[i], refs[i]) for i in range(len(reads))] == [(h["want"].node_number(x), b, k) for x, b, k in exp]
        check_tallies(t, e)


def seven_genomes(seed):
    """seven genomes: 1 is genome 0 with 1 % of its bases changed (a strain), 2 with 6 % (a species of the genus), the rest random"""
    g, go = synth.random_genomes(7, 15000, seed=seed)
    g = g.copy()
    rng = np.random.default_rng(seed + 1)
    L = 15000
    for k, rate in ((1, 0.01), (2, 0.06)):
        cp = g[:L].copy()
        pos = rng.random(L) < rate
        cp[pos] = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, size=int(pos.sum()))]
        g[k * L:(k + 1) * L] = cp
    return g, go


def world_species(lay):
    by = {int(ub): SEVEN[i] for i, ub in enumerate(lay["planted_user_bin"])}
    return [species(ub, *by[ub]) if ub in by else species(ub, f"2;9999;{100000 + ub}", f"k__Bacteria;p__Decoys;s__Decoy {ub}") for ub in range(lay["n_user_bins"])]


def make_world(seed):
    g, go = seven_genomes(seed)
    dummy = dummy_index()
    hs = Searcher(dummy, ratio=0.5)
    hoff, hashes = hs.seq_to_syncmers(g, go)
    hs.close()
    dummy.close()
    planted = [hashes[int(hoff[i]):int(hoff[i + 1])] for i in range(7)]
    lay = synth.make_layout(planted, root_bins=68, child_bins=40, n_children=3, seed=seed)
    return g, go, lay, synth.materialize_host(lay), world_species(lay)


@pytest.fixture(scope="module")
def world():
    g, go, lay, host, sp = make_world(61)
    idx = GpuIndex(host, lay["n_user_bins"])
    yield dict(g=g, go=go, lay=lay, host=host, sp=sp, idx=idx)
    idx.close()


def test_add_batch_after_a_real_search(world):
    w = world
    nb = w["lay"]["n_user_bins"]
    lin, want = Lineage(w["sp"], nb), le.Lineage(w["sp"], nb)
    bases, offs, origin = synth.synth_reads(w["g"], w["go"], 300, 1200, error_rate=0.02, frac_random=0.2, seed=9)
    lens = np.diff(offs.astype(np.int64))
    sr = Searcher(w["idx"])
    e = le.Expect(want)
    with Lca(w["idx"], lin) as lca:
        for first, (a, b) in ((0, (0, 170)), (170, (170, 300))):          # two batches on one searcher
            lo, hi = int(offs[a]), int(offs[b])
            res = sr.search_batch(bases[lo:hi], offs[a:b + 1] - offs[a])
            c = lca.add_batch(sr, first)
            exp = e.add_csr(res.read_off, res.user_bin, res.count, lens[a:b])
            assert c.first_read == first and np.array_equal(c.n_hashes, res.n_hashes)
            assert [int(x) for x in c.node] == [want.node_number(x) for x, _, _ in exp]
            assert [int(x) for x in c.best] == [m for _, m, _ in exp] and [int(x) for x in c.n_refs] == [k for _, _, k in exp]
        t = lca.results()
    sr.close()
    dr, db = e.tally_arrays()
    assert [int(x) for x in t.direct_reads] == dr and [int(x) for x in t.direct_bases] == db
    called = {x for x, _, _ in e.calls}
    assert {"562", "0"} <= called and ("561" in called or "564" in called), called       # the strains' species, random reads, the genus or its other species
    assert int(t.direct_bases.sum()) == int(lens.sum())


def test_index_from_the_gpu_builder(world):
    w = world
    bins = 64
    dummy = dummy_index()
    hs = Searcher(dummy, ratio=0.5)
    hoff, hashes = hs.seq_to_syncmers(w["g"], w["go"])
    hs.close()
    dummy.close()
    where = {2: 0, 9: 1, 40: 3}                                                         # bin -> genome
    keys = {b: np.unique(hashes[int(hoff[gi]):int(hoff[gi + 1])]) for b, gi in where.items()}
    n = max(k.size for k in keys.values())
    ixfs = [dict(bins=bins, stride=64, seg_len=synth.seg_len_for(n), seed=1, next_ixf=np.zeros(bins, np.int64), fname_idx=np.arange(bins), data=None)]
    idx = GpuIndex(ixfs, bins)
    idx.fill_random(0, 5)
    idx.build_ixf(0, keys, seed0=3)
    sp = [species(2, *ECOLI), species(9, *ECOLI, acc="GCF_STRAIN2"), species(40, *SENT)]
    lin, want = Lineage(sp, bins), le.Lineage(sp, bins)
    bases, offs, origin = synth.synth_reads(w["g"], w["go"], 120, 1200, error_rate=0.02, frac_random=0.1, seed=4)
    sr = Searcher(idx)
    res = sr.search_batch(bases, offs)
    e = le.Expect(want)
    exp = e.add_csr(res.read_off, res.user_bin, res.count, np.diff(offs.astype(np.int64)))
    with Lca(idx, lin) as lca:
        c = lca.add_batch(sr)
        t = lca.results()
    assert [int(x) for x in c.node] == [want.node_number(x) for x, _, _ in exp]
    dr, db = e.tally_arrays()
    assert [int(x) for x in t.direct_reads] == dr and [int(x) for x in t.direct_bases] == db
    assert e.reads.get("562", 0) > 0 and e.reads.get("28901", 0) > 0
    sr.close()
    idx.close()


def test_refusals_come_before_any_launch(hand, world):
    h, w = hand, world
    with pytest.raises(_lib.TaxorError) as ei:                                          # a lineage of another size
        Lca(w["idx"], h["lin"])
    assert ei.value.code == -1 and "n_user_bins" in str(ei.value)
    total = sum(3 * f["seg_len"] * f["stride"] + 8192 for f in w["host"])
    nb = w["lay"]["n_user_bins"]
    wl = Lineage(w["sp"], nb)
    paged = GpuIndex.paged(w["host"], nb, 4 * total)
    with pytest.raises(_lib.TaxorError) as ei:
        Lca(paged, wl)
    assert ei.value.code == -1 and "paged index" in str(ei.value)
    paged.close()
    with Lca(h["idx"], h["lin"]) as lca:
        with pytest.raises(_lib.TaxorError) as ei:                                      # a user bin outside the lineage
            lca.add_csr(*csr([[(0, 3)], [(1, 2), (N_BINS, 9)]]), [10, 20])
        assert ei.value.code == -1 and "user_bin" in str(ei.value) and str(N_BINS) in str(ei.value)
        with pytest.raises(_lib.TaxorError) as ei:
            lca.add_csr(*csr([[(-1, 3)]]), [10])
        assert "user_bin" in str(ei.value)
        sr = Searcher(w["idx"])                                                        # a searcher of another index
        bases, offs, _ = synth.synth_reads(w["g"], w["go"], 8, 600, seed=2)
        sr.search_batch(bases, offs)
        with pytest.raises(_lib.TaxorError) as ei:
            lca.add_batch(sr)
        assert ei.value.code == -1 and "index" in str(ei.value)
        sr.close()
        t = lca.results()
        assert not t.direct_reads.any() and not t.direct_bases.any() and t.n_reads == 0 and t.seconds_kernel == 0     # nothing was launched
