"""Where along its read each saved hash lies (taxor_gpu_search_capture_positions, taxor_gpu_saved_positions, `taxor search
--base-positions`).  The expectation is tests/positions_expect.py: the definition as a plain loop over p with the
CPU oracle's own canonical k-mer hash.  Every comparison is exact equality of the whole position array.
1. random reads at the lengths where the kernel's paths change: no k-mer, one, two, the 64-base word edges, the 4096-start tile, and
   exactly 2048 / 2049 hashes (one piece / two);
2. repeats: positions are the FIRST occurrence (a tandem unit, a read and its reverse complement), and the tie-rule reads;
3. k32/s20 (the k-mer fills the word), k16/s8, FracMinHash scaling 4, IUPAC codes;
4. the sub-batch cut and the 4-bit input route do not matter;
5. off is off, and every refusal names its reason;
6. the command line: leading columns unchanged, appended columns from the helper, the junction within k bases, both refusals."""
import os
import subprocess

import numpy as np
import pytest

from oracle import oracle as orc
from taxor_amd import GpuIndex, Searcher, synth
from taxor_amd.hixf_file import store_hixf
from taxor_amd._lib import TaxorError
from taxor_amd.search import read_bam
from tests import bam_writer as bw
from tests import positions_expect as pe

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TAXOR = os.path.join(ROOT, "taxor_amd", "taxor")
COMP = bytes.maketrans(b"ACGT", b"TGCA")


def _cat(reads):
    off = np.zeros(len(reads) + 1, np.uint64)
    off[1:] = np.cumsum([len(r) for r in reads])
    return np.frombuffer(b"".join(reads), np.uint8), off


@pytest.fixture(scope="module")
def genome():
    g, _ = synth.random_genomes(1, 40000, seed=4711)
    return bytes(g)


@pytest.fixture(scope="module")
def layout(genome):
    """one small planted layout for every index below: what the query finds does not matter here, only what is hashed"""
    planted = [orc.seq_to_syncmers(genome[i * 5000:(i + 1) * 5000]) for i in range(5)]
    lay = synth.make_layout(planted, root_bins=66, child_bins=24, n_children=2, seed=5)
    return synth.materialize_host(lay), lay["n_user_bins"]


def _index(layout, k=22, s=12, t=5, **kw):
    return GpuIndex(layout[0], layout[1], k, s, t, **kw)


def _saved(sr, reads, nibbles=None):
    """one batch with capture and positions on -> the SavedBatch"""
    sr.capture(True)
    sr.capture_positions(True)
    if nibbles is not None:
        sr.search_nibbles(nibbles)
    else:
        sr.search_batch(*_cat(reads))
    return sr.take_saved()


def _check(sv, reads, k, oracle_lists=None):
    """the saved batch's positions equal the definition, whole array; returns them per read"""
    assert sv.positions is not None and sv.positions.dtype == np.uint32 and sv.positions.size == sv.total_hashes
    if oracle_lists is not None:                       # the lists are the oracle's, so the expectation stands on them too
        for r, want in enumerate(oracle_lists):
            assert np.array_equal(sv.hashes[int(sv.hash_off[r]):int(sv.hash_off[r + 1])], want), r
    want = pe.batch_positions(reads, sv.hash_off, sv.hashes, k)
    assert want.size == sv.total_hashes and not (want == pe.SENTINEL).any()
    assert np.array_equal(sv.positions, want), [(i, int(a), int(b)) for i, (a, b) in enumerate(zip(sv.positions, want)) if a != b][:8]
    return [sv.positions[int(sv.hash_off[r]):int(sv.hash_off[r + 1])].astype(np.int64) for r in range(len(reads))]


@pytest.fixture(scope="module")
def piece_edge(genome):
    """prefix lengths of the genome that give exactly 2048 and 2049 hashes at k22/s12/t5, found with the oracle"""
    found = {}
    for L in range(21000, 26000):
        n = len(orc.seq_to_syncmers(genome[:L]))
        if n in (2048, 2049) and n not in found:
            found[n] = L
        if len(found) == 2:
            break
    assert sorted(found) == [2048, 2049]
    return found


def test_random_reads_at_every_edge(layout, genome, piece_edge):
    lens = [0, 21, 22, 23, 64, 4095, 4096, 4097, piece_edge[2048], piece_edge[2049]]
    reads = [genome[7:7 + L] if L < 5000 else genome[:L] for L in lens]
    idx = _index(layout)
    sr = Searcher(idx)
    sv = _saved(sr, reads)
    assert [int(x) for x in sv.n_hashes[-2:]] == [2048, 2049] and [int(x) for x in sv.n_hashes[:2]] == [0, 0]
    per_read = _check(sv, reads, 22, [orc.seq_to_syncmers(r) if len(r) else np.zeros(0, np.uint64) for r in reads])
    for r, p in zip(reads, per_read):                  # random reads: no k-mer twice, so the positions are the emitting windows'
        assert (np.diff(p) > 0).all() and (p + 22 <= len(r)).all()
    sv.close()
    sr.close()
    idx.close()


def test_repeats_resolve_to_the_first_occurrence(layout, genome):
    unit, half = genome[30000:30300], genome[31000:32500]
    tandem = unit * 8
    both = half + half.translate(COMP)[::-1]
    ties = [b"A" * 2000, b"AT" * 1000, (b"TTAGGG" * 334)[:2000]]
    reads = [tandem, both] + ties
    idx = _index(layout)
    sr = Searcher(idx)
    sv = _saved(sr, reads)
    per_read = _check(sv, reads, 22, [orc.seq_to_syncmers(r) for r in reads])
    assert per_read[0].size > 20 and (per_read[0] < 300).all()          # the first unit, or a k-mer across the first seam
    assert per_read[1].size > 100 and (per_read[1] + 22 <= len(half) + 21).all()   # a second-half k-mer is a first-half one's complement, or spans the joint
    assert all(p.size >= 1 for p in per_read[2:])                       # the tie-rule reads: equality with the definition only
    sv.close()
    sr.close()
    idx.close()


@pytest.mark.parametrize("k,s,t,scaling", [(32, 20, 4, 1), (16, 8, 3, 1), (22, 12, 5, 4)])
def test_parameter_edges(layout, genome, k, s, t, scaling):
    iupac = bytearray(genome[33000:34200])
    for i, c in zip(range(5, 1200, 37), b"NRYKMSWBDHVUnrykmacgt" * 2):
        iupac[i] = c
    reads = [genome[20000:23000], genome[100:100 + k], genome[200:200 + k + 1], bytes(iupac), b"N" * 100]
    idx = _index(layout, k, s, t, scaling=scaling)
    sr = Searcher(idx, ratio=0.5)                      # (the syncmer model has no row for k = 32; the threshold does not matter here)
    sv = _saved(sr, reads)
    assert sv.params["kmer_size"] == k and sv.params["scaling"] == scaling and sv.total_hashes > 50
    lists = []
    for r in reads:                                    # the oracle's list of the mapped read, thinned as the search thins it
        h = orc.seq_to_syncmers(orc.dna4_normalise(r), k, s, t)
        if scaling > 1:
            h = h[np.array([float(orc.wyhash(int(x))) <= float(2**64 - 1) / float(scaling) for x in h], dtype=bool)] if h.size else h
        lists.append(h)
    _check(sv, reads, k, lists)
    sv.close()
    sr.close()
    idx.close()


def test_the_cut_and_the_input_route_do_not_matter(layout, genome, tmp_path):
    rng = np.random.default_rng(12)
    reads = []
    for i in range(300):                               # 300 reads of 30 .. 700 bases, every tenth a tandem repeat
        a, L = int(rng.integers(0, 39000)), int(rng.integers(30, 700))
        reads.append(genome[a:a + 60] * (L // 60 + 1) if i % 10 == 9 else genome[a:a + L])
    idx = _index(layout)
    one = Searcher(idx)
    sv1 = _saved(one, reads)
    assert sv1.n_sub_batches == 1
    want = _check(sv1, reads, 22)
    want = np.concatenate(want)
    cut = Searcher(idx, sub_batch_reads=64)            # the sub-batch plan's knob: five sub-batches, both dense arrays used twice
    sv2 = _saved(cut, reads)
    assert sv2.n_sub_batches >= 3
    assert np.array_equal(sv2.hashes, sv1.hashes) and np.array_equal(sv2.positions, want)
    bw.write_bam(tmp_path / "r.bam", [(b"r%d" % i, bw.codes_of_ascii(r), 4) for i, r in enumerate(reads)], block=30000)
    _, seq4, boff, rlen, rev = read_bam(tmp_path / "r.bam")
    assert len(rlen) == len(reads)
    sv3 = _saved(cut, None, nibbles=[(seq4, boff, rlen, rev)])
    assert np.array_equal(sv3.hashes, sv1.hashes) and np.array_equal(sv3.positions, want)
    for sv in (sv1, sv2, sv3):
        sv.close()
    one.close()
    cut.close()
    idx.close()


def test_off_is_off_and_the_refusals_name_their_reason(layout, genome):
    reads = [genome[1000:3000], genome[5000:5500]]
    idx = _index(layout)
    sr = Searcher(idx)
    with pytest.raises(TaxorError, match="capture is off"):
        sr.capture_positions(True)
    sr.capture(True)
    sr.search_batch(*_cat(reads))
    plain = sr.take_saved()
    assert plain.positions is None
    plain_bytes = plain.nbytes
    sr.capture_positions(True)
    sr.search_batch(*_cat(reads))
    with_pos = sr.take_saved()
    assert with_pos.positions is not None and with_pos.nbytes == plain_bytes + 4 * with_pos.total_hashes
    # a replay ignores positions
    again = sr.search_saved(with_pos)
    assert np.array_equal(again.n_hashes, with_pos.n_hashes)
    sr.capture_positions(False)
    sr.search_batch(*_cat(reads))
    off = sr.take_saved()
    assert off.positions is None and off.nbytes == plain_bytes
    # plain capture off turns positions off too
    sr.capture_positions(True)
    sr.capture(False)
    sr.capture(True)
    sr.search_batch(*_cat(reads))
    off2 = sr.take_saved()
    assert off2.positions is None and off2.nbytes == plain_bytes
    # a batch in flight
    B, O = _cat(reads)
    sr.search_batch_begin(B, O)
    with pytest.raises(TaxorError, match="a batch is in flight"):
        sr.capture_positions(True)
    sr.search_batch_end()
    for sv in (plain, with_pos, off, off2):
        sv.close()
    sr.close()
    idx.close()
    # a minimiser index
    midx = GpuIndex(layout[0], layout[1], k=20, s=0, t=0, use_syncmer=False, window_size=28)
    ms = Searcher(midx)
    ms.capture(True)
    with pytest.raises(TaxorError, match="does not hash syncmers"):
        ms.capture_positions(True)
    ms.close()
    midx.close()


# ---- the command line ---------------------------------------------------------------------------------------------------------------------
def _cli(index, fq, extra, ok=True):
    cmd = [TAXOR, "search", "--index-file", str(index), "--query-file", str(fq), "--threads", "4", "--batch-reads", "30", "--percentage", "0.1"] + [str(x) for x in extra]
    cp = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert (cp.returncode == 0) == ok, cp.stderr
    return cp


def test_cli_appends_real_bases(tmp_path):
    from tests.test_gpu_lca import make_world
    g, go, lay, host, sp = make_world(63)
    index = tmp_path / "idx.hixf"
    store_hixf(index, host, lay["n_user_bins"], sp)
    G = [bytes(g[int(go[i]):int(go[i + 1])]) for i in range(len(go) - 1)]
    bases, offs, _ = synth.synth_reads(g, go, 40, 1200, error_rate=0.02, frac_random=0.2, seed=9)
    reads = [bytes(bases[int(offs[i]):int(offs[i + 1])]) for i in range(40)]
    # chimeras of two unrelated genomes with the junction where it was planted; one carries a low-complexity stretch inside its left half,
    # which brings a single hash for 400 bases: the evenly-spread BREAK_BASE_APPROX lies more than 100 bases off there
    chim = [(G[3][1000:5000], G[5][2000:6000]), (G[4][0:1500] + b"AT" * 200 + G[4][1500:3000], G[6][2000:4500]), (G[5][100:1900], G[3][7000:12000])]
    junction = {len(reads) + i: len(a) for i, (a, b) in enumerate(chim)}
    reads += [a + b for a, b in chim]
    ids = [b"r%d" % i for i in range(len(reads))]
    fq = tmp_path / "reads.fastq"
    with open(fq, "wb") as f:
        for rid, r in zip(ids, reads):
            f.write(b"@" + rid + b"\n" + r + b"\n+\n" + b"I" * len(r) + b"\n")
    k = 22
    _cli(index, fq, ["--breakpoint-file", tmp_path / "bp0.tsv", "--segments-file", tmp_path / "sg0.tsv"])
    _cli(index, fq, ["--breakpoint-file", tmp_path / "bp1.tsv", "--segments-file", tmp_path / "sg1.tsv", "--base-positions"])
    lists = {}

    def pos(r):                                        # the helper's positions of read r's ordered hash list
        if r not in lists:
            lists[r] = pe.positions(reads[r], orc.seq_to_syncmers(reads[r]), k)
        return lists[r]

    for name, extra_cols, lead in (("bp", ["LEFT_END_BASE", "BREAK_BASE"], 18), ("sg", ["BASE_START", "BASE_END"], 19)):
        old = open(tmp_path / f"{name}0.tsv").read().splitlines()
        new = open(tmp_path / f"{name}1.tsv").read().splitlines()
        assert len(old) == len(new) and len(new) > 3
        assert new[0] == old[0] + "\t" + "\t".join(extra_cols)
        for a, b in zip(old[1:], new[1:]):
            f = b.split("\t")
            assert len(f) == lead + 2 and "\t".join(f[:lead]) == a           # the leading columns are byte-identical
    seen = set()
    for line in open(tmp_path / "bp1.tsv").read().splitlines()[1:]:
        f = line.split("\t")
        r, brk = int(f[0][1:]), int(f[7])
        p = pos(r)
        assert int(f[2]) == p.size and 0 < brk < p.size
        assert int(f[18]) == int(p[brk - 1]) + k and int(f[19]) == int(p[brk])
        if r in junction:                              # halves that share no k-mer: the break is the junction, to within k bases
            seen.add(r)
            assert abs(int(f[19]) - junction[r]) <= k, (r, f[18], f[19], junction[r])
    assert seen == set(junction)
    n_seg = 0
    for line in open(tmp_path / "sg1.tsv").read().splitlines()[1:]:
        f = line.split("\t")
        r, a, b = int(f[0][1:]), int(f[9]), int(f[10])
        p = pos(r)
        assert 0 <= a < b <= p.size
        assert int(f[19]) == int(p[a]) and int(f[20]) == int(p[b - 1]) + k and int(f[20]) <= len(reads[r])
        n_seg += 1
    assert n_seg >= 6
    # the refusals: the switch alone, and an index that does not hash syncmers
    cp = _cli(index, fq, ["--output-file", tmp_path / "o.tsv", "--base-positions"], ok=False)
    assert "--base-positions" in cp.stderr and "needs one of them" in cp.stderr
    mini = tmp_path / "mini.hixf"
    store_hixf(mini, host, lay["n_user_bins"], sp, k=20, s=0, t=0, window_size=28, use_syncmer=False)
    cp = _cli(mini, fq, ["--breakpoint-file", tmp_path / "bpm.tsv", "--base-positions"], ok=False)
    assert "--base-positions" in cp.stderr and "does not hash syncmers" in cp.stderr
