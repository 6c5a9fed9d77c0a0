"""BAM input on the device: k_pack_nibbles alone against words computed from the restored ASCII reads, the alphabet flag, the library
route (taxor_gpu_search_nibbles_begin) against the ASCII route on the same reads, and `taxor search x.bam` against the same reads as
FASTQ -- one device, two workers sharing BAM batches, an index paged in three passes, search-to-profile.  The BAM files come from
tests/bam_writer.py, whose decoding (reverse complement on the IUPAC codes for flag 0x10) is the expected value everywhere."""
import os
import subprocess

import numpy as np
import pytest

from oracle import oracle as orc
from taxor_amd import GpuIndex, Searcher, synth
from taxor_amd._lib import TaxorError
from taxor_amd.search import read_bam
from tests import bam_writer as bw

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TAXOR = os.path.join(ROOT, "taxor_amd", "taxor")
E_ARG, E_ALPHABET = -1, -3
# 4095 / 4096 / 4097: one pass of a 256-thread block over 16-base words, and its edge
LENGTHS = [0, 1, 2, 15, 16, 17, 31, 32, 33, 63, 64, 65, 4095, 4096, 4097]


def _dummy_index():
    bins = 64
    return GpuIndex([dict(bins=bins, stride=64, seg_len=16, seed=1, next_ixf=np.zeros(bins, np.int64), fname_idx=np.arange(bins),
                          data=np.zeros(3 * 16 * 64, np.uint8))], bins)


def expected_words(ascii_reads):
    """k_pack_dna4's layout from ASCII: seqan3's dna4 rank of every letter (the oracle's normalisation), 16 bases per word, the first
    in the top bits, every read padded with zero words to a multiple of four"""
    rank = np.zeros(256, np.uint32)
    for i, ch in enumerate(b"ACGT"):
        rank[ch] = i
    off, words = [0], []
    for s in ascii_reads:
        r = rank[np.frombuffer(orc.dna4_normalise(s), np.uint8)].astype(np.uint64)
        nw = (len(s) + 15) // 16
        pad = np.zeros(nw * 16, np.uint64)
        pad[:len(s)] = r
        w = (pad.reshape(nw, 16) << (30 - 2 * np.arange(16, dtype=np.uint64))).sum(axis=1).astype(np.uint32) if nw else np.zeros(0, np.uint32)
        words.append(np.concatenate([w, np.zeros((-nw) % 4, np.uint32)]))
        off.append(off[-1] + words[-1].size)
    return np.array(off, np.uint64), np.concatenate(words) if words else np.zeros(0, np.uint32)


def lay_out(reads, aligns, spare=0xF, fill=0xEE):
    """the reads' SEQ fields in one buffer, read i starting at a byte offset that is aligns[i] mod 4 -> (seq4, byte_off, read_len, reverse)"""
    buf, boff = bytearray(), []
    for (codes, flag), a in zip(reads, aligns):
        while len(buf) % 4 != a:
            buf.append(fill)
        boff.append(len(buf))
        buf += bw.seq_bytes(codes, spare)
    return (np.frombuffer(bytes(buf), np.uint8), np.array(boff, np.uint64), np.array([len(c) for c, _ in reads], np.uint32),
            np.array([1 if f & 0x10 else 0 for _, f in reads], np.uint8))


@pytest.fixture(scope="module")
def packer():
    idx = _dummy_index()
    sr = Searcher(idx, ratio=0.5)
    yield sr
    sr.close()
    idx.close()


def test_pack_nibbles_against_words_from_the_restored_ascii(packer):
    rng = np.random.default_rng(41)
    reads, aligns = [], []
    for L in LENGTHS:
        for flag in (0, 0x10):
            for a in range(4):
                reads.append((rng.integers(1, 16, L).astype(np.uint8), flag))
                aligns.append(a)
    # two segments; the last read (4097 bases, reversed, odd: its spare nibble is 0xF) ends at its buffer's last byte
    half = len(reads) // 2
    segs = [lay_out(reads[:half], aligns[:half]), lay_out(reads[half:], aligns[half:])]
    assert int(segs[1][1][-1]) + (4097 + 1) // 2 == segs[1][0].size and segs[1][0][-1] & 0xF == 0xF
    want_off, want = expected_words([bw.restored(c, f) for c, f in reads])
    off, words = packer.pack_nibbles(segs)
    assert np.array_equal(off, want_off)
    bad = np.flatnonzero(words != want)
    assert bad.size == 0, (bad[:8], [int(np.searchsorted(want_off, b, side="right")) - 1 for b in bad[:8]])
    # all reads forward, no reverse array at all
    fwd = [(c, 0) for c, _ in reads[:half]]
    q, o, n, _ = lay_out(fwd, aligns[:half])
    off2, words2 = packer.pack_nibbles([(q, o, n, None)])
    w_off, w = expected_words([bw.restored(c, 0) for c, _ in fwd])
    assert np.array_equal(off2, w_off) and np.array_equal(words2, w)


def test_complement_comes_before_the_dna4_mapping(packer):
    """R (A or G) reversed is Y, which maps to C; mapping first would give A -> T"""
    q, o, n, r = lay_out([([5], 0x10), ([5], 0)], [0, 1])
    _, words = packer.pack_nibbles([(q, o, n, r)])
    assert bw.restored([5], 0x10) == b"Y" and bw.restored([5], 0) == b"R"
    assert words[0] == 1 << 30 and words[4] == 0


@pytest.mark.parametrize("flag", [0, 0x10])
@pytest.mark.parametrize("where", [0, 17, 99])
def test_nibble_zero_is_outside_the_alphabet(packer, flag, where):
    codes = np.full(100, 2, np.uint8)
    codes[where] = 0
    with pytest.raises(TaxorError) as e:
        packer.pack_nibbles([lay_out([(codes, flag)], [1])])
    assert e.value.code == E_ALPHABET
    with pytest.raises(TaxorError) as e:
        packer.search_nibbles([lay_out([(codes, flag)], [3])])
    assert e.value.code == E_ALPHABET
    # ... and the spare nibble of an odd read is not part of it
    q, o, n, r = lay_out([(np.full(99, 2, np.uint8), flag)], [2], spare=0)
    packer.pack_nibbles([(q, o, n, r)])


def test_arguments_are_checked_before_anything_runs(packer):
    q, o, n, r = lay_out([([1, 2, 4, 8, 1], 0), ([8, 4], 0x10)], [0, 0])
    L = [(q, o, n, r)]
    packer.pack_nibbles(L)
    for seg in ((q, o[::-1].copy(), n, r),                              # not ascending
                (q, np.array([0, 2], np.uint64), n, r),                # inside the read before (5 bases are 3 bytes)
                (q, o, np.array([5, 1 << 31], np.uint32), r),          # 2^31 bases
                (q, np.array([0, 1 << 40], np.uint64), n, r)):         # 2^40 bytes
        with pytest.raises(TaxorError) as e:
            packer.search_nibbles([seg])
        assert e.value.code == E_ARG, seg
    import ctypes as C
    from taxor_amd import _lib
    arr = (_lib.NibbleSegment * 1)(_lib.NibbleSegment(None, o.ctypes.data, n.ctypes.data, None, 2))
    assert _lib.lib().taxor_gpu_search_nibbles_begin(packer._h, arr, 1) == E_ARG
    arr = (_lib.NibbleSegment * 1)(_lib.NibbleSegment(q.ctypes.data, None, n.ctypes.data, None, 2))
    assert _lib.lib().taxor_gpu_search_nibbles_begin(packer._h, arr, 1) == E_ARG
    assert _lib.lib().taxor_gpu_search_nibbles_begin(packer._h, None, 1) == E_ARG
    assert _lib.lib().taxor_gpu_search_nibbles_begin(None, arr, 1) == E_ARG
    del C


def _bam_reads(g, go, n, seed, lo=300, hi=3000):
    """[(name, codes as stored, flag)]: reads of lo..hi bases from the genomes, a third stored reverse-complemented (flag 0x10), a few
    with IUPAC codes, every tenth random; plus secondary / supplementary records that must not be searched"""
    rng = np.random.default_rng(seed)
    acgt = np.frombuffer(b"ACGT", np.uint8)
    glen = int(go[1] - go[0])
    out = []
    for i in range(n):
        L = int(rng.integers(lo, min(hi, glen) + 1))
        if i % 10 == 9:
            seq = acgt[rng.integers(0, 4, L)].copy()
        else:
            j = int(rng.integers(0, go.size - 1))
            a = int(go[j]) + int(rng.integers(0, glen - L + 1))
            seq = np.array(g[a:a + L], dtype=np.uint8)
        if i % 7 == 3:
            seq[rng.integers(0, L, 5)] = np.frombuffer(b"NRYKM", np.uint8)
        codes = bw.codes_of_ascii(bytes(seq))
        flag = 4
        if i % 3 == 1:                                   # stored as the reverse complement: restoring it gives `seq` back
            codes = np.array([bw.COMPLEMENT[int(x)] for x in codes[::-1]], np.uint8)
            flag = 0x10
            assert bw.restored(codes, flag) == bytes(seq)
        out.append((b"read_%d" % ((i * 7919) % n), codes, flag))
        if i % 25 == 0:
            out.append((b"read_%d" % ((i * 7919) % n), codes[:L // 2], 0x800 | (flag & 0x10)))
        if i % 40 == 0:
            out.append((b"read_%d" % ((i * 7919) % n), codes, 0x100))
    return out


def _cat(reads):
    off = np.zeros(len(reads) + 1, np.uint64)
    off[1:] = np.cumsum([len(r) for r in reads])
    return np.frombuffer(b"".join(reads), np.uint8), off


@pytest.mark.parametrize("mode", ["syncmer", "minimiser"])
def test_search_nibbles_equals_search_batch_on_the_restored_reads(tmp_path, mode):
    if mode == "syncmer":
        from tests.test_gpu_parity import _planted_setup
        g, go, lay, host = _planted_setup(5)
        idx = GpuIndex(host, lay["n_user_bins"])
    else:
        from tests.test_gpu_minimiser import _planted
        g, go, lay, host = _planted(20, 28, seed=49)
        idx = GpuIndex(host, lay["n_user_bins"], k=20, s=0, t=0, use_syncmer=False, window_size=28)
    reads = _bam_reads(g, go, 200, seed=43)
    p = tmp_path / "lib.bam"
    bw.write_bam(p, reads, block=5000, spare=0xF)
    ids, seq4, boff, rlen, rev = read_bam(p)
    sel = bw.selected(reads)
    assert ids == [n for n, _ in sel] and 60 <= int(rev.sum()) <= 70 and len(sel) == 200
    B, O = _cat([s for _, s in sel])
    sr = Searcher(idx, sub_batch_reads=128)          # two sub-batches
    want = sr.search_batch(B, O)
    got = sr.search_nibbles([(seq4, boff, rlen, rev)])
    assert want.user_bin.size > 100
    for f in ("n_hashes", "read_off", "user_bin", "count"):
        assert np.array_equal(getattr(got, f), getattr(want, f)), f
    # the timed upload (k_pack_dna4 between two events) leaves what upload() leaves: the resident run gives the same results
    ms = sr.upload_timed(B, O)
    assert 0.0 < ms < 1000.0
    sr.run()
    sr.sync()
    r3 = sr.fetch()
    for f in ("n_hashes", "read_off", "user_bin", "count"):
        assert np.array_equal(getattr(r3, f), getattr(want, f)), f
    woff, words, ms_n = sr.pack_nibbles([(seq4, boff, rlen, rev)], timed=True)
    assert 0.0 < ms_n < 1000.0 and np.array_equal(words, expected_words([s for _, s in sel])[1])
    # the same reads as two segments
    h = 77
    cut = int(boff[h])
    got2 = sr.search_nibbles([(seq4[:cut], boff[:h], rlen[:h], rev[:h]), (seq4[cut:], boff[h:] - np.uint64(cut), rlen[h:], rev[h:])])
    for f in ("n_hashes", "read_off", "user_bin", "count"):
        assert np.array_equal(getattr(got2, f), getattr(want, f)), f
    sr.close()
    idx.close()


# ---- the command line -------------------------------------------------------------------------------------------------------------
N_GENOMES, GENOME_LEN = 40, 60000


def run(args, timeout=300, **kw):
    return subprocess.run([TAXOR] + [str(a) for a in args], capture_output=True, text=True, timeout=timeout, **kw)


@pytest.fixture(scope="module")
def world(tmp_path_factory):
    """the paged test's index (40 genomes, --tmax 6: every root bin a merged bin over a subtree), 200 reads as BAM and as FASTQ"""
    from tests.test_gpu_paged_search_cli import plan_of
    tmp = tmp_path_factory.mktemp("bam_cli")
    g, go = synth.random_genomes(N_GENOMES, GENOME_LEN, seed=31)
    gdir = tmp / "genomes"
    gdir.mkdir()
    lines = []
    for i in range(N_GENOMES):
        acc = f"GCF_{800000 + (i * 7) % N_GENOMES:09d}.1"
        stem = f"{acc}_ASM{i}v1_genomic"
        (gdir / (stem + ".fna")).write_bytes(b">chr1\n" + bytes(g[int(go[i]):int(go[i + 1])]) + b"\n")
        names = f"k__Bacteria;p__P{i % 2};c__C{i % 3};o__O{i % 5};f__F{i % 7};g__G{i};s__G{i} species{i}"
        ids = f"2;{20 + i % 2};{30 + i % 3};{40 + i % 5};{500 + i % 7};{6000 + i};{70000 + i}"
        lines.append("\t".join([acc, str(70000 + i), f"ftp://host/genomes/{acc}/{stem}", f"G{i} species{i}", names, ids]))
    tax = tmp / "tax.tsv"
    tax.write_text("\n".join(lines) + "\n")
    idx = tmp / "idx.hixf"
    cp = run(["build", "--input-file", tax, "--input-sequence-dir", gdir, "--output-filename", idx, "--threads", "4", "--use-syncmer",
              "--kmer-size", "22", "--syncmer-size", "12", "--tmax", "6"], timeout=600)
    assert cp.returncode == 0, cp.stdout + cp.stderr
    reads = _bam_reads(g, go, 200, seed=44)
    bam, fq = tmp / "reads.bam", tmp / "reads.fq"
    bw.write_bam(bam, reads, block=4000, spare=0xF)
    bw.write_fastq(fq, reads)
    budget = next((m for m in range(1, 64) if (plan_of(idx, m << 20) or 0) >= 3), None)
    assert budget is not None
    plain = tmp / "fastq.tsv"
    cp = run(["search", "--index-file", idx, "--query-file", fq, "--output-file", plain, "--threads", "4"])
    assert cp.returncode == 0, cp.stdout + cp.stderr
    assert plain.read_bytes().count(b"\n") > 100
    return dict(tmp=tmp, idx=idx, bam=bam, fq=fq, plain=plain, budget=budget, passes=plan_of(idx, budget << 20))


@pytest.mark.parametrize("name,extra", [("one_device", []), ("two_workers", ["--gpu-list", "0,0", "--batch-reads", "25"]), ("paged", None)])
def test_cli_tsv_from_bam_equals_tsv_from_fastq(world, name, extra):
    w = world
    if extra is None:
        extra = ["--device-index-budget", w["budget"], "--batch-reads", "64"]
    out = w["tmp"] / f"{name}.tsv"
    cp = run(["search", "--index-file", w["idx"], "--query-file", w["bam"], "--output-file", out, "--threads", "4", "--device-parse"] + extra,
             env=dict(os.environ, TAXOR_TUNING="1", TAXOR_CLI_TRACE="1"))
    assert cp.returncode == 0, cp.stdout + cp.stderr
    assert out.read_bytes() == w["plain"].read_bytes()
    assert cp.stderr.count("is BAM: the switch is ignored") == 1 and "it is parsed on the host" not in cp.stderr    # the one-line notice
    assert "13 skipped as secondary or supplementary" in cp.stderr
    if name == "paged":
        assert f"searched in {w['passes']} resident passes" in cp.stderr and w["passes"] >= 3


def test_cli_mixed_query_files(world):
    w = world
    out = w["tmp"] / "mixed.tsv"
    cp = run(["search", "--index-file", w["idx"], "--query-file", f"{w['fq']},{w['bam']}", "--output-file", out, "--threads", "4"])
    assert cp.returncode == 0, cp.stdout + cp.stderr
    plain = w["plain"].read_bytes()
    head, body = plain.split(b"\n", 1)
    assert out.read_bytes() == head + b"\n" + body + body


def test_cli_search_to_profile_from_bam(world):
    w = world

    def prof(d, q):
        os.makedirs(str(d), exist_ok=True)
        cp = run(["search", "--index-file", w["idx"], "--query-file", q, "--threads", "4", "--cami-report-file", d / "cami", "--seq-abundance-file", d / "seq",
                  "--binning-file", d / "bin", "--sample-id", "S"])
        assert cp.returncode == 0, cp.stdout + cp.stderr
        return {k: (d / k).read_bytes() for k in ("cami", "seq", "bin")}

    a = prof(w["tmp"] / "prof_fq", w["fq"])
    b = prof(w["tmp"] / "prof_bam", w["bam"])
    assert a == b and len(a["bin"]) > 0
