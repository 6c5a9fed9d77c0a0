"""Record scanning on the device (taxor_amd/csrc/fastx_scan.hip) through Searcher.search_fastx: for raw FASTA / FASTQ bytes the
results, ids and read lengths must equal, element for element, what search_batch returns for the bases and offsets the host
reader produces from the same bytes.  The host reader is driven as in test_fastx_reader_cpu.py: `taxor reads` prints id, length
and FNV-1a of every record it parses (range mode), which pins the plain-Python restatement below that supplies the bases.
Buffers are about three scan tiles (4096 bytes each) plus a partial one."""
import os
import subprocess

import numpy as np
import pytest

from taxor_amd import GpuIndex, Searcher, synth
from taxor_amd import _lib
from taxor_amd._lib import TaxorError

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "taxor_amd", "taxor")
TILE = 4096


def fnv1a(b: bytes) -> int:
    h = 1469598103934665603
    for c in b:
        h = ((h ^ c) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
    return h


def split_lines(raw: bytes):
    """lines without their terminator: '\\n' or the end of the buffer, and exactly one '\\r' before it"""
    out = []
    parts = raw.split(b"\n")
    if parts and parts[-1] == b"":
        parts.pop()
    for p in parts:
        out.append(p[:-1] if p.endswith(b"\r") else p)
    return out


def parse(raw: bytes, kind: str):
    """[(id, sequence)] by the grammar of fastx::FastxReader::next in range mode, for regular input"""
    lines = split_lines(raw)
    recs = []
    if kind == ">":
        for l in lines:
            if l.startswith(b">"):
                recs.append([l[1:], b""])
            elif recs:
                recs[-1][1] += l
            else:
                assert l == b""
        return [(i, s) for i, s in recs]
    while lines and lines[0] == b"":
        lines.pop(0)
    while lines and lines[-1] == b"":
        lines.pop()
    while len(lines) % 4:
        lines.append(b"")
    for a in range(0, len(lines), 4):
        assert lines[a].startswith(b"@") and lines[a + 2].startswith(b"+") and len(lines[a + 1]) == len(lines[a + 3])
        recs.append((lines[a][1:], lines[a + 1]))
    return recs


def host_reader(path):
    cp = subprocess.run([EXE, "reads", "--query-file", str(path), "--threads", "1"], capture_output=True)
    assert cp.returncode == 0, cp.stderr
    rows = [l.split(b"\t") for l in cp.stdout.split(b"\n") if l]
    return [(r[0], int(r[1]), int(r[2], 16)) for r in rows]


@pytest.fixture(scope="module")
def world():
    g, go = synth.random_genomes(6, 20000, seed=1)
    bins = 64
    dummy = GpuIndex([dict(bins=bins, stride=64, seg_len=16, seed=1, next_ixf=np.zeros(bins, np.int64),
                           fname_idx=np.arange(bins), data=np.zeros(3 * 16 * 64, np.uint8))], bins)
    hs = Searcher(dummy, ratio=0.5)
    hoff, hashes = hs.seq_to_syncmers(g, go)
    planted = [hashes[int(hoff[i]):int(hoff[i + 1])] for i in range(6)]
    hs.close()
    dummy.close()
    lay = synth.make_layout(planted, root_bins=64, child_bins=32, n_children=3, seed=2)
    host = synth.materialize_host(lay)
    idx = GpuIndex(host, lay["n_user_bins"])
    sr = Searcher(idx)
    sr.host_index = (host, lay["n_user_bins"])
    yield sr, bytes(np.asarray(g, dtype=np.uint8))
    sr.close()
    idx.close()


def pieces(genome: bytes, rng, total, lo, hi):
    """reads cut from the genomes, `total` bases in all"""
    out, have = [], 0
    while have < total:
        n = min(int(rng.integers(lo, hi)), total - have)
        a = int(rng.integers(0, len(genome) - n))
        out.append(genome[a:a + n])
        have += n
    return out


def fasta(recs, width=60, eol=b"\n", final_eol=True):
    out = []
    for i, s in recs:
        out.append(b">" + i + eol)
        w = width if width else max(1, len(s))
        out += [s[a:a + w] + eol for a in range(0, len(s), w)]
    raw = b"".join(out)
    return raw if final_eol else raw[:-len(eol)]


def fastq(recs, eol=b"\n", final_eol=True, qual=None, plus=None):
    out = []
    for j, (i, s) in enumerate(recs):
        q = (qual(j, len(s)) if qual else b"I" * len(s))
        out.append(b"@" + i + eol + s + eol + b"+" + (plus(j, i) if plus else b"") + eol + q + eol)
    raw = b"".join(out)
    return raw if final_eol else raw[:-len(eol)]


def ids(n, tag=b"read"):
    return [tag + b"_%d some description/%d" % (i, i % 7) for i in range(n)]


def make_cases(genome):
    rng = np.random.default_rng(11)
    size = 3 * TILE + 1500
    cases = []

    def add(name, kind, raw):
        cases.append((name, kind, raw))

    for w in (1, 15, 16, 17, 60, 63, 64, 65):
        total = (size - 1200) // 2 if w == 1 else size - 1200      # one base per line: two bytes of file per base
        rs = pieces(genome, rng, total, 40, 400)
        add(f"fasta_width_{w}", ">", fasta(list(zip(ids(len(rs)), rs)), width=w))
    rs = [genome[100:9100]] + pieces(genome, rng, 3000, 100, 300)
    add("fasta_long_read", ">", fasta(list(zip(ids(len(rs)), rs)), width=60))
    # '>' of the second record on the last byte of the first tile, the third record's header across the second tile boundary
    a_id, b_id, c_id = b"A", b"B tile edge", b"C header that straddles the tile boundary"
    a = b">" + a_id + b"\n"
    a_seq = genome[500:500 + TILE - 1 - len(a) - 1]
    first = a + a_seq + b"\n"
    assert len(first) == TILE - 1
    b = b">" + b_id + b"\n"
    b_seq = genome[7000:7000 + (2 * TILE - 7) - len(first) - len(b) - 1]
    second = b + b_seq + b"\n"
    assert len(first) + len(second) == 2 * TILE - 7
    third = b">" + c_id + b"\n" + genome[12000:12000 + 2000] + b"\n"
    raw = first + second + third
    assert raw[TILE - 1:TILE] == b">" and raw[2 * TILE - 7:2 * TILE - 6] == b">"
    add("fasta_record_on_tile_edge", ">", raw)

    rs = pieces(genome, rng, size // 2 - 600, 60, 300)
    qchars = np.frombuffer(b"@+!I5>#", np.uint8)
    qrng = np.random.default_rng(12)

    def qual(j, n):
        q = bytes(qrng.choice(qchars, size=n))
        return (b"@" if j % 2 else b"+") + q[1:] if n else q
    hdr = [b"r%d >x @y +z  two  spaces" % j for j in range(len(rs))]
    add("fastq_edges", "@", fastq(list(zip(hdr, rs)), qual=qual, plus=lambda j, i: i if j % 3 == 0 else b""))
    add("fastq_crlf", "@", fastq(list(zip(hdr, rs)), eol=b"\r\n", qual=qual))
    fr = pieces(genome, rng, size - 1500, 40, 400)
    add("fasta_crlf", ">", fasta(list(zip(ids(len(fr)), fr)), width=61, eol=b"\r\n"))
    add("fastq_no_final_newline", "@", fastq(list(zip(hdr, rs)), final_eol=False))
    add("fasta_no_final_newline", ">", fasta(list(zip(ids(len(fr)), fr)), final_eol=False))
    add("fastq_last_line_lone_cr", "@", fastq(list(zip(hdr, rs)), final_eol=False) + b"\r")
    add("fasta_last_line_lone_cr", ">", fasta(list(zip(ids(len(fr)), fr)), final_eol=False) + b"\r")
    some = list(zip(ids(8), pieces(genome, rng, 1600, 150, 250)))
    add("fasta_empty_reads_and_blank_lines", ">",
        b"\n\r\n\n" + b">empty first\n" + fasta(some[:4]) + b">e1\n>e2\n\n" + fasta(some[4:]) + b">empty last\n\n\n")
    add("fastq_empty_reads_and_blank_lines", "@",
        b"\n\n" + fastq(some[:4]) + b"@e1\n\n+\n\n" + fastq(some[4:]) + b"@e2 last\n\n+\n\n\n\n")
    add("fastq_empty_last_record_unterminated", "@", fastq(some[:2]) + b"@e\n\n+")
    low = [bytes(rng.choice(np.frombuffer(b"ACGTacgtNnRYKMSWBDHVUurykmswbdhv", np.uint8), size=200)) for _ in range(6)]
    add("fasta_iupac_lower", ">", fasta(list(zip(ids(6), low)), width=70))
    add("fastq_iupac_lower", "@", fastq(list(zip(ids(6), low))))
    add("fasta_one_read", ">", fasta([(b"only", genome[300:900])]))
    add("fastq_one_read", "@", fastq([(b"only", genome[300:900])]))
    add("fasta_one_read_shorter_than_k", ">", b">short\nACGTACGTAC\n")
    add("fastq_one_read_shorter_than_k", "@", b"@short\nACGTACGTAC\n+\nIIIIIIIIII\n")
    ones = [(b"%d" % i, b"ACGT"[i % 4:i % 4 + 1]) for i in range(1025)]
    add("fasta_1025_reads_of_one_base", ">", fasta(ones))
    add("fastq_1025_reads_of_one_base", "@", fastq(ones))
    return cases


def _genome_bytes():
    g, _ = synth.random_genomes(6, 20000, seed=1)
    return bytes(np.asarray(g, dtype=np.uint8))


CASES = make_cases(_genome_bytes())


def cat(reads):
    bases = np.frombuffer(b"".join(reads), dtype=np.uint8) if reads else np.zeros(0, np.uint8)
    return bases, np.cumsum([0] + [len(r) for r in reads]).astype(np.uint64)


def assert_same(got, want_res, recs):
    assert got.status == 0
    assert got.ids == [i for i, _ in recs]
    assert got.read_len.tolist() == [len(s) for _, s in recs]
    for f in ("read_off", "user_bin", "count", "n_hashes"):
        assert np.array_equal(getattr(got.results, f), getattr(want_res, f)), f


@pytest.mark.parametrize("name,kind,raw", CASES, ids=[c[0] for c in CASES])
def test_device_scan_equals_host_reader(world, tmp_path, name, kind, raw):
    sr, _ = world
    recs = parse(raw, kind)
    p = tmp_path / ("q.fa" if kind == ">" else "q.fq")
    p.write_bytes(raw)
    assert host_reader(p) == [(i, len(s), fnv1a(s)) for i, s in recs]      # the restatement is the host reader's parse
    want = sr.search_batch(*cat([s for _, s in recs]))
    got = sr.search_fastx(raw, kind)
    assert_same(got, want, recs)
    if not any(w in name for w in ("one_base", "shorter", "iupac")):
        assert want.user_bin.size > 0                                      # the reads do hit the index


def test_byte_outside_dna15_is_the_same_error(world):
    sr, genome = world
    seq = genome[100:300] + b"#" + genome[300:400]
    with pytest.raises(TaxorError) as e0:
        sr.search_batch(*cat([genome[0:100], seq]))
    for kind, raw in ((">", fasta([(b"a", genome[0:100]), (b"b", seq)])), ("@", fastq([(b"a", genome[0:100]), (b"b", seq)])),
                      (">", b">a\nACGT\rACGT\n")):                          # a '\r' that ends no line is an ordinary byte
        with pytest.raises(TaxorError) as e1:
            sr.search_fastx(raw, kind)
        assert e1.value.code == e0.value.code == -3 and str(e1.value) == str(e0.value)
    reads = [genome[1000:1400]]
    assert_same(sr.search_fastx(fasta([(b"x", reads[0])]), ">"), sr.search_batch(*cat(reads)), [(b"x", reads[0])])


def _irregular(genome):
    r = [(b"a", genome[0:200]), (b"b", genome[500:700])]
    wrapped = b"@a\n" + genome[0:100] + b"\n" + genome[100:200] + b"\n+\n" + b"I" * 200 + b"\n" + fastq(r[1:])
    return [("blank_line_between_records", "@", fastq(r[:1]) + b"\n" + fastq(r[1:])),
            ("wrapped_sequence", "@", wrapped),
            ("length_mismatch", "@", fastq(r[:1]) + b"@b\n" + genome[500:700] + b"\n+\n" + b"I" * 199 + b"\n"),
            ("first_byte_not_record_fastq", "@", b"X" + fastq(r)),
            ("first_byte_not_record_fasta", ">", b"\nACGT\n" + fasta(r)),
            ("fasta_given_as_fastq", "@", fasta(r)),
            ("fastq_truncated", "@", fastq(r)[:-150])]


@pytest.mark.parametrize("which", range(7))
def test_irregular_input_raises_the_status_and_nothing_else(world, which):
    sr, genome = world
    name, kind, raw = _irregular(genome)[which]
    reads = [genome[2000:2500], genome[3000:3300]]
    before = sr.search_batch(*cat(reads))
    got = sr.search_fastx(raw, kind)
    assert got.status == _lib.FASTX_IRREGULAR and got.results is None and got.ids is None, name
    after = sr.search_batch(*cat(reads))                                   # the searcher is as usable as before
    for f in ("read_off", "user_bin", "count", "n_hashes"):
        assert np.array_equal(getattr(after, f), getattr(before, f)), f
    recs = [(b"p", reads[0]), (b"q", reads[1])]
    assert_same(sr.search_fastx(fastq(recs), "@"), before, recs)


def test_sub_batches_and_an_empty_buffer(world):
    """sub_batch_reads cuts the scanned batch exactly as it cuts any other; no bytes are no reads"""
    sr, genome = world
    rng = np.random.default_rng(5)
    rs = pieces(genome, rng, 12000, 100, 300)
    recs = list(zip(ids(len(rs)), rs))
    sub = Searcher(sr.index, sub_batch_reads=7)
    want = sr.search_batch(*cat(rs))
    assert_same(sub.search_fastx(fastq(recs), "@"), want, recs)
    assert_same(sub.search_fastx(fasta(recs, width=50), ">"), want, recs)
    for raw in (b"", b"\n\n"):
        for kind in ">@":
            got = sub.search_fastx(raw, kind)
            assert got.status == 0 and got.ids == [] and got.results.read_off.tolist() == [0]
    sub.close()


@pytest.mark.parametrize("window,model", [(22, _lib.THR_KMER), (30, _lib.THR_FRACMINHASH)])
def test_host_evaluated_threshold_models_and_sub_batch_bases(world, window, model):
    """an index without syncmers takes the k-mer (window == k) or the FracMinHash model, whose thresholds the host evaluates per
    sub-batch; sub_batch_bases cuts the scanned batch after a few reads.  Both go through what every batch goes through"""
    sr, genome = world
    host, n_user_bins = sr.host_index
    idx = GpuIndex(host, n_user_bins, k=22, use_syncmer=False, window_size=window)
    rng = np.random.default_rng(6)
    rs = pieces(genome, rng, 9000, 100, 300) + [b"ACGTACGT"]                # the last read is shorter than k
    recs = list(zip(ids(len(rs)), rs))
    for kw in (dict(), dict(sub_batch_bases=1000), dict(sub_batch_reads=5)):
        one = Searcher(idx, **kw)
        assert one.model == model
        want = one.search_batch(*cat(rs))
        assert_same(one.search_fastx(fastq(recs), "@"), want, recs)
        assert_same(one.search_fastx(fasta(recs, width=33), ">"), want, recs)
        one.close()
    idx.close()
