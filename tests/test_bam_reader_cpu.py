"""The host side of BAM input (taxor_amd/csrc/bam.h) through `taxor reads`, which prints every selected record's id, length and the
FNV-1a of the restored read: round trip over the length and flag edges, BGZF block shapes, batches, malformed files, refusals.
The files are written by tests/bam_writer.py; its decoding is the expected value."""
import os
import struct
import subprocess

import numpy as np
import pytest

from tests import bam_writer as bw
from tests.test_fastx_reader_cpu import fnv1a

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "taxor_amd", "taxor")

pytestmark = pytest.mark.skipif(not os.path.exists(EXE), reason="taxor executable not built")

LENGTHS = [0, 1, 2, 15, 16, 17, 4097]
FLAGS = [0, 4, 0x10, 0x100, 0x800]


def run_reads(path, *extra, ok=True):
    cp = subprocess.run([EXE, "reads", "--query-file", str(path), *extra], capture_output=True, text=True)
    if not ok:
        return cp
    assert cp.returncode == 0, cp.stderr
    rows = [l.split("\t") for l in cp.stdout.split("\n") if l]
    n_batches = int(cp.stderr.split(" batches")[0].split(", ")[-1])
    return [(r[0].encode(), int(r[1]), int(r[2], 16)) for r in rows], n_batches, cp.stderr


def expected(reads):
    return [(n, len(s), fnv1a(s)) for n, s in bw.selected(reads)]


def make_reads():
    """every length with every flag; the first sixteen bases of a read walk through all sixteen codes, the rest is random"""
    rng = np.random.default_rng(5)
    reads = []
    for L in LENGTHS:
        for f in FLAGS:
            codes = np.concatenate([(np.arange(16) + len(reads)) % 16, rng.integers(0, 16, max(0, L - 16))])[:L].astype(np.uint8)
            reads.append((b"read/%d_len%d_flag%d" % (len(reads), L, f), codes, f))
    return reads


EXTRAS = {3: dict(cigar=[(10, 0), (3, 1), (4, 4)], tags=b"NMC\x03RGZgrp1\x00"), 12: dict(tags=b"MMZC+m,1,2;\x00MLB C\x02\x00\x00\x00\x10\x20"),
          27: dict(cigar=[(4097, 0)])}


def test_round_trip_lengths_flags_codes_cigar_tags(tmp_path):
    reads = make_reads()
    p = tmp_path / "a.bam"
    bw.write_bam(p, reads, extras=EXTRAS, spare=0xF)
    got, _, err = run_reads(p)
    exp = expected(reads)
    assert len(exp) == len(LENGTHS) * 3            # flags 0x100 and 0x800 are absent
    assert got == exp
    assert set(b"".join(s for _, s in bw.selected(reads))) == set(bw.ALPHABET)
    assert "warning" not in err.lower()


@pytest.mark.parametrize("threads", [1, 4])
def test_block_shapes_threads_and_batches_give_the_same_records(tmp_path, threads):
    reads = make_reads()
    exp = expected(reads)
    outs = []
    for blocking, block in (("record", 0), ("bytes", 300), ("one", 0)):
        p = tmp_path / f"{blocking}.bam"
        bw.write_bam(p, reads, blocking=blocking, block=block, extras=EXTRAS)
        got, nb, _ = run_reads(p, "--threads", str(threads))
        assert got == exp, blocking
        assert nb == 1
        got3, nb3, _ = run_reads(p, "--threads", str(threads), "--batch-reads", "3")
        assert got3 == exp and nb3 == (len(exp) + 2) // 3, blocking
        gots, _, _ = run_reads(p, "--threads", str(threads), "--sequential", "--batch-reads", "3")
        assert gots == exp
        outs.append(got)
    assert outs[0] == outs[1] == outs[2]


def _two(bad):
    """a good record, then the bytes `bad`"""
    return bw.header() + bw.record(b"good", [1, 2, 4, 8], 4) + bad


def _patched(rec, at, fmt, value):
    b = bytearray(rec)
    struct.pack_into(fmt, b, at, value)
    return bytes(b)


REC = bw.record(b"bad_one", [1, 2, 4, 8, 15], 4, cigar=[(5, 0)], tags=b"NMC\x00")
NO_NUL = bytearray(REC)
NO_NUL[36 + 7] = ord("x")
MALFORMED = {
    "block_size": (_two(_patched(REC, 0, "<I", 32 + 8 + 4 + 3 + 5 - 1)), "record 2", "block_size"),
    "block_size_below_fixed": (_two(_patched(REC, 0, "<I", 31) + b"\0" * 40), "record 2", "block_size"),
    "l_read_name_0": (_two(_patched(REC, 12, "<B", 0)), "record 2", "l_read_name is 0"),
    "name_without_nul": (_two(bytes(NO_NUL)), "record 2", "not NUL-terminated"),
    "negative_l_seq": (_two(_patched(REC, 20, "<i", -5)), "record 2", "l_seq"),
    "huge_l_seq": (_two(_patched(REC, 20, "<I", 1 << 31)), "record 2", "l_seq"),
    "ends_in_record": (_two(REC[:50]), "record 2", "ends inside the record"),
    "ends_in_block_size": (_two(REC[:2]), "record 2", "ends inside the record"),
    "ends_in_header": (bw.header()[:9], "", "ends inside the header"),
    "ends_in_references": (bw.header(refs=[(b"chr1", 1000), (b"chr2", 500)])[:-6], "", "ends inside the header"),
}


@pytest.mark.parametrize("case", sorted(MALFORMED))
def test_malformed_input_is_fatal_and_names_the_record(tmp_path, case):
    stream, where, what = MALFORMED[case]
    p = tmp_path / "bad.bam"
    p.write_bytes(bw.bgzf(stream))
    cp = run_reads(p, ok=False)
    assert cp.returncode != 0
    assert "[TAXOR SEARCH ERROR]" in cp.stderr and what in cp.stderr and where in cp.stderr, cp.stderr


def test_wrong_magic_is_fatal(tmp_path):
    p = tmp_path / "v2.bam"
    p.write_bytes(bw.bgzf(b"BAM\2" + bw.header()[4:] + REC))
    cp = run_reads(p, ok=False)
    assert cp.returncode != 0 and "wrong magic" in cp.stderr, cp.stderr


def test_references_in_the_header_are_skipped(tmp_path):
    reads = make_reads()[:9]
    p = tmp_path / "refs.bam"
    bw.write_bam(p, reads, head=bw.header(text=b"@HD\tVN:1.6\n@SQ\tSN:chr1\tLN:1000\n" * 50, refs=[(b"chr1", 1000), (b"chr2", 500)]), block=211)
    got, _, _ = run_reads(p)
    assert got == expected(reads)


def test_missing_eof_block_warns_and_succeeds(tmp_path):
    reads = make_reads()
    p = tmp_path / "noeof.bam"
    bw.write_bam(p, reads, eof=False, block=300)
    got, _, err = run_reads(p, "--threads", "4")
    assert got == expected(reads)
    assert "WARNING" in err and "end-of-file block is missing" in err


def test_cram_and_sam_are_refused_by_name(tmp_path):
    cram = tmp_path / "x.cram"
    cram.write_bytes(b"CRAM\x03\x00" + b"\0" * 64)
    cp = run_reads(cram, ok=False)
    assert cp.returncode != 0 and "CRAM" in cp.stderr, cp.stderr
    sam = tmp_path / "x.sam"
    sam.write_bytes(b"@HD\tVN:1.6\tSO:unsorted\nr1\t4\t*\t0\t0\t*\t*\t0\t0\tACGT\tIIII\n")
    cp = run_reads(sam, ok=False)
    assert cp.returncode != 0 and "SAM" in cp.stderr, cp.stderr
    # the search refuses them as well, in its input checks: before any index or device is touched
    for q, word in ((cram, "CRAM"), (sam, "SAM")):
        cp = subprocess.run([EXE, "search", "--index-file", str(cram), "--query-file", str(q), "--output-file", str(tmp_path / "o.tsv")],
                            capture_output=True, text=True)
        assert cp.returncode != 0 and word in cp.stderr and "not supported" in cp.stderr, cp.stderr


def test_bgzf_that_is_not_bam_goes_to_the_fastx_reader(tmp_path):
    """bgzip's output of a FASTQ file carries the same 'BC' subfield; its content decides"""
    rng = np.random.default_rng(9)
    recs = [(b"r%d" % i, bytes(rng.choice(np.frombuffer(b"ACGT", np.uint8), size=int(rng.integers(1, 500))))) for i in range(300)]
    raw = b"".join(b"@" + n + b"\n" + s + b"\n+\n" + b"I" * len(s) + b"\n" for n, s in recs)
    p = tmp_path / "reads.fastq.gz"
    p.write_bytes(bw.bgzf(raw, block=4000))
    got, _, _ = run_reads(p, "--threads", "4")
    assert got == [(n, len(s), fnv1a(s)) for n, s in recs]
    # ... whatever the file is called
    q = tmp_path / "reads.bam"
    q.write_bytes(p.read_bytes())
    got, _, _ = run_reads(q)
    assert got == [(n, len(s), fnv1a(s)) for n, s in recs]
    # and a BAM file is BAM under any name
    reads = make_reads()
    b = tmp_path / "reads2.fastq.gz"
    bw.write_bam(b, reads)
    got, _, _ = run_reads(b)
    assert got == expected(reads)


def test_chunks_cut_by_size_hold_the_same_records(tmp_path):
    """without --batch-reads a BAM file is cut into chunks by bases (2^27 by default; --batch-bases lowers it here)"""
    reads = make_reads()
    p = tmp_path / "a.bam"
    bw.write_bam(p, reads, block=300)
    got, nb, _ = run_reads(p, "--batch-bases", "1000")
    assert got == expected(reads) and nb == 3          # a chunk closes with the record that takes it to 1000 bases: each of the three 4097s does
    got1, nb1, _ = run_reads(p)
    assert got1 == got and nb1 == 1


@pytest.mark.parametrize("kind", ["fastq", "fastq.gz"])
def test_a_query_from_a_pipe_is_read_as_before(tmp_path, kind):
    """content detection looks at regular files only: a FIFO's bytes all reach the sequential FASTX reader, and its writer is not
    cut off"""
    import gzip
    import threading
    rng = np.random.default_rng(11)
    recs = [(b"r%d" % i, bytes(rng.choice(np.frombuffer(b"ACGT", np.uint8), size=int(rng.integers(1, 900))))) for i in range(800)]
    raw = b"".join(b"@" + n + b"\n" + s + b"\n+\n" + b"I" * len(s) + b"\n" for n, s in recs)
    assert len(raw) > 300000              # more than a pipe holds, and more than a detector would read
    data = gzip.compress(raw, 1) if kind.endswith(".gz") else raw
    fifo = tmp_path / "q.fifo"
    os.mkfifo(fifo)
    err = []

    def feed():
        try:
            with open(fifo, "wb") as f:
                f.write(data)
        except OSError as e:               # BrokenPipeError: the reader closed the pipe before it had everything
            err.append(e)

    t = threading.Thread(target=feed)
    t.start()
    try:
        cp = subprocess.run([EXE, "reads", "--query-file", str(fifo)], capture_output=True, text=True, timeout=60)
    finally:
        if t.is_alive():                   # a reader that never opened the pipe: let the writer's open() return
            fd = os.open(fifo, os.O_RDONLY | os.O_NONBLOCK)
            t.join(5)
            os.close(fd)
        t.join(5)
    assert cp.returncode == 0, cp.stderr
    assert not err, err
    rows = [l.split("\t") for l in cp.stdout.split("\n") if l]
    assert [(r[0].encode(), int(r[1]), int(r[2], 16)) for r in rows] == [(n, len(s), fnv1a(s)) for n, s in recs]


def test_summary_only_counts_without_printing(tmp_path):
    reads = make_reads()
    p = tmp_path / "a.bam"
    bw.write_bam(p, reads, block=300)
    cp = run_reads(p, "--summary-only", ok=False)
    sel = bw.selected(reads)
    assert cp.returncode == 0 and cp.stdout == ""
    assert cp.stderr.startswith("%d reads, %d bases, 1 batches" % (len(sel), sum(len(s) for _, s in sel))), cp.stderr
