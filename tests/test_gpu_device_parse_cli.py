"""`taxor search --device-parse` end to end: the byte ranges of a plain query file go to the device as they are read, and the
command must write what it writes without the switch, byte for byte -- for multi-line FASTA, FASTQ and CRLF FASTQ cut into
several ranges (one run on two workers' devices), through the host fallback for a file the device reports irregular, with the
search-to-profile options, and for a .gz file, which ignores the switch with a notice.  A malformed file dies as without it."""
import gzip
import os
import re
import subprocess

import numpy as np
import pytest

from taxor_amd import synth

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TAXOR = os.path.join(ROOT, "taxor_amd", "taxor")
N_GENOMES, GENOME_LEN, N_READS = 12, 8000, 400


TRACE = re.compile(r"--device-parse: (\d+) ranges scanned on the device, (\d+) parsed on the host")


def run(args, timeout=300):
    env = dict(os.environ, TAXOR_TUNING="1", TAXOR_CLI_TRACE="1")      # the trace counts the ranges the device took
    return subprocess.run([TAXOR] + [str(a) for a in args], capture_output=True, text=True, timeout=timeout, env=env)


def ranges(cp):
    """(scanned on the device, parsed on the host) of a run with the switch"""
    m = TRACE.search(cp.stderr)
    assert m, cp.stderr
    return int(m.group(1)), int(m.group(2))


def fasta(reads, width=70, eol=b"\n"):
    return b"".join(b">" + i + eol + b"".join(s[a:a + width] + eol for a in range(0, len(s), width)) for i, s in reads)


def fastq(reads, eol=b"\n"):
    return b"".join(b"@" + i + eol + s + eol + b"+" + eol + (b"@" if j % 2 else b"+") + b"I" * (len(s) - 1) + eol
                    for j, (i, s) in enumerate(reads))


@pytest.fixture(scope="module")
def world(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("device_parse")
    g, go = synth.random_genomes(N_GENOMES, GENOME_LEN, seed=31)
    gdir = tmp / "genomes"
    gdir.mkdir()
    lines = []
    for i in range(N_GENOMES):
        acc = f"GCF_{900000 + (i * 7) % N_GENOMES:09d}.1"
        stem = f"{acc}_ASM{i}v1_genomic"
        (gdir / (stem + ".fna")).write_bytes(b">chr1\n" + bytes(g[int(go[i]):int(go[i + 1])]) + b"\n")
        names = f"k__Bacteria;p__P;c__C;o__O;f__F{i % 3};g__G{i};s__G{i} species{i}"
        ids = f"2;20;30;40;{500 + i % 3};{6000 + i};{70000 + i}"
        lines.append("\t".join([acc, str(70000 + i), f"ftp://host/genomes/{acc}/{stem}", f"G{i} species{i}", names, ids]))
    tax = tmp / "tax.tsv"
    tax.write_text("\n".join(lines) + "\n")
    idx = tmp / "idx.hixf"
    cp = run(["build", "--input-file", tax, "--input-sequence-dir", gdir, "--output-filename", idx, "--threads", "4", "--use-syncmer",
              "--kmer-size", "22", "--syncmer-size", "12"], timeout=600)
    assert cp.returncode == 0, cp.stdout + cp.stderr
    rng = np.random.default_rng(32)
    acgt = np.frombuffer(b"ACGT", np.uint8)
    reads = []
    for i in range(N_READS):
        n = int(rng.integers(300, 1500))
        if i % 17 == 0:
            seq = bytes(acgt[rng.integers(0, 4, n)])
        else:
            j = int(rng.integers(0, N_GENOMES))
            a = int(go[j]) + int(rng.integers(0, GENOME_LEN - n + 1))
            seq = bytes(g[a:a + n])
        reads.append((b"read_%d runid=ab%d ch=%d" % ((i * 7919) % N_READS, i, i % 512), seq))
    return dict(tmp=tmp, idx=idx, reads=reads)


def search(w, query, out, *extra):
    return run(["search", "--index-file", w["idx"], "--query-file", query, "--output-file", out, "--threads", "4", *extra])


def both(w, name, raw, *extra, batch_reads=64):
    """the TSV without and with the switch, and the switch's count of ranges"""
    q = w["tmp"] / name
    q.write_bytes(raw)
    outs = []
    for sw in ([], ["--device-parse"]):
        out = w["tmp"] / (name + (".dev.tsv" if sw else ".host.tsv"))
        cp = search(w, q, out, "--batch-reads", batch_reads, *extra, *sw)
        assert cp.returncode == 0, cp.stdout + cp.stderr
        assert "is compressed or read sequentially" not in cp.stderr  # a plain file: no notice
        outs.append(out.read_bytes())
    return outs + [ranges(cp)]


@pytest.mark.parametrize("name,extra", [("multi.fa", ()), ("reads.fq", ()), ("crlf.fq", ()), ("reads2.fq", ("--gpu-list", "0,0")),
                                        ("multi2.fa", ("--gpu-list", "0,0", "--gather", "none"))])
def test_same_tsv_with_and_without_the_switch(world, name, extra):
    reads = world["reads"]
    raw = fasta(reads) if name.endswith(".fa") else fastq(reads, eol=b"\r\n" if name.startswith("crlf") else b"\n")
    host, dev, (scanned, parsed) = both(world, name, raw, *extra)     # 400 reads, 64 per range: at least four ranges
    assert host == dev
    assert scanned >= 4 and parsed == 0                               # and the device took every one of them
    assert host.count(b"\n") > N_READS and b"GCF_" in host            # every read has a line, most are classified


def test_blank_line_between_fastq_records_goes_through_the_fallback(world):
    reads = world["reads"][:120]
    raw = fastq(reads[:50]) + b"\n" + fastq(reads[50:])
    host, dev, (scanned, parsed) = both(world, "blank.fq", raw, batch_reads=1000)
    assert host == dev and host.count(b"\n") > 120
    assert (scanned, parsed) == (0, 1)                                # one range, refused by the device, parsed by the host reader


def test_short_quality_line_dies_as_without_the_switch(world):
    reads = world["reads"][:40]
    raw = fastq(reads[:20]) + b"@bad\n" + reads[20][1] + b"\n+\n" + b"I" * (len(reads[20][1]) - 3) + b"\n" + fastq(reads[21:])
    q = world["tmp"] / "short.fq"
    q.write_bytes(raw)
    a = search(world, q, world["tmp"] / "short.host.tsv", "--batch-reads", 1000)
    b = search(world, q, world["tmp"] / "short.dev.tsv", "--batch-reads", 1000, "--device-parse")
    assert a.returncode == b.returncode != 0
    msg = [l for l in a.stderr.splitlines() if l.startswith("[TAXOR SEARCH ERROR]")]
    assert msg and "quality" in msg[0]
    assert msg == [l for l in b.stderr.splitlines() if l.startswith("[TAXOR SEARCH ERROR]")]


def test_search_to_profile_with_the_switch_writes_the_same_three_files(world):
    q = world["tmp"] / "prof.fa"
    q.write_bytes(fasta(world["reads"]))
    got = []
    for sw in ([], ["--device-parse"]):
        d = world["tmp"] / ("prof_dev" if sw else "prof_host")
        d.mkdir()
        cp = run(["search", "--index-file", world["idx"], "--query-file", q, "--threads", "4", "--batch-reads", "64", "--cami-report-file",
                  d / "cami", "--seq-abundance-file", d / "seq", "--binning-file", d / "bin", "--sample-id", "SAMPLE", *sw])
        assert cp.returncode == 0, cp.stdout + cp.stderr
        if sw:
            scanned, parsed = ranges(cp)
            assert scanned >= 4 and parsed == 0
        got.append({k: (d / k).read_bytes() for k in ("cami", "seq", "bin")})
    assert got[0] == got[1]
    assert got[0]["bin"].count(b"\n") > N_READS // 2


def test_gz_query_ignores_the_switch_with_a_notice(world):
    q = world["tmp"] / "reads.fq.gz"
    with gzip.open(q, "wb") as f:
        f.write(fastq(world["reads"]))
    a = search(world, q, world["tmp"] / "gz.host.tsv")
    b = search(world, q, world["tmp"] / "gz.dev.tsv", "--device-parse")
    assert a.returncode == 0 and b.returncode == 0, a.stderr + b.stderr
    assert "is compressed or read sequentially" not in a.stderr
    assert b.stderr.count("is compressed or read sequentially: it is parsed on the host") == 1
    assert ranges(b) == (0, 0)
    assert (world["tmp"] / "gz.host.tsv").read_bytes() == (world["tmp"] / "gz.dev.tsv").read_bytes()


def test_two_index_files_with_the_switch(world):
    """every query file against every index in turn: the chunk buffers of the first index are released page-unlocked, so the
    second index's buffers can be page-locked again (none is copied from pageable memory) and the output is the same"""
    q = world["tmp"] / "two.fq"
    q.write_bytes(fastq(world["reads"]))
    two = f"{world['idx']},{world['idx']}"
    outs = []
    for sw in ([], ["--device-parse"]):
        out = world["tmp"] / ("two.dev.tsv" if sw else "two.host.tsv")
        cp = run(["search", "--index-file", two, "--query-file", q, "--output-file", out, "--threads", "4", "--batch-reads", "64", *sw])
        assert cp.returncode == 0, cp.stdout + cp.stderr
        outs.append(out.read_bytes())
    assert outs[0] == outs[1] and outs[0].count(b"\n") > 2 * N_READS
    lines = re.findall(r"--device-parse: (\d+) ranges scanned on the device, (\d+) parsed on the host; (\d+) copied from pageable memory", cp.stderr)
    assert len(lines) == 2, cp.stderr                                 # one line per index
    for scanned, parsed, pageable in lines:
        assert int(scanned) >= 4 and int(parsed) == 0 and int(pageable) == 0
