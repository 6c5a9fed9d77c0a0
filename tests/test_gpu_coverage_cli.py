"""`taxor search --coverage-file`: the file's bytes equal the text formatted from the CPU expectation (tests/coverage_expect.py; the
integer column through taxor_hll_estimate on the expected registers), READS and HASH_MATCHES are the sums over the TSV's lines, and
the TSV is the one the run without the option writes."""
import gzip
import os
import subprocess

import numpy as np
import pytest

from taxor_amd import synth
from taxor_amd.search import hll_estimate
from tests import bam_writer as bw
from tests.coverage_expect import Expect
from tests.test_gpu_cli import _setup

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TAXOR = os.path.join(ROOT, "taxor_amd", "taxor")
COLUMNS = "#ACCESSION\tREFERENCE_NAME\tTAXID\tREF_LEN\tREADS\tHASH_MATCHES\tDISTINCT_HASHES\tDUPLICITY\n"


def _format(e, sp, p=12):
    by_bin = {}
    for s in sp:
        by_bin.setdefault(s["user_bin"], s)
    reg = e.registers(p)
    out = COLUMNS
    for b in range(e.n_bins):
        if not e.reads[b]:
            continue
        hm = int(e.hash_matches[b])
        d = int(np.floor(hll_estimate(reg[b], p) + 0.5))
        if hm and d < 1:
            d = 1
        s = by_bin.get(b, sp[0])
        out += "\t".join([s["accession_id"], s["organism_name"], s["taxid"], str(s["seq_len"]), str(int(e.reads[b])), str(hm), str(d),
                          "%.2f" % (hm / d if d else 0.0)]) + "\n"
    return out


def _search(index, queries, out, cov=None, extra=()):
    cmd = [TAXOR, "search", "--index-file", str(index), "--query-file", ",".join(str(q) for q in queries), "--output-file", str(out), "--threads", "4",
           "--batch-reads", "40"] + (["--coverage-file", str(cov)] if cov else []) + list(extra)
    cp = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert cp.returncode == 0, cp.stderr
    return cp


def _fasta(path, ids, reads):
    with open(path, "wb") as f:
        for rid, r in zip(ids, reads):
            f.write(b">" + rid + b"\n" + r + b"\n")


def test_coverage_file(tmp_path):
    g, go, host, sp, index = _setup(tmp_path, 52)
    bases, offs, origin = synth.synth_reads(g, go, 200, 1200, error_rate=0.02, frac_random=0.2, seed=9)
    reads = [bytes(bases[int(offs[i]):int(offs[i + 1])]) for i in range(200)]
    hot = int(np.argmax(origin >= 0))                                             # a read that comes from a genome of the index
    reads += reads[:60] + reads[:60] + [reads[hot]] * 30 + [b"ACGTACGT"]          # duplicates, and a read without a hash
    ids = [b"r%d" % i for i in range(len(reads))]
    e = Expect(host)
    e.add_bases(reads)
    want = _format(e, sp)
    assert want.count("\n") > 8

    fa = tmp_path / "reads.fa"
    _fasta(fa, ids, reads)
    tsv, cov, plain = tmp_path / "out.tsv", tmp_path / "cov.tsv", tmp_path / "plain.tsv"
    cp = _search(index, [fa], tsv, cov, extra=["--coverage-precision", "12"])
    assert open(cov).read() == want
    _search(index, [fa], plain)
    assert open(tsv, "rb").read() == open(plain, "rb").read()                     # the TSV does not know about the option

    # READS and HASH_MATCHES are the TSV's lines counted and their QHASH_MATCH summed, per accession
    n_lines, summed = {}, {}
    for line in open(tsv).read().splitlines()[1:]:
        f = line.split("\t")
        if f[1] != "-":
            n_lines[f[1]] = n_lines.get(f[1], 0) + 1
            summed[f[1]] = summed.get(f[1], 0) + int(f[7])
    rows = [l.split("\t") for l in open(cov).read().splitlines()[1:]]
    assert {r[0]: int(r[4]) for r in rows} == n_lines and {r[0]: int(r[5]) for r in rows} == summed
    # the thirty copies of one read raise its reference's duplicity, not its distinct count
    deep = max(rows, key=lambda r: float(r[7]))
    assert float(deep[7]) > 5 and int(deep[6]) < int(deep[5])

    # two query files equal their concatenation
    fa1, fa2, cov2 = tmp_path / "a.fa", tmp_path / "b.fa", tmp_path / "cov2.tsv"
    _fasta(fa1, ids[:130], reads[:130])
    _fasta(fa2, ids[130:], reads[130:])
    _search(index, [fa1, fa2], tmp_path / "out2.tsv", cov2)
    assert open(cov2).read() == want
    assert open(tmp_path / "out2.tsv", "rb").read() == open(plain, "rb").read()

    # other precisions, and the device's record scanner
    cov4 = tmp_path / "cov4.tsv"
    _search(index, [fa], tmp_path / "out4.tsv", cov4, extra=["--coverage-precision", "4", "--device-parse"])
    assert open(cov4).read() == _format(e, sp, 4)

    # the same reads as .fastq.gz and as BAM
    fq = tmp_path / "reads.fastq.gz"
    with gzip.open(fq, "wb") as f:
        for rid, r in zip(ids, reads):
            f.write(b"@" + rid + b"\n" + r + b"\n+\n" + b"I" * len(r) + b"\n")
    bam = tmp_path / "reads.bam"
    bw.write_bam(bam, [(rid, bw.codes_of_ascii(r), 4) for rid, r in zip(ids, reads)], block=30000)
    for q in (fq, bam):
        c = tmp_path / ("cov_" + q.name + ".tsv")
        _search(index, [q], tmp_path / "out_q.tsv", c)
        assert open(c).read() == want, q.name
        assert open(tmp_path / "out_q.tsv", "rb").read() == open(plain, "rb").read()
