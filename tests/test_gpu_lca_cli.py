"""`taxor search --lca-file / --report-file`: both files equal, byte for byte, what tests/lca_expect.py makes of the TSV TEXT of the
same run; the TSV and the other outputs do not know about the options; every input kind gives the same bytes."""
import gzip
import os
import subprocess

import numpy as np
import pytest

from taxor_amd import synth
from taxor_amd.hixf_file import store_hixf
from tests import bam_writer as bw
from tests import lca_expect as le
from tests.test_gpu_lca import make_world

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TAXOR = os.path.join(ROOT, "taxor_amd", "taxor")


def _search(index, queries, out=None, lca=None, rep=None, extra=(), batch="40"):
    cmd = [TAXOR, "search", "--index-file", str(index), "--query-file", ",".join(str(q) for q in queries), "--threads", "4", "--batch-reads", batch]
    cmd += (["--output-file", str(out)] if out else []) + (["--lca-file", str(lca)] if lca else []) + (["--report-file", str(rep)] if rep else []) + list(extra)
    cp = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert cp.returncode == 0, cp.stderr
    return cp


def _fasta(path, ids, reads):
    with open(path, "wb") as f:
        for rid, r in zip(ids, reads):
            f.write(b">" + rid + b"\n" + r + b"\n")


@pytest.fixture(scope="module")
def setup(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("lca_cli")
    g, go, lay, host, sp = make_world(62)
    index = tmp / "idx.hixf"
    store_hixf(index, host, lay["n_user_bins"], sp)
    bases, offs, origin = synth.synth_reads(g, go, 200, 1200, error_rate=0.02, frac_random=0.2, seed=9)
    reads = [bytes(bases[int(offs[i]):int(offs[i + 1])]) for i in range(200)]
    reads += reads[:30] + [b"ACGTACGT", bytes(g[100:1500]), bytes(g[15000 + 200:15000 + 2500])]     # duplicates, a read without a hash, exact pieces of the two strains
    ids = [b"r%d some words" % i for i in range(len(reads))]
    fa = tmp / "reads.fa"
    _fasta(fa, ids, reads)
    lin = le.Lineage(sp, lay["n_user_bins"])
    # the run everything is compared with: all three files at once
    tsv, lca, rep = tmp / "out.tsv", tmp / "calls.tsv", tmp / "report.txt"
    env_cp = _search(index, [fa], tsv, lca, rep)
    want_calls, want_report = le.files_from_tsv(lin, open(tsv).read())
    return dict(tmp=tmp, index=index, fa=fa, ids=ids, reads=reads, lin=lin, sp=sp, tsv=tsv, lca=lca, rep=rep, calls=want_calls, report=want_report, cp=env_cp)


def test_both_files_equal_the_expectation_from_the_runs_own_tsv(setup):
    s = setup
    assert open(s["lca"]).read() == s["calls"]
    assert open(s["rep"]).read() == s["report"]
    lines = s["calls"].splitlines()
    assert lines[0] == le.CALL_HEADER.rstrip("\n") and len(lines) == 1 + len(s["reads"])
    hashless = [l for l in lines if l.split("\t")[1] == "r230 some words"]
    assert hashless == ["U\tr230 some words\t0\t8\t0\t0\t0"]                      # ACGTACGT: no hash, every reference with count 0 in the TSV, U here
    assert sum(1 for l in open(s["tsv"]) if l.startswith("r230 some words\t")) > 1
    taxa = {l.split("\t")[2] for l in lines[1:]}
    assert {"0", "562"} <= taxa and len(taxa) >= 5
    rep = s["report"].splitlines()
    assert rep[0].split("\t")[3:] == ["U", "0", "unclassified"] and rep[1].split("\t")[3:] == ["R", "1", "root"]
    assert any(l.endswith("\tS\t562\t" + " " * 14 + "Escherichia coli") for l in rep), s["report"]
    assert any(l.split("\t")[3] == "D" and l.split("\t")[5] == "  Bacteria" for l in rep)
    # the TSV does not know about the options
    plain = s["tmp"] / "plain.tsv"
    _search(s["index"], [s["fa"]], plain)
    assert open(plain, "rb").read() == open(s["tsv"], "rb").read()


def test_without_a_tsv_and_each_option_alone(setup):
    s = setup
    tmp = s["tmp"]
    _search(s["index"], [s["fa"]], None, tmp / "c1.tsv", tmp / "r1.txt")
    assert open(tmp / "c1.tsv").read() == s["calls"] and open(tmp / "r1.txt").read() == s["report"]
    _search(s["index"], [s["fa"]], None, tmp / "c2.tsv", None)
    assert open(tmp / "c2.tsv").read() == s["calls"]
    _search(s["index"], [s["fa"]], None, None, tmp / "r3.txt")
    assert open(tmp / "r3.txt").read() == s["report"]


def test_report_unit_bases(setup):
    s = setup
    tmp = s["tmp"]
    _search(s["index"], [s["fa"]], None, None, tmp / "rb.txt", extra=["--report-unit", "bases"])
    want = le.files_from_tsv(s["lin"], open(s["tsv"]).read(), unit="bases")[1]
    assert open(tmp / "rb.txt").read() == want and want != s["report"]
    _search(s["index"], [s["fa"]], None, None, tmp / "rr.txt", extra=["--report-unit", "reads"])
    assert open(tmp / "rr.txt").read() == s["report"]


def test_every_input_kind_gives_the_same_bytes(setup):
    s = setup
    tmp, ids, reads = s["tmp"], s["ids"], s["reads"]
    fq = tmp / "reads.fastq.gz"
    with gzip.open(fq, "wb") as f:
        for rid, r in zip(ids, reads):
            f.write(b"@" + rid + b"\n" + r + b"\n+\n" + b"I" * len(r) + b"\n")
    bam = tmp / "reads.bam"
    bw.write_bam(bam, [(rid.split(b" ")[0], bw.codes_of_ascii(r), 4) for rid, r in zip(ids, reads)], block=30000)
    bam_calls = s["calls"].replace(" some words\t", "\t")                          # a BAM read name carries no description
    for q, extra, calls in ((fq, [], s["calls"]), (bam, [], bam_calls), (s["fa"], ["--device-parse"], s["calls"])):
        c, r = tmp / "c_kind.tsv", tmp / "r_kind.txt"
        _search(s["index"], [q], None, c, r, extra=extra)
        assert open(c).read() == calls, (q.name, extra)
        assert open(r).read() == s["report"], (q.name, extra)
    # two query files equal their concatenation; --batch-reads 17 against 40
    fa1, fa2 = tmp / "a.fa", tmp / "b.fa"
    _fasta(fa1, ids[:130], reads[:130])
    _fasta(fa2, ids[130:], reads[130:])
    _search(s["index"], [fa1, fa2], tmp / "o2.tsv", tmp / "c2f.tsv", tmp / "r2f.txt")
    assert open(tmp / "c2f.tsv").read() == s["calls"] and open(tmp / "r2f.txt").read() == s["report"]
    assert open(tmp / "o2.tsv", "rb").read() == open(s["tsv"], "rb").read()
    _search(s["index"], [s["fa"]], None, tmp / "c17.tsv", tmp / "r17.txt", batch="17")
    assert open(tmp / "c17.tsv").read() == s["calls"] and open(tmp / "r17.txt").read() == s["report"]


def test_beside_the_coverage_file_and_the_profile_options(setup):
    s = setup
    tmp = s["tmp"]
    uniq = tmp / "uniq.fa"                                                        # the profile options want unique read ids (they cut at the first space)
    ids = [b"u%d" % i for i in range(len(s["reads"]))]
    _fasta(uniq, ids, s["reads"])
    prof = lambda d: ["--cami-report-file", str(tmp / d / "p.cami"), "--binning-file", str(tmp / d / "b.tsv"), "--sample-id", "s1"]
    for d in ("with", "without"):
        os.makedirs(tmp / d, exist_ok=True)
    _search(s["index"], [uniq], tmp / "with" / "o.tsv", tmp / "with" / "c.tsv", tmp / "with" / "r.txt",
            extra=["--coverage-file", str(tmp / "with" / "cov.tsv")] + prof("with"))
    _search(s["index"], [uniq], tmp / "without" / "o.tsv", None, None, extra=["--coverage-file", str(tmp / "without" / "cov.tsv")] + prof("without"))
    for f in ("o.tsv", "cov.tsv", "p.cami", "b.tsv"):
        assert open(tmp / "with" / f, "rb").read() == open(tmp / "without" / f, "rb").read(), f
    calls, report = le.files_from_tsv(s["lin"], open(tmp / "with" / "o.tsv").read())
    assert open(tmp / "with" / "c.tsv").read() == calls and open(tmp / "with" / "r.txt").read() == report == s["report"]


def test_an_empty_query_file_and_the_trace_line(setup):
    s = setup
    tmp = s["tmp"]
    empty = tmp / "empty.fa"
    empty.write_bytes(b"")
    _search(s["index"], [empty], None, tmp / "ce.tsv", tmp / "re.txt")
    assert open(tmp / "ce.tsv").read() == le.CALL_HEADER and open(tmp / "re.txt").read() == ""
    env = dict(os.environ, TAXOR_TUNING="1", TAXOR_CLI_TRACE="1")
    cp = subprocess.run([TAXOR, "search", "--index-file", str(s["index"]), "--query-file", str(s["fa"]), "--lca-file", str(tmp / "ct.tsv"), "--threads", "4"],
                        capture_output=True, text=True, timeout=300, env=env)
    assert cp.returncode == 0, cp.stderr
    assert f"[trace] lca: {len(s['lin'].ids)} nodes, {len(s['reads'])} reads called" in cp.stderr, cp.stderr
    assert open(tmp / "ct.tsv").read() == s["calls"]
