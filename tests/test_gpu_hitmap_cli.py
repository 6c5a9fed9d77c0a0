"""`taxor search --hitmap-file`: the file's bytes equal the text formatted from the CPU expectation (tests/hitmap_expect.py) for every
input kind, with and without a TSV, beside the other outputs; the TSV, the coverage file and the call file do not know about the option."""
import gzip
import os
import subprocess

import pytest

from taxor_amd import synth
from taxor_amd.hixf_file import store_hixf
from tests import bam_writer as bw
from tests.hitmap_expect import COLUMNS, HitExpect
from tests.test_gpu_lca import make_world

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TAXOR = os.path.join(ROOT, "taxor_amd", "taxor")


def _search(index, queries, out=None, hm=None, extra=(), batch="30"):
    # --percentage 0.3: under the syncmer model's threshold, about half of a read's hashes, a chimera reports only its larger half
    cmd = [TAXOR, "search", "--index-file", str(index), "--query-file", ",".join(str(q) for q in queries), "--threads", "4", "--batch-reads", batch,
           "--percentage", "0.3"]
    cmd += (["--output-file", str(out)] if out else []) + (["--hitmap-file", str(hm)] if hm else []) + [str(x) for x in extra]
    cp = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert cp.returncode == 0, cp.stderr
    return cp


def _fasta(path, ids, reads):
    with open(path, "wb") as f:
        for rid, r in zip(ids, reads):
            f.write(b">" + rid + b"\n" + r + b"\n")


@pytest.fixture(scope="module")
def setup(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("hitmap_cli")
    g, go, lay, host, sp = make_world(63)
    index = tmp / "idx.hixf"
    store_hixf(index, host, lay["n_user_bins"], sp)
    bases, offs, origin = synth.synth_reads(g, go, 100, 1200, error_rate=0.02, frac_random=0.2, seed=9)
    reads = [bytes(bases[int(offs[i]):int(offs[i + 1])]) for i in range(100)]
    G = [bytes(g[int(go[i]):int(go[i + 1])]) for i in range(len(go) - 1)]
    # a read without a hash in the middle, a chimera of two unrelated genomes, a read of more than one piece (2048 hashes)
    reads = reads[:50] + [b"ACGTACGT"] + reads[50:] + [G[3][1000:5000] + G[5][2000:6000], G[4] + G[6]]
    ids = [b"r%d some words" % i for i in range(len(reads))]
    fa = tmp / "reads.fa"
    _fasta(fa, ids, reads)
    e = HitExpect(host)
    e.add_bases(reads, percentage=0.3)
    assert max(e.n_hashes) > 2048 and e.n_hashes[50] == 0
    lens = [len(r) for r in reads]
    text = lambda S: COLUMNS + e.text(sp, [i.decode() for i in ids], lens, S)
    tsv, hm, plain = tmp / "out.tsv", tmp / "hm.tsv", tmp / "plain.tsv"
    _search(index, [fa], tsv, hm)
    _search(index, [fa], plain)
    return dict(tmp=tmp, index=index, fa=fa, ids=ids, reads=reads, e=e, sp=sp, lens=lens, text=text, tsv=tsv, hm=hm, plain=plain)


def test_the_file_equals_the_expectation_and_the_tsv_is_unchanged(setup):
    s = setup
    want = s["text"](16)
    got = open(s["hm"]).read()
    assert got == want
    assert open(s["tsv"], "rb").read() == open(s["plain"], "rb").read()          # the TSV does not know about the option
    lines = [l.split("\t") for l in got.splitlines()[1:]]
    # one line per line of the TSV that a read with hashes produced, in its order, with its numbers
    tsv = [l.split("\t") for l in open(s["tsv"]).read().splitlines()[1:]]
    mapped = [l for l in tsv if l[1] != "-" and l[6] != "0"]
    assert [(l[0], l[1], l[3], l[5], l[6], l[7]) for l in mapped] == [(l[0], l[1], l[2], l[3], l[4], l[5]) for l in lines]
    assert any(l[0] == "r50 some words" for l in tsv) and not any(l[0] == "r50 some words" for l in lines)
    for l in lines:
        sizes, hits = [int(x) for x in l[7].split(",")], [int(x) for x in l[8].split(",")]
        assert len(sizes) == 16 and len(hits) == 16 and sum(sizes) == int(l[4]) and sum(hits) == int(l[6])
        assert all(h <= z for h, z in zip(hits, sizes))
    # the chimera: two references, one in the low segments and one in the high ones
    chim = [l for l in lines if l[0] == "r%d some words" % (len(s["reads"]) - 2)]
    halves = sorted([int(x) for x in l[8].split(",")] for l in chim if int(l[6]) > 300)
    assert len(halves) >= 2
    lo = [h for h in halves if sum(h[:7]) > 10 * max(1, sum(h[9:]))]
    hi = [h for h in halves if sum(h[9:]) > 10 * max(1, sum(h[:7]))]
    assert lo and hi


def test_without_a_tsv_other_segment_counts_and_the_device_parser(setup):
    s = setup
    tmp = s["tmp"]
    _search(s["index"], [s["fa"]], None, tmp / "hm_only.tsv")
    assert open(tmp / "hm_only.tsv").read() == s["text"](16)
    _search(s["index"], [s["fa"]], tmp / "out4.tsv", tmp / "hm4.tsv", extra=["--hitmap-segments", "4", "--device-parse"])
    assert open(tmp / "hm4.tsv").read() == s["text"](4)
    assert open(tmp / "out4.tsv", "rb").read() == open(s["plain"], "rb").read()
    _search(s["index"], [s["fa"]], None, tmp / "hm64.tsv", extra=["--hitmap-segments", "64", "--device-parse"], batch="1000")
    assert open(tmp / "hm64.tsv").read() == s["text"](64)


def test_fastq_gz_and_bam(setup):
    s = setup
    tmp, ids, reads = s["tmp"], s["ids"], s["reads"]
    fq = tmp / "reads.fastq.gz"
    with gzip.open(fq, "wb") as f:
        for rid, r in zip(ids, reads):
            f.write(b"@" + rid + b"\n" + r + b"\n+\n" + b"I" * len(r) + b"\n")
    bam = tmp / "reads.bam"
    bw.write_bam(bam, [(rid.split(b" ")[0], bw.codes_of_ascii(r), 4) for rid, r in zip(ids, reads)], block=30000)
    _search(s["index"], [fq], tmp / "out_fq.tsv", tmp / "hm_fq.tsv")
    assert open(tmp / "hm_fq.tsv").read() == s["text"](16)
    assert open(tmp / "out_fq.tsv", "rb").read() == open(s["plain"], "rb").read()
    _search(s["index"], [bam], None, tmp / "hm_bam.tsv")                          # a BAM read name has no description
    assert open(tmp / "hm_bam.tsv").read() == COLUMNS + s["e"].text(s["sp"], [i.split(b" ")[0].decode() for i in ids], s["lens"], 16)


def test_beside_the_coverage_and_the_call_file(setup):
    s = setup
    tmp = s["tmp"]
    _search(s["index"], [s["fa"]], tmp / "o1.tsv", None, extra=["--coverage-file", tmp / "cov1.tsv", "--lca-file", tmp / "lca1.tsv", "--report-file", tmp / "rep1.txt"])
    _search(s["index"], [s["fa"]], tmp / "o2.tsv", tmp / "hm2.tsv", extra=["--coverage-file", tmp / "cov2.tsv", "--lca-file", tmp / "lca2.tsv", "--report-file", tmp / "rep2.txt"])
    assert open(tmp / "hm2.tsv").read() == s["text"](16)
    for a, b in (("cov1.tsv", "cov2.tsv"), ("lca1.tsv", "lca2.tsv"), ("rep1.txt", "rep2.txt"), ("o1.tsv", "o2.tsv")):
        assert open(tmp / a, "rb").read() == open(tmp / b, "rb").read(), a
    assert open(tmp / "o2.tsv", "rb").read() == open(s["plain"], "rb").read()
    assert open(tmp / "cov2.tsv").read().count("\n") > 3 and open(tmp / "lca2.tsv").read().count("\n") == 1 + len(s["reads"])
    # without a TSV, beside the call file alone
    _search(s["index"], [s["fa"]], None, tmp / "hm3.tsv", extra=["--lca-file", tmp / "lca3.tsv"])
    assert open(tmp / "hm3.tsv").read() == s["text"](16) and open(tmp / "lca3.tsv", "rb").read() == open(tmp / "lca1.tsv", "rb").read()


def test_two_query_files_give_the_concatenation(setup):
    s = setup
    tmp, ids, reads = s["tmp"], s["ids"], s["reads"]
    fa1, fa2 = tmp / "a.fa", tmp / "b.fa"
    _fasta(fa1, ids[:60], reads[:60])
    _fasta(fa2, ids[60:], reads[60:])
    _search(s["index"], [fa1], None, tmp / "hm_a.tsv")
    _search(s["index"], [fa2], None, tmp / "hm_b.tsv")
    _search(s["index"], [fa1, fa2], tmp / "out_ab.tsv", tmp / "hm_ab.tsv")
    a, b = open(tmp / "hm_a.tsv").read(), open(tmp / "hm_b.tsv").read()
    assert a.startswith(COLUMNS) and b.startswith(COLUMNS)
    assert open(tmp / "hm_ab.tsv").read() == a + b[len(COLUMNS):] == s["text"](16)
    assert open(tmp / "out_ab.tsv", "rb").read() == open(s["plain"], "rb").read()
