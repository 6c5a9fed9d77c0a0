"""`taxor search --breakpoint-file`: the file's bytes equal the text formatted from the restatement (tests/breakpoint_expect.py, fed
from the oracle's search of the same reads and its ordered hash lists) for every input kind, with and without a TSV, beside the other
outputs; the TSV, the coverage file, the hit map and the call files do not know about the option."""
import gzip
import os
import subprocess

import pytest

from taxor_amd import synth
from taxor_amd.hixf_file import store_hixf
from tests import bam_writer as bw
from tests.breakpoint_expect import COLUMNS, BpExpect
from tests.test_gpu_lca import make_world

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TAXOR = os.path.join(ROOT, "taxor_amd", "taxor")


def _search(index, queries, out=None, bp=None, extra=(), batch="30"):
    # --percentage 0.3: under the syncmer model's threshold, about half of a read's hashes, a chimera reports only its larger half
    cmd = [TAXOR, "search", "--index-file", str(index), "--query-file", ",".join(str(q) for q in queries), "--threads", "4", "--batch-reads", batch,
           "--percentage", "0.3"]
    cmd += (["--output-file", str(out)] if out else []) + (["--breakpoint-file", str(bp)] if bp else []) + [str(x) for x in extra]
    cp = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert cp.returncode == 0, cp.stderr
    return cp


def _fasta(path, ids, reads):
    with open(path, "wb") as f:
        for rid, r in zip(ids, reads):
            f.write(b">" + rid + b"\n" + r + b"\n")


@pytest.fixture(scope="module")
def setup(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("breakpoint_cli")
    g, go, lay, host, sp = make_world(63)
    index = tmp / "idx.hixf"
    store_hixf(index, host, lay["n_user_bins"], sp)
    bases, offs, origin = synth.synth_reads(g, go, 100, 1200, error_rate=0.02, frac_random=0.2, seed=9)
    reads = [bytes(bases[int(offs[i]):int(offs[i + 1])]) for i in range(100)]
    G = [bytes(g[int(go[i]):int(go[i + 1])]) for i in range(len(go) - 1)]
    # a read without a hash in the middle, two chimeras of unrelated genomes (one of more than one piece), a short insert at the end
    reads = reads[:50] + [b"ACGTACGT"] + reads[50:] + [G[3][1000:5000] + G[5][2000:6000], G[4] + G[6], G[2][100:3000] + G[0][500:2000]]
    ids = [b"r%d some words" % i for i in range(len(reads))]
    fa = tmp / "reads.fa"
    _fasta(fa, ids, reads)
    e = BpExpect(host)
    e.add_bases(reads, percentage=0.3)
    assert max(e.n_hashes) > 2048 and e.n_hashes[50] == 0
    lens = [len(r) for r in reads]
    text = lambda G=1, names=None: COLUMNS + e.text(sp, names or [i.decode() for i in ids], lens, G)
    assert text().count("\n") >= 4 and text(5).count("\n") >= 4                    # the three chimeras are reported
    tsv, bp, plain = tmp / "out.tsv", tmp / "bp.tsv", tmp / "plain.tsv"
    _search(index, [fa], tsv, bp)
    _search(index, [fa], plain)
    return dict(tmp=tmp, index=index, fa=fa, ids=ids, reads=reads, e=e, sp=sp, lens=lens, text=text, tsv=tsv, bp=bp, plain=plain)


def test_the_file_equals_the_expectation_and_the_tsv_is_unchanged(setup):
    s = setup
    got = open(s["bp"]).read()
    assert got == s["text"]()
    assert open(s["tsv"], "rb").read() == open(s["plain"], "rb").read()          # the TSV does not know about the option
    lines = [l.split("\t") for l in got.splitlines()[1:]]
    tsv = [l.split("\t") for l in open(s["tsv"]).read().splitlines()[1:]]
    n = len(s["reads"])
    by_id = {l[0]: l for l in lines}
    for k in (n - 3, n - 2):                                                     # the chimeras of two unrelated genomes
        l = by_id["r%d some words" % k]
        assert len(l) == 18 and int(l[17]) > 100 and l[9] != l[13]           # a half of 4 kb holds some 350 hashes
        hashes, brk = int(l[2]), int(l[7])
        assert 0 < brk < hashes and int(l[8]) == brk * int(l[1]) // hashes
        assert int(l[11]) + int(l[15]) == int(l[6]) + int(l[17])                 # LEFT_HITS + RIGHT_HITS = BEST_LOCATED + GAIN
        # both halves' references are lines of the TSV's read only if they survive its filter; LEFT and RIGHT differ and GAIN is what a single one misses
        assert {t[1] for t in tsv if t[0] == l[0]} & {l[9], l[13]}
    assert all(int(l[17]) >= 1 for l in lines) and "r50 some words" not in by_id


def test_without_a_tsv_min_gain_and_the_device_parser(setup):
    s = setup
    tmp = s["tmp"]
    _search(s["index"], [s["fa"]], None, tmp / "bp_only.tsv")
    assert open(tmp / "bp_only.tsv").read() == s["text"]()
    _search(s["index"], [s["fa"]], tmp / "out5.tsv", tmp / "bp5.tsv", extra=["--breakpoint-min-gain", "5", "--device-parse"])
    assert open(tmp / "bp5.tsv").read() == s["text"](5)
    assert open(tmp / "out5.tsv", "rb").read() == open(s["plain"], "rb").read()
    _search(s["index"], [s["fa"]], None, tmp / "bp_dp.tsv", extra=["--device-parse"], batch="1000")
    assert open(tmp / "bp_dp.tsv").read() == s["text"]()


def test_fastq_gz_and_bam(setup):
    s = setup
    tmp, ids, reads = s["tmp"], s["ids"], s["reads"]
    fq = tmp / "reads.fastq.gz"
    with gzip.open(fq, "wb") as f:
        for rid, r in zip(ids, reads):
            f.write(b"@" + rid + b"\n" + r + b"\n+\n" + b"I" * len(r) + b"\n")
    bam = tmp / "reads.bam"
    bw.write_bam(bam, [(rid.split(b" ")[0], bw.codes_of_ascii(r), 4) for rid, r in zip(ids, reads)], block=30000)
    _search(s["index"], [fq], tmp / "out_fq.tsv", tmp / "bp_fq.tsv")
    assert open(tmp / "bp_fq.tsv").read() == s["text"]()
    assert open(tmp / "out_fq.tsv", "rb").read() == open(s["plain"], "rb").read()
    _search(s["index"], [bam], None, tmp / "bp_bam.tsv")                          # a BAM read name has no description
    assert open(tmp / "bp_bam.tsv").read() == s["text"](1, [i.split(b" ")[0].decode() for i in ids])


def test_beside_the_other_outputs(setup):
    s = setup
    tmp = s["tmp"]
    others = lambda k: ["--coverage-file", tmp / f"cov{k}.tsv", "--hitmap-file", tmp / f"hm{k}.tsv", "--lca-file", tmp / f"lca{k}.tsv", "--report-file", tmp / f"rep{k}.txt",
                        "--lca-confidence", "0.1"]
    _search(s["index"], [s["fa"]], tmp / "o1.tsv", None, extra=others(1))
    _search(s["index"], [s["fa"]], tmp / "o2.tsv", tmp / "bp2.tsv", extra=others(2))
    assert open(tmp / "bp2.tsv").read() == s["text"]()
    for a, b in (("cov1.tsv", "cov2.tsv"), ("hm1.tsv", "hm2.tsv"), ("lca1.tsv", "lca2.tsv"), ("rep1.txt", "rep2.txt"), ("o1.tsv", "o2.tsv")):
        assert open(tmp / a, "rb").read() == open(tmp / b, "rb").read(), a
    assert open(tmp / "o2.tsv", "rb").read() == open(s["plain"], "rb").read()
    assert open(tmp / "hm2.tsv").read().count("\n") > 3 and open(tmp / "lca2.tsv").read().count("\n") == 1 + len(s["reads"])
    # without a TSV, beside the plain call file alone
    _search(s["index"], [s["fa"]], None, tmp / "bp3.tsv", extra=["--lca-file", tmp / "lca3.tsv"])
    _search(s["index"], [s["fa"]], None, None, extra=["--lca-file", tmp / "lca4.tsv"])
    assert open(tmp / "bp3.tsv").read() == s["text"]() and open(tmp / "lca3.tsv", "rb").read() == open(tmp / "lca4.tsv", "rb").read()


def test_two_query_files_give_the_concatenation(setup):
    s = setup
    tmp, ids, reads = s["tmp"], s["ids"], s["reads"]
    fa1, fa2 = tmp / "a.fa", tmp / "b.fa"
    _fasta(fa1, ids[:60], reads[:60])
    _fasta(fa2, ids[60:], reads[60:])
    _search(s["index"], [fa1], None, tmp / "bp_a.tsv")
    _search(s["index"], [fa2], None, tmp / "bp_b.tsv")
    _search(s["index"], [fa1, fa2], tmp / "out_ab.tsv", tmp / "bp_ab.tsv")
    a, b = open(tmp / "bp_a.tsv").read(), open(tmp / "bp_b.tsv").read()
    assert a.startswith(COLUMNS) and b.startswith(COLUMNS)
    assert open(tmp / "bp_ab.tsv").read() == a + b[len(COLUMNS):] == s["text"]()
    assert open(tmp / "out_ab.tsv", "rb").read() == open(s["plain"], "rb").read()
