"""`taxor search --segments-file`: the file's bytes equal the text formatted from the restatement (tests/segments_expect.py, fed from the
oracle's search of the same reads and its ordered hash lists) for every input kind, with and without a TSV, beside the other outputs;
the TSV, the breakpoint file and the call file do not know about the option."""
import gzip
import os
import subprocess

import pytest

from taxor_amd import synth
from taxor_amd.hixf_file import store_hixf
from tests import bam_writer as bw
from tests.segments_expect import COLUMNS, SgExpect
from tests.test_gpu_lca import make_world

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TAXOR = os.path.join(ROOT, "taxor_amd", "taxor")


def _search(index, queries, out=None, sg=None, extra=(), batch="30"):
    # --percentage 0.1: under the syncmer model's threshold, about half of a read's hashes, an insert of a fifth of the read is not reported
    cmd = [TAXOR, "search", "--index-file", str(index), "--query-file", ",".join(str(q) for q in queries), "--threads", "4", "--batch-reads", batch,
           "--percentage", "0.1"]
    cmd += (["--output-file", str(out)] if out else []) + (["--segments-file", str(sg)] if sg else []) + [str(x) for x in extra]
    cp = subprocess.run(cmd, capture_output=True, text=True, timeout=300, env=dict(os.environ, TAXOR_TUNING="1", TAXOR_CLI_TRACE="1"))
    assert cp.returncode == 0, cp.stderr
    return cp


def _fasta(path, ids, reads):
    with open(path, "wb") as f:
        for rid, r in zip(ids, reads):
            f.write(b">" + rid + b"\n" + r + b"\n")


@pytest.fixture(scope="module")
def setup(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("segments_cli")
    g, go, lay, host, sp = make_world(63)
    index = tmp / "idx.hixf"
    store_hixf(index, host, lay["n_user_bins"], sp)
    bases, offs, origin = synth.synth_reads(g, go, 100, 1200, error_rate=0.02, frac_random=0.2, seed=9)
    reads = [bytes(bases[int(offs[i]):int(offs[i + 1])]) for i in range(100)]
    G = [bytes(g[int(go[i]):int(go[i + 1])]) for i in range(len(go) - 1)]
    # a read without a hash in the middle; at the end a read across two strains of one species (genomes 0 and 2: whatever comes out), then
    # of unrelated genomes a chimera, a chimera of more than one piece, an insert and a three-way concatemer
    # (and in front of them an insert of 330 bases, some 28 hashes: it pays for two switches at cost 2, not at 16)
    reads = reads[:50] + [b"ACGTACGT"] + reads[50:] + [G[6][6000:6700] + G[3][500:830] + G[6][6700:7400], G[2][100:3000] + G[0][500:2000], G[3][1000:5000] + G[5][2000:6000], G[4] + G[6],
                                                       G[3][6000:10000] + G[5][8000:10000] + G[3][10000:14000], G[4][0:3000] + G[5][10000:13000] + G[6][2000:5000]]
    ids = [b"r%d some words" % i for i in range(len(reads))]
    fa = tmp / "reads.fa"
    _fasta(fa, ids, reads)
    e, e2 = SgExpect(host), SgExpect(host, L=2)
    e.add_bases(reads, percentage=0.1)
    e2.add_bases(reads, percentage=0.1)
    assert max(e.n_hashes) > 2048 and e.n_hashes[50] == 0
    lens = [len(r) for r in reads]
    names = [i.decode() for i in ids]
    text = lambda x=e, names=names: COLUMNS + x.text(sp, names, lens)
    n = len(reads)
    assert [e.reads[r]["n_segments"] for r in range(n - 4, n)] == [2, 2, 3, 3]
    assert [e.shape(r) for r in range(n - 4, n)] == ["split", "split", "insert", "mosaic"] and text(e2) != text()
    tsv, sg, plain = tmp / "out.tsv", tmp / "sg.tsv", tmp / "plain.tsv"
    cp = _search(index, [fa], tsv, sg)
    _search(index, [fa], plain)
    return dict(tmp=tmp, index=index, fa=fa, ids=ids, reads=reads, e=e, e2=e2, sp=sp, lens=lens, text=text, tsv=tsv, sg=sg, plain=plain, trace=cp.stderr)


def test_the_file_equals_the_expectation_and_the_tsv_is_unchanged(setup):
    s = setup
    got = open(s["sg"]).read()
    assert got == s["text"]()
    assert open(s["tsv"], "rb").read() == open(s["plain"], "rb").read()          # the TSV does not know about the option
    lines = [l.split("\t") for l in got.splitlines()[1:]]
    assert all(len(l) == 19 for l in lines) and "r50 some words" not in {l[0] for l in lines}
    n = len(s["reads"])
    ins = [l for l in lines if l[0] == "r%d some words" % (n - 2)]
    assert [l[5] for l in ins] == ["insert"] * 3 and [l[8] for l in ins] == ["0", "1", "2"] and ins[0][13] == ins[2][13] != ins[1][13]
    assert ins[0][9] == "0" and ins[2][10] == ins[0][2] and ins[2][12] == ins[0][1] and sum(int(l[15]) for l in ins) == int(ins[0][6])
    trace = [l for l in s["trace"].splitlines() if l.startswith("[trace] segments:")]
    rep = sum(1 for r in range(n) if s["e"].reported(r))
    assert len(trace) == 1 and f"{len(lines)} lines from {rep} reported reads of {sum(x['examined'] for x in s['e'].reads)} examined reads of {n};" in trace[0]


def test_without_a_tsv_the_cost_and_the_device_parser(setup):
    s = setup
    tmp = s["tmp"]
    _search(s["index"], [s["fa"]], None, tmp / "sg_only.tsv")
    assert open(tmp / "sg_only.tsv").read() == s["text"]()
    _search(s["index"], [s["fa"]], tmp / "out2.tsv", tmp / "sg2.tsv", extra=["--segments-switch-cost", "2", "--device-parse"])
    assert open(tmp / "sg2.tsv").read() == s["text"](s["e2"])
    assert open(tmp / "out2.tsv", "rb").read() == open(s["plain"], "rb").read()
    _search(s["index"], [s["fa"]], None, tmp / "sg_dp.tsv", extra=["--device-parse"], batch="1000")
    assert open(tmp / "sg_dp.tsv").read() == s["text"]()


def test_fastq_gz_and_bam(setup):
    s = setup
    tmp, ids, reads = s["tmp"], s["ids"], s["reads"]
    fq = tmp / "reads.fastq.gz"
    with gzip.open(fq, "wb") as f:
        for rid, r in zip(ids, reads):
            f.write(b"@" + rid + b"\n" + r + b"\n+\n" + b"I" * len(r) + b"\n")
    bam = tmp / "reads.bam"
    bw.write_bam(bam, [(rid.split(b" ")[0], bw.codes_of_ascii(r), 4) for rid, r in zip(ids, reads)], block=30000)
    _search(s["index"], [fq], tmp / "out_fq.tsv", tmp / "sg_fq.tsv")
    assert open(tmp / "sg_fq.tsv").read() == s["text"]()
    assert open(tmp / "out_fq.tsv", "rb").read() == open(s["plain"], "rb").read()
    _search(s["index"], [bam], None, tmp / "sg_bam.tsv")                          # a BAM read name has no description
    assert open(tmp / "sg_bam.tsv").read() == s["text"](s["e"], [i.split(b" ")[0].decode() for i in ids])


def test_beside_the_breakpoint_and_the_call_file(setup):
    s = setup
    tmp = s["tmp"]
    others = lambda k: ["--breakpoint-file", tmp / f"bp{k}.tsv", "--lca-file", tmp / f"lca{k}.tsv", "--coverage-file", tmp / f"cov{k}.tsv", "--hitmap-file", tmp / f"hm{k}.tsv"]
    _search(s["index"], [s["fa"]], tmp / "o1.tsv", None, extra=others(1))
    _search(s["index"], [s["fa"]], tmp / "o2.tsv", tmp / "sg2b.tsv", extra=others(2))
    assert open(tmp / "sg2b.tsv").read() == s["text"]()
    for a, b in (("bp1.tsv", "bp2.tsv"), ("lca1.tsv", "lca2.tsv"), ("cov1.tsv", "cov2.tsv"), ("hm1.tsv", "hm2.tsv"), ("o1.tsv", "o2.tsv")):
        assert open(tmp / a, "rb").read() == open(tmp / b, "rb").read(), a     # byte-identical with and without the option
    assert open(tmp / "o2.tsv", "rb").read() == open(s["plain"], "rb").read()
    assert open(tmp / "bp2.tsv").read().count("\n") > 3 and open(tmp / "lca2.tsv").read().count("\n") == 1 + len(s["reads"])
    # without a TSV, beside each of the two alone
    _search(s["index"], [s["fa"]], None, tmp / "sg3.tsv", extra=["--lca-file", tmp / "lca3.tsv"])
    _search(s["index"], [s["fa"]], None, tmp / "sg4.tsv", extra=["--breakpoint-file", tmp / "bp4.tsv"])
    assert open(tmp / "sg3.tsv").read() == s["text"]() == open(tmp / "sg4.tsv").read()
    assert open(tmp / "lca3.tsv", "rb").read() == open(tmp / "lca1.tsv", "rb").read() and open(tmp / "bp4.tsv", "rb").read() == open(tmp / "bp1.tsv", "rb").read()


def test_two_query_files_give_the_concatenation(setup):
    s = setup
    tmp, ids, reads = s["tmp"], s["ids"], s["reads"]
    fa1, fa2 = tmp / "a.fa", tmp / "b.fa"
    _fasta(fa1, ids[:60], reads[:60])
    _fasta(fa2, ids[60:], reads[60:])
    _search(s["index"], [fa1], None, tmp / "sg_a.tsv")
    _search(s["index"], [fa2], None, tmp / "sg_b.tsv")
    _search(s["index"], [fa1, fa2], tmp / "out_ab.tsv", tmp / "sg_ab.tsv")
    a, b = open(tmp / "sg_a.tsv").read(), open(tmp / "sg_b.tsv").read()
    assert a.startswith(COLUMNS) and b.startswith(COLUMNS)
    assert open(tmp / "sg_ab.tsv").read() == a + b[len(COLUMNS):] == s["text"]()
    assert open(tmp / "out_ab.tsv", "rb").read() == open(s["plain"], "rb").read()
