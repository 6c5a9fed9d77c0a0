"""`taxor search --exclusive-file` / `--exclusive-reads-file`: both files' bytes equal the text formatted from the restatement
(tests/exclusive_expect.py, fed from the oracle's search of the same reads and its ordered hash lists; DISTINCT_EXCLUSIVE through
taxor_hll_estimate on the expected registers) for an index of three close "strains", for every input kind, with and without a TSV, either
file alone; the TSV does not know about the options.  And the planted outcome: reads of one strain give exclusive hashes to that strain
alone, beyond what the oracle's own fingerprint collisions allow the others."""
import gzip
import os
import subprocess

import numpy as np
import pytest

from oracle import oracle as orc
from taxor_amd import synth
from taxor_amd.hixf_file import store_hixf
from taxor_amd.search import hll_estimate
from tests import bam_writer as bw
from tests.exclusive_expect import BIN_COLUMNS, READ_COLUMNS, ExExpect
from tests.test_hixf_file_cpu import make_species

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TAXOR = os.path.join(ROOT, "taxor_amd", "taxor")
SHARED, PRIVATE, SOURCE = 12000, 3000, 1


def _search(index, queries, out=None, ex=None, exr=None, extra=(), batch="30"):
    cmd = [TAXOR, "search", "--index-file", str(index), "--query-file", ",".join(str(q) for q in queries), "--threads", "4", "--batch-reads", batch,
           "--percentage", "0.3"]
    cmd += (["--output-file", str(out)] if out else []) + (["--exclusive-file", str(ex)] if ex else []) + (["--exclusive-reads-file", str(exr)] if exr else [])
    cp = subprocess.run(cmd + [str(x) for x in extra], capture_output=True, text=True, timeout=300)
    assert cp.returncode == 0, cp.stderr
    return cp


def _fasta(path, ids, reads):
    with open(path, "wb") as f:
        for rid, r in zip(ids, reads):
            f.write(b">" + rid + b"\n" + r + b"\n")


def _texts(host, sp, ids, reads, p=12):
    """(the --exclusive-file text, the --exclusive-reads-file text, the expectation) of one run over `reads`"""
    e = ExExpect(host)
    e.add_bases(reads, percentage=0.3)
    reg = e.registers(p)
    distinct = lambda b: max(int(np.floor(hll_estimate(reg[b], p) + 0.5)), 1) if e.exclusive_hits[b] else int(np.floor(hll_estimate(reg[b], p) + 0.5))
    return BIN_COLUMNS + e.bin_text(sp, distinct), READ_COLUMNS + e.read_text(sp, [i.decode() for i in ids], [len(r) for r in reads]), e


def cli_world():
    """the index and the reads; host work only"""
    # three strains: one shared sequence, a private stretch each; three unrelated genomes beside them
    g, _ = synth.random_genomes(1, SHARED + 3 * PRIVATE + 3 * 15000, seed=77)
    g = bytes(g)
    strains = [g[:SHARED] + g[SHARED + i * PRIVATE:SHARED + (i + 1) * PRIVATE] for i in range(3)]
    others = [g[SHARED + 3 * PRIVATE + i * 15000:SHARED + 3 * PRIVATE + (i + 1) * 15000] for i in range(3)]
    G = strains + others
    planted = [np.unique(orc.seq_to_syncmers(x)) for x in G]
    lay = synth.make_layout(planted, root_bins=68, child_bins=40, n_children=3, seed=77)
    host, sp = synth.materialize_host(lay), make_species(lay)
    ub = [int(x) for x in lay["planted_user_bin"]]
    src = strains[SOURCE]
    # error-free reads of the source strain: from the shared part, from its private part, spanning both
    planted_reads = [src[2000:4000], src[7000:9500], src[SHARED + 300:SHARED + 2300], src[SHARED + 900:SHARED + 2900], src[SHARED - 1500:SHARED + 1000],
                     src[SHARED - 600:SHARED + 2600]]
    go = np.cumsum([0] + [len(x) for x in G]).astype(np.uint64)
    bases, offs, _ = synth.synth_reads(np.frombuffer(b"".join(G), np.uint8), go, 60, 1200, error_rate=0.02, frac_random=0.2, seed=5)
    ordinary = [bytes(bases[int(offs[i]):int(offs[i + 1])]) for i in range(60)]
    reads = ordinary[:30] + [b"ACGTACGT"] + planted_reads + ordinary[30:] + [others[0] + others[1]]     # one without a hash; one of several pieces
    ids = [b"r%d some words" % i for i in range(len(reads))]
    return dict(lay=lay, host=host, sp=sp, ub=ub, planted=planted, planted_reads=planted_reads, reads=reads, ids=ids)


@pytest.fixture(scope="module")
def setup(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("exclusive_cli")
    w = cli_world()
    lay, host, sp, ub, planted, planted_reads, reads, ids = (w[k] for k in ("lay", "host", "sp", "ub", "planted", "planted_reads", "reads", "ids"))
    index = tmp / "idx.hixf"
    store_hixf(index, host, lay["n_user_bins"], sp)
    fa = tmp / "reads.fa"
    _fasta(fa, ids, reads)
    bins_text, reads_text, e = _texts(host, sp, ids, reads)
    assert max(e.n_hashes) > 2048 and e.n_hashes[30] == 0 and reads_text.count("\n") > 10 and bins_text.count("\n") > 6
    tsv, ex, exr, plain = tmp / "out.tsv", tmp / "ex.tsv", tmp / "exr.tsv", tmp / "plain.tsv"
    _search(index, [fa], tsv, ex, exr)
    _search(index, [fa], plain)
    return dict(tmp=tmp, index=index, fa=fa, ids=ids, reads=reads, host=host, sp=sp, ub=ub, planted=planted, planted_reads=planted_reads, bins_text=bins_text,
                reads_text=reads_text, e=e, tsv=tsv, ex=ex, exr=exr, plain=plain)


def test_both_files_equal_the_expectation_and_the_tsv_is_unchanged(setup):
    s = setup
    assert open(s["ex"]).read() == s["bins_text"]
    assert open(s["exr"]).read() == s["reads_text"]
    assert open(s["tsv"], "rb").read() == open(s["plain"], "rb").read()          # the TSV does not know about the options
    # the reads file holds the TSV's lines of the reads with two candidates or more, with the TSV's QHASH_MATCH
    tsv = {(l[0], l[1]): l for l in (x.split("\t") for x in open(s["tsv"]).read().splitlines()[1:])}
    lines = [l.split("\t") for l in open(s["exr"]).read().splitlines()[1:]]
    assert lines and all(len(l) == 11 and int(l[8]) >= 2 for l in lines)
    for l in lines:
        t = tsv[(l[0], l[1])]
        assert (t[3], t[5], t[6], t[7]) == (l[2], l[3], l[4], l[5])
        assert int(l[7]) <= int(l[6]) and int(l[10]) <= int(l[9]) <= int(l[4])
    assert "r30 some words" not in {l[0] for l in lines}


def test_the_source_strain_alone_has_exclusive_hashes(setup):
    """Reads of strain 1 without an error: every hash of theirs is a key of strain 1, which the filter answers yes for.  So while strain 1
    is a candidate, another strain cannot own a hash at all; where a short read missed strain 1's threshold it could, and only through
    a hash it does not hold but its filter answers yes for.  The allowance per other strain is the number of such answers the ORACLE
    gives over these reads -- an upper bound, counted from the oracle's matches and the planted key sets alone."""
    s = setup
    tmp, ub, cov = s["tmp"], s["ub"], s["e"].cov
    ids = [b"p%d" % i for i in range(len(s["planted_reads"]))]
    fa = tmp / "planted.fa"
    _fasta(fa, ids, s["planted_reads"])
    _search(s["index"], [fa], None, tmp / "ex_p.tsv", tmp / "exr_p.tsv")
    bins_text, reads_text, e = _texts(s["host"], s["sp"], ids, s["planted_reads"])
    assert open(tmp / "ex_p.tsv").read() == bins_text and open(tmp / "exr_p.tsv").read() == reads_text
    allowance = {}
    for k in (0, 2):
        allowance[k] = 0
        for r in s["planted_reads"]:
            h = orc.seq_to_syncmers(r)
            allowance[k] += int((cov.matches(ub[k], h) & ~np.isin(h, s["planted"][k])).sum())
    acc = {k: s["sp"][ub[k]]["accession_id"] for k in range(3)}
    rows = {l[0]: l for l in (x.split("\t") for x in open(tmp / "ex_p.tsv").read().splitlines()[1:])}
    private = sum(int((~np.isin(orc.seq_to_syncmers(r), s["planted"][0])).sum()) for r in s["planted_reads"])    # hashes the other strains do not hold
    assert private > 300 and max(allowance.values()) < private // 10, (private, allowance)
    assert all(acc[k] in rows for k in range(3))                                                   # the shared part makes all three candidates
    # a truly private hash is lost only to a collision in another candidate's leaf bins, 1/256 per bin: nine tenths stay by a wide margin
    assert int(rows[acc[SOURCE]][4]) >= private * 9 // 10 and int(rows[acc[SOURCE]][5]) >= 4 and int(rows[acc[SOURCE]][6]) >= 1
    for k in (0, 2):
        assert int(rows[acc[k]][4]) <= allowance[k], (k, rows[acc[k]], allowance)
        # the two reads of the shared part alone hold some 390 hashes (4500 bases, a hash per 11): hits by the hundred, hardly one its own
        assert int(rows[acc[k]][3]) > 300 and float(rows[acc[k]][7]) < 0.05


def test_either_file_alone_and_without_a_tsv(setup):
    s = setup
    tmp = s["tmp"]
    _search(s["index"], [s["fa"]], None, tmp / "ex_only.tsv")
    assert open(tmp / "ex_only.tsv").read() == s["bins_text"] and not (tmp / "exr_only.tsv").exists()
    _search(s["index"], [s["fa"]], None, None, tmp / "exr_only.tsv", extra=["--device-parse"], batch="1000")
    assert open(tmp / "exr_only.tsv").read() == s["reads_text"]
    _search(s["index"], [s["fa"]], tmp / "out_p.tsv", tmp / "ex_p5.tsv", extra=["--exclusive-precision", "5"])
    want, _, _ = _texts(s["host"], s["sp"], s["ids"], s["reads"], p=5)
    assert open(tmp / "ex_p5.tsv").read() == want
    assert open(tmp / "out_p.tsv", "rb").read() == open(s["plain"], "rb").read()


def test_fastq_gz_and_bam(setup):
    s = setup
    tmp, ids, reads = s["tmp"], s["ids"], s["reads"]
    fq = tmp / "reads.fastq.gz"
    with gzip.open(fq, "wb") as f:
        for rid, r in zip(ids, reads):
            f.write(b"@" + rid + b"\n" + r + b"\n+\n" + b"I" * len(r) + b"\n")
    bam = tmp / "reads.bam"
    bw.write_bam(bam, [(rid.split(b" ")[0], bw.codes_of_ascii(r), 4) for rid, r in zip(ids, reads)], block=30000)
    _search(s["index"], [fq], tmp / "out_fq.tsv", tmp / "ex_fq.tsv", tmp / "exr_fq.tsv")
    assert open(tmp / "ex_fq.tsv").read() == s["bins_text"] and open(tmp / "exr_fq.tsv").read() == s["reads_text"]
    assert open(tmp / "out_fq.tsv", "rb").read() == open(s["plain"], "rb").read()
    _search(s["index"], [bam], None, tmp / "ex_bam.tsv", tmp / "exr_bam.tsv")     # a BAM read name has no description
    assert open(tmp / "ex_bam.tsv").read() == s["bins_text"]
    assert open(tmp / "exr_bam.tsv").read() == s["reads_text"].replace(" some words\t", "\t")


def test_two_query_files_give_the_concatenation(setup):
    s = setup
    tmp, ids, reads = s["tmp"], s["ids"], s["reads"]
    fa1, fa2 = tmp / "a.fa", tmp / "b.fa"
    _fasta(fa1, ids[:40], reads[:40])
    _fasta(fa2, ids[40:], reads[40:])
    _search(s["index"], [fa1], None, None, tmp / "exr_a.tsv")
    _search(s["index"], [fa2], None, None, tmp / "exr_b.tsv")
    _search(s["index"], [fa1, fa2], tmp / "out_ab.tsv", tmp / "ex_ab.tsv", tmp / "exr_ab.tsv")
    a, b = open(tmp / "exr_a.tsv").read(), open(tmp / "exr_b.tsv").read()
    assert a.startswith(READ_COLUMNS) and b.startswith(READ_COLUMNS)
    assert open(tmp / "exr_ab.tsv").read() == a + b[len(READ_COLUMNS):] == s["reads_text"]
    assert open(tmp / "ex_ab.tsv").read() == s["bins_text"]                      # the run's table sums over both files
    assert open(tmp / "out_ab.tsv", "rb").read() == open(s["plain"], "rb").read()
