"""`taxor search --lca-confidence`: the call file and the report equal, byte for byte, the text of the Python restatement
(tests/confidence_expect.py, fed by the oracle's search of the same reads) for every input kind, with and without a TSV and beside the
other outputs; 0 gives today's files; the TSV and the other outputs do not know about the option."""
import gzip
import os
import subprocess

import numpy as np
import pytest

from taxor_amd import synth
from taxor_amd.hixf_file import store_hixf
from tests import bam_writer as bw
from tests import confidence_expect as ce
from tests import lca_expect as le
from tests.coverage_expect import Expect as CovExpect
from tests.test_gpu_lca import make_world

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TAXOR = os.path.join(ROOT, "taxor_amd", "taxor")
C = "0.62"


def _search(index, queries, out=None, lca=None, rep=None, conf=C, extra=(), batch="30"):
    # --percentage 0.3: below the syncmer model's threshold, so that reads report references that do not survive the 0.8 * max filter
    cmd = [TAXOR, "search", "--index-file", str(index), "--query-file", ",".join(str(q) for q in queries), "--threads", "4", "--batch-reads", batch,
           "--percentage", "0.3"]
    cmd += (["--output-file", str(out)] if out else []) + (["--lca-file", str(lca)] if lca else []) + (["--report-file", str(rep)] if rep else [])
    cmd += (["--lca-confidence", conf] if conf is not None else []) + [str(x) for x in extra]
    cp = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert cp.returncode == 0, cp.stderr
    return cp


def _fasta(path, ids, reads):
    with open(path, "wb") as f:
        for rid, r in zip(ids, reads):
            f.write(b">" + rid + b"\n" + r + b"\n")


@pytest.fixture(scope="module")
def setup(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("confidence_cli")
    g, go, lay, host, sp = make_world(64)
    index = tmp / "idx.hixf"
    store_hixf(index, host, lay["n_user_bins"], sp)
    bases, offs, origin = synth.synth_reads(g, go, 90, 1200, error_rate=0.02, frac_random=0.2, seed=9)
    reads = [bytes(bases[int(offs[i]):int(offs[i + 1])]) for i in range(90)]
    G = [bytes(g[int(go[i]):int(go[i + 1])]) for i in range(len(go) - 1)]
    # a read without a hash in the middle, exact pieces of the two strains, a chimera of unrelated genomes, a read of more than one piece
    reads = reads[:45] + [b"ACGTACGT"] + reads[45:] + [G[0][100:1500], G[1][200:2500], G[3][1000:5000] + G[5][2000:6000], G[4] + G[6]]
    # two reads picked by hand for C = 0.62.  Half of the first is genome 0, a quarter genome 2 (the other species of its genus, no
    # survivor) and a quarter random: the species has 58 % of its hashes, the genus 75 %.  Two fifths of the second are genome 3
    rng = np.random.default_rng(5)
    rnd = lambda n: bytes(rng.choice(np.frombuffer(b"ACGT", np.uint8), size=n))
    reads += [G[0][1000:3600] + G[2][8000:9200] + rnd(1200), G[3][2000:4000] + rnd(3000)]
    ids = [b"r%d some words" % i for i in range(len(reads))]
    fa = tmp / "reads.fa"
    _fasta(fa, ids, reads)
    lin = le.Lineage(sp, lay["n_user_bins"])
    cov = CovExpect(host)
    names, lens = [i.decode() for i in ids], [len(r) for r in reads]
    want = {}
    for c in (0.0, float(C)):                                                     # computed once, shared, never changed
        e = ce.Expect(lin, cov, c)
        e.add_bases(reads, percentage=0.3)
        want[c] = dict(e=e, files=ce.files(e, names, lens), bases=ce.files(e, names, lens, unit="bases")[1],
                       bam=ce.files(e, [n.split(" ")[0] for n in names], lens)[0])
    kinds = [ce.outcome(x) for x in want[float(C)]["e"].calls]
    assert {"never", "stays", "dropped", "climbs 1"} <= set(kinds) and kinds[-2:] == ["climbs 1", "dropped"], kinds
    assert max(x["n_hashes"] for x in want[0.0]["e"].calls) > 2048
    tsv, lca, rep, plain = tmp / "out.tsv", tmp / "calls.tsv", tmp / "report.txt", tmp / "plain.tsv"
    _search(index, [fa], tsv, lca, rep)
    _search(index, [fa], plain, conf=None)
    return dict(tmp=tmp, index=index, fa=fa, ids=ids, reads=reads, want=want, tsv=tsv, lca=lca, rep=rep, plain=plain)


def test_both_files_equal_the_expectation_and_the_tsv_is_unchanged(setup):
    s = setup
    calls, report = s["want"][float(C)]["files"]
    assert open(s["lca"]).read() == calls
    assert open(s["rep"]).read() == report
    assert open(s["tsv"], "rb").read() == open(s["plain"], "rb").read()          # the TSV does not know about the option
    lines = calls.splitlines()
    assert lines[0] == ce.CALL_HEADER.rstrip("\n") and len(lines) == 1 + len(s["reads"])
    assert lines[1 + 45] == "U\tr45 some words\t0\t8\t0\t0\t0\t0\t0\t0"            # no hash: unclassified anyway, zeros
    dropped = [l.split("\t") for l in lines[1:] if l.startswith("U\t") and l.split("\t")[8] != "0"]
    assert dropped and dropped[-1][1] == "r%d some words" % (len(s["reads"]) - 1)  # U with its real counts, the call it lost and why
    assert all(int(l[4]) > 0 and int(l[5]) > 0 and int(l[6]) > 0 and float(l[7]) < float(C) * int(l[4]) for l in dropped)


def test_zero_gives_todays_files(setup):
    s = setup
    tmp = s["tmp"]
    _search(s["index"], [s["fa"]], None, tmp / "c_plain.tsv", tmp / "r_plain.txt", conf=None)
    _search(s["index"], [s["fa"]], None, tmp / "c0.tsv", tmp / "r0.txt", conf="0")
    assert open(tmp / "r0.txt", "rb").read() == open(tmp / "r_plain.txt", "rb").read()
    zero, plain = open(tmp / "c0.tsv").read().splitlines(), open(tmp / "c_plain.tsv").read().splitlines()
    assert plain[0] + "\n" == le.CALL_HEADER and [l.split("\t")[:7] for l in zero] == [l.split("\t") for l in plain]
    assert (open(tmp / "c0.tsv").read(), open(tmp / "r0.txt").read()) == s["want"][0.0]["files"]


def test_without_a_tsv_each_option_alone_and_bases(setup):
    s = setup
    tmp = s["tmp"]
    calls, report = s["want"][float(C)]["files"]
    _search(s["index"], [s["fa"]], None, tmp / "c1.tsv", tmp / "r1.txt")
    assert open(tmp / "c1.tsv").read() == calls and open(tmp / "r1.txt").read() == report
    _search(s["index"], [s["fa"]], None, tmp / "c2.tsv", None, batch="1000")
    assert open(tmp / "c2.tsv").read() == calls
    _search(s["index"], [s["fa"]], None, None, tmp / "r3.txt", extra=["--report-unit", "bases"], batch="17")
    assert open(tmp / "r3.txt").read() == s["want"][float(C)]["bases"] != report


def test_every_input_kind_gives_the_same_bytes(setup):
    s = setup
    tmp, ids, reads = s["tmp"], s["ids"], s["reads"]
    calls, report = s["want"][float(C)]["files"]
    fq = tmp / "reads.fastq.gz"
    with gzip.open(fq, "wb") as f:
        for rid, r in zip(ids, reads):
            f.write(b"@" + rid + b"\n" + r + b"\n+\n" + b"I" * len(r) + b"\n")
    bam = tmp / "reads.bam"
    bw.write_bam(bam, [(rid.split(b" ")[0], bw.codes_of_ascii(r), 4) for rid, r in zip(ids, reads)], block=30000)
    for q, extra, want in ((fq, [], calls), (bam, [], s["want"][float(C)]["bam"]), (s["fa"], ["--device-parse"], calls)):
        c, r = tmp / "c_kind.tsv", tmp / "r_kind.txt"
        _search(s["index"], [q], None, c, r, extra=extra)
        assert open(c).read() == want, (q.name, extra)
        assert open(r).read() == report, (q.name, extra)


def test_beside_the_coverage_the_hit_map_and_the_profile_options(setup):
    s = setup
    tmp = s["tmp"]
    uniq = tmp / "uniq.fa"                                                        # the profile options want unique read ids (they cut at the first space)
    ids = [b"u%d" % i for i in range(len(s["reads"]))]
    _fasta(uniq, ids, s["reads"])
    for d in ("with", "without"):
        os.makedirs(tmp / d, exist_ok=True)
    others = lambda d: ["--coverage-file", tmp / d / "cov.tsv", "--hitmap-file", tmp / d / "hm.tsv", "--cami-report-file", tmp / d / "p.cami",
                        "--binning-file", tmp / d / "b.tsv", "--sample-id", "s1"]
    _search(s["index"], [uniq], tmp / "with" / "o.tsv", tmp / "with" / "c.tsv", tmp / "with" / "r.txt", extra=others("with"))
    _search(s["index"], [uniq], tmp / "without" / "o.tsv", None, None, conf=None, extra=others("without"))
    for f in ("o.tsv", "cov.tsv", "hm.tsv", "p.cami", "b.tsv"):
        assert open(tmp / "with" / f, "rb").read() == open(tmp / "without" / f, "rb").read(), f
    e = s["want"][float(C)]["e"]
    assert (open(tmp / "with" / "c.tsv").read(), open(tmp / "with" / "r.txt").read()) == ce.files(e, [i.decode() for i in ids], [len(r) for r in s["reads"]])
