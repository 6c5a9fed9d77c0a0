"""`taxor census` and `taxor search --coverage-file --coverage-breadth`: the bytes of refs.tsv and ixfs.tsv equal the text formatted in
Python from the host layout's own columns (tests/census_expect.py); the coverage file with the flag equals the expectation -- its
first eight columns from tests/coverage_expect.Expect, the other four from the census expectation -- and, its last four columns cut,
the file written without the flag; the TSV does not know about the flag."""
import os
import subprocess

import numpy as np
import pytest

from taxor_amd import synth
from taxor_amd.search import hll_estimate
from tests import census_expect as ce
from tests.coverage_expect import Expect
from tests.test_gpu_cli import _setup

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TAXOR = os.path.join(ROOT, "taxor_amd", "taxor")
COLUMNS = "#ACCESSION\tREFERENCE_NAME\tTAXID\tREF_LEN\tREADS\tHASH_MATCHES\tDISTINCT_HASHES\tDUPLICITY"


def _run(args):
    cp = subprocess.run([TAXOR] + [str(a) for a in args], capture_output=True, text=True, timeout=300)
    assert cp.returncode == 0, cp.stderr
    return cp


@pytest.fixture(scope="module")
def world(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("census_cli")
    g, go, host, sp, index = _setup(tmp, 61)
    e = Expect(host)
    census = ce.Census(host, ce.nonzero_of(host), e.n_bins)
    return dict(tmp=tmp, g=g, go=go, host=host, sp=sp, index=index, e=e, census=census)


def test_census_files(world):
    w, tmp = world, world["tmp"]
    refs, ixfs = tmp / "refs.tsv", tmp / "ixfs.tsv"
    cp = _run(["census", "--index-file", w["index"], "--output-file", refs, "--ixf-file", ixfs])
    c = w["census"]
    assert open(refs).read() == c.refs_text(w["sp"])
    assert open(ixfs).read() == c.ixfs_text()
    assert "census:" in cp.stdout and "GB/s" in cp.stdout
    # the planted references are peeled filters with a count, the random-filled decoys are not
    counted = [v for v in c.index_hashes if v is not None]
    assert len(counted) >= 7 and min(counted) > 100 and c.index_hashes.count(None) > len(counted)
    assert c.leaf_bins[0] == 3                                                   # make_layout's split user bin
    # refs.tsv alone
    refs2 = tmp / "refs2.tsv"
    _run(["census", "--index-file", w["index"], "--output-file", refs2])
    assert open(refs2, "rb").read() == open(refs, "rb").read()


def test_coverage_breadth(world):
    w, tmp = world, world["tmp"]
    g, go, sp, e, c = w["g"], w["go"], w["sp"], w["e"], w["census"]
    bases, offs, origin = synth.synth_reads(g, go, 160, 1200, error_rate=0.02, frac_random=0.2, seed=4)
    reads = [bytes(bases[int(offs[i]):int(offs[i + 1])]) for i in range(160)]
    hot = int(np.argmax(origin >= 0))
    reads += reads[:40] + [reads[hot]] * 20 + [b"ACGTACGT"]
    fa = tmp / "reads.fa"
    with open(fa, "wb") as f:
        for i, r in enumerate(reads):
            f.write(b">r%d\n" % i + r + b"\n")
    e.clear()
    e.add_bases(reads)
    reg = e.registers(12)
    by_bin = {}
    for s in sp:
        by_bin.setdefault(s["user_bin"], s)
    want, want_plain = COLUMNS + ce.BREADTH_COLUMNS + "\n", COLUMNS + "\n"
    with_number = 0
    for b in range(e.n_bins):
        if not e.reads[b]:
            continue
        hm = int(e.hash_matches[b])
        d = int(np.floor(hll_estimate(reg[b], 12) + 0.5))
        if hm and d < 1:
            d = 1
        s = by_bin.get(b, sp[0])
        line = "\t".join([s["accession_id"], s["organism_name"], s["taxid"], str(s["seq_len"]), str(int(e.reads[b])), str(hm), str(d), "%.2f" % (hm / d if d else 0.0)])
        want += line + ce.breadth_columns(d, hm, c.index_hashes[b]) + "\n"
        want_plain += line + "\n"
        with_number += c.index_hashes[b] is not None
    assert want.count("\n") > 6 and with_number >= 3

    base = ["search", "--index-file", w["index"], "--query-file", fa, "--threads", "4", "--batch-reads", "40"]
    tsv, cov, tsv0, cov0, tsv1 = tmp / "out.tsv", tmp / "cov.tsv", tmp / "out0.tsv", tmp / "cov0.tsv", tmp / "plain.tsv"
    _run(base + ["--output-file", tsv, "--coverage-file", cov, "--coverage-breadth"])
    _run(base + ["--output-file", tsv0, "--coverage-file", cov0])
    _run(base + ["--output-file", tsv1])
    got = open(cov).read()
    assert got == want
    assert open(cov0).read() == want_plain                                        # without the flag: the file as it always was
    assert "".join("\t".join(l.split("\t")[:-4]) + "\n" for l in got.splitlines()) == want_plain
    assert open(tsv, "rb").read() == open(tsv1, "rb").read() == open(tsv0, "rb").read()     # the TSV does not know about the flag
    # a reference the reads came from: a breadth above 0, an expectation, a ratio
    rows = [l.split("\t") for l in got.splitlines()[1:]]
    full = [r for r in rows if r[8] != "NA" and r[11] != "NA"]
    assert full and all(0.0 < float(r[9]) <= 1.0 and 0.0 < float(r[10]) <= 1.0 for r in full)
