"""The host side of `taxor census` / `taxor search --coverage-breadth` (taxor_amd/csrc/census_format.h through the library's host-only
exports) against the Python restatement (tests/census_expect.py); the estimator on columns the HOST builder peeled (fixed seeds: the
bound is five standard deviations of the binomial plus the rounding, derived and not measured); and the refusals that come before
any HIP call.  No device."""
import math
import os
import subprocess

import numpy as np
import pytest

from taxor_amd import synth
from taxor_amd.search import census_breadth_columns, census_capacity, census_ixf_line, census_keys_est, census_peeled, census_ref_line
from tests import census_expect as ce

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TAXOR = os.path.join(ROOT, "taxor_amd", "taxor")


def run(args):
    env = dict(os.environ, HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="")        # nothing below may need a device
    return subprocess.run([TAXOR] + args, capture_output=True, text=True, timeout=60, env=env)


def refused(cp, *needles):
    assert cp.returncode == 255, (cp.returncode, cp.stderr)
    assert "[TAXOR SEARCH ERROR] " in cp.stderr, cp.stderr
    for n in needles:
        assert n in cp.stderr, cp.stderr


def test_keys_est_equals_the_restatement():
    for nz in list(range(0, 1200)) + [254, 255, 256, 509, 510, 511, 65535, 10**6, 10**9, 2**40, 2**52]:
        assert census_keys_est(nz) == ce.keys_est(nz), nz
    assert [census_keys_est(v) for v in (0, 1, 127, 128, 255, 996)] == [0, 1, 127, 129, 256, 1000]


def test_capacity_equals_the_restatement_and_holds_what_the_ixf_was_sized_for():
    for seg in list(range(0, 400)) + [1000, 4099, 8210, 10**5, 10**6 + 1, 2**31 // 3]:
        c = census_capacity(seg)
        assert c == ce.capacity(seg), seg
        if seg >= 10:
            assert c == synth.capacity_of(seg), seg
            assert synth.seg_len_for(c) <= seg < synth.seg_len_for(c + 1), seg
        else:
            assert c == 0                       # not even an empty bin's 32 slots fit
    for n in (0, 1, 2, 1000, 10**6):
        assert census_capacity(synth.seg_len_for(n)) >= n, n
        assert ce.seg_len_of(n) == synth.seg_len_for(n)


def test_both_line_formatters_equal_the_restatement():
    for args in [("GCF_1", "Some organism", "1280", 15000, 1, 2345), ("a", "b", "c", 0, 0, 0), ("a", "b", "c", 0, 3, 17), ("a", "b", "c", 7, 2, None),
                 ("x", "y z", "9", 3, 1, 2**40), ("x", "y", "9", 2**63, 70000, 2**64 - 1), ("x", "y", "9", 3000, 1, 1), ("x", "y", "9", 200000, 1, 1)]:
        assert census_ref_line(*args) == ce.ref_line(*args), args
    assert census_ref_line(None, None, None, 1000, 1, 5) == "-\t-\t-\t1000\t1\t5\t5.00\n"
    assert census_ref_line("a", "b", "c", 15000, 2, 2345) == "a\tb\tc\t15000\t2\t2345\t156.33\n"
    for args in [(0, 68, 60, 2053, 128, 4900), (3, 1, 1, 16, 64, 0), (4, 1025, 1000, 85, 1088, None), (2**32, 64, 0, 3, 64, 1), (1, 64, 64, 23333, 64, 56000)]:
        assert census_ixf_line(*args) == ce.ixf_line(*args), args
    assert census_ixf_line(1, 64, 60, 420, 64, 500) == "1\t64\t60\t4\t1260\t%d\t500\t%.3f\t80640\n" % (ce.capacity(420), 500 / ce.capacity(420))
    assert census_ixf_line(1, 64, 60, 3, 64, 0) == "1\t64\t60\t4\t9\t0\t0\tNA\t576\n"          # an IXF too small for any key


def test_the_breadth_columns_equal_the_restatement():
    cases = [(0, 0, 1000), (10, 10, 1000), (500, 700, 1000), (1000, 5000, 1000), (1200, 5000, 1000), (1, 1, 10**9), (3, 40000, 2), (7, 9, 0), (7, 9, None),
             (1, 1, 19999), (1, 1, 20000), (1, 1, 20001), (2**40, 2**50, 2**41), (5, 5, 1), (123, 456, 789)]
    for d, hm, ih in cases:
        assert census_breadth_columns(d, hm, ih) == ce.breadth_columns(d, hm, ih), (d, hm, ih)
    assert census_breadth_columns(500, 700, 1000) == "\t1000\t0.5000\t%.4f\t%.2f" % (1 - math.exp(-0.7), 0.5 / (1 - math.exp(-0.7)))
    assert census_breadth_columns(1200, 5000, 1000).startswith("\t1000\t1.0000\t0.9933\t")                # BREADTH is capped at 1
    assert census_breadth_columns(7, 9, 0) == "\t0\tNA\tNA\tNA" and census_breadth_columns(7, 9, None) == "\tNA\tNA\tNA\tNA"
    assert census_breadth_columns(1, 1, 10**9) == "\t1000000000\t0.0000\t0.0000\tNA"                      # an expectation that prints as 0.0000


# (keys, keys the IXF is sized for, seed of the keys, seed0 of the builder): full capacity four times, and a bin far below its IXF's
ESTIMATOR_CASES = [(1, 1, 11, 3), (100, 100, 12, 5), (1000, 1000, 13, 7), (20000, 20000, 14, 9), (3000, 20000, 15, 11)]


@pytest.mark.parametrize("n,sized_for,key_seed,seed0", ESTIMATOR_CASES)
def test_the_estimate_on_columns_of_the_host_builder(n, sized_for, key_seed, seed0):
    rng = np.random.default_rng(key_seed)
    keys = np.unique(rng.integers(0, 2**63, size=n + 64, dtype=np.uint64))[:n]
    assert keys.size == n
    seg = synth.seg_len_for(sized_for)
    _, cols = synth.build_columns({0: keys}, seg, seed0)
    nz = int(np.count_nonzero(cols[0]))
    est = census_keys_est(nz)
    print(f"n={n} sized_for={sized_for} rows={3 * seg} nonzero={nz} keys_est={est} sigma={math.sqrt(n / 255.0):.3f} bound={ce.bound(n):.3f}")
    assert nz <= n                                              # a key owns one slot, a free slot stays 0
    assert abs(est - n) <= ce.bound(n)
    assert census_peeled(nz, seg) and nz <= census_capacity(seg)


def test_all_zero_and_all_ff_columns_of_a_small_ixf():
    seg = synth.seg_len_for(40)
    rows = 3 * seg
    zero, ff = np.zeros(rows, np.uint8), np.full(rows, 0xFF, np.uint8)
    assert census_keys_est(np.count_nonzero(zero)) == 0 and census_peeled(np.count_nonzero(zero), seg)
    assert not census_peeled(np.count_nonzero(ff), seg)          # every row nonzero: more than the IXF has room for keys -- not peeled
    shapes = [dict(bins=2, stride=64, seg_len=seg, fname_idx=np.array([0, 1]))]
    c = ce.Census(shapes, [np.array([0, rows], np.uint64)], 2)
    assert c.index_hashes == [0, None] and c.ixf[0][5] is None
    assert c.refs_text([dict(user_bin=0, accession_id="a", organism_name="o", taxid="1", seq_len=0), dict(user_bin=1, accession_id="b", organism_name="p", taxid="2", seq_len=9)]) == \
        ce.REF_COLUMNS + "a\to\t1\t0\t1\t0\tNA\n" + "b\tp\t2\t9\t1\tNA\tNA\n"


def test_coverage_breadth_needs_the_coverage_file(tmp_path):
    cp = run(["search", "--index-file", str(tmp_path / "a.hixf"), "--query-file", str(tmp_path / "q.fa"), "--output-file", str(tmp_path / "o.tsv"), "--coverage-breadth"])
    refused(cp, "--coverage-breadth", "--coverage-file", "needs that option")


def test_census_needs_its_index_file_and_its_output_file(tmp_path):
    refused(run(["census", "--output-file", str(tmp_path / "refs.tsv")]), "usage: taxor census", "--index-file")
    refused(run(["census", "--index-file", str(tmp_path / "a.hixf")]), "usage: taxor census", "--output-file")
    refused(run(["census", "--index-file", str(tmp_path / "none.hixf"), "--output-file", str(tmp_path / "refs.tsv")]), "--index-file", "does not exist")
    assert not (tmp_path / "refs.tsv").exists()
    refused(run(["census", "--index-file", str(tmp_path / "a.hixf"), "--output-file", str(tmp_path / "refs.tsv"), "--bogus"]), "unknown or incomplete option --bogus")


def test_the_help_names_the_flag_and_its_limits():
    cp = run(["search", "--advanced-help"])
    assert cp.returncode == 0
    for needle in ("--coverage-breadth", "INDEX_HASHES", "BREADTH", "EXPECTED_BREADTH", "BREADTH_RATIO", "Reported, not thresholded", "8-bit fingerprints", "free slots assumed zero",
                   "taxor census"):
        assert needle in cp.stderr, needle
    assert "--coverage-breadth" in run(["search", "--help"]).stderr
