"""`taxor search --exclusive-file` / `--exclusive-reads-file` refuse what they cannot do before the first HIP call
(taxor_amd/csrc/search_cmd.h), so all of this runs without a device: a comma list of index files, several devices, a --gather transport,
an empty file name, an index that would have to be paged, an --exclusive-precision outside 4..16 or without the option it belongs to.
Each message names the option; the exit status is that of every other refusal."""
import os
import subprocess

import numpy as np
import pytest

from taxor_amd import synth
from taxor_amd.hixf_file import store_hixf
from tests.test_hixf_file_cpu import make_species

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TAXOR = os.path.join(ROOT, "taxor_amd", "taxor")
OPTIONS = ["--exclusive-file", "--exclusive-reads-file"]


def run(args):
    env = dict(os.environ, HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="")        # nothing below may need a device
    return subprocess.run([TAXOR, "search"] + args, capture_output=True, text=True, timeout=60, env=env)


def refused(cp, *needles):
    assert cp.returncode == 255, (cp.returncode, cp.stderr)
    assert "[TAXOR SEARCH ERROR] " in cp.stderr, cp.stderr
    for n in needles:
        assert n in cp.stderr, cp.stderr


def base(tmp_path, opt="--exclusive-file", **extra):
    a = {"--index-file": str(tmp_path / "a.hixf"), "--query-file": str(tmp_path / "q.fa"), "--output-file": str(tmp_path / "out.tsv"), opt: str(tmp_path / "ex.tsv")}
    a.update(extra)
    return [x for k, v in a.items() if v is not None for x in (k, v)]


@pytest.mark.parametrize("o", OPTIONS)
def test_a_comma_list_of_index_files(tmp_path, o):
    refused(run(base(tmp_path, o, **{"--index-file": f"{tmp_path}/a.hixf,{tmp_path}/b.hixf"})), "Validation failed for option --index-file", o + " takes", "ONE index file")


@pytest.mark.parametrize("o", OPTIONS)
@pytest.mark.parametrize("opt,value", [("--gpus", "2"), ("--gpu-list", "0,1"), ("--gpu-list", "0,0")])
def test_several_devices(tmp_path, o, opt, value):
    refused(run(base(tmp_path, o, **{opt: value})), f"Validation failed for option {opt}", o + " examines", "ONE device")


@pytest.mark.parametrize("o", OPTIONS)
@pytest.mark.parametrize("value", ["host", "rccl"])
def test_a_gather_transport(tmp_path, o, value):
    refused(run(base(tmp_path, o, **{"--gather": value})), "Validation failed for option --gather", o + " runs")


@pytest.mark.parametrize("o", OPTIONS)
def test_an_empty_file_name_and_a_missing_value(tmp_path, o):
    refused(run(base(tmp_path, o, **{o: ""})), f"Validation failed for option {o}: the file name is empty.")
    refused(run(base(tmp_path, o, **{o: None}) + [o]), f"Missing value for option {o}")


def test_both_files_with_the_first_named(tmp_path):
    """both options given: the refusal names --exclusive-file"""
    refused(run(base(tmp_path, **{"--exclusive-reads-file": str(tmp_path / "r.tsv"), "--gpus": "2"})), "--exclusive-file examines", "ONE device")


@pytest.mark.parametrize("value", ["3", "17", "0", "-1"])
def test_precision_out_of_range(tmp_path, value):
    refused(run(base(tmp_path, **{"--exclusive-precision": value})), "Validation failed for option --exclusive-precision: Value not in range [4,16].")


def test_precision_that_does_not_parse_or_stands_without_its_file(tmp_path):
    refused(run(base(tmp_path, **{"--exclusive-precision": "5x"})), "Value parse failed for --exclusive-precision")
    refused(run(base(tmp_path, **{"--exclusive-file": None, "--exclusive-precision": "5"})), "--exclusive-precision", "--exclusive-file", "needs that option")
    # the reads file has no sketch to size
    refused(run(base(tmp_path, "--exclusive-reads-file", **{"--exclusive-precision": "5"})), "--exclusive-precision", "--exclusive-file", "needs that option")


def test_expect_needs_the_tsv(tmp_path):
    refused(run(base(tmp_path, **{"--output-file": None, "--expect": str(tmp_path / "e.tsv")})), "--expect compares the TSV", "--output-file")


@pytest.mark.parametrize("o", OPTIONS)
def test_an_index_that_would_be_paged(tmp_path, o):
    """--device-index-budget below the index's size: refused once the index file's tables are read, before anything is uploaded"""
    rng = np.random.default_rng(8)
    planted = [np.unique(rng.integers(0, 2**63, size=6000, dtype=np.uint64)) for _ in range(6)]
    lay = synth.make_layout(planted, root_bins=66, child_bins=24, n_children=2, seed=8)
    host = synth.materialize_host(lay)
    assert sum(f["data"].size for f in host) > (2 << 20)
    store_hixf(tmp_path / "a.hixf", host, lay["n_user_bins"], make_species(lay))
    (tmp_path / "q.fa").write_text(">r\n" + "ACGT" * 20 + "\n")
    cp = run(base(tmp_path, o, **{"--device-index-budget": "1"}))
    refused(cp, f"Validation failed for option {o}", "--device-index-budget 1 MiB", "resident passes", "exclusive hashes pass by pass")
    assert not (tmp_path / "ex.tsv").exists() or o == "--exclusive-reads-file"      # the run's table is written at the end only


def test_the_help_says_what_the_columns_are_and_both_limits():
    cp = run(["--advanced-help"])
    assert cp.returncode == 0
    for needle in ("--exclusive-file", "--exclusive-reads-file", "--exclusive-precision", "CANDIDATE_READS", "EXCLUSIVE_HITS", "EXCLUSIVE_READS", "DISTINCT_EXCLUSIVE",
                   "EXCLUSIVE_FRACTION", "MATCHED", "SHARED", "0.5 is no verdict", "the references the read REPORTED", "below the search threshold", "1/256"):
        assert needle in cp.stderr, needle
    assert "--exclusive-file" in run(["--help"]).stderr and "--exclusive-reads-file" in run(["--help"]).stderr
