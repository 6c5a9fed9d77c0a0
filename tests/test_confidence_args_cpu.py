"""`taxor search --lca-confidence` refuses what it cannot do before the first HIP call (taxor_amd/csrc/search_cmd.h), so all of this
runs without a device: a value outside [0,1] or no number, the option without --lca-file / --report-file, a comma list of index files,
several devices, a --gather transport, an index that would have to be paged.  Each message names the option; the exit status is that
of every other refusal."""
import os
import subprocess

import numpy as np
import pytest

from taxor_amd import synth
from taxor_amd.hixf_file import store_hixf
from tests.test_hixf_file_cpu import make_species

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TAXOR = os.path.join(ROOT, "taxor_amd", "taxor")


def run(args):
    env = dict(os.environ, HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="")        # nothing below may need a device
    return subprocess.run([TAXOR, "search"] + args, capture_output=True, text=True, timeout=60, env=env)


def refused(cp, *needles):
    assert cp.returncode == 255, (cp.returncode, cp.stderr)
    assert "[TAXOR SEARCH ERROR] " in cp.stderr, cp.stderr
    for n in needles:
        assert n in cp.stderr, cp.stderr


def base(tmp_path, **extra):
    a = {"--index-file": str(tmp_path / "a.hixf"), "--query-file": str(tmp_path / "q.fa"), "--lca-file": str(tmp_path / "calls.tsv"), "--lca-confidence": "0.1"}
    a.update(extra)
    return [x for k, v in a.items() if v is not None for x in (k, v)]


@pytest.mark.parametrize("value", ["-0.1", "1.5", "nan", "inf"])
def test_a_value_outside_the_range(tmp_path, value):
    refused(run(base(tmp_path, **{"--lca-confidence": value})), "Validation failed for option --lca-confidence: Value not in range [0,1].")


def test_a_value_that_does_not_parse_or_is_missing(tmp_path):
    refused(run(base(tmp_path, **{"--lca-confidence": "0.1x"})), "Value parse failed for --lca-confidence")
    refused(run(base(tmp_path, **{"--lca-confidence": None}) + ["--lca-confidence"]), "Missing value for option --lca-confidence")


def test_the_option_alone(tmp_path):
    refused(run(base(tmp_path, **{"--lca-file": None, "--output-file": str(tmp_path / "o.tsv")})), "--lca-confidence", "--lca-file / --report-file", "needs one of them")


@pytest.mark.parametrize("with_file", ["--lca-file", "--report-file"])
def test_a_comma_list_of_index_files(tmp_path, with_file):
    args = base(tmp_path, **{"--index-file": f"{tmp_path}/a.hixf,{tmp_path}/b.hixf", "--lca-file": None, with_file: str(tmp_path / "f")})
    refused(run(args), "Validation failed for option --index-file", "--lca-confidence", "ONE index file")


@pytest.mark.parametrize("opt,value", [("--gpus", "2"), ("--gpu-list", "0,1"), ("--gpu-list", "0,0")])
def test_several_devices(tmp_path, opt, value):
    refused(run(base(tmp_path, **{opt: value})), f"Validation failed for option {opt}", "--lca-confidence", "ONE device")


@pytest.mark.parametrize("value", ["host", "rccl"])
def test_a_gather_transport(tmp_path, value):
    refused(run(base(tmp_path, **{"--gather": value})), "Validation failed for option --gather", "--lca-confidence")


def test_an_index_that_would_be_paged(tmp_path):
    """--device-index-budget below the index's size: refused once the index file's tables are read, before anything is uploaded"""
    rng = np.random.default_rng(8)
    planted = [np.unique(rng.integers(0, 2**63, size=6000, dtype=np.uint64)) for _ in range(6)]
    lay = synth.make_layout(planted, root_bins=66, child_bins=24, n_children=2, seed=8)
    host = synth.materialize_host(lay)
    assert sum(f["data"].size for f in host) > (2 << 20)
    store_hixf(tmp_path / "a.hixf", host, lay["n_user_bins"], make_species(lay))
    (tmp_path / "q.fa").write_text(">r\n" + "ACGT" * 20 + "\n")
    cp = run(base(tmp_path, **{"--device-index-budget": "1"}))
    refused(cp, "Validation failed for option --lca-confidence", "--device-index-budget 1 MiB", "resident passes")


def test_the_help_says_what_the_columns_are():
    cp = run(["--advanced-help"])
    assert cp.returncode == 0
    for needle in ("--lca-confidence", "SUPPORT", "LCA_TAXID", "LCA_SUPPORT", "C * QHASH_COUNT", "counts once"):
        assert needle in cp.stderr, needle
    assert "--lca-confidence" in run(["--help"]).stderr
