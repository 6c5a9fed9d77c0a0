"""`taxor search --segments-file` refuses what it cannot do before the first HIP call (taxor_amd/csrc/search_cmd.h), so all of this runs
without a device: a comma list of index files, several devices, a --gather transport, an empty file name, an index that would have to
be paged, a --segments-switch-cost outside [1,2^20] or without the option it belongs to.  Each message names the option; the exit
status is that of every other refusal."""
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
    a = {"--index-file": str(tmp_path / "a.hixf"), "--query-file": str(tmp_path / "q.fa"), "--output-file": str(tmp_path / "out.tsv"),
         "--segments-file": str(tmp_path / "sg.tsv")}
    a.update(extra)
    return [x for k, v in a.items() if v is not None for x in (k, v)]


def test_a_comma_list_of_index_files(tmp_path):
    refused(run(base(tmp_path, **{"--index-file": f"{tmp_path}/a.hixf,{tmp_path}/b.hixf"})), "Validation failed for option --index-file", "--segments-file", "ONE index file")


@pytest.mark.parametrize("opt,value", [("--gpus", "2"), ("--gpu-list", "0,1"), ("--gpu-list", "0,0")])
def test_several_devices(tmp_path, opt, value):
    refused(run(base(tmp_path, **{opt: value})), f"Validation failed for option {opt}", "--segments-file", "ONE device")


@pytest.mark.parametrize("value", ["host", "rccl"])
def test_a_gather_transport(tmp_path, value):
    refused(run(base(tmp_path, **{"--gather": value})), "Validation failed for option --gather", "--segments-file")


def test_an_empty_file_name_and_a_missing_value(tmp_path):
    refused(run(base(tmp_path, **{"--segments-file": ""})), "Validation failed for option --segments-file: the file name is empty.")
    refused(run(base(tmp_path, **{"--segments-file": None}) + ["--segments-file"]), "Missing value for option --segments-file")


@pytest.mark.parametrize("value", ["0", "-1", "1048577", "4294967296"])
def test_switch_cost_out_of_range(tmp_path, value):
    refused(run(base(tmp_path, **{"--segments-switch-cost": value})), "Validation failed for option --segments-switch-cost: Value not in range [1,1048576].")


def test_switch_cost_that_does_not_parse_or_stands_alone(tmp_path):
    refused(run(base(tmp_path, **{"--segments-switch-cost": "3x"})), "Value parse failed for --segments-switch-cost")
    refused(run(base(tmp_path, **{"--segments-file": None, "--segments-switch-cost": "3"})), "--segments-switch-cost", "--segments-file", "needs that option")


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
    refused(cp, "Validation failed for option --segments-file", "--device-index-budget 1 MiB", "resident passes")


def test_the_help_says_what_the_columns_are():
    cp = run(["--advanced-help"])
    assert cp.returncode == 0
    for needle in ("--segments-file", "--segments-switch-cost", "SHAPE", "HASH_START", "BASE_END_APPROX", "HITS_OF_BEST", "split", "insert", "mosaic",
                   "a choice, not a measurement", "carries no positions", "did not pass the search threshold"):
        assert needle in cp.stderr, needle
    assert "--segments-file" in run(["--help"]).stderr
