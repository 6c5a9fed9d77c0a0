"""`taxor search --lca-file / --report-file` refuse what they cannot do before the first HIP call (taxor_amd/csrc/search_cmd.h), so all
of this runs without a device: a comma list of index files, several devices, a --gather transport, an index that would have to be
paged, --report-unit without --report-file.  Each message names the option; the exit status is that of every other refusal."""
import os
import subprocess

import numpy as np
import pytest

from taxor_amd import synth
from taxor_amd.hixf_file import store_hixf
from tests.test_hixf_file_cpu import make_species

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TAXOR = os.path.join(ROOT, "taxor_amd", "taxor")
OPTIONS = [("--lca-file", "calls.tsv"), ("--report-file", "report.txt")]


def run(args):
    env = dict(os.environ, HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="")        # nothing below may need a device
    return subprocess.run([TAXOR, "search"] + args, capture_output=True, text=True, timeout=60, env=env)


def refused(cp, *needles):
    assert cp.returncode == 255, (cp.returncode, cp.stderr)
    assert "[TAXOR SEARCH ERROR] " in cp.stderr, cp.stderr
    for n in needles:
        assert n in cp.stderr, cp.stderr


def base(tmp_path, opt, name, **extra):
    a = {"--index-file": str(tmp_path / "a.hixf"), "--query-file": str(tmp_path / "q.fa"), opt: str(tmp_path / name)}
    a.update(extra)
    return [x for k, v in a.items() if v is not None for x in (k, v)]


@pytest.mark.parametrize("opt,name", OPTIONS)
def test_a_comma_list_of_index_files(tmp_path, opt, name):
    refused(run(base(tmp_path, opt, name, **{"--index-file": f"{tmp_path}/a.hixf,{tmp_path}/b.hixf"})), "Validation failed for option --index-file", opt, "ONE index file")


@pytest.mark.parametrize("opt,name", OPTIONS)
@pytest.mark.parametrize("dev,value", [("--gpus", "2"), ("--gpu-list", "0,1"), ("--gpu-list", "0,0")])
def test_several_devices(tmp_path, opt, name, dev, value):
    refused(run(base(tmp_path, opt, name, **{dev: value})), f"Validation failed for option {dev}", opt, "ONE device")


@pytest.mark.parametrize("opt,name", OPTIONS)
def test_a_gather_transport(tmp_path, opt, name):
    refused(run(base(tmp_path, opt, name, **{"--gather": "host"})), "Validation failed for option --gather", opt)


def test_report_unit(tmp_path):
    refused(run(base(tmp_path, "--lca-file", "calls.tsv", **{"--report-unit": "bases"})), "--report-unit", "--report-file", "needs that option")
    refused(run(base(tmp_path, "--report-file", "r.txt", **{"--report-unit": "hashes"})), "Validation failed for option --report-unit: Value not in {reads, bases}.")
    refused(run(base(tmp_path, "--report-file", "r.txt") + ["--report-unit"]), "Missing value for option --report-unit")
    refused(run(base(tmp_path, "--lca-file", "c.tsv") + ["--report-file"]), "Missing value for option --report-file")


@pytest.mark.parametrize("opt,name", OPTIONS)
def test_an_index_that_would_be_paged(tmp_path, opt, name):
    """--device-index-budget below the index's size: refused once the index file's tables are read, before anything is uploaded"""
    rng = np.random.default_rng(8)
    planted = [np.unique(rng.integers(0, 2**63, size=6000, dtype=np.uint64)) for _ in range(6)]
    lay = synth.make_layout(planted, root_bins=66, child_bins=24, n_children=2, seed=8)
    host = synth.materialize_host(lay)
    assert sum(f["data"].size for f in host) > (2 << 20)
    store_hixf(tmp_path / "a.hixf", host, lay["n_user_bins"], make_species(lay))
    (tmp_path / "q.fa").write_text(">r\n" + "ACGT" * 20 + "\n")
    cp = run(base(tmp_path, opt, name, **{"--device-index-budget": "1"}))
    refused(cp, f"Validation failed for option {opt}", "--device-index-budget 1 MiB", "resident passes")
    assert not (tmp_path / "report.txt").exists()


def test_a_taxonomy_that_is_not_a_tree_is_refused_before_the_device(tmp_path):
    rng = np.random.default_rng(9)
    planted = [np.unique(rng.integers(0, 2**63, size=300, dtype=np.uint64)) for _ in range(6)]
    lay = synth.make_layout(planted, root_bins=66, child_bins=24, n_children=2, seed=9)
    sp = make_species(lay)
    sp[1]["taxid_string"] = "2;99;" + sp[0]["taxid_string"].split(";")[-1]          # species 0's leaf under another parent
    store_hixf(tmp_path / "a.hixf", synth.materialize_host(lay), lay["n_user_bins"], sp)
    (tmp_path / "q.fa").write_text(">r\n" + "ACGT" * 20 + "\n")
    cp = run(base(tmp_path, "--lca-file", "calls.tsv"))
    refused(cp, "Validation failed for option --lca-file", "not a tree", "has two parents", sp[0]["accession_id"], sp[1]["accession_id"])


def test_the_help_says_what_the_columns_are():
    cp = run(["--advanced-help"])
    assert cp.returncode == 0
    for needle in ("--lca-file", "--report-file", "--report-unit", "BEST_QHASH_MATCH", "unclassified", "nothing matched", "longest common prefix"):
        assert needle in cp.stderr, needle
