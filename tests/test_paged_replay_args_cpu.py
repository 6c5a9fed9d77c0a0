"""Paged search, the part that needs no GPU: --paged-replay and --paged-reread are options `taxor search` knows and --advanced-help documents; the bound
of the saved hash lists' store is host arithmetic on the query's size and the index's (k, s, t), and the decision between replaying and
re-reading follows from it and an available-memory figure; the saved batch's host code runs clean under ASan + UBSan."""
import os
import shutil
import subprocess

import pytest

from taxor_amd.search import saved_bytes_bound, saved_store_fits
from tests.test_sanitizers_cpu import SAN, _build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TAXOR = os.path.join(ROOT, "taxor_amd", "taxor")


def run(*args):
    return subprocess.run([TAXOR, "search"] + [str(a) for a in args], capture_output=True, text=True, timeout=60)


def test_paged_reread_is_accepted_and_documented(tmp_path):
    cp = run("--advanced-help")
    assert cp.returncode == 0
    text = cp.stdout + cp.stderr
    assert "--paged-reread" in text and "--paged-replay" in text and "--device-index-budget" in text and "Not the default" in text
    short = (lambda c: c.stdout + c.stderr)(run("--help"))
    assert "--paged-reread" not in short and "--paged-replay" not in short                     # hidden: the short help lists neither
    # accepted: the run gets past option parsing and fails on the index file that does not exist, not on the option
    cp = run("--index-file", tmp_path / "none.hixf", "--query-file", tmp_path / "none.fq", "--output-file", tmp_path / "o.tsv", "--device-index-budget", 4,
             "--paged-reread", "--paged-replay")
    assert cp.returncode != 0 and "Unknown option" not in cp.stdout + cp.stderr and "does not exist" in cp.stdout + cp.stderr
    cp = run("--index-file", tmp_path / "none.hixf", "--query-file", tmp_path / "none.fq", "--output-file", tmp_path / "o.tsv", "--paged-rerea")
    assert cp.returncode != 0 and "Unknown option --paged-rerea" in cp.stdout + cp.stderr


def test_store_bound_from_the_query_size():
    """8 B per hash at one hash per min(t, k-s+1-t+1) bases (syncmers; k22/s12/t5: 5) or per base (minimisers), one more per k bases
    (a read with any hash has k of them), and 28 B per read at one read per 200 bases"""
    for bases, syn, k, s, t, gap in ((0, 1, 22, 12, 5, 5), (1_000_000, 1, 22, 12, 5, 5), (10**12, 1, 22, 12, 5, 5), (123_456_789, 1, 28, 20, 4, 4),
                                    (5_000, 1, 32, 31, 1, 1), (77_777, 0, 20, 0, 0, 1), (3 * 10**9, 1, 22, 12, 8, 4)):
        want = (bases // gap + bases // k + 1) * 8 + (bases // 200 + 1) * 28
        assert saved_bytes_bound(bases, bool(syn), k, s, t) == want, (bases, k, s, t)
    # a 1-Gbp FASTQ against a k22/s12 index: 1.6 GB of hashes at the bound, whatever the reads' lengths
    assert 1.9e9 < saved_bytes_bound(10**9) < 2.2e9


def test_bound_exceeds_available_memory_so_reread():
    gib = 1 << 30
    bound = saved_bytes_bound(4 * 10**9)
    assert saved_store_fits(bound, 0)                          # MemAvailable unknown: the running check decides
    assert saved_store_fits(bound, bound + gib)
    assert saved_store_fits(bound, bound + (gib >> 2))         # a quarter of a gibibyte to spare is the line
    assert not saved_store_fits(bound, bound + (gib >> 2) - 1)
    assert not saved_store_fits(bound, bound - 1)
    assert not saved_store_fits(bound, 1)


@pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")
def test_saved_batch_host_code_under_asan_ubsan(tmp_path):
    exe = _build(tmp_path, "saved_batch_check", [os.path.join(SAN, "saved_batch_check.cpp")], ["-fsanitize=address,undefined"])
    cp = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert cp.returncode == 0 and cp.stdout.startswith("ok "), cp.stdout + cp.stderr[-2000:]
    assert "ERROR" not in cp.stderr and "runtime error" not in cp.stderr, cp.stderr[-2000:]
