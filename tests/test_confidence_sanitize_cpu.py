"""The host side of `taxor search --lca-confidence` (taxor_amd/csrc/confidence_format.h: the accepted thresholds, "depth d holds", the
line formatter) as a stand-alone program under AddressSanitizer + UBSan, and the formatter's text against the Python restatement the
GPU tests compare with (tests/confidence_expect.py).  Host code only."""
import os
import shutil
import subprocess

import pytest

from tests import confidence_expect as ce
from tests.test_sanitizers_cpu import SAN, _build

pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")


def test_confidence_format_under_asan_ubsan(tmp_path):
    exe = _build(tmp_path, "confidence_check", [os.path.join(SAN, "confidence_check.cpp")], ["-fsanitize=address,undefined"])
    cp = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert cp.returncode == 0 and cp.stdout.startswith("ok "), cp.stdout + cp.stderr[-2000:]
    assert "ERROR" not in cp.stderr and "runtime error" not in cp.stderr, cp.stderr[-2000:]


def test_the_python_restatement_writes_the_lines_the_program_checks():
    c = dict(node="561", depth=6, lca_node="562", lca_depth=7, support=70, lca_support=40, any_support=80, best=60, n_refs=2, n_hashes=100)
    assert ce.call_line(c, "r", 1200) == "C\tr\t561\t1200\t100\t60\t2\t70\t562\t40\n"
    c.update(node="0", depth=0, support=14, lca_support=12, best=12, n_refs=1)
    assert ce.call_line(c, "r", 1200) == "U\tr\t0\t1200\t100\t12\t1\t14\t562\t12\n"
    c.update(lca_node="0")
    assert ce.call_line(c, "r", 8) == "U\tr\t0\t8\t0\t0\t0\t0\t0\t0\n"
    assert ce.holds(5, 0.5, 10) and not ce.holds(4, 0.5, 10) and ce.holds(0, 0.0, 0) and not ce.holds(9, 1.0, 10)
    assert ce.CALL_HEADER.count("\t") == 9
