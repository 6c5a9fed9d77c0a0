"""The lineage builder of `taxor search --lca-file / --report-file` (taxor_amd/csrc/lineage.h) as a stand-alone program under
AddressSanitizer + UBSan: the edge inputs of tests/test_lineage_cpu.py, null strings included.  Host code only."""
import os
import shutil
import subprocess

import pytest

from tests.test_sanitizers_cpu import SAN, _build

pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")


def test_lineage_under_asan_ubsan(tmp_path):
    exe = _build(tmp_path, "lineage_check", [os.path.join(SAN, "lineage_check.cpp")], ["-fsanitize=address,undefined"])
    cp = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert cp.returncode == 0 and cp.stdout.startswith("ok "), cp.stdout + cp.stderr[-2000:]
    assert "ERROR" not in cp.stderr and "runtime error" not in cp.stderr, cp.stderr[-2000:]
