"""The host side of `taxor census` / `taxor search --coverage-breadth` (taxor_amd/csrc/census_format.h: the estimate, the capacity's
bisection, the sums per user bin and IXF, the line formatters) as a stand-alone program under AddressSanitizer + UBSan.  Host code
only."""
import os
import subprocess

import pytest

from tests.test_sanitizers_cpu import SAN, _build

# (no skip where g++ is missing: the stand-alone sanitizer run is part of the feature's checks, and its absence must show)


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return _build(tmp_path_factory.mktemp("census_check"), "census_check", [os.path.join(SAN, "census_check.cpp")], ["-fsanitize=address,undefined"])


def test_census_format_under_asan_ubsan(exe):
    cp = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert cp.returncode == 0 and cp.stdout.startswith("ok "), cp.stdout + cp.stderr[-2000:]
    assert "ERROR" not in cp.stderr and "runtime error" not in cp.stderr, cp.stderr[-2000:]
