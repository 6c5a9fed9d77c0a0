"""The host side of `taxor search --exclusive-file` / `--exclusive-reads-file` (taxor_amd/csrc/exclusive_format.h: the fraction, the
rounded distinct count and the two line formatters) as a stand-alone program under AddressSanitizer + UBSan, and the fraction against the
Python restatement the GPU tests compare with (tests/exclusive_expect.py formats it with "%.4f").  Host code only."""
import os
import subprocess

import pytest

from tests import exclusive_expect as xe
from tests.test_sanitizers_cpu import SAN, _build

# (no skip where g++ is missing: the stand-alone sanitizer run is part of the feature's checks, and its absence must show)


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return _build(tmp_path_factory.mktemp("exclusive_check"), "exclusive_check", [os.path.join(SAN, "exclusive_check.cpp")], ["-fsanitize=address,undefined"])


def test_exclusive_format_under_asan_ubsan(exe):
    cp = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert cp.returncode == 0 and cp.stdout.startswith("ok "), cp.stdout + cp.stderr[-2000:]
    assert "ERROR" not in cp.stderr and "runtime error" not in cp.stderr, cp.stderr[-2000:]


def test_the_fraction_equals_the_restatement(exe):
    for e, h in ((0, 0), (0, 9), (1, 3), (2, 3), (1, 20000), (1, 20001), (3, 20000), (5, 80000), (12345, 67891), (2**64 - 2, 2**64 - 1), (7, 7)):
        cp = subprocess.run([str(exe), str(e), str(h)], capture_output=True, text=True, timeout=60)
        assert cp.returncode == 0 and "runtime error" not in cp.stderr, cp.stderr[-2000:]
        assert cp.stdout.strip() == "%.4f" % (e / h if h else 0.0), (e, h)


def test_the_restatements_own_identities_refuse_a_wrong_matrix():
    """exclusive() asserts the header's identities on every read; a matrix by hand gives the counts one expects"""
    hits, excl, shared, matched, own = xe.exclusive([[1, 1, 0, 0, 1], [0, 1, 0, 1, 0], [0, 1, 0, 0, 0]])
    assert (hits, excl, shared, matched, own) == ([3, 2, 1], [2, 1, 0], 1, 4, [[0, 4], [3], []])
    hits, excl, shared, matched, own = xe.exclusive([[1, 0, 1]])
    assert (hits, excl, shared, matched) == ([2], [2], 0, 2)
    hits, excl, shared, matched, own = xe.exclusive([[1, 0, 1], [1, 0, 1]])          # a user bin in two tuples: nothing is exclusive
    assert (hits, excl, shared, matched) == ([2, 2], [0, 0], 2, 2)
