"""The host side of `taxor search --breakpoint-file` (taxor_amd/csrc/breakpoint_format.h: the approximate base position of a break, the
line formatter) as a stand-alone program under AddressSanitizer + UBSan, and its base-position function against the Python restatement
the GPU tests compare with (tests/breakpoint_expect.py).  Host code only."""
import os
import subprocess

import pytest

from tests import breakpoint_expect as be
from tests.test_sanitizers_cpu import SAN, _build

# (no skip where g++ is missing: the stand-alone sanitizer run is part of the feature's checks, and its absence must show)


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return _build(tmp_path_factory.mktemp("breakpoint_check"), "breakpoint_check", [os.path.join(SAN, "breakpoint_check.cpp")], ["-fsanitize=address,undefined"])


def test_breakpoint_format_under_asan_ubsan(exe):
    cp = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert cp.returncode == 0 and cp.stdout.startswith("ok "), cp.stdout + cp.stderr[-2000:]
    assert "ERROR" not in cp.stderr and "runtime error" not in cp.stderr, cp.stderr[-2000:]


def test_the_base_position_equals_the_restatement(exe):
    triples = [(p, L, n) for n in (1, 2, 63, 64, 65, 2048, 2049, 5245, 2**32 - 1) for L in (0, 1, 22, 1200, 12000, 2**31 - 1, 2**40 + 7, 2**64 - 1)
               for p in sorted({0, 1 % n, n // 3, n // 2, n - 1})]
    cp = subprocess.run([str(exe)] + [str(v) for t in triples for v in t], capture_output=True, text=True, timeout=300)
    assert cp.returncode == 0 and "runtime error" not in cp.stderr, cp.stderr[-2000:]
    assert [int(x) for x in cp.stdout.split()] == [be.base(*t) for t in triples]
    assert be.base(1024, 12000, 2048) == 6000 and be.base(5, 1000, 0) == 0


def test_the_restatement_of_the_split_follows_the_tie_rules():
    s = be.best_split([[1, 1, 0, 0, 0], [0, 0, 0, 1, 1]])                     # split(2) = split(3) = 4: the smaller p
    assert (s["p"], s["gain"], s["A"], s["B"], s["pre_a"], s["suf_b"], s["pre_b"], s["suf_a"], s["single"], s["best"]) == (2, 2, 0, 1, 2, 2, 0, 0, 2, 0)
    s = be.best_split([[1, 0, 1], [1, 0, 1], [0, 1, 0]])                      # equal candidates: the lower index, everywhere
    assert (s["A"], s["B"], s["best"]) == (0, 0, 0) and s["gain"] == 0 and s["p"] == 0
    s = be.best_split([[1, 1, 1, 1], [1, 1, 0, 0]])                           # one dominates: no gain, the break stays at 0
    assert (s["gain"], s["p"], s["single"]) == (0, 0, 4)
