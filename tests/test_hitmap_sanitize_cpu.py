"""The host side of `taxor search --hitmap-file` (taxor_amd/csrc/hitmap_format.h: the segment of a hash, the size of a segment, the line
formatter) as a stand-alone program under AddressSanitizer + UBSan, and its two functions against the Python restatement the GPU tests
compare with (tests/hitmap_expect.py).  Host code only."""
import os
import shutil
import subprocess

import pytest

from tests.hitmap_expect import seg, size
from tests.test_sanitizers_cpu import SAN, _build

pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")


def test_hitmap_format_under_asan_ubsan(tmp_path):
    exe = _build(tmp_path, "hitmap_check", [os.path.join(SAN, "hitmap_check.cpp")], ["-fsanitize=address,undefined"])
    cp = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert cp.returncode == 0 and cp.stdout.startswith("ok "), cp.stdout + cp.stderr[-2000:]
    assert "ERROR" not in cp.stderr and "runtime error" not in cp.stderr, cp.stderr[-2000:]


def test_the_python_restatement_agrees_with_itself():
    """size(j) counts the hashes seg() puts into segment j, and the sizes sum to the read's count"""
    for S in (1, 2, 3, 16, 63, 64):
        for n in (1, 2, 15, 16, 17, 63, 64, 65, 2048, 2049, 5245):
            cnt = [0] * S
            for i in range(n):
                cnt[seg(i, S, n)] += 1
            assert cnt == [size(j, S, n) for j in range(S)] and sum(cnt) == n, (S, n)
