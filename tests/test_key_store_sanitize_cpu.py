"""The host side of a build beyond device memory (taxor_amd/csrc/key_store.h: the key store, the parts' offsets, the cut into waves, the
refusals) as a stand-alone program under AddressSanitizer + UBSan."""
import os
import shutil
import subprocess

import pytest

from tests.test_sanitizers_cpu import SAN, _build

pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")


def test_key_store_under_asan_ubsan(tmp_path):
    exe = _build(tmp_path, "key_store_check", [os.path.join(SAN, "key_store_check.cpp")], ["-fsanitize=address,undefined"])
    mem = tmp_path / "meminfo"
    mem.write_text("MemTotal:       999999 kB\nMemFree:        1 kB\nMemAvailable:   123456 kB\nBuffers:        5 kB\n")
    cp = subprocess.run([str(exe), str(mem)], capture_output=True, text=True, timeout=300)
    assert cp.returncode == 0 and cp.stdout.startswith("ok "), cp.stdout + cp.stderr[-2000:]
    assert "ERROR" not in cp.stderr and "runtime error" not in cp.stderr, cp.stderr[-2000:]
