"""The BAM reader (taxor_amd/csrc/bam.h) as a stand-alone program under AddressSanitizer + UBSan: whole files in every block shape,
the malformed ones, and the inflated stream of one file cut at every byte of its header and first two records."""
import os
import shutil
import subprocess

import pytest

from tests import bam_writer as bw
from tests.test_bam_reader_cpu import EXTRAS, MALFORMED, make_reads
from tests.test_fastx_reader_cpu import fnv1a
from tests.test_sanitizers_cpu import SAN, _build

pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")


def _clean(cp):
    assert cp.returncode == 0, cp.stdout + cp.stderr[-2000:]
    assert "ERROR" not in cp.stderr and "runtime error" not in cp.stderr, cp.stderr[-2000:]


def test_bam_reader_under_asan_ubsan(tmp_path):
    exe = _build(tmp_path, "bam_read", [os.path.join(SAN, "bam_read.cpp")], ["-fsanitize=address,undefined", "-ldl"])
    reads = make_reads()
    sel = bw.selected(reads)
    h = 1469598103934665603
    for _, s in sel:
        for c in s:
            h = ((h ^ c) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
    assert fnv1a(b"".join(s for _, s in sel)) == h
    want = "%d records %d bases %d skipped fnv %016x" % (len(sel), sum(len(s) for _, s in sel), len(reads) - len(sel), h)
    for blocking, block, eof in (("record", 0, True), ("bytes", 300, True), ("one", 0, True), ("bytes", 300, False)):
        p = tmp_path / f"{blocking}{int(eof)}.bam"
        bw.write_bam(p, reads, blocking=blocking, block=block, eof=eof, extras=EXTRAS, spare=0xF)
        cp = subprocess.run([str(exe), str(p)], capture_output=True, text=True, timeout=300)
        _clean(cp)
        assert cp.stdout.split("\n")[:2] == [want, want], cp.stdout
    for case in sorted(MALFORMED):
        p = tmp_path / "bad.bam"
        p.write_bytes(bw.bgzf(MALFORMED[case][0], block=97))
        cp = subprocess.run([str(exe), str(p)], capture_output=True, text=True, timeout=300)
        _clean(cp)
        lines = cp.stdout.split("\n")[:2]
        assert all(l.startswith("error: ") and MALFORMED[case][2] in l for l in lines), (case, cp.stdout)
    # every truncation of the header and the first two records: an error, except at the three places where the stream may end
    p = tmp_path / "cut.bam"
    bw.write_bam(p, reads[1:], extras={2: EXTRAS[3]})
    cp = subprocess.run([str(exe), str(p), "truncate"], capture_output=True, text=True, timeout=600)
    _clean(cp)
    n = len(bw.header()) + len(bw.record(*reads[1])) + len(bw.record(*reads[2])) + 1
    assert cp.stdout.strip() == f"{n} cuts: 3 clean ends, {n - 3} errors", cp.stdout
