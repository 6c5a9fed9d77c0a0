"""The host side of `taxor search --segments-file` (taxor_amd/csrc/segments_format.h: SHAPE and the line formatter) as a stand-alone
program under AddressSanitizer + UBSan, and the Python restatement the GPU tests compare with (tests/segments_expect.py) against its own
brute force: for EVERY matrix x of M <= 3 candidates and n <= 7 hashes and L in {1, 2} the recurrence's value is the greatest value
over all M^n paths.  Host code only.

That is 2^21 matrices of 3^7 paths at the far end, so the two sides are walked in bulk: the recurrence along the tree of column
prefixes with the very step() that viterbi() uses, the brute force path by path with the matrices side by side in numpy.  The returned
PATH is scored from the definition on every matrix up to M * n <= 15 (M = 3: n <= 5; M = 2: n <= 7) and on every 61st of the larger
ones; the plainly written brute() is compared with the bulk one on the same sample."""
import os
import subprocess

import numpy as np
import pytest

from tests import segments_expect as se
from tests.test_sanitizers_cpu import SAN, _build

# (no skip where g++ is missing: the stand-alone sanitizer run is part of the feature's checks, and its absence must show)


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return _build(tmp_path_factory.mktemp("segments_check"), "segments_check", [os.path.join(SAN, "segments_check.cpp")], ["-fsanitize=address,undefined"])


def test_segments_format_under_asan_ubsan(exe):
    cp = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert cp.returncode == 0 and cp.stdout.startswith("ok "), cp.stdout + cp.stderr[-2000:]
    assert "ERROR" not in cp.stderr and "runtime error" not in cp.stderr, cp.stderr[-2000:]


def test_the_shape_equals_the_restatement(exe):
    for bins in ([1, 2], [5, 5], [1, 2, 1], [1, 2, 3], [1, 1, 2], [1, 2, 1, 2], [3, 4, 3, 4, 3], [0, 2**63 - 1, 0]):
        cp = subprocess.run([str(exe)] + [str(b) for b in bins], capture_output=True, text=True, timeout=60)
        assert cp.returncode == 0 and "runtime error" not in cp.stderr, cp.stderr[-2000:]
        assert cp.stdout.strip() == se.shape(bins), bins
    assert se.base(600, 12000, 1200) == 6000 and se.base(3, 10, 3) == 10 and se.base(0, 10, 0) == 0


@pytest.mark.parametrize("M", [1, 2, 3])
def test_the_recurrence_attains_the_brute_force_on_every_matrix(M):
    for n in range(1, 8):
        best = se.brute_all(M, n)
        for L in (1, 2):
            want = se.brute_values(best, L)
            got = se.all_values(M, n, L)
            bad = np.flatnonzero(got != want)
            assert bad.size == 0, (M, n, L, [(int(m), int(got[m]), int(want[m])) for m in bad[:4]])
            every = 1 if M * n <= 15 else 61
            for m in range(0, 1 << (M * n), every):
                x = se.matrix(M, n, m)
                value, path = se.viterbi(x, L)
                assert value == int(want[m]) == se.score(x, path, L), (M, n, L, m)
                if M * n <= 12 or m % (61 * 64) == 0:
                    assert se.brute(x, L) == value, (M, n, L, m)


def test_the_tie_rules_on_matrices_made_by_hand():
    seg = lambda x, L: [(g[0], g[1], g[2]) for g in se.segment(x, L)["segs"]]
    # equal candidates take the lower index, at the end as at a switch
    assert seg([[1, 0, 1], [1, 0, 1]], 1) == [(0, 3, 0)]
    assert seg([[0, 0, 0, 0], [1, 1, 0, 0], [1, 1, 0, 0], [0, 0, 1, 1]], 1) == [(0, 2, 1), (2, 4, 3)]
    assert seg([[0, 0, 1, 1], [0, 0, 1, 1], [1, 1, 0, 0]], 1) == [(0, 2, 2), (2, 4, 0)]
    # a switch that only ties is not taken: one hit gained for a cost of one
    assert seg([[1, 1, 0], [0, 0, 1]], 1) == [(0, 3, 0)] and se.segment([[1, 1, 0], [0, 0, 1]], 1)["hits"] == 2
    assert seg([[1, 1, 0, 0], [0, 0, 1, 1]], 1) == [(0, 2, 0), (2, 4, 1)]                   # two hits for one: taken
    assert seg([[1, 1, 0, 0], [0, 0, 1, 1]], 2) == [(0, 4, 0)]                             # two hits for two: a tie, not taken
    assert seg([[1, 0, 1, 0, 1, 0], [0, 1, 0, 1, 0, 1]], 1) == [(0, 6, 0)]                 # alternation at every hash
    # A | nothing | B: every boundary in the empty stretch scores the same.  Through the stretch V_B rides on J, which stands still, so
    # sw_B ties and stays unset there: the last set bit, the boundary, is the stretch's first position
    A, B = [1] * 5 + [0] * 3 + [0] * 5, [0] * 5 + [0] * 3 + [1] * 5
    assert seg([A, B], 2) == [(0, 5, 0), (5, 13, 1)]
    g = se.segment([A, B], 2)
    assert (g["hits"], g["K"], g["single"], g["best"]) == (10, 2, 5, 0) and [s[3] for s in g["segs"]] == [5, 5] and [s[4] for s in g["segs"]] == [5, 0]
    # A|B|A and A|B|C, and the shapes from user bins alone
    assert seg([[1, 1, 1, 0, 0, 0, 1, 1, 1], [0, 0, 0, 1, 1, 1, 0, 0, 0]], 1) == [(0, 3, 0), (3, 6, 1), (6, 9, 0)]
    assert seg([[1, 1, 0, 0, 0, 0], [0, 0, 1, 1, 0, 0], [0, 0, 0, 0, 1, 1]], 1) == [(0, 2, 0), (2, 4, 1), (4, 6, 2)]
    assert (se.shape([4, 9]), se.shape([4, 9, 4]), se.shape([4, 9, 5]), se.shape([4, 4, 9]), se.shape([4, 9, 4, 9])) == ("split", "insert", "mosaic", "mosaic", "mosaic")
