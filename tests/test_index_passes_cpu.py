"""taxor_index_plan_passes (host only): which subtrees of an index larger than the device are searched together.

Hand-written views; every expectation is worked out here from the rule the header states: bytes are rows * stride rounded up to
4 KiB per IXF, the root carries the slab's 4-KiB tail pad, subtrees go in root-bin order into groups that are closed at half of what
the root leaves, and root + group g + group g+1 <= budget."""
import ctypes as C

import numpy as np
import pytest

from taxor_amd import _lib
from taxor_amd.search import GpuIndex, plan_passes

ROOT = _lib.PASS_ROOT
K = 4096


def ixf(bins, seg_len, children=None):
    """children: {bin: child IXF id}; every other bin is a leaf with a user bin of its own (numbered by the caller's view())"""
    stride = (bins + 63) // 64 * 64
    nx = np.zeros(bins, np.int64)
    fn = np.zeros(bins, np.int64)
    for b, c in (children or {}).items():
        nx[b] = c
        fn[b] = -1
    return dict(bins=bins, stride=stride, seg_len=seg_len, seed=1, next_ixf=nx, fname_idx=fn, data=None)


def view(ixfs):
    ub = 0
    for i, f in enumerate(ixfs):
        for b in range(f["bins"]):
            if f["fname_idx"][b] >= 0:
                f["fname_idx"][b] = ub
                f["next_ixf"][b] = i
                ub += 1
    return ixfs, ub


def nbytes(f):
    return (3 * f["seg_len"] * f["stride"] + K - 1) // K * K


def refused(ixfs, n_ub, budget):
    with pytest.raises(_lib.TaxorError) as e:
        plan_passes(ixfs, n_ub, budget)
    assert e.value.code == -1                     # TAXOR_E_ARG
    return _lib.lib().taxor_gpu_last_error().decode()


def five_subtrees():
    """root of 64 bins, merged bins 3, 10, 11, 40, 63 -> subtrees of 1, 2, 3, 4 and 2 units of 12 KiB (IXFs of 64 bins, seg_len 64)"""
    unit = lambda: ixf(64, 64)                    # 3 * 64 rows * 64 B = 12288 B = 3 pages exactly
    fs = [ixf(64, 100, {3: 1, 10: 2, 11: 4, 40: 7, 63: 11})]
    fs += [unit()]                                             # 1
    fs += [ixf(64, 64, {5: 3}), unit()]                        # 2 -> 3
    fs += [ixf(64, 64, {0: 5}), ixf(64, 64, {63: 6}), unit()]  # 4 -> 5 -> 6: three levels deep
    fs += [ixf(64, 64, {1: 8, 2: 9, 3: 10}), unit(), unit(), unit()]   # 7 -> 8, 9, 10
    fs += [ixf(64, 64, {7: 12}), unit()]                       # 11 -> 12
    return view(fs)


def test_everything_fits_is_one_pass():
    fs, n = five_subtrees()
    total = sum(nbytes(f) for f in fs) + K
    for budget in (total, total + 1, 1 << 40):
        plan, of, by = plan_passes(fs, n, budget)
        assert plan["n_passes"] == 1 and plan["n_subtrees"] == 5
        assert plan["root_bytes"] == nbytes(fs[0]) + K and plan["index_bytes"] == total and plan["slab_bytes"] == total
        assert of[0] == ROOT and np.all(of[1:] == 0) and list(by) == [total - plan["root_bytes"]]


def test_group_boundaries_at_the_exact_budget_and_one_byte_below():
    fs, n = five_subtrees()
    U = 12288
    root = nbytes(fs[0]) + K
    sizes = [1 * U, 2 * U, 3 * U, 4 * U, 2 * U]
    assert [sum(nbytes(fs[i]) for i in ids) for ids in ([1], [2, 3], [4, 5, 6], [7, 8, 9, 10], [11, 12])] == sizes
    # one byte short of the whole index (12 U): the root leaves 12 U - 1, half of it is 6 U - 1 (integer division).
    #   g0 = {1 U, 2 U} (adding 3 U would make 6 U > half); g1 = {3 U} (3 + 4 = 7 U > half); g2 = {4 U} (4 + 2 = 6 U > half); g3 = {2 U}
    #   pairs: 3+3, 3+4, 4+2 <= 12 U - 1
    plan, of, by = plan_passes(fs, n, root + 12 * U - 1)
    assert plan["n_passes"] == 4 and list(by) == [3 * U, 3 * U, 4 * U, 2 * U]
    assert list(of) == [ROOT, 0, 0, 0, 1, 1, 1, 2, 2, 2, 2, 3, 3]
    assert plan["slab_bytes"] == root + 7 * U
    # the smallest budget this index can be searched under: the largest subtree (4 U) beside its larger neighbour group.
    #   avail = 7 U, half = 3 U + U/2:  g0 = {1 U, 2 U} (3 U <= half; + 3 U would exceed it), g1 = {3 U}, g2 = {4 U} needs g1 + 4 U = 7 U <= 7 U,
    #   g3 = {2 U}
    need = root + 7 * U
    plan, of, by = plan_passes(fs, n, need)
    assert plan["n_passes"] == 4 and list(by) == [3 * U, 3 * U, 4 * U, 2 * U] and plan["slab_bytes"] == need
    msg = refused(fs, n, need - 1)
    assert "subtree-exceeds-budget" in msg and "root bin 40" in msg and "child IXF 7" in msg and "--tmax" in msg
    # a budget between the two: avail = 8 U, half = 4 U: g0 = {1, 2}, g1 = {3}, g2 = {4}, g3 = {2}: the same groups;
    # avail = 10 U, half = 5 U: g0 = {1 U, 2 U} (+ 3 U = 6 U > 5 U), g1 = {3 U} (+ 4 U > 5 U), g2 = {4 U} (+ 2 U > 5 U), g3 = {2 U}
    plan, _, by = plan_passes(fs, n, root + 10 * U)
    assert list(by) == [3 * U, 3 * U, 4 * U, 2 * U]
    # avail = 11 U + 2 (half = 5 U + U/2 + 1): still 6 U > half for every candidate pair -> the same four groups
    plan, _, by = plan_passes(fs, n, root + 11 * U + 2)
    assert plan["n_passes"] == 4


def test_two_subtrees_share_a_group_when_half_allows_it():
    """sizes 1, 1, 2, 1 (units): avail = 4 -> half = 2: g0 = {1, 1}, g1 = {2}, g2 = {1}; at avail = 4 - 1 byte half = 1 U + U/2 - 1:
    g0 = {1}, g1 = {1}, g2 = {2}, g3 = {1}"""
    U = 12288
    fs, n = view([ixf(64, 10, {0: 1, 1: 2, 2: 3, 3: 5}), ixf(64, 64), ixf(64, 64), ixf(64, 64, {9: 4}), ixf(64, 64), ixf(64, 64)])
    root = nbytes(fs[0]) + K
    plan, of, by = plan_passes(fs, n, root + 4 * U)
    assert plan["n_passes"] == 3 and list(by) == [2 * U, 2 * U, U] and list(of) == [ROOT, 0, 0, 1, 1, 2]
    assert plan["slab_bytes"] == root + 4 * U
    plan, of, by = plan_passes(fs, n, root + 4 * U - 1)
    assert plan["n_passes"] == 4 and list(by) == [U, U, 2 * U, U] and list(of) == [ROOT, 0, 1, 2, 2, 3]
    assert plan["slab_bytes"] == root + 3 * U


def test_root_without_merged_bins():
    fs, n = view([ixf(100, 50)])
    root = nbytes(fs[0]) + K
    plan, of, by = plan_passes(fs, n, root)
    assert plan["n_passes"] == 1 and plan["n_subtrees"] == 0 and plan["slab_bytes"] == root and list(by) == [0] and list(of) == [ROOT]
    msg = refused(fs, n, root - 1)
    assert "root-exceeds-budget" in msg and str(root) in msg and str(root - 1) in msg


def test_chain_three_levels_deep_stays_in_one_group():
    """subtrees of 3 U (a chain root -> 1 -> 2 -> 3), 1 U and 1 U.  avail = 4 U, half = 2 U: the chain is larger than half and is a group of
    its own; g1 = {1 U} is closed by the pair rule (3 + 1 + 1 > 4), g2 = {1 U}.  (Two passes never occur: two groups that fit beside the
    root together are one pass.)"""
    U = 12288
    fs, n = view([ixf(64, 10, {5: 1, 6: 4, 7: 5}), ixf(64, 64, {0: 2}), ixf(64, 64, {0: 3}), ixf(64, 64), ixf(64, 64), ixf(64, 64)])
    root = nbytes(fs[0]) + K
    plan, of, by = plan_passes(fs, n, root + 4 * U)
    assert plan["n_passes"] == 3 and list(of) == [ROOT, 0, 0, 0, 1, 2] and list(by) == [3 * U, U, U]
    assert plan["slab_bytes"] == root + 4 * U
    msg = refused(fs, n, root + 4 * U - 1)                   # the chain beside its neighbour no longer fits
    assert "subtree-exceeds-budget" in msg and "root bin 6" in msg and "child IXF 4" in msg
    msg = refused(fs, n, root + 3 * U - 1)                   # the chain alone no longer fits beside the root
    assert "subtree-exceeds-budget" in msg and "root bin 5" in msg and "child IXF 1" in msg and "--tmax" in msg


def test_refusals_come_before_any_work_and_bad_trees_are_named():
    fs, n = five_subtrees()
    assert "root-exceeds-budget" in refused(fs, n, 1)
    fs2, n2 = view([ixf(64, 10, {0: 1, 1: 1}), ixf(64, 64)])
    assert "referenced twice" in refused(fs2, n2, 1 << 30)
    fs3, n3 = view([ixf(64, 10, {0: 7}), ixf(64, 64)])
    assert "bad child" in refused(fs3, n3, 1 << 30)


def test_plan_makes_no_device_call():
    """the symbol lives in the host-only part of the library: planning works where no GPU exists (this test runs without one)"""
    fs, n = five_subtrees()
    v, keep = GpuIndex._view(fs, n, 22, 12, 5, True, 1, None)
    plan = _lib.PassPlan()
    assert _lib.lib().taxor_index_plan_passes(C.byref(v), 1 << 40, C.byref(plan), None, None) == 0 and plan.n_passes == 1
