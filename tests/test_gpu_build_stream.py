"""Construction with a bounded part of the keys on the device (taxor_gpu_index_build_hixf_stream, _build_ixf_bins, taxor_gpu_keys_union;
DESIGN.md section 9, "Beyond device memory").  The columns of an IXF are a function of its bins' key sets and its seed, so the bar is
identity: every IXF's bytes and every IXF's seed equal what taxor_gpu_index_build_hixf leaves on the same keys and seed0, whatever the
budget cuts the work into.  Nothing here carries a tolerance."""
import ctypes as C
import re
import time

import numpy as np
import pytest

from taxor_amd import GpuIndex, _lib, synth
from taxor_amd._lib import TaxorError, check
from taxor_amd.genome_keys import keys_union

pytestmark = pytest.mark.gpu
SEED0 = 0x5EED5EED


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def _mixed(b):
    """bins of 0, 1, ~500 and ~20 000 keys"""
    return 20000 + b if b % 16 == 5 else 0 if b % 7 == 3 else 1 if b % 5 == 0 else 480 + b


def _small(b):
    return 3000 if b == 9 else 0 if b % 11 == 4 else 1 if b % 6 == 0 else 250 + b


class Shape:
    """A hierarchy of 64-bin IXFs with leaf key lists from taxor_synth_key: neighbouring bins share a quarter of their keys, so a merged
    bin's union is smaller than the sum below it.  tree[i] = {bin: child}; sizes(i, b) = keys of leaf bin b of IXF i."""

    def __init__(self, tree, sizes, salt):
        self.tree, self.n_ixf = tree, len(tree)
        nxt, self.leaf, below = 0, {}, [None] * self.n_ixf
        for i in range(self.n_ixf):
            for b in range(64):
                if b in tree[i]:
                    continue
                n = sizes(i, b)
                self.leaf[(i, b)] = synth.synth_keys_host(nxt, n, salt)
                nxt += max(1, n * 3 // 4)
        for i in reversed(range(self.n_ixf)):                # children have larger ids than their parents
            parts = [below[tree[i][b]] if b in tree[i] else self.leaf[(i, b)] for b in range(64)]
            below[i] = np.unique(np.concatenate(parts))
        self.below = below
        self.ixfs = []
        for i in range(self.n_ixf):
            mx = max([1] + [below[tree[i][b]].size if b in tree[i] else self.leaf[(i, b)].size for b in range(64)])
            self.ixfs.append(dict(bins=64, stride=64, seg_len=synth.seg_len_for(mx), seed=1,
                                  next_ixf=np.array([tree[i].get(b, i) for b in range(64)], np.int64),
                                  fname_idx=np.array([-1 if b in tree[i] else 64 * i + b for b in range(64)], np.int64), data=None))
        lists = [self.leaf.get((i, b), np.zeros(0, np.uint64)) for i in range(self.n_ixf) for b in range(64)]
        self.off = np.zeros(len(lists) + 1, np.uint64)
        np.cumsum([l.size for l in lists], out=self.off[1:])
        self.keys = np.concatenate(lists)
        self.input = [sum(below[tree[i][b]].size if b in tree[i] else self.leaf[(i, b)].size for b in range(64)) for i in range(self.n_ixf)]
        self.root_bins = [below[tree[0][b]].size if b in tree[0] else self.leaf[(0, b)].size for b in range(64)]
        self._ref = None

    def index(self):
        idx = GpuIndex(self.ixfs, 64 * self.n_ixf)
        for i in range(self.n_ixf):
            idx.fill_random(i, 77 + i)                       # bins without keys and the padding keep this
        return idx

    def reference(self):
        """what the resident path leaves: computed once, shared, never changed"""
        if self._ref is None:
            idx = self.index()
            rounds = C.c_uint32()
            check(_lib.lib().taxor_gpu_index_build_hixf(idx._h, _p(self.keys), _p(self.off), SEED0, C.byref(rounds)))
            self._ref = ([idx.download_ixf(i) for i in range(self.n_ixf)], [idx.ixf_seed(i) for i in range(self.n_ixf)])
            idx.close()
        return self._ref

    def ranges(self, budget_keys):
        """bin ranges the root is cut into: bins join a range while its keys fit"""
        n, k = 1, 0
        for s in self.root_bins:
            if k + s > budget_keys:
                n, k = n + 1, 0
            k += s
        return n

    def budget_for_ranges(self, want):
        for bk in range(max(self.root_bins), self.input[0]):
            if self.ranges(bk) == want:
                return bk
        raise AssertionError(f"no budget cuts the root into {want} ranges")


def _three_level():
    return Shape([{0: 1, 1: 2}, {2: 3, 40: 4}, {}, {}, {}], lambda i, b: _mixed(b) if i == 0 else _small(b + i), salt=3)


SHAPES = {
    "flat": lambda: Shape([{}], lambda i, b: _mixed(b), salt=1),
    "flat-uniform": lambda: Shape([{}], lambda i, b: 500, salt=4),
    # (one larger bin sizes the IXF: 32 bins filled to the last row would not all peel under any of 32 seeds)
    "flat-alternating-empty": lambda: Shape([{}], lambda i, b: 0 if b % 2 else 1400 if b == 0 else 1000, salt=5),
    "two-level": lambda: Shape([{b: 1 + b for b in range(8)}] + [{}] * 8, lambda i, b: _mixed(b) if i == 0 else _small(b + i), salt=2),
    "three-level": _three_level,
    # children larger than any bin of the root: a budget can lie between the two
    "large-children": lambda: Shape([{0: 1, 1: 2}, {}, {}], lambda i, b: _small(b) if i == 0 else _mixed(b), salt=6),
}
_cache = {}


def shape(name):
    if name not in _cache:
        _cache[name] = SHAPES[name]()
    return _cache[name]


def stream_equals_resident(sh, budget_bytes):
    want, seeds = sh.reference()
    idx = sh.index()
    st = idx.build_hixf_stream(sh.keys, sh.off, budget_bytes, SEED0)
    try:
        for i in range(sh.n_ixf):
            assert idx.ixf_seed(i) == seeds[i], f"seed of IXF {i}"
            assert np.array_equal(idx.download_ixf(i), want[i]), f"bytes of IXF {i}"
    finally:
        idx.close()
    return st


@pytest.mark.parametrize("name", list(SHAPES))
def test_one_group_per_level(name):
    sh = shape(name)
    st = stream_equals_resident(sh, 1 << 40)
    levels = 1 + (sh.n_ixf > 1) + (name == "three-level")                   # one group per level
    assert st["stream_groups"] == levels and st["stream_ranges"] == 0
    assert st["stream_bytes_uploaded"] == 8 * sum(sh.input)


@pytest.mark.parametrize("name", ["two-level", "three-level"])
def test_many_groups_per_level_and_a_ranged_root(name):
    sh = shape(name)
    budget_keys = max(max(sh.input[1:]), max(sh.root_bins))          # one child's subtree at a time
    assert sh.input[0] > budget_keys
    st = stream_equals_resident(sh, 8 * budget_keys)
    assert st["stream_groups"] >= (8 if name == "two-level" else 3) and st["stream_ranges"] == sh.ranges(budget_keys) >= 2


@pytest.mark.parametrize("name,want", [("flat", 2), ("flat", 3), ("two-level", 2), ("two-level", 3), ("flat-uniform", 64), ("flat-alternating-empty", 32)])
def test_root_in_bin_ranges(name, want):
    """the root cut into 2, 3 and 64 ranges (a budget of one bin's keys), and range edges beside empty bins"""
    sh = shape(name)
    budget_keys = max(sh.root_bins) if want >= 32 else sh.budget_for_ranges(want)
    if name == "two-level":
        budget_keys = max(budget_keys, max(sh.input[1:]))
    assert sh.ranges(budget_keys) == want
    st = stream_equals_resident(sh, 8 * budget_keys)
    assert st["stream_ranges"] == want       # (restarts happen where the resident path reseeds too: the seeds are compared above)


def test_budget_below_a_childs_subtree_names_the_ixf():
    sh = shape("large-children")
    budget_keys = max(sh.input[1:]) - 1
    assert budget_keys >= max(sh.root_bins)
    idx = sh.index()
    with pytest.raises(TaxorError) as e:
        idx.build_hixf_stream(sh.keys, sh.off, 8 * budget_keys, SEED0)
    m = re.search(r"subtree of IXF (\d+) brings (\d+) keys", str(e.value))
    assert e.value.code == -1 and m and sh.input[int(m.group(1))] == int(m.group(2)) > budget_keys, str(e.value)
    idx.close()


def test_a_bin_of_2_to_32_declared_keys_is_refused_by_name():
    """offsets only: no memory stands behind them, so the calls must return before they read a key"""
    sh = shape("flat")
    idx = sh.index()
    off = np.zeros(65, np.uint64)
    off[8:] = 2**32 - 1                                              # bin 7
    dummy = np.zeros(8, np.uint64)
    with pytest.raises(TaxorError) as e:
        idx.build_hixf_stream(dummy, off, 1 << 20, SEED0)
    assert e.value.code == -1 and "bin 7 of IXF 0" in str(e.value) and "4294967295" in str(e.value)
    with pytest.raises(TaxorError) as e:
        idx.build_ixf_bins(0, 0, 64, dummy, off, SEED0)
    assert e.value.code == -1 and "bin 7 of IXF 0" in str(e.value)
    with pytest.raises(TaxorError):
        idx.build_ixf_bins(0, 3, 65, dummy, np.zeros(65, np.uint64), SEED0)
    idx.close()


@pytest.mark.parametrize("cut", [1, 63, 10])                        # (bin 10 of the mixed shape is empty: 10 % 7 == 3)
def test_build_ixf_bins_in_two_calls_equals_one(cut):
    sh = shape("flat")
    assert sh.root_bins[10] == 0
    _, seeds = sh.reference()
    one, two = sh.index(), sh.index()
    assert one.build_ixf_bins(0, 0, 64, sh.keys, sh.off, seeds[0])
    assert two.build_ixf_bins(0, 0, cut, sh.keys, sh.off, seeds[0]) and two.build_ixf_bins(0, cut, 64, sh.keys, sh.off, seeds[0])
    a, b = one.download_ixf(0), two.download_ixf(0)
    assert np.array_equal(a, b) and np.array_equal(a, sh.reference()[0][0])
    assert one.ixf_seed(0) == two.ixf_seed(0) == seeds[0]
    one.close()
    two.close()


def test_build_ixf_bins_clear_flags():
    """an IXF all of whose bins have keys is cleared as a whole, once: first call CLEAR, later calls CLEARED"""
    sh = shape("flat-uniform")
    want, seeds = sh.reference()
    idx = sh.index()
    assert idx.build_ixf_bins(0, 0, 20, sh.keys, sh.off, seeds[0], _lib.BINS_CLEAR)
    assert idx.build_ixf_bins(0, 20, 64, sh.keys, sh.off, seeds[0], _lib.BINS_CLEARED)
    assert np.array_equal(idx.download_ixf(0), want[0])
    idx.close()


def test_reseed_ends_on_the_same_seed_and_bytes():
    """a bin filled to the last row fails to peel under many seeds: one such (keys, seed) pair, found on the
    CPU, sits in a late bin range -- the stream path starts the IXF again from bin 0 under the next seed, like the resident path"""
    L = _lib.lib()
    seg = 14
    n = int(3 * seg / 1.23)
    col = np.zeros(3 * seg, np.uint8)
    found, t_end = None, time.monotonic() + 1.0
    salt = 100
    while found is None and time.monotonic() < t_end:
        ks = synth.synth_keys_host(0, n, salt)
        if L.taxor_ixf_build_bin(_p(ks), n, SEED0, seg, _p(col)) == 1:
            found = ks
        salt += 1
    if found is None:
        pytest.skip("no non-peeling (keys, seed) pair found on the CPU within a second")
    lists = [found if b == 50 else synth.synth_keys_host(1000 * b, 12, 7) for b in range(64)]
    off = np.zeros(65, np.uint64)
    np.cumsum([l.size for l in lists], out=off[1:])
    keys = np.concatenate(lists)
    ixf = dict(bins=64, stride=64, seg_len=seg, seed=1, next_ixf=np.zeros(64, np.int64), fname_idx=np.arange(64), data=None)
    res, stream = GpuIndex([ixf], 64), GpuIndex([ixf], 64)
    rounds = C.c_uint32()
    check(L.taxor_gpu_index_build_hixf(res._h, _p(keys), _p(off), SEED0, C.byref(rounds)))
    st = stream.build_hixf_stream(keys, off, 8 * 100, SEED0)
    assert st["stream_ranges"] >= 8 and st["stream_restarts"] >= 1
    assert stream.ixf_seed(0) == res.ixf_seed(0) != SEED0
    assert np.array_equal(stream.download_ixf(0), res.download_ixf(0))
    res.close()
    stream.close()


MARK = np.uint64(2**64 - 1)


def _lists(case):
    a = synth.synth_keys_host(0, 5000, 9)
    b = synth.synth_keys_host(5000, 3000, 9)
    m = np.array([MARK], np.uint64)
    return {
        "disjoint": [a, b],
        "identical": [a, a.copy(), a[::-1].copy()],
        "nested": [a, a[1000:2000], a[:10]],
        "with-an-empty-list": [a[:100], np.zeros(0, np.uint64), b[:50]],
        "all-empty": [np.zeros(0, np.uint64)] * 2,
        "marker-in-one": [a[:700], np.concatenate([b[:300], m])],
        "marker-in-all": [np.concatenate([m, a[:700]]), np.concatenate([a[300:900], m]), m],
        "more-than-one-launch-block": [synth.synth_keys_host(0, 70001, 11), synth.synth_keys_host(35000, 70001, 11)],
    }[case]


@pytest.mark.parametrize("on_device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("case", ["disjoint", "identical", "nested", "with-an-empty-list", "all-empty", "marker-in-one", "marker-in-all",
                                  "more-than-one-launch-block"])
def test_keys_union_against_numpy(case, on_device):
    lists = _lists(case)
    want = np.zeros(0, np.uint64)
    for l in lists:
        want = np.union1d(want, l)
    n, got = keys_union(lists, on_device=on_device)
    assert n == want.size and np.array_equal(got, want)
    assert keys_union(lists, want_keys=False, on_device=on_device) == (want.size, None)


def test_keys_union_output_too_small():
    a = synth.synth_keys_host(0, 100, 1)
    ptrs = (C.c_void_p * 1)(a.ctypes.data)
    cnt = np.array([100], np.uint64)
    out = np.zeros(10, np.uint64)
    n = C.c_uint64()
    assert _lib.lib().taxor_gpu_keys_union(0, ptrs, _p(cnt), 1, 0, _p(out), 0, 10, C.byref(n)) == -1
    assert n.value == 100 and not out.any()
