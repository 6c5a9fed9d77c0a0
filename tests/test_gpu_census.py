"""Nonzero fingerprint bytes per bin of a resident index (taxor_gpu_census_*, taxor_amd/csrc/census.hip): every word EQUALS
numpy.count_nonzero per column of the bytes taxor_gpu_index_download_ixf returns -- over IXFs of every stride class with padding
columns, rows 3, 255 and 258, and one 64-bin IXF of 70 002 rows whose packed byte counters must flush -- for the default cut and for
cuts and grids that share nothing with it; two calls give the same words.  On an index the device builder made, every bin's count
obeys nonzero <= n and the five-sigma bound of the binomial against its true key count (leaf bins) or union size (merged bins)."""
import numpy as np
import pytest

from taxor_amd import GpuIndex, _lib, synth
from taxor_amd.search import census_capacity, census_keys_est, census_peeled
from tests import census_expect as ce

pytestmark = pytest.mark.gpu

# (bins, seg_len): the root first -- its merged bins 0 .. 6 lead to the others.  Strides 1088, 64, 64, 64, 128, 1024, 64, 1088
SHAPES = [(1025, 86), (1, 1), (63, 85), (64, 86), (65, 1), (1000, 85), (64, 23334), (1025, 1)]
LONG = 6


def _shapes():
    out, ub = [], 0
    for i, (bins, seg) in enumerate(SHAPES):
        fn = np.arange(ub, ub + bins, dtype=np.int64)
        nx = np.full(bins, i, dtype=np.int64)
        if i == 0:
            fn[:len(SHAPES) - 1] = -1
            nx[:len(SHAPES) - 1] = np.arange(1, len(SHAPES))
        ub += bins
        out.append(dict(bins=bins, stride=(bins + 63) // 64 * 64, seg_len=seg, seed=1 + i, next_ixf=nx, fname_idx=fn, data=None))
    return out, ub


@pytest.fixture(scope="module")
def world():
    """the index, its bytes as the device holds them and their column counts (computed once), and the default census"""
    shapes, ub = _shapes()
    assert [f["stride"] for f in shapes] == [1088, 64, 64, 64, 128, 1024, 64, 1088] and 3 * SHAPES[LONG][1] >= 70000
    idx = GpuIndex(shapes, ub)
    for i in range(len(shapes)):
        idx.fill_random(i, 1000 + i)
    rows = lambda i: 3 * SHAPES[i][1]
    first, last = np.zeros(rows(0), np.uint8), np.zeros(rows(0), np.uint8)
    first[0], last[-1] = 7, 0x80
    idx.upload_bin(0, 9, np.zeros(rows(0), np.uint8))              # all zero
    idx.upload_bin(0, 10, np.full(rows(0), 0xFF, np.uint8))        # all 0xFF
    idx.upload_bin(0, 1023, first)                                 # nonzero only in the first row
    idx.upload_bin(0, 1024, last)                                  # nonzero only in the last row, in the last bin before the padding
    for b in range(64):                                            # IXF 4: nonzero only in the last bin before the padding
        idx.upload_bin(4, b, np.zeros(rows(4), np.uint8))
    idx.upload_bin(4, 64, np.full(rows(4), 0x01, np.uint8))
    lfirst, llast = np.zeros(rows(LONG), np.uint8), np.zeros(rows(LONG), np.uint8)
    lfirst[0], llast[-1] = 1, 1
    idx.upload_bin(LONG, 0, lfirst)
    idx.upload_bin(LONG, 63, llast)
    idx.upload_bin(LONG, 31, np.full(rows(LONG), 0xFF, np.uint8))  # 70 002 nonzero bytes in one column: past 255 many times over
    idx.upload_bin(LONG, 32, np.zeros(rows(LONG), np.uint8))
    data = [idx.download_ixf(i).reshape(rows(i), shapes[i]["stride"]) for i in range(len(shapes))]
    want = [np.count_nonzero(d[:, :f["bins"]], axis=0).astype(np.uint64) for d, f in zip(data, shapes)]
    for d, f in zip(data, shapes):                                 # the padding columns are there, and they are not zero
        assert f["stride"] == f["bins"] or np.count_nonzero(d[:, f["bins"]:]) > 0
    table = idx.census(runs=2)
    yield dict(idx=idx, shapes=shapes, want=want, table=table, n_user_bins=ub)
    idx.close()


def _same(table, want):
    assert table.nonzero.dtype == np.uint64 and table.nonzero.size == sum(w.size for w in want)
    assert list(table.bin_first) == list(np.cumsum([0] + [w.size for w in want]))
    for x, w in enumerate(want):
        got = table.of_ixf(x)
        assert np.array_equal(got, w), (x, np.flatnonzero(got != w)[:8], got[got != w][:8], w[got != w][:8])


def test_every_word_equals_count_nonzero_and_two_calls_agree(world):
    w = world
    _same(w["table"], w["want"])
    assert np.array_equal(w["table"].all_runs[0], w["table"].all_runs[1])
    want = w["want"]
    assert want[0][9] == 0 and want[0][10] == 258 and want[0][1023] == 1 and want[0][1024] == 1
    assert list(want[4][:64]) == [0] * 64 and want[4][64] == 3
    assert want[LONG][0] == 1 and want[LONG][63] == 1 and want[LONG][31] == 70002 and want[LONG][32] == 0
    assert w["table"].bytes_read == sum(3 * f["seg_len"] * f["stride"] for f in w["shapes"]) and w["table"].seconds_kernel > 0 and w["table"].launches == 1


@pytest.mark.parametrize("tile_iters,max_blocks", [(1, 3), (7, 1), (251, 100000), (252, 5), (253, 64), (100000, 2048)])
def test_the_words_do_not_depend_on_the_cut_or_the_grid(world, tile_iters, max_blocks):
    t = world["idx"].census(tile_iters=tile_iters, max_blocks=max_blocks)
    _same(t, world["want"])
    assert t.n_tiles != world["table"].n_tiles


def test_a_random_filled_ixf_is_flagged(world):
    w = world
    for x in (0, 5, LONG):
        seg = w["shapes"][x]["seg_len"]
        nz = w["table"].of_ixf(x)
        filled = [j for j in range(nz.size) if int(w["want"][x][j]) > 3 * seg * 0.9]       # the columns fill_random left as they were
        assert len(filled) >= nz.size - 8
        assert not any(census_peeled(int(nz[j]), seg) for j in filled)
    c = ce.Census(w["shapes"], [w["table"].of_ixf(x) for x in range(len(w["shapes"]))], w["n_user_bins"])
    assert c.ixf[LONG][5] is None and c.index_hashes[int(w["shapes"][LONG]["fname_idx"][5])] is None
    assert c.index_hashes[int(w["shapes"][LONG]["fname_idx"][32])] == 0                    # the zero column is a peeled (empty) filter


def test_a_paged_index_is_refused_by_name():
    rng = np.random.default_rng(3)
    nx, fn = np.array([1, 0, 0, 0], dtype=np.int64), np.array([-1, 0, 1, 2], dtype=np.int64)
    host = [dict(bins=4, stride=64, seg_len=64, seed=1, next_ixf=nx, fname_idx=fn, data=rng.integers(0, 256, 3 * 64 * 64, dtype=np.uint8)),
            dict(bins=4, stride=64, seg_len=64, seed=2, next_ixf=np.full(4, 1, np.int64), fname_idx=np.array([3, 4, 5, 6], np.int64),
                 data=rng.integers(0, 256, 3 * 64 * 64, dtype=np.uint8))]
    paged = GpuIndex.paged(host, 7, 4 * sum(f["data"].size + 8192 for f in host))
    with pytest.raises(_lib.TaxorError) as ei:
        paged.census()
    assert ei.value.code == -1 and "paged index" in str(ei.value)
    paged.close()


def test_an_index_of_the_device_builder_obeys_the_binomial_bound():
    """root: user bin 0 split over bins 0 and 1, a leaf, a merged bin -> child; child: a leaf, a merged bin -> grandchild, leaves;
    every leaf bin holds synthetic keys.  Leaf bins against their key counts, merged bins against their union sizes"""
    sizes = {(0, 0): 1500, (0, 1): 1499, (0, 2): 8000, (0, 4): 1, (0, 5): 37,
             (1, 0): 3000, (1, 2): 500, (1, 3): 2, (1, 4): 1200,
             (2, 0): 700, (2, 1): 2500, (2, 2): 90}
    leaf, at = {}, 0
    for key, n in sizes.items():
        leaf[key] = synth.synth_keys_host(at, n, 99)
        at += n
    assert np.unique(np.concatenate(list(leaf.values()))).size == at
    n_of = dict(sizes)
    n_of[(1, 1)] = sum(n for (i, _), n in sizes.items() if i == 2)                      # the grandchild's union
    n_of[(0, 3)] = sum(n for (i, _), n in sizes.items() if i == 1) + n_of[(1, 1)]       # the child's, the grandchild included
    fn = [np.array([0, 0, 1, -1, 2, 3], np.int64), np.array([4, -1, 5, 6, 7], np.int64), np.array([8, 9, 10], np.int64)]
    nx = [np.array([0, 0, 0, 1, 0, 0], np.int64), np.array([1, 2, 1, 1, 1], np.int64), np.array([2, 2, 2], np.int64)]
    shapes = [dict(bins=len(fn[i]), stride=64, seg_len=synth.seg_len_for(max(n for (x, _), n in n_of.items() if x == i)), seed=7 + i, next_ixf=nx[i], fname_idx=fn[i], data=None)
              for i in range(3)]
    idx = GpuIndex(shapes, 11)
    idx.build_hixf(leaf, seed0=11)
    t = idx.census()
    data = [idx.download_ixf(i).reshape(3 * shapes[i]["seg_len"], 64) for i in range(3)]
    idx.close()
    for (x, j), n in sorted(n_of.items()):
        nz = int(t.of_ixf(x)[j])
        est = census_keys_est(nz)
        print(f"IXF {x} bin {j}: n={n} nonzero={nz} keys_est={est} bound={ce.bound(n):.2f}")
        assert nz == np.count_nonzero(data[x][:, j])
        assert nz <= n, (x, j)
        assert abs(est - n) <= ce.bound(n), (x, j, n, est)
        assert census_peeled(nz, shapes[x]["seg_len"]) and n <= census_capacity(shapes[x]["seg_len"])
    c = ce.Census(shapes, [t.of_ixf(x) for x in range(3)], 11)
    assert c.leaf_bins[0] == 2 and c.index_hashes[0] == census_keys_est(int(t.of_ixf(0)[0])) + census_keys_est(int(t.of_ixf(0)[1]))
    assert all(v is not None for v in c.index_hashes) and [s[5] is not None for s in c.ixf] == [True] * 3
