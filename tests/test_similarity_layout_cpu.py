"""The host half of `taxor build --group-similar` ("Similarity-aware layout"): single-linkage cluster order
over shared / union matrices, and the layout that cuts its groups along a rank instead of along the key counts."""
import numpy as np
import pytest

from taxor_amd import _lib
from taxor_amd.genome_keys import build_layout, cluster_order


def matrices(n, links, uni=100):
    """shared / uni of n rows of `uni` values each: `links` maps (i, j) to the shared count"""
    s = np.zeros((n, n), np.uint32)
    u = np.full((n, n), uni, np.uint32)
    for (i, j), v in links.items():
        s[i, j] = s[j, i] = v
    np.fill_diagonal(s, uni)
    return s, u


def test_chain_is_one_cluster_single_linkage():
    # 1 - 3 - 4 chained, 1 and 4 not linked directly; 0 and 2 alone
    s, u = matrices(5, {(1, 3): 30, (3, 4): 25, (1, 4): 2, (0, 2): 9})
    order, cluster = cluster_order(s, u, 0.1)
    assert order.tolist() == [0, 1, 3, 4, 2]
    assert cluster.tolist() == [0, 1, 2, 1, 1]


def test_clusters_are_ordered_by_smallest_member_members_ascending():
    s, u = matrices(7, {(5, 0): 50, (6, 1): 50, (4, 6): 50, (2, 3): 50})
    order, cluster = cluster_order(s, u, 0.2)
    assert order.tolist() == [0, 5, 1, 4, 6, 2, 3]
    assert cluster.tolist() == [0, 1, 2, 2, 1, 0, 1]


def test_pair_exactly_at_the_threshold_is_linked():
    # 0.25 * 80 = 20 exactly in double arithmetic
    s, u = matrices(3, {(0, 2): 20, (0, 1): 19}, uni=80)
    order, cluster = cluster_order(s, u, 0.25)
    assert order.tolist() == [0, 2, 1] and cluster.tolist() == [0, 1, 0]
    s[0, 2] = s[2, 0] = 19
    order, cluster = cluster_order(s, u, 0.25)
    assert order.tolist() == [0, 1, 2] and cluster.tolist() == [0, 1, 2]


def test_rows_without_a_union_link_nothing():
    # empty bins: uni = 0 against everything, themselves included; shared = 0 >= jmin * 0 must not link them
    s, u = matrices(4, {(1, 2): 60})
    for e in (0, 3):
        s[e, :] = s[:, e] = 0
        u[e, :] = u[:, e] = 0
    u[0, 1] = u[1, 0] = u[3, 1] = u[1, 3] = u[0, 2] = u[2, 0] = u[3, 2] = u[2, 3] = 100   # an empty bin against a full one: |B| alone
    order, cluster = cluster_order(s, u, 0.1)
    assert order.tolist() == [0, 1, 2, 3] and cluster.tolist() == [0, 1, 1, 2]


def test_one_row():
    order, cluster = cluster_order(np.array([[7]], np.uint32), np.array([[7]], np.uint32), 0.1)
    assert order.tolist() == [0] and cluster.tolist() == [0]
    order, cluster = cluster_order(np.zeros((1, 1), np.uint32), np.zeros((1, 1), np.uint32), 1.0)
    assert order.tolist() == [0] and cluster.tolist() == [0]


def test_arguments_are_checked():
    s, u = matrices(2, {})
    for jmin in (0.0, -1.0, float("nan")):
        with pytest.raises(_lib.TaxorError):
            cluster_order(s, u, jmin)


def same_layout(a, b):
    assert (a["t_max"], a["depth"], a["bytes_per_hash"], a["index_bytes"], len(a["ixfs"])) == \
           (b["t_max"], b["depth"], b["bytes_per_hash"], b["index_bytes"], len(b["ixfs"]))
    for x, y in zip(a["ixfs"], b["ixfs"]):
        assert x["bins"] == y["bins"]
        for f in ("next_ixf", "fname_idx", "part", "parts"):
            assert np.array_equal(x[f], y[f]), f


def count_vectors():
    rng = np.random.default_rng(5)
    return [np.full(40, 1000), rng.integers(0, 5000, 300), np.r_[200000, rng.integers(500, 600, 149)], rng.integers(1, 50, 1000) ** 3, np.array([7])]


@pytest.mark.parametrize("t_max", [0, 2, 16, 64])
def test_without_a_rank_the_layout_is_the_unranked_one(t_max):
    for counts in count_vectors():
        same_layout(build_layout(counts, t_max), build_layout(counts, t_max, rank=None))


@pytest.mark.parametrize("t_max", [2, 16, 64])
def test_the_count_order_as_rank_changes_nothing(t_max):
    # rank = position in descending count order (ties on index): the order the unranked rule cuts along
    for counts in count_vectors():
        p = np.lexsort((np.arange(counts.size), -counts.astype(np.int64)))
        rank = np.empty(counts.size, np.uint64)
        rank[p] = np.arange(counts.size)
        same_layout(build_layout(counts, t_max), build_layout(counts, t_max, rank=rank))


def users_below(lay, i):
    f = lay["ixfs"][i]
    out = set()
    for b in range(f["bins"]):
        if f["fname_idx"][b] >= 0:
            out.add(int(f["fname_idx"][b]))
        else:
            out |= users_below(lay, int(f["next_ixf"][b]))
    return out


def root_bin_of(lay, n):
    """user bin -> the root bin it lies in or under"""
    root, where = lay["ixfs"][0], np.full(n, -1)
    for b in range(root["bins"]):
        if root["fname_idx"][b] >= 0:
            where[int(root["fname_idx"][b])] = b
        else:
            where[sorted(users_below(lay, int(root["next_ixf"][b])))] = b
    assert (where >= 0).all()
    return where


@pytest.mark.parametrize("n_fam,fam_size,t_max", [(16, 8, 16), (40, 5, 16), (64, 8, 64), (30, 4, 8)])
def test_a_rank_that_puts_families_together_keeps_each_under_two_root_groups(n_fam, fam_size, t_max):
    # member j of family f is user bin n_fam * j + f: interleaved, and counts close but not equal, so the count order scatters them
    n = n_fam * fam_size
    rng = np.random.default_rng(n)
    counts = rng.integers(540, 560, n)
    family = np.arange(n) % n_fam
    assert n > t_max and n // t_max >= fam_size             # groups hold at least a family
    rank = np.empty(n, np.uint64)
    rank[np.lexsort((np.arange(n), family))] = np.arange(n)
    lay = build_layout(counts, t_max, rank=rank)
    where = root_bin_of(lay, n)
    assert sorted(users_below(lay, 0)) == list(range(n))
    assert max(np.unique(where[family == f]).size for f in range(n_fam)) <= 2
    # the premise: the unranked layout does scatter them
    plain = root_bin_of(build_layout(counts, t_max), n)
    assert max(np.unique(plain[family == f]).size for f in range(n_fam)) > 2


def test_large_bins_stay_leaves_whatever_their_rank():
    rng = np.random.default_rng(9)
    counts = rng.integers(900, 1100, 200)
    big = [3, 77, 150]
    counts[big] = [40000, 25000, 90000]
    t_max = 16
    target = counts.sum() / t_max
    assert all(counts[b] >= target for b in big)
    for rank in (np.arange(200)[::-1].copy(), rng.permutation(200), np.zeros(200)):
        lay = build_layout(counts, t_max, rank=rank.astype(np.uint64))
        root, plain = lay["ixfs"][0], build_layout(counts, t_max)["ixfs"][0]
        leaves = {int(u): int((root["fname_idx"] == u).sum()) for u in root["fname_idx"] if u >= 0}
        for b in big:
            assert leaves.get(b, 0) >= 1
        # the same leaves with the same number of parts as without a rank
        assert leaves == {int(u): int((plain["fname_idx"] == u).sum()) for u in plain["fname_idx"] if u >= 0}
        assert sorted(users_below(lay, 0)) == list(range(200))
        assert all(f["bins"] <= t_max for f in lay["ixfs"])
