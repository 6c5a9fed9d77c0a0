"""The device accumulator between `taxor search` and `taxor profile` (taxor_amd/csrc/profile_feed.hip),
through taxor_amd.profile.ProfileFeed.

1. The output filter at its edges: for every max in 1..4096 the counts around 0.8 * max, 2^32 - 1, all-zero counts, reads of 0, 1,
   63, 64, 65, 129 and 5000 tuples -- kept set and order equal a restatement of taxor_search.cpp:268-306 (kept(), below).
2. One CSR fed as one batch, as seven uneven batches, reversed and shuffled: the finished arrays are identical.
3. Reads come out in byte-wise order of their ids.
4. Two user bins of one accession share a reference id and keep their own ref_len and user_bin.
5. A gap or an overlap of the batches' ranges, ranks that are no permutation, a user bin outside the table: TaxorError.
6. The golden search files through the feed: every array of the result equals run_profile on the same file's host CSR (the pair
   table as rows sorted by key: its slot order is not determined by the input, see sorted_pairs) -- once with the feed's references
   exactly those that appear, once with more than as many again that nothing matches, interleaved in byte order.
7. A searcher's device-resident results (add_batch) give the CSR that its fetched results give through add_csr."""
import json
import os
import random

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "profile")
CASES = {c["name"]: c for c in json.load(open(os.path.join(GOLDEN, "cases.json")))}
CSR_KEYS = ("read_off", "csr_ref", "csr_ref_len", "hash_match", "user_bin", "query_len", "hash_count")


def kept(counts):
    """taxor_search.cpp:275-286: the positions of a read's tuples that are written, in order"""
    mx = max(counts)
    return [i for i, c in enumerate(counts) if not (float(c) < float(mx) * 0.8)]


def expected_csr(reads, ref_of_bin, ref_len_of_bin, order, keep_all=False):
    """reads: (query_len, n_hashes, [(user_bin, count)]) in input order; order = input indices in output order"""
    off, ref, ref_len, hm, ub, ql, hc = [0], [], [], [], [], [], []
    for i in order:
        q, nh, tup = reads[i]
        keep = [] if not tup else list(range(len(tup))) if keep_all else kept([c for _, c in tup])
        if keep:                                                    # :287-305
            for j in keep:
                b, c = tup[j]
                ref.append(int(ref_of_bin[b]))
                ref_len.append(int(ref_len_of_bin[b]))
                hm.append(c)
                ub.append(b)
        else:                                                       # :268-273, the "-" line
            ref.append(-1)
            ref_len.append(0)
            hm.append(0)
            ub.append(-1)
        off.append(len(ref))
        ql.append(q)
        hc.append(nh if keep else 0)
    return dict(read_off=np.array(off, np.uint64), csr_ref=np.array(ref, np.int32), csr_ref_len=np.array(ref_len, np.uint64),
                hash_match=np.array(hm, np.uint64), user_bin=np.array(ub, np.int64), query_len=np.array(ql, np.uint64),
                hash_count=np.array(hc, np.uint64))


def to_csr(reads):
    off = np.zeros(len(reads) + 1, np.uint64)
    off[1:] = np.cumsum([len(t) for _, _, t in reads])
    ub = np.array([b for _, _, t in reads for b, _ in t], np.int64)
    cnt = np.array([c for _, _, t in reads for _, c in t], np.uint32)
    nh = np.array([n for _, n, _ in reads], np.uint32)
    ql = np.array([q for q, _, _ in reads], np.uint64)
    return off, ub, cnt, nh, ql


def assert_same(got, want, keys=CSR_KEYS):
    for k in keys:
        assert got[k].dtype == want[k].dtype and np.array_equal(got[k], want[k]), (k, got[k][:20], want[k][:20])


def bin_table(n_bins, n_refs, seed):
    rng = np.random.default_rng(seed)
    return rng.integers(0, n_refs, n_bins).astype(np.int32), rng.integers(1000, 10**7, n_bins).astype(np.uint64)


def test_filter_edge_sweep():
    from taxor_amd.profile import ProfileFeed

    rng = random.Random(3)
    n_bins = 6000
    ref_of_bin, ref_len_of_bin = bin_table(n_bins, 900, 1)
    reads = []

    def add(counts):
        bins = rng.sample(range(n_bins), len(counts))
        reads.append((rng.randrange(500, 40000), rng.randrange(1, 5000), list(zip(bins, counts))))

    for mx in range(1, 4097):
        lo, hi = (4 * mx) // 5 - 1, -((-4 * mx) // 5) + 1           # floor(0.8 max) - 1 .. ceil(0.8 max) + 1
        add([mx] + [c for c in range(lo, hi + 1) if 0 <= c <= mx])
    add([0, 0, 0, 0, 0])                                              # 0 < 0 is false: all of them stay
    top = 2**32 - 1
    edge = -((-4 * top) // 5)
    add([edge - 1, top, edge, edge + 1])
    add([edge + 1, edge - 1, edge, top, 0])
    for n in (0, 1, 63, 64, 65, 129, 5000):                           # wave edges, a wide read; the maximum anywhere
        add([rng.randrange(0, 1000) for _ in range(n)])
        add([rng.choice((79, 80, 81, 100)) for _ in range(n)])
    add([])
    want = expected_csr(reads, ref_of_bin, ref_len_of_bin, range(len(reads)))
    dropped = sum(len(t) for _, _, t in reads) - int((want["csr_ref"] >= 0).sum())
    assert dropped > 4096 and int((want["csr_ref"] < 0).sum()) == 3   # the sweep drops and keeps; three reads without a tuple
    with ProfileFeed(ref_of_bin, ref_len_of_bin, 900) as feed:
        feed.add_csr(0, *to_csr(reads))
        got = feed.finish(np.arange(len(reads), dtype=np.uint64), run=False)
    assert_same(got, want)
    miss = np.flatnonzero(want["csr_ref"] < 0)
    rd = np.searchsorted(want["read_off"], miss, side="right") - 1
    assert np.all(got["hash_count"][rd] == 0) and np.all(got["query_len"][rd] == [reads[int(r)][0] for r in rd])


def random_reads(n, n_bins, seed):
    rng = random.Random(seed)
    reads = []
    for i in range(n):
        m = rng.choice((0, 0, 1, 1, 1, 2, 3, 5, 8, 70, 130)) if i % 97 else 300
        reads.append((rng.randrange(300, 20000), rng.randrange(1, 3000), [(rng.randrange(n_bins), rng.randrange(0, 400)) for _ in range(m)]))
    return reads


def test_arrival_order_and_splits():
    from taxor_amd.profile import ProfileFeed

    n, n_bins = 2003, 500
    ref_of_bin, ref_len_of_bin = bin_table(n_bins, 120, 2)
    reads = random_reads(n, n_bins, 4)
    off, ub, cnt, nh, ql = to_csr(reads)
    rank = np.random.default_rng(5).permutation(n).astype(np.uint64)
    order = np.argsort(rank)
    want = expected_csr(reads, ref_of_bin, ref_len_of_bin, [int(i) for i in order])
    cuts = [0, 1, 1, 700, 701, 1300, 1999, n]                         # seven batches: an empty one, one-read ones, uneven ones
    batches = list(zip(cuts, cuts[1:]))
    assert len(batches) == 7
    shuffled = batches[:]
    random.Random(6).shuffle(shuffled)
    results = []
    for plan in ([(0, n)], batches, batches[::-1], shuffled):
        with ProfileFeed(ref_of_bin, ref_len_of_bin, 120) as feed:
            for a, b in plan:
                feed.add_csr(a, off[a:b + 1], ub, cnt, nh[a:b], ql[a:b])
            results.append(feed.finish(rank, run=False))
    for got in results:
        assert_same(got, want)


def test_scans_beyond_one_block_of_tile_sums():
    """530 000 reads of 0, 1 or 2 tuples in two batches, ranks reversed: both scans (a batch's kept counts, the finish's counts by
    rank) run over more than 256 tiles of 2048 reads, where the block that scans the tile sums carries from pass to pass"""
    from taxor_amd.profile import ProfileFeed

    n, n_bins = 2048 * 256 + 2048 * 2 + 1618, 300
    rng = np.random.default_rng(12)
    ref_of_bin, ref_len_of_bin = bin_table(n_bins, 40, 13)
    m = rng.integers(0, 3, n)
    off = np.zeros(n + 1, np.uint64)
    off[1:] = np.cumsum(m)
    ub = rng.integers(0, n_bins, int(off[-1])).astype(np.int64)
    cnt = rng.integers(0, 1000, ub.size).astype(np.uint32)
    nh = rng.integers(1, 2000, n).astype(np.uint32)
    ql = rng.integers(200, 30000, n).astype(np.uint64)
    rank = np.arange(n, dtype=np.uint64)[::-1].copy()
    cut = 2048 * 257 + 5
    with ProfileFeed(ref_of_bin, ref_len_of_bin, 40) as feed:
        feed.add_csr(cut, off[cut:], ub, cnt, nh[cut:], ql[cut:], keep_all=True)
        feed.add_csr(0, off[:cut + 1], ub, cnt, nh[:cut], ql[:cut], keep_all=True)
        got = feed.finish(rank, run=False)
    # expected, vectorised: every input read emits max(m, 1) matches (one "-" match where it has no tuple)
    k = np.maximum(m, 1)
    in_off = np.zeros(n + 1, np.int64)
    in_off[1:] = np.cumsum(k)
    e_ub = np.full(int(in_off[-1]), -1, np.int64)
    e_hm = np.zeros(e_ub.size, np.uint64)
    has = np.repeat(m > 0, k)
    e_ub[has] = ub
    e_hm[has] = cnt
    order = np.arange(n)[::-1]
    out_off = np.zeros(n + 1, np.int64)
    out_off[1:] = np.cumsum(k[order])
    src = np.repeat(in_off[order] - out_off[:-1], k[order]) + np.arange(int(out_off[-1]))
    w_ub = e_ub[src]
    want = dict(read_off=out_off.astype(np.uint64), user_bin=w_ub, hash_match=e_hm[src],
                csr_ref=np.where(w_ub >= 0, ref_of_bin[np.maximum(w_ub, 0)], -1).astype(np.int32),
                csr_ref_len=np.where(w_ub >= 0, ref_len_of_bin[np.maximum(w_ub, 0)], 0).astype(np.uint64),
                query_len=ql[order], hash_count=np.where(m[order] > 0, nh[order], 0).astype(np.uint64))
    assert_same(got, want)


def test_rank_order_is_bytewise():
    from taxor_amd.profile import ProfileFeed, rank_read_ids

    same = b"x" * 40
    ids = [b"r10", b"r1a", b"r1", b"r\xc3\xa9", b"r2", same + b"b", same + b"a", same, b"R1", b"r", b"~", b"\x80"]
    assert sorted(ids) != ids and sorted(ids)[-1] == b"\x80"         # bytes compare as unsigned: 0x80 is after '~'
    ref_of_bin, ref_len_of_bin = bin_table(50, 20, 7)
    reads = [(1000 + i, 100 + i, [(i, 90 + i), (i + 20, 89)]) for i in range(len(ids))]
    rank = rank_read_ids(ids)
    order = sorted(range(len(ids)), key=lambda i: ids[i])
    assert [int(rank[i]) for i in order] == list(range(len(ids)))
    with ProfileFeed(ref_of_bin, ref_len_of_bin, 20) as feed:
        feed.add_csr(0, *to_csr(reads))
        got = feed.finish(rank, run=False)
    assert_same(got, expected_csr(reads, ref_of_bin, ref_len_of_bin, order))
    assert got["query_len"].tolist() == [1000 + i for i in order]
    with pytest.raises(ValueError, match="occurs twice"):
        rank_read_ids([b"a", b"b", b"a"])


def test_shared_accession():
    from taxor_amd.profile import ProfileFeed

    ref_of_bin = np.array([0, 1, 1, 2], np.int32)                     # user bins 1 and 2: one accession
    ref_len_of_bin = np.array([1000, 2000, 3000, 4000], np.uint64)
    reads = [(500, 50, [(1, 40), (2, 39), (0, 38)]), (600, 60, [(2, 30)]), (700, 70, [(3, 10), (1, 10)])]
    with ProfileFeed(ref_of_bin, ref_len_of_bin, 3) as feed:
        feed.add_csr(0, *to_csr(reads))
        got = feed.finish(np.arange(3, dtype=np.uint64), run=False)
    assert got["csr_ref"].tolist() == [1, 1, 0, 1, 2, 1]
    assert got["csr_ref_len"].tolist() == [2000, 3000, 1000, 3000, 4000, 2000]
    assert got["user_bin"].tolist() == [1, 2, 0, 2, 3, 1]


def test_refusals():
    from taxor_amd._lib import TaxorError
    from taxor_amd.profile import ProfileFeed

    ref_of_bin, ref_len_of_bin = bin_table(10, 4, 8)
    reads = random_reads(40, 10, 9)
    off, ub, cnt, nh, ql = to_csr(reads)
    ident = np.arange(40, dtype=np.uint64)

    def feed_ranges(ranges):
        feed = ProfileFeed(ref_of_bin, ref_len_of_bin, 4)
        for first, a, b in ranges:
            feed.add_csr(first, off[a:b + 1], ub, cnt, nh[a:b], ql[a:b])
        return feed

    with feed_ranges([(0, 0, 20), (25, 20, 35)]) as feed:                           # reads 20..24 never added
        with pytest.raises(TaxorError, match="gap"):
            feed.finish(ident, run=False)
    with feed_ranges([(0, 0, 20), (15, 15, 40)]) as feed:                           # reads 15..19 twice
        with pytest.raises(TaxorError, match="overlap"):
            feed.finish(ident, run=False)
    with feed_ranges([(0, 0, 40)]) as feed:
        with pytest.raises(TaxorError, match="reads were added"):                   # n_reads_total does not cover them
            feed.finish(ident[:39], run=False)
        bad = ident.copy()
        bad[7] = 8
        with pytest.raises(TaxorError, match="not a permutation"):
            feed.finish(bad, run=False)
        bad[7] = 40
        with pytest.raises(TaxorError, match="not below"):
            feed.finish(bad, run=False)
        got = feed.finish(ident, run=False)                                         # the feed is intact after the refusals
    assert_same(got, expected_csr(reads, ref_of_bin, ref_len_of_bin, range(40)))
    with ProfileFeed(ref_of_bin, ref_len_of_bin, 4) as feed:
        for wrong in (10, -1, 2**40):
            ub2 = ub.copy()
            ub2[3] = wrong
            with pytest.raises(TaxorError, match="outside the feed's table"):
                feed.add_csr(0, off, ub2, cnt, nh, ql)
        feed.add_csr(0, off, ub, cnt, nh, ql)                                       # nothing of the refused batches was kept
        got = feed.finish(ident, run=False)
    assert_same(got, expected_csr(reads, ref_of_bin, ref_len_of_bin, range(40)))
    with pytest.raises(TaxorError, match="out of range"):
        ProfileFeed(np.array([0, 4], np.int32), np.array([1, 1], np.uint64), 4)


# ---- the golden search files: the feed against the host CSR route -------------------------------------------------------------
def parse_tsv(name):
    """reads in file order: (id cut at the first space, query_len, hash_count, [(bin key, ref_len, hash_match)]); a '-' line is a
    read without a tuple"""
    reads = []
    for line in open(os.path.join(GOLDEN, name), "rb").read().split(b"\n")[1:]:
        if not line:
            continue
        f = line.split(b"\t")
        rid = f[0].split(b" ")[0]
        if f[1] == b"-":
            reads.append([rid, int(f[5]), 0, []])
            continue
        key = (f[1], f[3], int(f[4]), f[8], f[9])
        if not reads or reads[-1][0] != rid or not reads[-1][3]:
            reads.append([rid, int(f[5]), int(f[6]), []])
        assert (reads[-1][1], reads[-1][2]) == (int(f[5]), int(f[6]))
        reads[-1][3].append((key, int(f[4]), int(f[7])))
    return reads


FEED_CASES = ["unique", "round1", "round2", "explained", "chain", "ties", "many"]
PER_MATCH = ("ref_len", "alive", "best", "alive_round1", "alive_round2", "alive_round3")
PER_REF = ("has_prior", "taxa_len", "ref_nts", "log_prior", "unique_reads", "all_reads")
SCALARS = ("all_nts", "unclassified_nts", "log_unclassified", "em_steps_needed", "em_iterations")


def sorted_pairs(key, count):
    """the pair table as (key, count) rows sorted by key.  The table is open addressing filled with atomics by many waves at
    once: which of two colliding keys gets the earlier slot depends on which wave inserts first, so the ORDER in which
    taxor_profile_results lists the pairs is not determined by the input (profile.hip sorts them by key before it uses them).
    The multiset is: sorted, a key that is listed twice or missing shows."""
    o = np.argsort(key, kind="stable")
    return key[o], count[o]


def golden_through_feed(name, spare):
    """one golden search file through the feed, and run_profile on the same file's host CSR numbered over the accessions that
    appear (what the TSV route does).  spare: the feed's tables also hold accessions and user bins that no row matches --
    before, between and after the appearing ones in byte order -- as an index's species table does for a sample that holds
    only some of its species; the feed's reference ids are then dense over ALL of them.  Returns (got, want, id of every
    appearing accession in the feed's numbering, number of the feed's references)."""
    from taxor_amd.profile import ProfileFeed, rank_read_ids, run_profile

    reads = parse_tsv(name + ".tsv")
    ids = [r[0] for r in reads]
    assert len(set(ids)) == len(ids)                                   # contiguous reads with unique ids
    keys = sorted({k for r in reads for k, _, _ in r[3]})
    accs = sorted({k[0] for k in keys})
    all_keys, all_accs = keys, accs
    if spare:
        extra = [b"!" + accs[0], accs[-1] + b"~"] + [a + b"!" for a in accs] + [a[:-1] + bytes([a[-1] - 1]) + b"z" for a in accs]
        extra = sorted(set(extra) - set(accs))
        all_accs = sorted(accs + extra)
        assert all_accs[0] not in accs and all_accs[-1] not in accs and len(all_accs) >= 2 * len(accs)
        # a second, never-matched user bin of an appearing accession too (another ref_len: it must not leak into taxa_len)
        all_keys = sorted(keys + [(e, b"9", 777 + i, b"k__X", b"1") for i, e in enumerate(extra)] + [(accs[0], b"9", 5, b"k__X", b"1")])
    bin_of = {k: i for i, k in enumerate(all_keys)}
    ref_of_bin = np.array([all_accs.index(k[0]) for k in all_keys], np.int32)
    ref_len_of_bin = np.array([k[2] for k in all_keys], np.uint64)
    id_of = np.array([all_accs.index(a) for a in accs], np.int64)
    below = sum(1 for r in reads if r[3] for _, _, m in r[3] if float(m) < float(max(x[2] for x in r[3])) * 0.8)
    if name == "many":
        assert below == 381 and sum(len(r[3]) for r in reads) == 690  # rows below 0.8 * max: the reason for KEEP_ALL
    feed_reads = [(q, hc, [(bin_of[k], m) for k, _, m in tup]) for _, q, hc, tup in reads]
    rank = rank_read_ids(ids)
    with ProfileFeed(ref_of_bin, ref_len_of_bin, len(all_accs)) as feed:
        half = len(reads) // 2
        off, ub, cnt, nh, ql = to_csr(feed_reads)
        feed.add_csr(half, off[half:], ub, cnt, nh[half:], ql[half:], keep_all=True)
        feed.add_csr(0, off[:half + 1], ub, cnt, nh[:half], ql[:half], keep_all=True)
        got = feed.finish(rank)
    order = sorted(range(len(ids)), key=lambda i: ids[i])
    assert_same(got, expected_csr(feed_reads, ref_of_bin, ref_len_of_bin, order, keep_all=True))
    # the host CSR of the TSV route: the same rows, references numbered over the appearing accessions only
    tsv_bin_of = {k: i for i, k in enumerate(keys)}
    tsv_reads = [(q, hc, [(tsv_bin_of[k], m) for k, _, m in tup]) for _, q, hc, tup in reads]
    host = expected_csr(tsv_reads, np.array([accs.index(k[0]) for k in keys], np.int32), np.array([k[2] for k in keys], np.uint64), order, keep_all=True)
    want = run_profile(host["read_off"], host["csr_ref"], host["csr_ref_len"], host["hash_match"], host["query_len"], host["hash_count"], len(accs))
    assert got["em_steps_needed"] == want["em_steps_needed"] == int(CASES[name]["em_steps_line"].rsplit(" ", 1)[1])
    assert {"alive_round1", "alive_round2", "alive_round3", "iter_ref_nts"} <= set(want)
    assert set(want) - {"seconds_filter", "seconds_em", "pair_slots", "pair_key", "pair_count", "ref", "explained_by", "iter_ref_nts"} \
        == set(PER_MATCH) | set(PER_REF) | set(SCALARS)               # no array of the result is left out below
    return got, want, id_of, len(all_accs)


@pytest.mark.parametrize("name", FEED_CASES)
def test_golden_tsv_through_the_feed(name):
    """every array of the result equals run_profile on the same file's host CSR; the pair table as sorted rows (sorted_pairs)"""
    got, want, id_of, n_refs = golden_through_feed(name, spare=False)
    assert np.array_equal(id_of, np.arange(n_refs))
    for k, v in want.items():
        if k in ("seconds_filter", "seconds_em", "pair_key", "pair_count"):
            continue
        if isinstance(v, np.ndarray):
            assert got[k].dtype == v.dtype and got[k].shape == v.shape and np.array_equal(got[k], v), k
        else:
            assert got[k] == v, k
    (gk, gc), (wk, wc) = sorted_pairs(got["pair_key"], got["pair_count"]), sorted_pairs(want["pair_key"], want["pair_count"])
    assert gk.dtype == wk.dtype and gc.dtype == wc.dtype and np.array_equal(gk, wk) and np.array_equal(gc, wc)
    assert np.unique(gk).size == gk.size


@pytest.mark.parametrize("name", FEED_CASES)
def test_golden_tsv_with_references_that_never_match(name):
    """DESIGN.md section 10.1, numbering: reference ids dense over an index's accessions give, per accession, what ids dense over
    the appearing accessions give -- the stages depend on the ids' order only.  The feed's tables hold more than twice the
    accessions that appear, interleaved with them in byte order."""
    got, want, id_of, n_refs = golden_through_feed(name, spare=True)
    spare = np.setdiff1d(np.arange(n_refs), id_of)
    assert spare.size > id_of.size and not np.array_equal(id_of, np.arange(id_of.size))

    def renum(a):                                                      # reference ids of the TSV route in the feed's numbering; -1 stays
        a = a.astype(np.int64)
        return np.where(a >= 0, id_of[np.maximum(a, 0)], a)

    for k in SCALARS:
        assert got[k] == want[k], k
    for k in PER_MATCH:
        assert got[k].dtype == want[k].dtype and np.array_equal(got[k], want[k]), k
    assert np.array_equal(got["ref"].astype(np.int64), renum(want["ref"]))                    # after round 3's renames
    for k in PER_REF:
        assert got[k].dtype == want[k].dtype and got[k].shape == (n_refs,) and np.array_equal(got[k][id_of], want[k]), k
    assert np.array_equal(got["explained_by"][id_of].astype(np.int64), renum(want["explained_by"]))
    assert got["iter_ref_nts"].shape == (want["em_iterations"], n_refs) and np.array_equal(got["iter_ref_nts"][:, id_of], want["iter_ref_nts"])
    # a reference nothing matches: no read, no prior, no length, no nucleotides, explained by nothing
    for k in ("has_prior", "taxa_len", "ref_nts", "unique_reads", "all_reads"):
        assert not got[k][spare].any(), k
    assert np.all(got["explained_by"][spare] == -1) and not got["iter_ref_nts"][:, spare].any()
    wk = want["pair_key"]
    wk = (id_of[(wk >> np.uint64(32)).astype(np.int64)].astype(np.uint64) << np.uint64(32)) | id_of[(wk & np.uint64(0xFFFFFFFF)).astype(np.int64)].astype(np.uint64)
    (gk, gc), (wk, wc) = sorted_pairs(got["pair_key"], got["pair_count"]), sorted_pairs(wk, want["pair_count"])
    assert np.array_equal(gk, wk) and np.array_equal(gc, wc) and np.unique(gk).size == gk.size


def test_names_tsv_is_refused_at_the_ranking():
    """names.tsv repeats a read id after other reads: the TSV route merges the two, the feed's ranking names the id"""
    from taxor_amd.profile import rank_read_ids

    reads = parse_tsv("names.tsv")
    ids = [r[0] for r in reads]
    assert len(set(ids)) < len(ids)
    with pytest.raises(ValueError, match="occurs twice"):
        rank_read_ids(ids)


@pytest.mark.parametrize("small_path", [True, False], ids=["lanes", "pipeline"])
def test_add_batch_reads_the_searchers_device_results(small_path):
    """300 reads against a planted index: the searcher's device-resident results through add_batch, its fetched results through
    add_csr (QUERY_LEN from the offsets either way); a call of this size goes through the small-call lanes unless they are off"""
    from taxor_amd import GpuIndex, Searcher, synth
    from taxor_amd.profile import ProfileFeed

    g, go = synth.random_genomes(6, 20000, seed=1)
    dummy = GpuIndex([dict(bins=64, stride=64, seg_len=16, seed=1, next_ixf=np.zeros(64, np.int64), fname_idx=np.arange(64),
                           data=np.zeros(3 * 16 * 64, np.uint8))], 64)
    hs = Searcher(dummy, ratio=0.5)
    hoff, hashes = hs.seq_to_syncmers(g, go)
    planted = [hashes[int(hoff[i]):int(hoff[i + 1])] for i in range(6)]
    hs.close()
    dummy.close()
    lay = synth.make_layout(planted, root_bins=64, child_bins=32, n_children=3, seed=2)
    idx = GpuIndex(synth.materialize_host(lay), lay["n_user_bins"])
    sr = Searcher(idx, ratio=0.1, small_path=small_path)
    nb = int(lay["n_user_bins"])
    ref_of_bin, ref_len_of_bin = bin_table(nb, max(2, nb // 2), 10)
    first, second = (synth.synth_reads(g, go, n, 1500, error_rate=0.02, frac_random=0.2, seed=s)[:2] for n, s in ((300, 3), (77, 4)))
    with ProfileFeed(ref_of_bin, ref_len_of_bin, max(2, nb // 2)) as dev, ProfileFeed(ref_of_bin, ref_len_of_bin, max(2, nb // 2)) as host:
        at = {0: 77, 1: 0}                                             # the second batch holds the first reads
        for j, (bases, offs) in enumerate((first, second)):
            res = sr.search_batch(bases, offs)
            dev.add_batch(sr, at[j])
            host.add_csr(at[j], res.read_off, res.user_bin, res.count, res.n_hashes, np.diff(offs.astype(np.uint64)))
        rank = np.random.default_rng(11).permutation(377).astype(np.uint64)
        a, b = dev.finish(rank, run=False), host.finish(rank, run=False)
    assert_same(a, b)
    assert int((a["csr_ref"] >= 0).sum()) > 200 and int((a["csr_ref"] < 0).sum()) > 20
    sr.close()
    idx.close()
