"""The device keyer of `taxor build` (taxor_amd/csrc/genome_keys.hip) over the whole domain that taxor_gpu_keyer_create admits, at
the lengths where its tiles, fix-up chains, per-bin sets and compactions change.  The keyer's counterpart of
test_gpu_selector_domain.py.

Syncmers: every (k, s) with 2 <= k <= 32, 1 <= s <= min(16, k-1), at t in {1, (k-s+1)//2 (the build default), w}, every t in 1..w
for a handful of pairs, and a few pairs beyond s = 16 that keyer_create also admits.  Minimisers: k = 1..32 x (w-k+1) in
{1, 2, 11, 64, 97-k (the build's window 96), 511, 512}.  Every configuration runs two add() calls over interleaved user bins: records
with 0, 1, GT-1, GT, GT+1, 2GT and 3GT+1 windows, empty and sub-k records first, last and in the middle of a call, periodic tie
tracts laid across tile edges (an anchor-less chain through a whole tile, to the last window of a record, from window 0 of a
record), a bin re-added with a record it already holds, and a bin whose second call holds only sub-k records.  Each bin must
equal the oracle (test_gpu_genome_keys.oracle_keys) as an exact array and, for syncmers with k <= 31 where oracle/_ref/ holds the
reference's own selector, wyhash of the reference's selection.

Then the compaction and merge edges of _finish, FracMinHash scaling, the key equal to the tables' empty marker (2^64 - 1: wyhash
of the canonical 32-mers (AT)^16, (CG)^16, (GC)^16, (TA)^16), the refusals of the C ABI, and every byte value of the alphabet.
Every length comes from genome_keys.hip's own constants."""
import os
import re
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

from oracle import oracle as orc
from taxor_amd._lib import TaxorError
from taxor_amd.genome_keys import GenomeKeyer
from tests.test_gpu_genome_keys import oracle_keys
from tests.test_gpu_selector_domain import _Reads, _wyhash

pytestmark = pytest.mark.gpu

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "taxor_amd", "csrc")
MARKER = 2**64 - 1
E_ARG, E_ALPHABET = -1, -3


def _constants():
    """`constexpr int|uint64_t NAME = EXPR;` at the top level of genome_keys.hip, EXPR over earlier names"""
    env = {}
    src = open(os.path.join(CSRC, "genome_keys.hip")).read()
    for name, expr in re.findall(r"^constexpr (?:int|uint64_t) (\w+) = ([^;]+);", src, re.M):
        env[name] = int(eval(expr.replace("/", "//"), {}, dict(env)))
    return env


K = _constants()
GB, GC, GT, GMAX_W, CC_BLOCK, REGION_MIN = (K[n] for n in ("GB", "GC", "GT", "GMAX_W", "CC_BLOCK", "REGION_MIN"))
REF = orc.ref_syncmer_lib()
orc.lib()                 # load (and, on a new host, rebuild) the oracle here, before the pool's threads first call it
POOL = ThreadPoolExecutor(8)


def test_keyer_constants_read():
    assert (GB, GC, GT, GMAX_W, CC_BLOCK, REGION_MIN) == (256, 8, 2048, 512, 4096, 4096)
    assert GT == GB * GC


# ------------------------------------------------------------------------------------------------ records and calls
def _tract(R, P, n):
    """n bases of period P (a random unit of P bases repeated)"""
    u = R.rnd(P)
    return (u * (n // P + 1))[:n]


def _lay(base, pos, tract):
    g = bytearray(base)
    pos = max(0, pos)
    g[pos:pos + len(tract)] = tract[:max(0, len(g) - pos)]
    return bytes(g)


def _sync_records(k, s, t, ci):
    """(main records, sub-k record) for one syncmer configuration; ci picks which (period, start offset) pairs it lays"""
    w = k - s + 1
    R = _Reads(k * 10007 + s * 101 + t)
    W = lambda nwin: R.rnd(nwin + k - 1)                       # a random record of nwin windows
    periods = [1, 2, 3, 4, 6, max(1, w - 1)]
    ds = [0, 1, t - 1, w - 1, k, k + w]
    pd = [(periods[(ci + j) % 6], ds[(ci // 6 + 2 * j) % 6]) for j in range(5)]
    # tile edges at GT, 4GT, 5GT: a tract over two whole tiles, one just a window long, one that runs to the end of the record
    rt = W(5 * GT + 50)
    rt = _lay(rt, GT - pd[0][1], _tract(R, pd[0][0], 5 * GT // 2))
    rt = _lay(rt, 4 * GT - pd[1][1], _tract(R, pd[1][0], k + pd[1][0]))
    rt = _lay(rt, 5 * GT - pd[2][1], _tract(R, pd[2][0], GT // 2))
    # an anchor-less chain from GT - 300 to the record's last window; the next tile of the call is another record's
    rend = _lay(W(3 * GT - 100), GT - 300, _tract(R, pd[3][0], 3 * GT))
    # a record that starts inside a tie tract (window 0 takes the leftmost minimum)
    rstart = _tract(R, pd[4][0], GT // 2 + 77) + R.rnd(GT)
    main = [W(GT - 1), rt, W(1), W(GT), rend, W(2 * GT), rstart, W(GT + 1), W(3 * GT + 1), W(0)]
    return main, R.rnd(k - 1)


def _seed_kmer(k):
    """the k-mer whose minimiser value is 0 (its bits equal hixf::adjust_seed(k)): the smallest value there is"""
    seed = 0x8F3F73B5CF1C9ADE >> (64 - 2 * k)
    return bytes(b"ACGT"[(seed >> (2 * (k - 1 - i))) & 3] for i in range(k))


def _mini_records(k, wm):
    R = _Reads(k * 7919 + wm)
    W = lambda nwin: R.rnd(nwin + wm - 1 + k - 1)              # nwin windows of wm k-mers
    # the window minimum of tile 0's last windows lies only in the wm-1 k-mers that tile 0 shares with tile 1
    rt = W(3 * GT + 10)
    if wm > 1:
        rt = _lay(rt, GT + wm - 2, _seed_kmer(k))
    rt = _lay(rt, 2 * GT - 5, b"A" * (wm + k + 100))
    rt = _lay(rt, 3 * GT - 20, b"AT" * (wm + k))
    short = [R.rnd(max(1, wm // 2) + k - 1)] if wm > 1 else []   # fewer k-mers than a window: the window shrinks to the text
    main = [W(GT - 1), rt, R.rnd(wm + k - 1), W(GT), _tract(R, 3, GT + wm + k), W(2 * GT + 1), _tract(R, 2, wm + k + 40) + R.rnd(300),
            W(GT + 1)] + short + [R.rnd(k + 3)]
    return main, R.rnd(k - 1)


def _calls(main, sub):
    """two calls over interleaved user bins 0..5: empty and sub-k records first, last and in the middle; bin 1 re-adds main[1] in
    call 2; bin 4 has keys in call 1 and only sub-k records in call 2; bin 5 never has a window"""
    m = list(main)
    c1 = [(5, b""), (0, m[0]), (1, m[1]), (0, sub), (2, m[2]), (1, m[3]), (3, m[4]), (4, m[5]), (2, b""), (5, sub)]
    c2 = [(3, sub), (1, m[6]), (4, sub), (0, m[7])] + [(2 + j % 2, r) for j, r in enumerate(m[8:])] + [(1, m[1]), (4, b"")]
    return [c1, c2]


def _nwin(L, k, wm):
    nk = L - k + 1
    if nk <= 0:
        return 0
    return nk if wm is None else nk - min(wm, nk) + 1


def _run(calls, n_bins, **kw):
    kr = GenomeKeyer(n_bins, **kw)
    try:
        for call in calls:
            recs = [r for _, r in call]
            kr.add(b"".join(recs), np.cumsum([0] + [len(r) for r in recs]).astype(np.uint64), [b for b, _ in call])
        off, keys = kr.finish()
        return kr, off, keys
    except BaseException:
        kr.close()
        raise


def _bins(calls, n_bins):
    out = [[] for _ in range(n_bins)]
    for call in calls:
        for b, r in call:
            out[b].append(r)
    return out


def _expected(calls, n_bins, k, s, t, scaling, wm):
    per_bin = _bins(calls, n_bins)
    return list(POOL.map(lambda recs: oracle_keys(recs, k, s, t, scaling, None if wm is None else wm + k - 1), per_bin))


def _ref_keys(recs, k, s, t):
    parts = [np.zeros(0, np.uint64)] + [orc.ref_seq_to_syncmers(orc.dna4_normalise(r), k, s, t) for r in recs]
    return np.unique(_wyhash(np.concatenate(parts)))


def check_config(calls, n_bins, k, s=0, t=0, wm=None, scaling=1, label=""):
    """run the keyer on `calls`; every bin == the oracle; returns (off, keys, kr) with kr still open"""
    kw = dict(k=k, scaling=scaling)
    kw.update(dict(s=s, t=t) if wm is None else dict(use_syncmer=False, window=wm + k - 1))
    want = _expected(calls, n_bins, k, s, t, scaling, wm)
    kr, off, keys = _run(calls, n_bins, **kw)
    tag = f"{label} k={k} " + (f"s={s} t={t}" if wm is None else f"wm={wm}") + f" scaling={scaling}"
    for b in range(n_bins):
        got = keys[int(off[b]):int(off[b + 1])]
        assert np.all(got[1:] > got[:-1]), f"{tag} bin {b}: keys not strictly ascending"
        if got.size != want[b].size or not np.array_equal(got, want[b]):
            extra, miss = np.setdiff1d(got, want[b]).size, np.setdiff1d(want[b], got).size
            raise AssertionError(f"{tag} bin {b}: {got.size} keys, oracle {want[b].size} ({extra} extra, {miss} missing)")
    st = kr.stats()
    tiles = sum((_nwin(len(r), k, wm) + GT - 1) // GT for c in calls for _, r in c)
    assert st["tiles"] == tiles and st["calls"] == len(calls) and st["keys"] == keys.size, (tag, st, tiles)
    if wm is None and scaling == 1 and REF is not None and k <= 31:
        per_bin = _bins(calls, n_bins)
        ref = list(POOL.map(lambda recs: _ref_keys(recs, k, s, t), per_bin))
        for b in range(n_bins):
            assert np.array_equal(keys[int(off[b]):int(off[b + 1])], ref[b]), f"{tag} bin {b}: differs from the reference's selection"
    return off, keys, kr


# ------------------------------------------------------------------------------------------------ syncmer domain
def _sync_cfgs(k):
    full_t = {(17, 16), (3, 2), (22, 12), (32, 1), (30, 16)}
    out = []
    for s in range(1, min(16, k - 1) + 1):
        w = k - s + 1
        ts = range(1, w + 1) if (k, s) in full_t else sorted({1, w // 2, w})
        out += [(k, s, t) for t in ts]
    return out


BEYOND_16 = [(32, 20), (31, 30), (32, 31), (24, 17), (20, 19)]


def _sweep(cfgs):
    for ci, (k, s, t) in enumerate(cfgs):
        main, sub = _sync_records(k, s, t, ci + 7 * k)
        off, keys, kr = check_config(_calls(main, sub), 6, k, s, t)
        try:
            assert off[6] == off[5], (k, s, t)                             # bin 5: only empty and sub-k records
            assert off[5] > off[4] and off[4] > off[3], (k, s, t)          # bins 3 and 4 have windows of random sequence
        finally:
            kr.close()


@pytest.mark.parametrize("k", range(2, 33))
def test_syncmer_domain(k):
    _sweep(_sync_cfgs(k))


def test_syncmer_beyond_s16():
    """keyer_create admits s > 16 (index_create does not)"""
    cfgs = []
    for k, s in BEYOND_16:
        w = k - s + 1
        cfgs += [(k, s, t) for t in sorted({1, w // 2, w})]
    _sweep(cfgs)


# ------------------------------------------------------------------------------------------------ minimiser domain
@pytest.mark.parametrize("k", range(1, 33))
def test_minimiser_domain(k):
    for wm in sorted({1, 2, 11, 64, 97 - k, 511, 512}):
        assert wm <= GMAX_W
        main, sub = _mini_records(k, wm)
        off, keys, kr = check_config(_calls(main, sub), 6, k, wm=wm)
        try:
            assert off[6] == off[5], (k, wm)
        finally:
            kr.close()


# ------------------------------------------------------------------------------------------------ scaling
SCALED_SYNC = [(22, 12, 5), (32, 1, 16), (15, 5, 1), (2, 1, 1), (30, 16, 7), (21, 11, 11)]
SCALED_MINI = [(20, 1), (32, 65), (1, 96), (13, 512)]


@pytest.mark.parametrize("scaling", [10, 37, 1000])
def test_scaling(scaling):
    """FracMinHash on a subset of the domain; at 1000 some bins with windows end with no key"""
    empty_with_windows = 0
    for ci, (k, s, t) in enumerate(SCALED_SYNC + [(k, 0, 0) for k, _ in SCALED_MINI]):
        wm = SCALED_MINI[ci - len(SCALED_SYNC)][1] if ci >= len(SCALED_SYNC) else None
        main, sub = _sync_records(k, s, t, ci) if wm is None else _mini_records(k, wm)
        calls = _calls(main, sub)
        R = _Reads(ci + scaling)
        calls[1] += [(6, R.rnd(k + 60)), (7, R.rnd(k + 400))]             # small bins
        off, keys, kr = check_config(calls, 8, k, s, t, wm=wm, scaling=scaling)
        kr.close()
        empty_with_windows += sum(int(off[b + 1] == off[b]) for b in (6, 7))
    if scaling == 1000:
        assert empty_with_windows > 0


# ------------------------------------------------------------------------------------------------ compaction and merge edges
def test_finish_compaction_bounds_mid_block():
    """~3000 user bins over three calls, many empty: _finish's dedup compaction runs over bin_off, whose bounds fall in the middle
    of CC_BLOCK-key blocks (a call's own bounds are multiples of REGION_MIN = CC_BLOCK); union_size over subsets of them"""
    n_bins = 3001
    R = _Reads(99)
    rng = np.random.default_rng(99)
    k, s, t = 22, 12, 5
    lens = np.where(rng.random(n_bins) < 0.4, 0, rng.integers(k - 1, 2600, n_bins))
    recs = {b: R.rnd(int(lens[b])) for b in range(n_bins) if lens[b]}
    calls = [[], [], []]
    for b, r in recs.items():
        c = int(rng.integers(0, 3))
        calls[c].append((b, r))
        if b % 7 == 0:                                                      # this bin again in a later call: multi-call dedup
            calls[(c + 1) % 3].append((b, r))
        if b % 11 == 0:
            calls[(c + 2) % 3].append((b, R.rnd(300)))
    for c in calls:
        rng.shuffle(c)
    off, keys, kr = check_config(calls, n_bins, k, s, t)
    try:
        bounds = off[1:-1]
        assert np.count_nonzero(bounds % CC_BLOCK) > 100 and keys.size > 4 * CC_BLOCK
        sets = [keys[int(off[b]):int(off[b + 1])] for b in range(n_bins)]
        empty = [b for b in range(n_bins) if sets[b].size == 0]
        assert len(empty) > 100
        for j in range(12):
            sub = rng.choice(n_bins, size=int(rng.integers(1, 60)), replace=False).tolist()
            sub += sub[:3] + empty[j:j + 2]                                 # repeated and empty bins
            want = np.unique(np.concatenate([sets[b] for b in sub])).size
            assert kr.union_size(sub) == want, sub
        assert kr.union_size(list(range(n_bins))) == np.unique(keys).size
        assert kr.union_size(empty[:5]) == 0 and kr.union_size([]) == 0
    finally:
        kr.close()


def test_adjacent_identical_bins():
    """adjacent bins with identical key sets, each over several calls: the dedup after the sort must not merge the run of equal
    keys across a bin boundary (k_gk_starts).  Bins 1, 2 hold one key each (a homopolymer at t = 1), bins 3, 4 a random set"""
    R = _Reads(5)
    k, s, t = 22, 12, 1
    g = [R.rnd(3000), R.rnd(2500)]
    calls = [[(0, R.rnd(5000)), (1, b"A" * k), (2, b"A" * (k + 3)), (3, g[0]), (4, g[1])],
             [(2, b"A" * k), (4, g[0]), (1, b"A" * (k + 9)), (3, g[1]), (0, R.rnd(100))],
             [(1, b"T" * (k + 1)), (2, b"T" * k), (3, g[0]), (4, g[1])]]
    off, keys, kr = check_config(calls, 5, k, s, t)
    try:
        sets = [keys[int(off[b]):int(off[b + 1])] for b in range(5)]
        assert sets[1].size == 1 and np.array_equal(sets[1], sets[2])
        assert sets[3].size > 100 and np.array_equal(sets[3], sets[4])
        assert kr.union_size([1, 2]) == 1 and kr.union_size([3, 4]) == sets[3].size
    finally:
        kr.close()


def test_one_bin_over_twelve_calls():
    R = _Reads(12)
    k, s, t = 22, 12, 5
    rec = R.rnd(3 * GT + 500)
    calls = [[(0, rec), (1 + c % 3, R.rnd(700))] + ([(4, b"")] if c % 2 else []) for c in range(12)]
    off, keys, kr = check_config(calls, 5, k, s, t)
    try:
        assert off[1] - off[0] == orc.seq_to_syncmers(rec, k, s, t).size and off[5] == off[4]
    finally:
        kr.close()


# ------------------------------------------------------------------------------------------------ the empty-marker key
def _at_cg(R, n):
    """random sequence with (AT)n and (CG)n tracts"""
    g = bytearray(R.rnd(n))
    for p, unit in ((200, b"AT"), (GT - 30, b"CG"), (n // 2, b"GC"), (n - 300, b"TA")):
        g[p:p + 120] = (unit * 60)[:max(0, min(120, n - p))]
    return bytes(g)


@pytest.mark.parametrize("s,t", [(1, 1), (5, 1), (12, 3), (16, 1), (16, 8), (2, 2), (3, 4), (1, 32)])
def test_marker_key(s, t):
    """k = 32 syncmers over (AT)n and (CG)n: the key 2^64 - 1 (the empty marker of the per-bin sets) appears exactly once, last, in
    every bin that met it, over one call (bin 3) or several (bins 0, 1, 4); a bin whose only key is the marker (bin 2, t = 1);
    union_size counts it once"""
    k = 32
    R = _Reads(s * 100 + t)
    a, b, c = _at_cg(R, 3 * GT), _at_cg(R, 5000), _at_cg(R, 2000)
    only = b"AT" * 16 if t == 1 else b"CG" * 40
    calls = [[(0, a), (1, b), (3, _at_cg(R, 4000)), (2, only)],
             [(1, c), (4, b), (0, a), (2, b"GC" * 16 if t == 1 else b"TA" * 50)],
             [(1, b), (4, R.rnd(100))]]
    want = _expected(calls, 5, k, s, t, 1, None)
    assert all(MARKER in want[b_] for b_ in range(5)), [MARKER in w_ for w_ in want]
    off, keys, kr = check_config(calls, 5, k, s, t, label="marker")
    try:
        sets = [keys[int(off[b_]):int(off[b_ + 1])] for b_ in range(5)]
        for b_ in range(5):
            assert np.count_nonzero(sets[b_] == MARKER) == 1 and sets[b_][-1] == MARKER, b_
        if t == 1:
            assert sets[2].tolist() == [MARKER]                            # the marker as a bin's only key
        assert kr.union_size(list(range(5))) == np.unique(keys).size
        assert kr.union_size([2, 0, 2]) == np.unique(np.concatenate([sets[0], sets[2]])).size
    finally:
        kr.close()
    # FracMinHash: wyhash(2^64 - 1) = 2^64 - 1 is above every limit, so the marker is always dropped (the oracle agrees)
    off10, keys10, kr10 = check_config(calls, 5, k, s, t, scaling=10, label="marker")
    kr10.close()
    assert not np.any(keys10 == MARKER) and all(MARKER not in w_ for w_ in _expected(calls, 5, k, s, t, 10, None))


def test_marker_only_bins_adjacent():
    """bins whose only key is the marker, side by side and each over several calls, next to a bin with keys in several calls"""
    R = _Reads(3)
    k, s, t = 32, 7, 1
    r = R.rnd(3000)
    calls = [[(0, r), (1, b"AT" * 16), (2, b"TA" * 16)], [(2, b"AT" * 20), (0, r), (1, b"CG" * 16)], [(1, b"GC" * 16), (3, b"CG" * 30)]]
    off, keys, kr = check_config(calls, 4, k, s, t, label="marker-only")
    try:
        for b in (1, 2, 3):
            assert keys[int(off[b]):int(off[b + 1])].tolist() == [MARKER], b
        assert kr.union_size([1, 2, 3]) == 1 and kr.union_size([0, 1, 2]) == off[1] - off[0] + 1
    finally:
        kr.close()


# ------------------------------------------------------------------------------------------------ refusals and alphabet
def _create_code(n_bins=4, **kw):
    try:
        GenomeKeyer(n_bins, **kw).close()
    except TaxorError as e:
        return e.code
    return 0


def test_keyer_create_refuses_the_domain_edges():
    assert _create_code(k=32, s=16, t=17) == 0 and _create_code(k=32, use_syncmer=False, window=32 + GMAX_W - 1) == 0
    assert _create_code(k=33, s=12, t=5) == E_ARG
    assert _create_code(k=22, s=0, t=1) == E_ARG
    assert _create_code(k=22, s=22, t=1) == E_ARG
    assert _create_code(k=22, s=12, t=0) == E_ARG
    assert _create_code(k=22, s=12, t=12) == E_ARG                          # t = w + 1
    assert _create_code(k=33, use_syncmer=False, window=40) == E_ARG
    assert _create_code(k=20, use_syncmer=False, window=19) == E_ARG        # window < k
    assert _create_code(k=20, use_syncmer=False, window=20 + GMAX_W) == E_ARG
    assert _create_code(n_bins=0, k=22, s=12, t=5) == E_ARG


def _add_code(kr, bases, off, bins):
    try:
        kr.add(bases, off, bins)
    except TaxorError as e:
        return e.code
    return 0


def test_keyer_add_and_union_refusals():
    R = _Reads(1)
    kr = GenomeKeyer(3, k=22, s=12, t=5)
    try:
        b = R.rnd(300)
        assert _add_code(kr, b, [0, 200, 100, 300], [0, 1, 2]) == E_ARG   # decreasing offsets
        assert _add_code(kr, b, [0, 100, 300], [0, 3]) == E_ARG             # bin >= n_bins
        with pytest.raises(TaxorError) as e:
            kr.union_size([0])                                                # before finish
        assert e.value.code == E_ARG
        assert _add_code(kr, b, [0, 100, 300], [0, 2]) == 0
        off, keys = kr.finish()
        assert _add_code(kr, b, [0, 300], [1]) == E_ARG                     # after finish
        with pytest.raises(TaxorError) as e:
            kr.union_size([0, 3])
        assert e.value.code == E_ARG
        assert kr.union_size([0, 2]) == np.unique(keys).size
    finally:
        kr.close()


@pytest.mark.parametrize("use_syncmer", [True, False])
def test_alphabet_every_byte(use_syncmer):
    """each of the 256 byte values inside a record: TAXOR_E_ALPHABET exactly when the oracle's dna4 normalisation refuses it,
    otherwise the oracle's keys"""
    R = _Reads(256)
    k, s, t, wm = 15, 7, 3, 5
    kw = dict(k=k, s=s, t=t) if use_syncmer else dict(k=k, use_syncmer=False, window=wm + k - 1)
    left, right = R.rnd(40), R.rnd(40)
    for v in range(256):
        rec = left + bytes([v]) + right
        try:
            orc.dna4_normalise(rec)
            bad = False
        except ValueError:
            bad = True
        calls = [[(0, R.rnd(50)), (1, rec)]]
        if bad:
            kr = GenomeKeyer(2, **kw)
            try:
                assert _add_code(kr, b"".join(r for _, r in calls[0]), [0, 50, 50 + len(rec)], [0, 1]) == E_ALPHABET, v
            finally:
                kr.close()
        else:
            _, _, kr = check_config(calls, 2, k, s, t, wm=None if use_syncmer else wm, label=f"byte {v}")
            kr.close()
