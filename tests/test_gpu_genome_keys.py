"""The device keyer of `taxor build` (taxor_amd/csrc/genome_keys.hip) against the oracle, user bin by user bin, as sets: the union
over a bin's records of oracle.seq_to_syncmers (syncmer mode) or oracle.minimiser_hash (minimiser mode), FracMinHash-filtered,
sorted ascending.  Tie-heavy tracts straddle the keyer's tile edges (2048 windows), so a tile whose first windows depend on the
previous tile's history is resolved exactly."""
import numpy as np
import pytest

from oracle import oracle as orc
from taxor_amd.genome_keys import GenomeKeyer

pytestmark = pytest.mark.gpu
TILE = 2048


def rand_seq(rng, n):
    return np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, n)].tobytes()


def with_tracts(rng, n):
    """random sequence with a homopolymer, (AT)n, TTAGGG and a three-tile homopolymer laid across tile edges"""
    g = bytearray(rand_seq(rng, n))
    for pos, tract in ((TILE - 150, b"A" * 400), (2 * TILE - 37, b"AT" * 1500), (5 * TILE - 300, b"TTAGGG" * 700),
                       (8 * TILE - 5, b"C" * (2 * TILE + 900)), (12 * TILE - 1, b"GA" * 9)):
        if pos + len(tract) <= n:
            g[pos:pos + len(tract)] = tract
    return bytes(g)


def messy(rng, n):
    """IUPAC codes, N runs and lowercase in random sequence"""
    g = bytearray(rand_seq(rng, n))
    iupac = b"NRYSWKMBDHVNacgtnrykmu"
    for p in rng.integers(0, n, n // 40):
        g[p] = iupac[int(rng.integers(0, len(iupac)))]
    for p in rng.integers(0, n - 200, 6):
        g[p:p + 150] = b"N" * 150
    return bytes(g)


def oracle_keys(records, k, s, t, scaling, minimiser_w=None):
    parts = [np.zeros(0, np.uint64)]
    for r in records:
        nr = orc.dna4_normalise(r)
        parts.append(orc.minimiser_hash(nr, k, minimiser_w) if minimiser_w else orc.seq_to_syncmers(nr, k, s, t))
    u = np.unique(np.concatenate(parts))
    if scaling > 1:
        lim = float(2**64 - 1) / scaling
        u = u[np.array([float(orc.wyhash(int(x))) <= lim for x in u], dtype=bool)]
    return u


def run_keyer(calls, n_bins, **kw):
    """calls: list of lists of (bin, record bytes)"""
    kr = GenomeKeyer(n_bins, **kw)
    for call in calls:
        recs = [r for _, r in call]
        off = np.cumsum([0] + [len(r) for r in recs]).astype(np.uint64)
        kr.add(b"".join(recs), off, [b for b, _ in call])
    off, keys = kr.finish()
    return kr, off, keys


def bins_of(calls, n_bins):
    out = [[] for _ in range(n_bins)]
    for call in calls:
        for b, r in call:
            out[b].append(r)
    return out


def check(calls, n_bins, k, s, t, scaling, minimiser_w=None, ref=False):
    kw = dict(k=k, scaling=scaling)
    kw.update(dict(use_syncmer=False, window=minimiser_w) if minimiser_w else dict(s=s, t=t))
    kr, off, keys = run_keyer(calls, n_bins, **kw)
    per_bin = bins_of(calls, n_bins)
    for b in range(n_bins):
        got = keys[int(off[b]):int(off[b + 1])]
        assert np.all(got[1:] > got[:-1]), f"bin {b}: keys not strictly ascending"
        want = oracle_keys(per_bin[b], k, s, t, scaling, minimiser_w)
        assert got.size == want.size and np.array_equal(got, want), f"bin {b}: {got.size} keys, oracle {want.size}"
        if ref and not minimiser_w and scaling == 1:
            refk = [orc.ref_seq_to_syncmers(orc.dna4_normalise(r), k, s, t) for r in per_bin[b]]
            if all(x is not None for x in refk):
                hs = np.unique(np.array([orc.wyhash(int(x)) for r in refk for x in r], dtype=np.uint64))
                assert np.array_equal(got, hs)
    # a second run is byte-identical
    kr2, off2, keys2 = run_keyer(calls, n_bins, **kw)
    assert np.array_equal(off, off2) and keys.tobytes() == keys2.tobytes()
    st = kr.stats()
    assert st["keys"] == keys.size and st["bases"] == sum(len(r) for c in calls for _, r in c)
    kr.close()
    kr2.close()
    return off, keys


def mixed_calls(rng, k):
    """several user bins per call, one bin over three calls, an empty bin, records of 1 and k - 1 bases"""
    g2 = [with_tracts(rng, 9 * TILE + 333) for _ in range(3)]
    return [
        [(0, b"A"), (1, with_tracts(rng, 14 * TILE + 77)), (0, rand_seq(rng, k - 1)), (2, g2[0]), (3, messy(rng, 30000))],
        [(2, g2[1]), (0, with_tracts(rng, 5 * TILE)), (4, b"ACGTN" * 2000)],
        [(2, g2[2]), (4, b"acgtnRYKM" * 500), (0, b"C" * (k + 3))],
    ]


@pytest.mark.parametrize("k,s", [(22, 12), (15, 5), (30, 26), (21, 11)])
@pytest.mark.parametrize("scaling", [1, 10])
def test_syncmer_keys_match_the_oracle(k, s, scaling):
    rng = np.random.default_rng(k * 100 + s + scaling)
    t = (k - s + 1) // 2
    off, keys = check(mixed_calls(rng, k), 6, k, s, t, scaling, ref=(scaling == 1))
    assert off[6] == off[5]                                              # bin 5 has no records


@pytest.mark.parametrize("k,w", [(20, 20), (19, 31)])
@pytest.mark.parametrize("scaling", [1, 10])
def test_minimiser_keys_match_the_oracle(k, w, scaling):
    rng = np.random.default_rng(k * 100 + w + scaling)
    check(mixed_calls(rng, k), 6, k, 0, 0, scaling, minimiser_w=w)


def test_genome_sized_records():
    """3 Mb and 13 Mb records (thousands of tiles each), with tie tracts, next to small genomes in one call"""
    rng = np.random.default_rng(7)
    big = bytearray(rand_seq(rng, 13_000_000))
    for j in range(40):
        p = int(rng.integers(1, 13_000_000 // TILE - 3)) * TILE - int(rng.integers(0, 60))
        tract = (b"A", b"AT", b"TTAGGG", b"CG")[j % 4] * int(rng.integers(100, 3 * TILE))
        big[p:p + len(tract)] = tract[:max(0, min(len(tract), len(big) - p))]
    calls = [[(0, with_tracts(rng, 3_000_000)), (1, bytes(big)), (2, rand_seq(rng, 5000)), (0, rand_seq(rng, 20000))]]
    check(calls, 3, 22, 12, 5, 1)


def test_union_size_is_exact():
    rng = np.random.default_rng(3)
    base = rand_seq(rng, 60000)
    calls = [[(0, base), (1, base[:30000] + rand_seq(rng, 10000)), (2, rand_seq(rng, 40000))]]
    kr, off, keys = run_keyer(calls, 3, k=22, s=12, t=5)
    sets = [keys[int(off[b]):int(off[b + 1])] for b in range(3)]
    assert kr.union_size([0, 1]) == np.union1d(sets[0], sets[1]).size < sets[0].size + sets[1].size
    assert kr.union_size([0, 1, 2]) == np.unique(keys).size
    assert kr.union_size([]) == 0
    kr.close()
