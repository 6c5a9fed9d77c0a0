"""Bottom-m sketches of key lists and all-pairs shared / union counts on the device (taxor_amd/csrc/sketch.hip; DESIGN.md section 9,
"Similarity-aware layout") against a numpy reference.  The mixer is restated here from DESIGN.md."""
import functools

import numpy as np
import pytest

from taxor_amd.genome_keys import keys_sketch, sketch_pairs

pytestmark = pytest.mark.gpu
U64 = np.uint64
MAX = U64(2**64 - 1)


def mix(x):
    """x += 0x9E3779B97F4A7C15; x = (x ^ x >> 30) * 0xBF58476D1CE4E5B9; x = (x ^ x >> 27) * 0x94D049BB133111EB; x ^ x >> 31"""
    with np.errstate(over="ignore"):
        x = np.asarray(x, U64) + U64(0x9E3779B97F4A7C15)
        x = (x ^ (x >> U64(30))) * U64(0xBF58476D1CE4E5B9)
        x = (x ^ (x >> U64(27))) * U64(0x94D049BB133111EB)
        return x ^ (x >> U64(31))


def unmix(v):
    """the inverse of mix: keys whose mixed values are chosen"""
    def unshift(x, s):
        r, t = x.copy(), x >> U64(s)
        while t.any():
            r ^= t
            t = t >> U64(s)
        return r

    with np.errstate(over="ignore"):
        x = unshift(np.asarray(v, U64), 31) * U64(pow(0x94D049BB133111EB, -1, 2**64))
        x = unshift(x, 27) * U64(pow(0xBF58476D1CE4E5B9, -1, 2**64))
        return unshift(x, 30) - U64(0x9E3779B97F4A7C15)


def test_the_reference_mixer_is_a_bijection_with_its_inverse():
    x = np.r_[np.random.default_rng(1).integers(0, 2**64, 1000, dtype=U64), U64(0), MAX]
    assert np.array_equal(unmix(mix(x)), x) and np.array_equal(mix(unmix(x)), x)
    assert int(mix(U64(0))) == 0xE220A8397B1DCDAF          # splitmix64's first output from state 0


def distinct(rng, n, lo=0, hi=2**64):
    out = np.unique(rng.integers(lo, hi, int(n * 1.01) + 8, dtype=U64))
    assert out.size >= n
    return np.sort(rng.permutation(out)[:n])


@functools.lru_cache(maxsize=None)
def sketch_case(m):
    """bins of 0, 1, m-1, m, m+1, 5m and 200 000 keys -- random 64-bit keys with 0 and 2^64 - 1 among them, and the small
    consecutive integers a k-mer scheme gives -- and two bins whose mixed values all lie in the top of the range, so that the
    first thresholds keep nothing of them.  -> (keys, off, reference sketch rows)"""
    rng = np.random.default_rng(100 + m)
    bins = []
    for n in (0, 1, m - 1, m, m + 1, 5 * m, 200000):
        k = distinct(rng, n, 1, 2**64 - 1)
        if n >= 2:
            k[0], k[-1] = 0, MAX
        bins.append(k)
    bins.append(np.array([MAX], U64))
    bins.append(np.array([0], U64))
    bins.append(np.arange(200000, dtype=U64))
    bins.append(np.sort(unmix(distinct(rng, 5 * m, 2**63, 2**64))))
    bins.append(np.sort(unmix(distinct(rng, 200000, 2**64 - 2**57, 2**64))))
    bins.append(np.zeros(0, U64))
    off = np.cumsum([0] + [b.size for b in bins]).astype(U64)
    ref = [np.sort(mix(b))[:m] for b in bins]
    return np.concatenate(bins), off, ref


@pytest.mark.parametrize("on_device", [False, True], ids=["host-keys", "device-keys"])
@pytest.mark.parametrize("m", [1, 16, 1024])
def test_sketch_equals_the_reference(m, on_device):
    keys, off, ref = sketch_case(m)
    sk, ln = keys_sketch(keys, off, m, on_device=on_device)
    assert sk.shape == (off.size - 1, m)
    assert ln.tolist() == [r.size for r in ref]
    for b, r in enumerate(ref):
        assert np.array_equal(sk[b, :r.size], r), f"bin {b}"


def ref_sketches(sets, m):
    sk = np.zeros((len(sets), m), U64)
    ln = np.zeros(len(sets), np.uint32)
    for i, s in enumerate(sets):
        v = np.sort(mix(s))[:m]
        sk[i, :v.size] = v
        ln[i] = v.size
    return sk, ln, np.array([s.size for s in sets], U64)


def ref_pairs(sk, ln, count, m):
    n = ln.size
    rows = [sk[i, :ln[i]] for i in range(n)]
    tau = [MAX if count[i] <= m else rows[i][-1] for i in range(n)]
    shared = np.zeros((n, n), np.uint32)
    uni = np.zeros((n, n), np.uint32)
    for a in range(n):
        for b in range(n):
            t = min(tau[a], tau[b])
            x, y = rows[a][rows[a] <= t], rows[b][rows[b] <= t]
            s = np.intersect1d(x, y, assume_unique=True).size
            shared[a, b] = s
            uni[a, b] = x.size + y.size - s
    return shared, uni


def pair_sets(n, m, seed):
    """complete and truncated sketches, empty bins, identical bins, disjoint bins, a bin nested in another; complete ones next to
    truncated ones.  The overlapping bins draw from one pool of 6m keys"""
    rng = np.random.default_rng(seed)
    pool = distinct(rng, 6 * m)
    sets = []
    for i in range(n):
        t = i % 8
        if t == 0:
            s = rng.choice(pool, int(rng.integers(1, m + 1)), replace=False)          # complete
        elif t == 1:
            s = rng.choice(pool, int(rng.integers(m + 1, 3 * m + 1)), replace=False)  # truncated
        elif t == 2:
            s = np.zeros(0, U64)                                                      # empty
        elif t == 3:
            s = sets[i - 2].copy()                                                    # identical to the truncated one
        elif t == 4:
            s = distinct(rng, m // 2 + 1)                                             # disjoint from everything, complete
        elif t == 5:
            s = rng.choice(sets[i - 4], max(1, sets[i - 4].size // 2), replace=False)   # nested in the truncated one
        elif t == 6:
            s = rng.choice(pool, m, replace=False)                                    # complete, exactly m keys
        else:
            s = distinct(rng, 2 * m)                                                  # disjoint, truncated
        sets.append(np.sort(np.asarray(s, U64)))
    return sets


@functools.lru_cache(maxsize=None)
def pairs_case(n, m):
    sk, ln, count = ref_sketches(pair_sets(n, m, 1000 * m + n), m)
    return sk, ln, count, ref_pairs(sk, ln, count, m)


@pytest.mark.parametrize("m", [16, 1024])
@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 130])
def test_pairs_equal_the_reference(n, m):
    sk, ln, count, (shared, uni) = pairs_case(n, m)
    got_s, got_u = sketch_pairs(sk, ln, count)
    assert np.array_equal(got_s, shared)
    assert np.array_equal(got_u, uni)


@pytest.mark.parametrize("m", [16, 1024])
@pytest.mark.parametrize("n", [1, 65, 130])
def test_pairs_are_symmetric_and_the_diagonal_is_the_length(n, m):
    sk, ln, count, _ = pairs_case(n, m)
    got_s, got_u = sketch_pairs(sk, ln, count)
    assert np.array_equal(got_s, got_s.T) and np.array_equal(got_u, got_u.T)
    assert np.array_equal(np.diag(got_s), ln) and np.array_equal(np.diag(got_u), ln)
    empty = np.flatnonzero(ln == 0)
    assert not got_s[np.ix_(empty, empty)].any() and not got_u[np.ix_(empty, empty)].any()


def test_complete_sketches_give_the_exact_jaccard_index():
    m, n = 64, 24
    rng = np.random.default_rng(3)
    pool = distinct(rng, 150)
    sets = [np.sort(rng.choice(pool, int(rng.integers(0, m + 1)), replace=False)) for _ in range(n - 2)]
    sets += [np.array([0, MAX], U64), np.array([MAX], U64)]
    off = np.cumsum([0] + [s.size for s in sets]).astype(U64)
    sk, ln = keys_sketch(np.concatenate(sets), off, m)
    shared, uni = sketch_pairs(sk, ln, np.diff(off))
    for a in range(n):
        for b in range(n):
            inter, union = np.intersect1d(sets[a], sets[b]).size, np.union1d(sets[a], sets[b]).size
            assert (shared[a, b], uni[a, b]) == (inter, union)
            if union:
                assert shared[a, b] / uni[a, b] == inter / union


def test_pairs_refuse_lengths_that_do_not_follow_from_the_counts():
    from taxor_amd import _lib
    sk, ln, count, _ = pairs_case(2, 16)
    with pytest.raises(_lib.TaxorError, match="sketch values"):
        sketch_pairs(sk, ln, np.zeros_like(count))
