"""The oracle's syncmer selector against the REFERENCE's own selector for s-mer sizes 17 to 31 (34- to 62-bit s-mer values).

tests/golden/ref_syncmers_wide.npz (tests/golden/make_ref_golden_wide.py) holds what the reference's hashing::seq_to_syncmers
selects for a stored read set at every (k, s) with 17 <= s < k <= 32 -- 120 pairs -- and t in {1, 2, w//2, ceil(w/2), w-1, w,
w+1}, in the layout of ref_syncmers.npz (tests/test_syncmer_ref_cpu.py): per-read counts, a SHA-256 of the selected canonical
k-mers and one of their wyhash, and full vectors for a few configurations.  The read set has random, tie-heavy and N / IUPAC
reads and the "high-bit" reads: periodic reads with sparse substitutions on which s-mers of one window agree in their low 32 bits
and differ only above them, with their reverse complements.  The oracle is held to the stored answers for k <= 31; k = 32 is
the documented divergence of test_syncmer_ref_cpu.py (the reference's kmask is 0 there) and is asserted in the same way.  This
pins the oracle over the range before any GPU result is compared with it."""
import hashlib
import os

import numpy as np
import pytest

from oracle import oracle as orc

HERE = os.path.dirname(os.path.abspath(__file__))
PATH = os.path.join(HERE, "golden", "ref_syncmers_wide.npz")
G = np.load(PATH)
REF = orc.ref_syncmer_lib()

BASES, OFFS = G["bases"].tobytes(), G["offsets"].astype(np.int64)
READS = [BASES[OFFS[i]:OFFS[i + 1]] for i in range(OFFS.size - 1)]
CFG = [tuple(int(x) for x in c) for c in G["cfg"]]
ROW = {c: i for i, c in enumerate(CFG)}
N_HIGH = int(G["n_high_bit"])
_COMP = bytes.maketrans(b"ACGT", b"TGCA")


def _digest(values):
    return hashlib.sha256(np.ascontiguousarray(values, dtype=np.uint64).tobytes()).digest()


def _ts(k, s):
    w = k - s + 1
    return sorted({t for t in (1, 2, w // 2, (w + 1) // 2, w - 1, w, w + 1) if t >= 1})


def test_fixture_covers_the_wide_domain():
    pairs = [(k, s) for k in range(18, 33) for s in range(17, 32) if s < k]
    assert len(pairs) == 120
    assert CFG == [(k, s, t) for k, s in pairs for t in _ts(k, s)]
    lens = {len(r) for r in READS}
    assert set(range(1, 34)) <= lens                        # shorter than s, k - 1, k and k + 1 for every k
    assert any(b"N" in r for r in READS) and any(set(r) & set(b"RYKMSWBDHV") for r in READS)
    assert G["counts"].max() > 0
    assert os.path.getsize(PATH) <= os.path.getsize(os.path.join(HERE, "golden", "ref_syncmers.npz"))


def test_high_bit_reads_are_what_they_claim():
    """the last N_HIGH reads come in (read, reverse complement) pairs; every read holds two 17-mers (and two 31-mers) with equal
    last 16 bases and different bases before them -- a whole unit of 16 apart in the first pair (neighbouring windows), and
    fewer than 16 starts apart, inside one window of up to 16 s-mers, in the reads of the shorter units"""
    hb = READS[-N_HIGH:]
    assert N_HIGH >= 8 and N_HIGH % 2 == 0
    for a, b in zip(hb[0::2], hb[1::2]):
        assert b == a.translate(_COMP)[::-1]
    for s in (17, 31):
        for n, r in enumerate(hb):
            found = False
            reach = 17 if n < 2 else 16
            for i in range(len(r) - s + 1):
                for j in range(i + 1, min(i + reach, len(r) - s + 1)):
                    if r[i + s - 16:i + s] == r[j + s - 16:j + s] and r[i:i + s - 16] != r[j:j + s - 16]:
                        found = True
                        break
                if found:
                    break
            assert found, (s, r[:40])


def _check_config(k, s, t):
    c = ROW[(k, s, t)]
    got = [orc.seq_to_syncmers(r, k, s, t) for r in READS]
    cnt = np.array([g.size for g in got])
    bad = np.flatnonzero(cnt != G["counts"][c])
    assert bad.size == 0, f"k={k} s={s} t={t}: read {bad[0]} (len {len(READS[bad[0]])}): oracle {cnt[bad[0]]} vs reference {G['counts'][c][bad[0]]}"
    assert _digest(np.concatenate(got)) == G["sha_hash"][c].tobytes(), f"k={k} s={s} t={t}: same counts, different values"
    if REF is not None:          # the stored answers are the library's (the fixture against a rebuild)
        vals = [orc.ref_seq_to_syncmers(r, k, s, t) for r in READS]
        assert [v.size for v in vals] == G["counts"][c].tolist(), (k, s, t)
        assert _digest(np.concatenate(vals)) == G["sha_kmer"][c].tobytes(), (k, s, t)


@pytest.mark.parametrize("k", range(18, 32))
def test_oracle_selector_is_the_references_wide(k):
    cfgs = [c for c in CFG if c[0] == k]
    assert cfgs
    for k_, s, t in cfgs:
        _check_config(k_, s, t)


@pytest.mark.parametrize("kst", [tuple(int(x) for x in d) for d in G["diag"] if int(d[0]) <= 31])
def test_oracle_selector_diagnostic_vectors_wide(kst):
    """full stored vectors: a mismatch names the read and the position within its selection"""
    k, s, t = kst
    c = ROW[kst]
    allv = G[f"diag_{k}_{s}_{t}"]
    ends = np.cumsum(G["counts"][c].astype(np.int64))
    assert ends[-1] == allv.size
    for i, r in enumerate(READS):
        want = [orc.wyhash(int(v)) for v in allv[ends[i] - G["counts"][c][i]:ends[i]]]
        got = orc.seq_to_syncmers(r, k, s, t).tolist()
        assert len(got) == len(want), (kst, i, len(got), len(want))
        for j, (a, b) in enumerate(zip(got, want)):
            assert a == b, f"{kst}: read {i} (len {len(r)}), selection {j}: oracle {a:#x} vs wyhash(reference) {b:#x}"


def test_high_bit_reads_strand_symmetry():
    """Open-syncmer selection is strand-symmetric only for an odd w with t = (w+1)/2 (the minimum at offset t-1 of a window lies
    at offset w-t of the reversed one) AND windows whose minimum is unique: the reference breaks ties by position (leftmost in
    the first window, rightmost after a rescan), which is not mirrored on the other strand.  So a read and its reverse complement
    give the same hash set exactly where the reference's own selection does -- stated here on the reference's stored counts: the
    periodic high-bit reads are tie-heavy, and at symmetric t some pairs agree and some do not; the oracle follows the
    reference on both strands (test_oracle_selector_is_the_references_wide), which is the property the GPU tests hold."""
    hb = READS[-N_HIGH:]
    same = differ = 0
    for k, s, t in ((19, 17, 2), (21, 17, 3), (31, 17, 8), (26, 24, 2), (32, 24, 5), (31, 29, 2), (32, 30, 2)):
        for a, b in zip(hb[0::2], hb[1::2]):
            ha, hb_ = orc.seq_to_syncmers(a, k, s, t), orc.seq_to_syncmers(b, k, s, t)
            assert ha.size > 0 and hb_.size > 0
            if set(ha.tolist()) == set(hb_.tolist()):
                same += 1
            else:
                differ += 1
    assert same > 0 and differ > 0, (same, differ)


def test_k32_divergence_wide():
    """k = 32: the stored reference answer is empty or [0] for every read (kmask = 0), exactly where the oracle selects
    anything; the oracle keeps the full-mask reading"""
    k32 = [c for c in CFG if c[0] == 32]
    assert {s for _, s, _ in k32} == set(range(17, 32))
    many = 0
    for k, s, t in k32:
        c = ROW[(k, s, t)]
        ref_cnt = G["counts"][c]
        assert set(ref_cnt.tolist()) <= {0, 1}, (k, s, t)
        assert G["sha_kmer"][c].tobytes() == _digest(np.zeros(int(ref_cnt.sum()), np.uint64)), (k, s, t)
        got = [orc.seq_to_syncmers(r, k, s, t) for r in READS]
        assert [int(g.size > 0) for g in got] == ref_cnt.tolist(), (k, s, t)
        many += sum(g.size > 1 for g in got)
        if REF is not None:
            for r, n in zip(READS, ref_cnt):
                assert orc.ref_seq_to_syncmers(r, k, s, t).tolist() == [0] * int(n), (k, s, t)
    assert many > 0
