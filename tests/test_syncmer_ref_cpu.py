"""The oracle's syncmer selector against the REFERENCE's own selector over the whole admitted syncmer domain.

tests/golden/ref_syncmers.npz holds what hashing::seq_to_syncmers (src/hashing/syncmer.cpp, compiled where it lies with the
reference's flags against the stand-ins of oracle/ref_standin/, whose hash is the identity) selects for a stored read set at
every (k, s) that taxor_gpu_index_create admits (2 <= k <= 32, 1 <= s <= 16, s < k, k-s+1 <= 32) and t in {1, 2, w//2, ceil(w/2),
w-1, w, w+1}: per-read counts, a SHA-256 of the selected canonical k-mers and one of their wyhash, and full vectors for a few
configurations (tests/golden/make_ref_golden.py).  This pins positions, the stateful tie rule, the N reset and the canonical
k-mer for k <= 31; wyhash itself stays the oracle's (unpinned, see oracle/taxor_oracle.h).  Where oracle/_ref/libtaxor_ref_syncmer.so
is at hand the stored answers are also held against it.

k = 32 is a documented divergence: the reference's kmask = (1ULL << 2*k) - 1 (syncmer.cpp:86) shifts by 64 there and comes out 0,
so every selected canonical k-mer is 0 and a read yields nothing or [0].  The reference's own `taxor build` refuses syncmer
indexes with k > 30 (taxor_build.cpp:124-127); the product and the oracle keep the full-mask reading.  test_k32_divergence states
that exactly, so a compiler that changes the reference's behaviour there fails it instead of hiding the exception."""
import hashlib
import importlib.util
import os

import numpy as np
import pytest

from oracle import oracle as orc

HERE = os.path.dirname(os.path.abspath(__file__))
G = np.load(os.path.join(HERE, "golden", "ref_syncmers.npz"))
REF = orc.ref_syncmer_lib()

BASES, OFFS = G["bases"].tobytes(), G["offsets"].astype(np.int64)
READS = [BASES[OFFS[i]:OFFS[i + 1]] for i in range(OFFS.size - 1)]
CFG = [tuple(int(x) for x in c) for c in G["cfg"]]
ROW = {c: i for i, c in enumerate(CFG)}


def _digest(values):
    return hashlib.sha256(np.ascontiguousarray(values, dtype=np.uint64).tobytes()).digest()


def _ts(k, s):
    w = k - s + 1
    return sorted({t for t in (1, 2, w // 2, (w + 1) // 2, w - 1, w, w + 1) if t >= 1})


def test_fixture_covers_the_admitted_domain():
    want = [(k, s, t) for k in range(2, 33) for s in range(1, 17) if s < k and k - s + 1 <= 32 for t in _ts(k, s)]
    assert CFG == want
    assert len({(k, s) for k, s, _ in CFG}) == 376
    lens = {len(r) for r in READS}
    assert set(range(1, 34)) <= lens                        # shorter than k, k and k+1 for every k
    assert any(b"N" in r for r in READS) and any(set(r) & set(b"RYKMSWBDHV") for r in READS)
    assert any(set(r) & set(b"acgtuU") for r in READS)
    assert G["counts"].max() > 0


def _check_config(k, s, t):
    """one stored configuration: oracle counts per read, then the digest of its hashes in read order"""
    c = ROW[(k, s, t)]
    got = [orc.seq_to_syncmers(r, k, s, t) for r in READS]
    cnt = np.array([g.size for g in got])
    bad = np.flatnonzero(cnt != G["counts"][c])
    assert bad.size == 0, f"k={k} s={s} t={t}: read {bad[0]} (len {len(READS[bad[0]])}): oracle {cnt[bad[0]]} vs reference {G['counts'][c][bad[0]]}"
    if _digest(np.concatenate(got)) != G["sha_hash"][c].tobytes():
        msg = f"k={k} s={s} t={t}: same counts, different values"
        if REF is not None:
            for i, r in enumerate(READS):
                want = [orc.wyhash(int(v)) for v in orc.ref_seq_to_syncmers(r, k, s, t)]
                if got[i].tolist() != want:
                    j = next(j for j in range(len(want)) if got[i][j] != want[j])
                    msg += f"; first at read {i}, selection {j}"
                    break
        raise AssertionError(msg)
    if REF is not None:          # the stored answers are the library's (the fixture against a rebuild)
        vals = [orc.ref_seq_to_syncmers(r, k, s, t) for r in READS]
        assert [v.size for v in vals] == G["counts"][c].tolist(), (k, s, t)
        assert _digest(np.concatenate(vals)) == G["sha_kmer"][c].tobytes(), (k, s, t)


@pytest.mark.parametrize("k", range(2, 32))
def test_oracle_selector_is_the_references(k):
    """every stored (s, t) at this k: orc.seq_to_syncmers == wyhash of the reference's selection, counts, order and values;
    reads with N and IUPAC codes go in raw (the reset branch, syncmer.cpp:147-153)"""
    cfgs = [c for c in CFG if c[0] == k]
    assert cfgs
    for k_, s, t in cfgs:
        _check_config(k_, s, t)


@pytest.mark.parametrize("kst", [tuple(int(x) for x in d) for d in G["diag"] if int(d[0]) <= 31])
def test_oracle_selector_diagnostic_vectors(kst):
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
        if REF is not None:
            assert orc.ref_seq_to_syncmers(r, k, s, t).tolist() == allv[ends[i] - len(want):ends[i]].tolist(), (kst, i)


def _python_restatement():
    spec = importlib.util.spec_from_file_location("make_golden", os.path.join(HERE, "golden", "make_golden.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_k32_divergence():
    """k = 32: the stored reference answer is empty or [0] for every read (kmask = 0, syncmer.cpp:86), exactly where the
    oracle selects anything; the oracle keeps the full-mask reading, which the independent Python restatement shares"""
    k32 = [c for c in CFG if c[0] == 32]
    assert {s for _, s, _ in k32} == set(range(1, 17))
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
    assert many > 0           # the divergence is real: the full-mask reading selects more than one k-mer somewhere
    mg = _python_restatement()
    for k, s, t in ((32, 16, 8), (32, 1, 1), (32, 9, 24)):
        for r in READS[33:45]:
            assert orc.seq_to_syncmers(r, k, s, t).tolist() == mg.seq_to_syncmers(r.decode(), k, s, t), (k, s, t, len(r))


def test_k32_palindromes_hash_to_the_empty_marker():
    """wyhash(x) = lo64 ^ hi64 of x * 0x9E3779B97F4A7C15 is 2^64 - 1 exactly for x = 0x33..33, 0x66..66, 0x99..99, 0xCC..CC: the
    32-mers (AT)^16, (CG)^16, (GC)^16, (TA)^16, each its own reverse complement.  2^64 - 1 is the empty-slot marker of the
    device key sets (keyset.h), so k = 32 syncmers over (AT)n or (CG)n emit the marker as a key; the GPU tests of the keyer
    and the builder rest on this"""
    marker = 2**64 - 1
    assert [orc.wyhash(int(c * 16, 16)) for c in "369C"] == [marker] * 4
    assert orc.wyhash(marker) == marker                       # FracMinHash drops it at every scaling > 1
    for unit in (b"AT", b"CG", b"GC", b"TA"):
        assert orc.seq_to_syncmers(unit * 16, 32, 1, 1).tolist() == [marker], unit
    for s in range(1, 17):
        assert orc.seq_to_syncmers(b"AT" * 40, 32, s, 1).tolist() == [marker], s
