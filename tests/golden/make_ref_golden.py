#!/usr/bin/env python3
"""Writes tests/golden/ref_vectors.npz: what the REFERENCE's own object code returns for the inputs of tests/test_oracle_ref.py,
so that those tests hold the oracle and the product's host functions against the reference on any machine, also where the
reference's sources are absent.  The values come from oracle/_ref/libtaxor_ref.so (`make -C oracle ref REF=<reference checkout>`,
see oracle/ref_driver.cpp); nothing of the reference's sources is stored, only its answers.
It also writes tests/golden/ref_syncmers.npz: the reference's own syncmer selector (src/hashing/syncmer.cpp, built against the
stand-ins of oracle/ref_standin/ into oracle/_ref/libtaxor_ref_syncmer.so; its hash is the identity, so it returns the selected
canonical k-mers) over a stored read set at every admitted (k, s) and t in sync_ts(k, s).  Read by tests/test_syncmer_ref_cpu.py.
Run:  python tests/golden/make_ref_golden.py          (needs both libraries; `... syncmers` writes ref_syncmers.npz alone)"""
import ctypes as C
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

from oracle import oracle as orc  # noqa: E402

# the inputs (tests/test_oracle_ref.py reads them back from the file)
SMR_K = np.arange(12, 31, 2)
SMR_E100 = np.arange(0, 2001)
SMR_EXTRA_ERR = np.array([0.15, 0.05, 0.04, 0.1, 0.2, 0.0, 0.07, 0.29 / 2])       # fp-rounding-sensitive row indices at k = 22
THR_K = np.array([16, 20, 22, 31, 32])
THR_ERR = np.array([0.001, 0.01, 0.04, 0.1, 0.2, 0.5])
THR_SF = np.array([1e-3, 0.05, 1 / 7, 0.5, 0.999])
XOR_N = (1, 2, 10, 1000, 50000)
SLICES = ((1024, 32), (1000, 32), (31, 32), (5, 3), (1, 1), (0, 4), (1024, 7))


def thr_ns():
    rng = np.random.default_rng(3)
    return np.array([0, 1, 2, 3, 5, 7, 10, 20, 50, 99, 100, 435, 871, 4981, 9979, 99979, 10**6] + [int(x) for x in rng.integers(0, 300000, 400)],
                    dtype=np.uint64)


def canonical_nan(a):
    """one bit pattern for every NaN (the test's NaN == NaN), so that a digest compares the tables value for value"""
    a = np.array(a, dtype=np.float64)
    a[np.isnan(a)] = np.nan
    return a


def digest(*arrays):
    import hashlib
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


# ---- ref_syncmers.npz ---------------------------------------------------------------------------------------------------------
def sync_domain():
    """every (k, s) taxor_gpu_index_create admits for a syncmer index: 2 <= k <= 32, 1 <= s <= 16, s < k, w = k-s+1 <= 32"""
    return [(k, s) for k in range(2, 33) for s in range(1, 17) if s < k and k - s + 1 <= 32]


def sync_ts(k, s):
    """t in {1, 2, w//2 (the build default, taxor_build.cpp:510), ceil(w/2), w-1, w, w+1}, distinct and >= 1"""
    w = k - s + 1
    return sorted({t for t in (1, 2, w // 2, (w + 1) // 2, w - 1, w, w + 1) if t >= 1})


# configurations whose full vectors are stored, so that a failure there names the read and the position
SYNC_DIAG = ((22, 12, 5), (5, 1, 2), (9, 3, 4), (16, 8, 1), (27, 11, 17), (31, 16, 16), (32, 16, 8))


def sync_reads():
    """the stored read set: every length 1..33 (shorter than k, k, k+1 for every k), random reads up to a few kb, homopolymers,
    (AT)n, TTAGGG repeats, low-complexity mixes, and reads with N, IUPAC codes, lower case and U"""
    rng = np.random.default_rng(20261016)
    acgt = np.frombuffer(b"ACGT", np.uint8)
    rnd = lambda n: bytes(rng.choice(acgt, size=int(n)))
    reads = [rnd(n) for n in range(1, 34)]
    reads += [rnd(n) for n in (63, 64, 65, 100, 257, 511, 1000, 2048, 3001, 4100)]
    reads += [b"A" * 300, b"C" * 77, b"AT" * 200, b"TTAGGG" * 150, b"CCCTAA" * 40 + b"TTAGGG" * 40, b"ACGTTGCA" * 80,
              b"AAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAC" * 12]
    for _ in range(4):                                     # low-complexity mixes: random runs, homopolymers, short repeat units
        parts, tot, n = [], 0, int(rng.integers(800, 1600))
        while tot < n:
            c = rng.random()
            if c < 0.3:
                p = rnd(rng.integers(3, 60))
            elif c < 0.6:
                p = bytes([int(rng.choice(acgt))]) * int(rng.integers(5, 90))
            else:
                p = rnd(rng.integers(2, 7)) * int(rng.integers(3, 40))
            parts.append(p)
            tot += len(p)
        reads.append(b"".join(parts)[:n])
    for frac, alphabet in ((0.01, b"N"), (0.05, b"N"), (0.02, b"NRYKMSWBDHV"), (0.03, b"acgtuUn")):
        r = bytearray(rnd(1500))
        for p in rng.integers(0, len(r), size=max(1, int(len(r) * frac))):
            r[int(p)] = int(rng.choice(np.frombuffer(alphabet, np.uint8)))
        reads.append(bytes(r))
    reads += [b"ACGTACGTAC" + b"N" * 40 + b"ACGT" * 30, b"N" * 50, b"ACGT" * 8 + b"NN" + b"ACGT" * 8 + b"N" + b"TTAGGG" * 20]
    return reads


def sync_digest(values):
    import hashlib
    return np.frombuffer(hashlib.sha256(np.ascontiguousarray(values, dtype=np.uint64).tobytes()).digest(), np.uint8)


def wyhash_np(x):
    """orc_wyhash_u64 over a uint64 array (lo64 ^ hi64 of x * 0x9E3779B97F4A7C15), checked against the oracle below"""
    x = np.asarray(x, dtype=np.uint64)
    m32, c = np.uint64(0xFFFFFFFF), np.uint64(0x9E3779B97F4A7C15)
    s32 = np.uint64(32)
    a_lo, a_hi, b_lo, b_hi = x & m32, x >> s32, c & m32, c >> s32
    ll, lh, hl, hh = a_lo * b_lo, a_lo * b_hi, a_hi * b_lo, a_hi * b_hi
    mid = (ll >> s32) + (lh & m32) + (hl & m32)
    lo = (ll & m32) | (mid << s32)
    hi = hh + (lh >> s32) + (hl >> s32) + (mid >> s32)
    return lo ^ hi


def write_syncmers():
    if orc.ref_syncmer_lib() is None:
        raise SystemExit("oracle/_ref/libtaxor_ref_syncmer.so is not built (make -C oracle ref REF=<reference checkout>)")
    probe = np.random.default_rng(1).integers(0, 2**64, size=1000, dtype=np.uint64)
    assert wyhash_np(probe).tolist() == [orc.wyhash(int(v)) for v in probe]
    reads = sync_reads()
    offs = np.cumsum([0] + [len(r) for r in reads]).astype(np.uint32)
    cfg = np.array([(k, s, t) for k, s in sync_domain() for t in sync_ts(k, s)], dtype=np.uint8)
    counts = np.zeros((len(cfg), len(reads)), np.uint16)
    sha_kmer = np.zeros((len(cfg), 32), np.uint8)
    sha_hash = np.zeros((len(cfg), 32), np.uint8)
    g = {}
    for c, (k, s, t) in enumerate(cfg.tolist()):
        vals = [orc.ref_seq_to_syncmers(r, k, s, t) for r in reads]
        counts[c] = [v.size for v in vals]
        allv = np.concatenate(vals)
        sha_kmer[c] = sync_digest(allv)
        sha_hash[c] = sync_digest(wyhash_np(allv))
        if (k, s, t) in SYNC_DIAG:
            g[f"diag_{k}_{s}_{t}"] = allv
    g.update(bases=np.frombuffer(b"".join(reads), np.uint8), offsets=offs, cfg=cfg, counts=counts, sha_kmer=sha_kmer,
             sha_hash=sha_hash, diag=np.array(SYNC_DIAG, np.uint8))
    path = os.path.join(HERE, "ref_syncmers.npz")
    np.savez_compressed(path, **g)
    print(f"{path}: {len(cfg)} configurations x {len(reads)} reads ({offs[-1]} bases), {os.path.getsize(path)} bytes")


def main():
    if sys.argv[1:] == ["syncmers"]:
        return write_syncmers()
    write_syncmers()
    R = orc.ref_lib()
    if R is None:
        raise SystemExit("oracle/_ref/libtaxor_ref.so is not built (make -C oracle ref REF=<reference checkout>)")
    g = {"smr_k": SMR_K, "smr_e100": SMR_E100, "smr_extra_err": SMR_EXTRA_ERR}
    g["smr_table"] = np.array([[R.ref_syncmer_match_ratio(int(k), e / 10000.0) for e in SMR_E100] for k in SMR_K])
    g["smr_extra"] = np.array([R.ref_syncmer_match_ratio(22, float(e)) for e in SMR_EXTRA_ERR])
    ns = thr_ns()
    g.update(thr_k=THR_K, thr_err=THR_ERR, thr_sf=THR_SF, thr_n=ns)
    g["nmut_kmer_ci_high"] = np.array([[[R.ref_nmut_kmer_ci_high(float(e), int(k), int(n), 0.95) for n in ns] for e in THR_ERR] for k in THR_K],
                                      dtype=np.uint64)
    low = np.array([[[[R.ref_containment_index_ci_low(float(e), int(k), int(n), float(sf), 0.95) for sf in THR_SF]
                       for n in ns] for e in THR_ERR] for k in THR_K])
    g["containment_index_ci_low_sha256"] = np.array(digest(canonical_nan(low)))          # 62 550 doubles: their digest, not 460 kB
    g["normal_cdf_inverse_0975"] = np.array(R.ref_normal_cdf_inverse(0.975))
    g["adjust_seed"] = np.array([R.ref_adjust_seed(k) for k in range(1, 33)], dtype=np.uint64)
    # the in-repo XOR-filter prototype: the test's keys, probes and foreign keys, and what the prototype answers for them
    rng = np.random.default_rng(5)
    for n in XOR_N:
        keys = np.unique(rng.integers(0, 2**63, size=n, dtype=np.uint64))
        seed, blk, arr = C.c_uint64(), C.c_uint64(), C.c_uint64()
        h = R.ref_xor_build(keys.ctypes.data, keys.size, C.byref(seed), C.byref(blk), C.byref(arr))
        assert h, "prototype construction failed"
        fps = np.ctypeslib.as_array(R.ref_xor_fingerprints(h), shape=(int(arr.value),)).copy()
        probe = np.concatenate([keys[:200], rng.integers(0, 2**64, size=200, dtype=np.uint64)])
        rows, fp = (C.c_uint64 * 3)(), C.c_uint8()
        prow, pfp = np.zeros((probe.size, 3), np.uint64), np.zeros(probe.size, np.uint8)
        for i, key in enumerate(probe):
            R.ref_xor_probe(h, int(key), rows, C.byref(fp))
            prow[i], pfp[i] = list(rows), fp.value
        others = rng.integers(0, 2**64, size=20000, dtype=np.uint64)[:3000]
        # the keys are drawn again by the test from the same generator; the digest says they are the ones answered for here
        g.update({f"xor{n}_inputs_sha256": np.array(digest(keys, probe, others)), f"xor{n}_seed": np.array(seed.value, np.uint64),
                  f"xor{n}_blk": np.array(blk.value, np.uint64), f"xor{n}_fingerprints": fps[:3 * blk.value], f"xor{n}_probe_rows": prow,
                  f"xor{n}_probe_fp": pfp, f"xor{n}_others_contained": np.array(sum(R.ref_xor_contain(h, int(x)) for x in others))})
        R.ref_xor_free(h)
    # hixf::do_parallel's slices, observed from its object code
    for n, th in SLICES:
        out = np.zeros(2 * th, dtype=np.uint64)
        R.ref_do_parallel_slices(n, th, out.ctypes.data_as(C.c_void_p))
        g[f"slices_{n}_{th}"] = out
    path = os.path.join(HERE, "ref_vectors.npz")
    np.savez_compressed(path, **g)
    print(f"{path}: {len(g)} arrays, {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
