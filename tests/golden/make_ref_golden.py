#!/usr/bin/env python3
"""Writes tests/golden/ref_vectors.npz: what the REFERENCE's own object code returns for the inputs of tests/test_oracle_ref.py,
so that those tests hold the oracle and the product's host functions against the reference on any machine, also where the
reference's sources are absent.  The values come from oracle/_ref/libtaxor_ref.so (`make -C oracle ref REF=<reference checkout>`,
see oracle/ref_driver.cpp); nothing of the reference's sources is stored, only its answers.
Run:  python tests/golden/make_ref_golden.py          (needs oracle/_ref/libtaxor_ref.so)"""
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


def main():
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
