#!/usr/bin/env python3
"""Writes tests/golden/ref_syncmers_wide.npz: the reference's own syncmer selector (oracle/_ref/libtaxor_ref_syncmer.so, see
make_ref_golden.py) over a stored read set at every (k, s) with 17 <= s < k <= 32 -- s-mer values of 34 to 62 bits, the range
beyond 32-bit s-mers -- and t in sync_ts(k, s).  Same layout as ref_syncmers.npz: per-read counts, a SHA-256 of the selected
canonical k-mers and one of their wyhash per configuration, full vectors for a few.  Nothing of the reference's sources is
stored, only its answers.  Read by tests/test_syncmer_wide_ref_cpu.py.
Run:  python tests/golden/make_ref_golden_wide.py     (needs oracle/_ref/libtaxor_ref_syncmer.so)"""
import importlib.util
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

from oracle import oracle as orc  # noqa: E402

_spec = importlib.util.spec_from_file_location("make_ref_golden", os.path.join(HERE, "make_ref_golden.py"))
base = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(base)
sync_ts, sync_digest, wyhash_np = base.sync_ts, base.sync_digest, base.wyhash_np

WIDE_DIAG = ((28, 20, 4), (18, 17, 1), (24, 17, 4), (31, 30, 1), (30, 26, 2), (32, 31, 1))

_COMP = bytes.maketrans(b"ACGT", b"TGCA")


def wide_domain():
    """every (k, s) with 17 <= s < k <= 32: 120 pairs, w = k-s+1 in 2..16"""
    return [(k, s) for k in range(18, 33) for s in range(17, 32) if s < k]


def revcomp(r):
    return r.translate(_COMP)[::-1]


def high_bit_reads(seed, n_units=40):
    """Reads on which s-mers of ONE window agree in their low 32 bits (their last 16 bases) and differ only above bit 31, and
    their reverse complements, on which the difference lies only below: a unit of 16, 8, 4 or 2 random bases repeated (every
    one of them 16-periodic, so s-mers a unit apart are equal) with single substitutions 41 bases apart, more than 16, so that
    at most one falls into the part of an s-mer above its last 16 bases and its phase within the unit moves along the read."""
    rng = np.random.default_rng(seed)
    acgt = np.frombuffer(b"ACGT", np.uint8)
    out = []
    for unit_len in (16, 8, 4, 2):
        unit = bytes(rng.choice(acgt, size=unit_len))
        while len(set(unit)) < 2:
            unit = bytes(rng.choice(acgt, size=unit_len))
        r = bytearray(unit * (16 * n_units // unit_len))
        for p in range(int(rng.integers(0, 41)), len(r), 41):
            r[p] = int(rng.choice([c for c in acgt if c != r[p]]))
        out += [bytes(r), revcomp(bytes(r))]
    return out


def wide_reads():
    """every length 1..33, random reads up to a few kb, tie-heavy reads, N / IUPAC / lower-case reads, the high-bit reads"""
    rng = np.random.default_rng(20261019)
    acgt = np.frombuffer(b"ACGT", np.uint8)
    rnd = lambda n: bytes(rng.choice(acgt, size=int(n)))
    reads = [rnd(n) for n in range(1, 34)]
    reads += [rnd(n) for n in (63, 64, 65, 257, 1000, 2100)]
    reads += [b"A" * 200, b"AT" * 120, b"TTAGGG" * 80, b"ACGTTGCA" * 50, b"AAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAC" * 8]
    for _ in range(2):
        parts, tot, n = [], 0, int(rng.integers(800, 1400))
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
    for frac, alphabet in ((0.01, b"N"), (0.02, b"NRYKMSWBDHV"), (0.03, b"acgtuUn")):
        r = bytearray(rnd(1200))
        for p in rng.integers(0, len(r), size=max(1, int(len(r) * frac))):
            r[int(p)] = int(rng.choice(np.frombuffer(alphabet, np.uint8)))
        reads.append(bytes(r))
    reads += [b"ACGTACGTAC" * 4 + b"N" * 40 + b"ACGT" * 30, b"N" * 50]
    return reads + high_bit_reads(17)


def main():
    if orc.ref_syncmer_lib() is None:
        raise SystemExit("oracle/_ref/libtaxor_ref_syncmer.so is not built (make -C oracle ref REF=<reference checkout>)")
    reads = wide_reads()
    offs = np.cumsum([0] + [len(r) for r in reads]).astype(np.uint32)
    cfg = np.array([(k, s, t) for k, s in wide_domain() for t in sync_ts(k, s)], dtype=np.uint8)
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
        if (k, s, t) in WIDE_DIAG:
            g[f"diag_{k}_{s}_{t}"] = allv
    g.update(bases=np.frombuffer(b"".join(reads), np.uint8), offsets=offs, cfg=cfg, counts=counts, sha_kmer=sha_kmer,
             sha_hash=sha_hash, diag=np.array(WIDE_DIAG, np.uint8), n_high_bit=np.array(len(high_bit_reads(17))))
    path = os.path.join(HERE, "ref_syncmers_wide.npz")
    np.savez_compressed(path, **g)
    print(f"{path}: {len(cfg)} configurations x {len(reads)} reads ({offs[-1]} bases), {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
