"""The restatement of a saved hash's position in its read (include/taxor_gpu_tools.h, taxor_gpu_search_capture_positions; DESIGN.md
section 10.11), as a plain loop over p:

    pos[i] = min { p in [0, L-k] : wyhash(min(f_p, revcomp(f_p))) == hashes[i] }

with f_p the k-mer at base p of the read after the dna4 mapping.  The hash of one k-mer is the CPU oracle's own: orc_seq_to_syncmers on
the k bases alone with s-mers of k - 1 bases -- a window of two s-mers, whose leftmost minimum stands first (t = 1) or second (t = 2), so
exactly one of the two calls selects the k-mer and returns wyhash(canonical k-mer) as the oracle computes it.  Nothing here restates
wyhash, the reverse complement or the canonical form.  Shared by the position tests."""
import ctypes as C

import numpy as np

from oracle import oracle as orc

SENTINEL = 0xFFFFFFFF


def kmer_hashes(read: bytes, k: int) -> np.ndarray:
    """wyhash(canonical k-mer) at every base p in [0, L-k] of a read (any dna15 letters), from the oracle, one k-mer at a time"""
    seq = orc.dna4_normalise(read)
    n = len(seq) - k + 1
    out = np.zeros(max(n, 0), np.uint64)
    L = orc.lib()
    one = np.zeros(2, np.uint64)
    ptr = one.ctypes.data_as(C.c_void_p)
    for p in range(max(n, 0)):
        kmer = seq[p:p + k]
        got = L.orc_seq_to_syncmers(kmer, k, k, k - 1, 1, ptr, 2)
        if got == 0:
            got = L.orc_seq_to_syncmers(kmer, k, k, k - 1, 2, ptr, 2)
        assert got == 1, (p, kmer)
        out[p] = one[0]
    return out


def positions(read: bytes, hashes, k: int) -> np.ndarray:
    """pos[i] for the read's saved list `hashes`; SENTINEL where no k-mer of the read hashes to it (never, for a list the read emitted)"""
    first = {}
    for p, h in enumerate(kmer_hashes(read, k).tolist()):          # the plain loop over p: the first p wins
        if h not in first:
            first[h] = p
    return np.array([first.get(int(h), SENTINEL) for h in np.asarray(hashes, np.uint64).tolist()], np.uint32)


def batch_positions(reads, hash_off, hashes, k: int) -> np.ndarray:
    """the whole position array of a saved batch: reads in batch order, their lists at hash_off"""
    parts = [np.zeros(0, np.uint32)]
    for r, read in enumerate(reads):
        lo, hi = int(hash_off[r]), int(hash_off[r + 1])
        if hi > lo:
            parts.append(positions(read, hashes[lo:hi], k))
    return np.concatenate(parts)
