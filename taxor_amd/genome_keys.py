"""`taxor build`'s two library stages from Python (taxor_amd/csrc/genome_keys.hip, host_util.cpp): the device keyer -- whole genomes
-> the distinct, FracMinHash-filtered, ascending keys of every user bin -- and the IXF layout over their counts."""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import check


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


class GenomeKeyer:
    """Accumulates records (ASCII bases, any number of add() calls; a user bin's records may span calls); finish() -> CSR.
    Syncmer mode uses t = (k - s + 1) // 2 unless t is given (taxor_build.cpp:509-510)."""

    def __init__(self, n_bins, k=22, s=12, t=None, use_syncmer=True, window=None, scaling=1, device=0):
        if t is None:
            t = (k - s + 1) // 2
        prm = _lib.KeyerParams(k, s if use_syncmer else 0, t if use_syncmer else 0, 1 if use_syncmer else 0,
                               window if window is not None else k, scaling, 0, n_bins)
        h = C.c_void_p()
        check(_lib.lib().taxor_gpu_keyer_create(device, C.byref(prm), C.byref(h)))
        self._h = h
        self.n_bins = n_bins
        self._out = None

    def add(self, bases, rec_off, rec_bin):
        b = np.frombuffer(bases, dtype=np.uint8) if isinstance(bases, (bytes, bytearray)) else np.ascontiguousarray(bases, dtype=np.uint8)
        o = np.ascontiguousarray(rec_off, dtype=np.uint64)
        r = np.ascontiguousarray(rec_bin, dtype=np.uint32)
        assert o.size == r.size + 1
        check(_lib.lib().taxor_gpu_keyer_add(self._h, _p(b) if b.size else None, _p(o), _p(r), r.size))

    def finish(self):
        """(bin_off uint64[n_bins + 1], keys uint64[bin_off[-1]]), each bin ascending"""
        if self._out is None:
            off = C.POINTER(C.c_uint64)()
            keys = C.POINTER(C.c_uint64)()
            dk = C.POINTER(C.c_uint64)()
            check(_lib.lib().taxor_gpu_keyer_finish(self._h, C.byref(off), C.byref(keys), C.byref(dk)))
            o = np.ctypeslib.as_array(off, shape=(self.n_bins + 1,)).copy()
            n = int(o[-1])
            k = np.ctypeslib.as_array(keys, shape=(n,)).copy() if n else np.zeros(0, np.uint64)
            self._out = (o, k)
        return self._out

    def union_size(self, bins):
        b = np.ascontiguousarray(bins, dtype=np.uint32)
        out = C.c_uint64(0)
        check(_lib.lib().taxor_gpu_keyer_union_size(self._h, _p(b), b.size, C.byref(out)))
        return int(out.value)

    def stats(self):
        st = _lib.KeyerStats()
        check(_lib.lib().taxor_gpu_keyer_stats(self._h, C.byref(st)))
        return {name: getattr(st, name) for name, _ in _lib.KeyerStats._fields_}

    def close(self):
        if getattr(self, "_h", None):
            _lib.lib().taxor_gpu_keyer_destroy(self._h)
            self._h = None

    __del__ = close


def keys_union(lists, device=0, want_keys=True, on_device=False):
    """taxor_gpu_keys_union: the duplicate-free union of uint64 key lists through the device set -> (size, sorted keys or None).
    on_device: the lists are first put into device memory and handed over as device pointers, and the union comes back from a
    device buffer (the path a caller with resident keys takes)."""
    L = _lib.lib()
    arrs = [np.ascontiguousarray(a, dtype=np.uint64) for a in lists]
    counts = np.array([a.size for a in arrs], dtype=np.uint64)
    total = int(counts.sum())
    ptrs = (C.c_void_p * max(1, len(arrs)))()
    dev = []
    try:
        for i, a in enumerate(arrs):
            if on_device:
                d = C.c_void_p()
                check(L.taxor_gpu_malloc(device, a.size * 8, C.byref(d)))
                dev.append(d)
                if a.size:
                    check(L.taxor_gpu_memcpy_from_host(d, _p(a), a.size * 8))
                ptrs[i] = d.value
            else:
                ptrs[i] = a.ctypes.data if a.size else None
        n = C.c_uint64(0)
        if not want_keys:
            check(L.taxor_gpu_keys_union(device, ptrs, _p(counts), len(arrs), 1 if on_device else 0, None, 0, 0, C.byref(n)))
            return int(n.value), None
        out = np.empty(max(1, total), dtype=np.uint64)
        if on_device:
            d_out = C.c_void_p()
            check(L.taxor_gpu_malloc(device, out.size * 8, C.byref(d_out)))
            dev.append(d_out)
            check(L.taxor_gpu_keys_union(device, ptrs, _p(counts), len(arrs), 1, d_out, 1, total, C.byref(n)))
            if n.value:
                check(L.taxor_gpu_memcpy_to_host(_p(out), d_out, int(n.value) * 8))
        else:
            check(L.taxor_gpu_keys_union(device, ptrs, _p(counts), len(arrs), 0, _p(out), 0, total, C.byref(n)))
        return int(n.value), out[:int(n.value)].copy()
    finally:
        for d in dev:
            L.taxor_gpu_free(d)


def keys_sketch(keys, off, m, device=0, on_device=False):
    """taxor_gpu_keys_sketch: bottom-m sketches of the bins keys[off[b]:off[b+1]] (distinct keys) -> (sketch uint64[n_bins, m],
    len uint32[n_bins]); row b holds the len[b] = min(m, n_b) smallest mix(key), ascending.  on_device: the keys are first put into
    device memory and handed over as a device pointer."""
    L = _lib.lib()
    k = np.ascontiguousarray(keys, dtype=np.uint64)
    o = np.ascontiguousarray(off, dtype=np.uint64)
    n = o.size - 1
    sk = np.zeros((max(n, 1), int(m)), dtype=np.uint64)
    ln = np.zeros(max(n, 1), dtype=np.uint32)
    d = None
    try:
        if on_device:
            d = C.c_void_p()
            check(L.taxor_gpu_malloc(device, max(k.size, 1) * 8, C.byref(d)))
            if k.size:
                check(L.taxor_gpu_memcpy_from_host(d, _p(k), k.size * 8))
        check(L.taxor_gpu_keys_sketch(device, d if on_device else (_p(k) if k.size else None), 1 if on_device else 0, _p(o), n, int(m), _p(sk), _p(ln)))
    finally:
        if d is not None:
            L.taxor_gpu_free(d)
    return sk[:n], ln[:n]


def sketch_pairs(sketch, length, count, device=0, want_ms=False):
    """taxor_gpu_sketch_pairs: (shared uint32[n, n], uni uint32[n, n]) of n sketches (rows of `sketch`, `length` values each, from
    bins of `count` keys); with want_ms also the kernel's milliseconds."""
    sk = np.ascontiguousarray(sketch, dtype=np.uint64)
    ln = np.ascontiguousarray(length, dtype=np.uint32)
    ct = np.ascontiguousarray(count, dtype=np.uint64)
    n, m = sk.shape
    assert ln.size == n and ct.size == n
    shared = np.zeros((n, n), dtype=np.uint32)
    uni = np.zeros((n, n), dtype=np.uint32)
    ms = C.c_float(0)
    check(_lib.lib().taxor_gpu_sketch_pairs(device, _p(sk), _p(ln), _p(ct), n, m, _p(shared), _p(uni), C.byref(ms)))
    return (shared, uni, float(ms.value)) if want_ms else (shared, uni)


def cluster_order(shared, uni, jmin):
    """taxor_cluster_order (host only): single-linkage clusters of the rows linked by shared >= jmin * uni (uni > 0) ->
    (order uint64[n], cluster uint64[n])."""
    s = np.ascontiguousarray(shared, dtype=np.uint32)
    u = np.ascontiguousarray(uni, dtype=np.uint32)
    n = s.shape[0]
    assert s.shape == (n, n) and u.shape == (n, n)
    order = np.zeros(n, dtype=np.uint64)
    cluster = np.zeros(n, dtype=np.uint64)
    check(_lib.lib().taxor_cluster_order(_p(s), _p(u), n, float(jmin), _p(order), _p(cluster)))
    return order, cluster


def similarity_rank(sketch, length, counts, window=4096, jmin=0.1, device=0):
    """taxor_similarity_rank: the bins in descending count, in windows of `window`, each paired on the device and cluster-ordered ->
    (rank uint64[n], clusters with more than one member)."""
    sk = np.ascontiguousarray(sketch, dtype=np.uint64)
    ln = np.ascontiguousarray(length, dtype=np.uint32)
    ct = np.ascontiguousarray(counts, dtype=np.uint64)
    n, m = sk.shape
    rank = np.zeros(n, dtype=np.uint64)
    multi = C.c_uint64(0)
    check(_lib.lib().taxor_similarity_rank(device, _p(sk), _p(ln), _p(ct), n, m, int(window), float(jmin), _p(rank), C.byref(multi), None))
    return rank, int(multi.value)


def build_layout(counts, t_max=0, rank=None):
    """taxor_build_layout: the IXF tree for these per-user-bin distinct key counts.  Returns a dict with t_max, depth,
    bytes_per_hash, index_bytes and ixfs: [{bins, next_ixf, fname_idx, part, parts}] (IXF 0 = root).  rank (one value per user bin):
    taxor_build_layout_ranked -- the bins that are cut into groups are ordered by it instead of by count."""
    c = np.ascontiguousarray(counts, dtype=np.uint64)
    L = C.POINTER(_lib.Layout)()
    if rank is None:
        check(_lib.lib().taxor_build_layout(_p(c), c.size, int(t_max), C.byref(L)))
    else:
        r = np.ascontiguousarray(rank, dtype=np.uint64)
        assert r.size == c.size
        check(_lib.lib().taxor_build_layout_ranked(_p(c), c.size, int(t_max), _p(r), C.byref(L)))
    try:
        l = L.contents
        first = np.ctypeslib.as_array(l.bin_first, shape=(l.n_ixf + 1,))
        tb = int(l.n_bins_total)
        nx = np.ctypeslib.as_array(l.next_ixf, shape=(tb,))
        fn = np.ctypeslib.as_array(l.fname_idx, shape=(tb,))
        part = np.ctypeslib.as_array(l.part, shape=(tb,))
        parts = np.ctypeslib.as_array(l.parts, shape=(tb,))
        ixfs = []
        for i in range(int(l.n_ixf)):
            a, b = int(first[i]), int(first[i + 1])
            ixfs.append(dict(bins=b - a, next_ixf=nx[a:b].copy(), fname_idx=fn[a:b].copy(), part=part[a:b].copy(), parts=parts[a:b].copy()))
        return dict(t_max=int(l.t_max), depth=int(l.depth), bytes_per_hash=float(l.bytes_per_hash), index_bytes=float(l.index_bytes), ixfs=ixfs)
    finally:
        _lib.lib().taxor_layout_free(L)
