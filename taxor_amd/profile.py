"""`taxor profile`'s device pipeline from Python (taxor_amd/csrc/profile.hip): the three filtering rounds and the EM of the
reference's taxor_profile.cpp over a CSR read -> matches, with the per-stage outputs the stage tests compare."""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import check


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def _arr(ptr, n, dtype):
    return np.ctypeslib.as_array(ptr, shape=(n,)).astype(dtype, copy=True) if n and ptr else np.zeros(0, dtype)


def run_profile(read_off, ref, ref_len, hash_match, query_len, hash_count, n_refs, em_steps=100, device=0, trace=True):
    """Reads and references in byte-wise name order, matches in file order, ref -1 = the '-' line.  Returns a dict of the
    arrays of taxor_profile_results (include/taxor_gpu_tools.h); with trace also alive_round1..3 and iter_ref_nts
    [em_iterations, n_refs].  Raises TaxorError for the inputs the reference leaves undefined."""
    off = np.ascontiguousarray(read_off, dtype=np.uint64)
    r = np.ascontiguousarray(ref, dtype=np.int32)
    rl = np.ascontiguousarray(ref_len, dtype=np.uint64)
    hm = np.ascontiguousarray(hash_match, dtype=np.uint64)
    ql = np.ascontiguousarray(query_len, dtype=np.uint64)
    hc = np.ascontiguousarray(hash_count, dtype=np.uint64)
    assert off.size == ql.size + 1 == hc.size + 1 and r.size == rl.size == hm.size == int(off[-1])
    csr = _lib.ProfileCsr(ql.size, int(n_refs), r.size, _p(off), _p(r), _p(rl), _p(hm), _p(ql), _p(hc))
    h = C.c_void_p()
    L = _lib.lib()
    check(L.taxor_gpu_profile_create(device, C.byref(csr), C.byref(h)))
    try:
        return _run_and_collect(L, h, em_steps, trace)
    finally:
        L.taxor_gpu_profile_destroy(h)


def _run_and_collect(L, h, em_steps, trace):
    check(L.taxor_gpu_profile_run(h, int(em_steps), _lib.PROFILE_TRACE if trace else 0))
    o = _lib.ProfileResults()
    check(L.taxor_gpu_profile_results(h, C.byref(o)))
    M, F = int(o.n_matches), int(o.n_refs)
    out = dict(ref=_arr(o.ref, M, np.int32), ref_len=_arr(o.ref_len, M, np.uint64), alive=_arr(o.alive, M, np.uint8),
               best=_arr(o.best, M, np.uint8), has_prior=_arr(o.has_prior, F, np.uint8), taxa_len=_arr(o.taxa_len, F, np.uint64),
               ref_nts=_arr(o.ref_nts, F, np.uint64), log_prior=_arr(o.log_prior, F, np.float64),
               explained_by=_arr(o.explained_by, F, np.int32), unique_reads=_arr(o.unique_reads, F, np.uint32),
               all_reads=_arr(o.all_reads, F, np.uint32), all_nts=int(o.all_nts), unclassified_nts=int(o.unclassified_nts),
               log_unclassified=float(o.log_unclassified), em_steps_needed=int(o.em_steps_needed), em_iterations=int(o.em_iterations),
               pair_slots=int(o.pair_slots), pair_key=_arr(o.pair_key, int(o.n_pairs), np.uint64),
               pair_count=_arr(o.pair_count, int(o.n_pairs), np.uint32), seconds_filter=float(o.seconds_filter),
               seconds_em=float(o.seconds_em))
    if trace:
        for k in ("alive_round1", "alive_round2", "alive_round3"):
            out[k] = _arr(getattr(o, k), M, np.uint8)
        out["iter_ref_nts"] = _arr(o.iter_ref_nts, int(o.em_iterations) * F, np.uint64).reshape(int(o.em_iterations), F)
    return out


def rank_read_ids(ids):
    """rank_of_read for ProfileFeed.finish: the position of every read id (bytes, or str encoded as UTF-8) in byte-wise order,
    bytes compared as unsigned like std::string::operator<.  A read id that occurs twice is refused: the feed cannot merge two
    reads into one the way the TSV route does."""
    b = [x.encode() if isinstance(x, str) else bytes(x) for x in ids]
    order = sorted(range(len(b)), key=b.__getitem__)
    for i, j in zip(order, order[1:]):
        if b[i] == b[j]:
            raise ValueError(f"read id {b[i].decode(errors='replace')} occurs twice (reads {i} and {j}); search-to-profile in one run "
                             "needs unique read ids")
    rank = np.empty(len(b), np.uint64)
    rank[np.asarray(order, np.int64)] = np.arange(len(b), dtype=np.uint64)
    return rank


class ProfileFeed:
    """Search results -> the profile's CSR on the device, without the TSV (taxor_amd/csrc/profile_feed.hip).  ref_of_bin[u] = dense
    id of user bin u's accession (ids in byte-wise order of the distinct accessions), ref_len_of_bin[u] = its seq_len.  Batches are
    added in any order under the index of their first read; finish() takes the reads' ranks (rank_read_ids), runs the profile and
    returns run_profile's dictionary plus the finished CSR: read_off, user_bin, csr_ref, csr_ref_len, hash_match, query_len,
    hash_count (ref / ref_len in the dictionary are the profile's, after round 3's renames)."""

    def __init__(self, ref_of_bin, ref_len_of_bin, n_refs, device=0):
        rb = np.ascontiguousarray(ref_of_bin, dtype=np.int32)
        rl = np.ascontiguousarray(ref_len_of_bin, dtype=np.uint64)
        assert rb.size == rl.size
        self._L = _lib.lib()
        self._h = C.c_void_p()
        check(self._L.taxor_gpu_profile_feed_create(device, rb.size, _p(rb), _p(rl), int(n_refs), C.byref(self._h)))

    def add_csr(self, first_read, read_off, user_bin, count, n_hashes, query_len, keep_all=False):
        """tuples of read r at [read_off[r], read_off[r+1]) of user_bin / count (read_off[0] need not be 0: a slice of a larger CSR
        over the same tuple arrays)"""
        off = np.ascontiguousarray(read_off, dtype=np.uint64)
        ub = np.ascontiguousarray(user_bin, dtype=np.int64)
        cnt = np.ascontiguousarray(count, dtype=np.uint32)
        nh = np.ascontiguousarray(n_hashes, dtype=np.uint32)
        ql = np.ascontiguousarray(query_len, dtype=np.uint64)
        assert off.size == nh.size + 1 == ql.size + 1 and ub.size == cnt.size and (off.size == 0 or int(off[-1]) <= ub.size)
        check(self._L.taxor_gpu_profile_feed_add_csr(self._h, int(first_read), nh.size, _p(off), _p(ub), _p(cnt), _p(nh), _p(ql),
                                                     _lib.FEED_KEEP_ALL if keep_all else 0))

    def add_batch(self, searcher, first_read, keep_all=False):
        """the results of the Searcher's last run, where they lie on the device"""
        check(self._L.taxor_gpu_profile_feed_add_batch(self._h, searcher._h, int(first_read), _lib.FEED_KEEP_ALL if keep_all else 0))

    def finish(self, rank_of_read, em_steps=100, trace=True, run=True):
        """run=False: only the finished CSR (the stages refuse some inputs the reference leaves undefined)"""
        rank = np.ascontiguousarray(rank_of_read, dtype=np.uint64)
        p = C.c_void_p()
        check(self._L.taxor_gpu_profile_feed_finish(self._h, _p(rank), rank.size, C.byref(p)))
        try:
            csr = _lib.ProfileCsr()
            ub = C.POINTER(C.c_int64)()
            check(self._L.taxor_gpu_profile_feed_matches(self._h, C.byref(csr), C.byref(ub)))
            R, M = int(csr.n_reads), int(csr.n_matches)

            def host(ptr, n, ctype, dtype):
                return _arr(C.cast(ptr, C.POINTER(ctype)), n, dtype)

            fin = dict(read_off=host(csr.read_off, R + 1, C.c_uint64, np.uint64), user_bin=_arr(ub, M, np.int64),
                       csr_ref=host(csr.ref, M, C.c_int32, np.int32), csr_ref_len=host(csr.ref_len, M, C.c_uint64, np.uint64),
                       hash_match=host(csr.hash_match, M, C.c_uint64, np.uint64), query_len=host(csr.query_len, R, C.c_uint64, np.uint64),
                       hash_count=host(csr.hash_count, R, C.c_uint64, np.uint64))
            if not run:
                return fin
            out = _run_and_collect(self._L, p, em_steps, trace)
            out.update(fin)
            return out
        finally:
            self._L.taxor_gpu_profile_destroy(p)

    def close(self):
        if self._h:
            self._L.taxor_gpu_profile_feed_destroy(self._h)
            self._h = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
