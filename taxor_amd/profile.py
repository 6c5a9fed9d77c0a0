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
    finally:
        L.taxor_gpu_profile_destroy(h)
