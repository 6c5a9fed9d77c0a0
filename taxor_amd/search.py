"""Host-side mirror (Python) of the reference's search interface on top of the C ABI.

Names follow the reference: GpuIndex stands where `taxor_index<hixf_t>` does (src/main/index.hpp:25-287),
Searcher where the worker's `membership_agent` + `threshold` do (src/main/taxor_search.cpp:196-313,
src/hixf/build/hierarchical_interleaved_xor_filter.hpp:290-413).  All computation happens in
libtaxor_gpu.so; this module only marshals numpy arrays."""
import ctypes as C
from dataclasses import dataclass

import numpy as np

from . import _lib
from ._lib import check


def _p(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def threshold_ratio(kmer_size=22, error_rate=0.04, percentage=-1.0):
    """hixf::threshold::threshold + get_min_syncmer_match_ratio (threshold.hpp:22-81, syncmer_model.hpp:38-50)"""
    r = _lib.lib().taxor_threshold_ratio(int(kmer_size), float(error_rate), float(percentage))
    if r < 0:
        raise ValueError(f"no syncmer threshold model for k={kmer_size}, error_rate={error_rate}")
    return r


def threshold(hash_count, ratio):
    return int(_lib.lib().taxor_threshold(int(hash_count), float(ratio)))


def threshold_kind(use_syncmer, kmer_size, window_size, percentage=-1.0):
    """threshold::threshold's choice of model (threshold.hpp:22-47) -> _lib.THR_*"""
    return int(_lib.lib().taxor_threshold_kind(1 if use_syncmer else 0, int(kmer_size), int(window_size), float(percentage)))


def threshold_model(kind, count, kmer_size, error_rate=0.04, percentage=-1.0, scaling_factor=1.0):
    """threshold::get for every kind (threshold.hpp:51-81), host arithmetic identical to the reference's"""
    return int(_lib.lib().taxor_threshold_model(int(kind), int(count), int(kmer_size), float(error_rate), float(percentage),
                                                float(scaling_factor)))


def arith_code(key_hash=0, seed_mode=0, rot=21, reduce=0, fp_mode=0):
    """code of a reading of the un-vendored IXF arithmetic (taxor_ixf_variant's five arithmetic fields); 0 = the library's"""
    v = _lib.IxfVariant(0, 1, 64, key_hash, seed_mode, rot, reduce, fp_mode, 0)
    return int(_lib.lib().taxor_ixf_arith_code(C.byref(v)))


def classify_filter(counts):
    c = np.ascontiguousarray(counts, dtype=np.uint32)
    keep = np.zeros(c.size, dtype=np.uint8)
    _lib.lib().taxor_classify_filter(_p(c), c.size, _p(keep))
    return keep.astype(bool)


@dataclass
class SearchResults:
    """CSR per-read tuples in the reference's DFS emission order, before the 0.8*max filter."""
    read_off: np.ndarray   # uint64[n_reads+1]
    user_bin: np.ndarray   # int64[n_tuples]
    count: np.ndarray      # uint32[n_tuples]
    n_hashes: np.ndarray   # uint32[n_reads]   (QHASH_COUNT)

    def tuples(self, r):
        lo, hi = int(self.read_off[r]), int(self.read_off[r + 1])
        return [(int(a), int(b)) for a, b in zip(self.user_bin[lo:hi], self.count[lo:hi])]


@dataclass
class PassResults:
    """one pass's results of a batch on a paged index, with the tuples' DFS keys: what merge_prior takes"""
    results: SearchResults
    key: np.ndarray        # uint32[n_tuples], ascending within a read


def plan_passes(ixfs, n_user_bins, budget_bytes, **kw):
    """taxor_index_plan_passes (host only) -> (plan dict, pass_of_ixf uint32[n_ixf] with _lib.PASS_ROOT for the root, pass_bytes uint64[n_passes])"""
    view, keep = GpuIndex._view(ixfs, n_user_bins, kw.get("k", 22), kw.get("s", 12), kw.get("t", 5), kw.get("use_syncmer", True), 1, kw.get("window_size"))
    plan = _lib.PassPlan()
    of = np.zeros(len(ixfs), np.uint32)
    by = np.zeros(len(ixfs), np.uint64)
    check(_lib.lib().taxor_index_plan_passes(C.byref(view), int(budget_bytes), C.byref(plan), _p(of), _p(by)))
    del keep
    return {f: int(getattr(plan, f)) for f, _ in _lib.PassPlan._fields_}, of, by[:plan.n_passes].copy()


@dataclass
class FastxResults:
    """search_fastx: status 0 and the reads' results, ids and lengths -- or status FASTX_IRREGULAR and nothing else"""
    status: int
    results: SearchResults = None
    ids: list = None            # bytes per read: the header line without its first character and its terminator
    read_len: np.ndarray = None  # uint64[n_reads]


def _results(res: _lib.Results, copy=True) -> SearchResults:
    """copy=False: views of the library's own result arrays, valid until the next call on that searcher (the C ABI's
    convention; what a C++ host sees) -- for callers that time the library and not numpy's memcpy of 100 MB of tuples"""
    n, t = int(res.n_reads), int(res.n_tuples)
    c = (lambda a: a.copy()) if copy else (lambda a: a)
    ro = c(np.ctypeslib.as_array(res.read_off, shape=(n + 1,)))
    ub = c(np.ctypeslib.as_array(res.user_bin, shape=(t,))) if t else np.zeros(0, np.int64)
    ct = c(np.ctypeslib.as_array(res.count, shape=(t,))) if t else np.zeros(0, np.uint32)
    nh = c(np.ctypeslib.as_array(res.n_hashes, shape=(n,))) if n else np.zeros(0, np.uint32)
    return SearchResults(ro, ub, ct, nh)


def source_bytes(layout, f):
    """bytes a source holds for IXF dict f under layout code `layout` (taxor_amd/csrc/ixf_layout.h ixf_src_bytes)"""
    rows, kind = 3 * f["seg_len"], int(layout) & 0xFF
    # (ixf_layout.h ixf_src_pitch: the explicit pitch, else what the code's pitch rule names -- `bins` when unpadded, the index's stride otherwise)
    pitch = int(f.get("src_stride", 0)) or (f["bins"] if (int(layout) & 0x600) == _lib.LAYOUT_PITCH_BINS else f["stride"])
    if kind == _lib.LAYOUT_BIT_SLICED:
        return rows * ((f["bins"] + 63) // 64) * 64
    return rows * pitch


def to_source_layout(f, layout):
    """numpy restatement of ixf_layout.h, independent of the library: the bytes ANOTHER writer would store for IXF dict f (data in
    the search layout data[row * stride + bin]) under `layout` -> (bytes, src_stride).  Test infrastructure for the re-layout."""
    bins, stride, seg = f["bins"], f["stride"], f["seg_len"]
    rows, kind, rule = 3 * seg, int(layout) & 0xFF, int(layout) & 0x600
    D = np.asarray(f["data"], dtype=np.uint8).reshape(rows, stride)[:, :bins]
    if layout & _lib.LAYOUT_POSITION_MAJOR:          # source row pos*3 + segment holds search row segment*seg_len + pos
        D = D.reshape(3, seg, bins).transpose(1, 0, 2).reshape(rows, bins)
    S = (bins + 63) // 64 * 64
    pitch = S if kind == _lib.LAYOUT_BIT_SLICED else bins if rule == _lib.LAYOUT_PITCH_BINS else stride if rule == _lib.LAYOUT_PITCH_STORED else S
    if kind == _lib.LAYOUT_ROWS:
        out = np.zeros((rows, pitch), np.uint8)
        out[:, :bins] = D
    elif kind == _lib.LAYOUT_BIN_MAJOR:
        out = np.zeros((pitch, rows), np.uint8)
        out[:bins, :] = D.T
    else:
        P = np.zeros((rows, S), np.uint8)
        P[:, :bins] = D
        planes = (P[:, :, None] >> np.arange(8, dtype=np.uint8)[None, None, :]) & 1            # [row][bin][plane]
        planes = planes.reshape(rows, S // 64, 64, 8).transpose(0, 1, 3, 2)                      # [row][group][plane][bin in group]
        out = np.packbits(planes, axis=-1, bitorder="little")                                    # 8 bytes per plane word, little endian
    return np.ascontiguousarray(out).reshape(-1), pitch


class GpuIndex:
    """A HIXF resident in one GPU's HBM."""

    def __init__(self, ixfs, n_user_bins, k=22, s=12, t=5, device=0, use_syncmer=True, scaling=1, window_size=None, arith=0, layout=0):
        """ixfs: list of dicts {bins, stride, seg_len, seed, next_ixf, fname_idx, data (np.uint8 or None)[, src_stride]};
        layout != 0 (_lib.LAYOUT_*): `data` holds the bytes as ANOTHER writer's file would (ixf_layout.h, pitch / column count in
        src_stride); the library transposes them into the search layout on the device while uploading"""
        L = _lib.lib()
        view, keep = self._view(ixfs, n_user_bins, k, s, t, use_syncmer, scaling, window_size, layout)
        view.ixf_arith = int(arith)      # 0 = the library's reading of the IXF arithmetic; else arith_code(...)
        view.ixf_layout = int(layout)
        h = C.c_void_p()
        check(L.taxor_gpu_index_create(C.byref(view), device, C.byref(h)))
        del keep                 # the library copied everything into HBM
        self._adopt(h, ixfs, n_user_bins, k, s, t, device, use_syncmer, window_size)

    @staticmethod
    def _view(ixfs, n_user_bins, k, s, t, use_syncmer, scaling, window_size, layout=0):
        """taxor_hixf_view over numpy arrays (+ the arrays that must stay alive while the library reads it)"""
        keep = []
        arr = (_lib.IxfView * len(ixfs))()
        for i, f in enumerate(ixfs):
            nx = np.ascontiguousarray(f["next_ixf"], dtype=np.int64)
            fn = np.ascontiguousarray(f["fname_idx"], dtype=np.int64)
            assert nx.size == f["bins"] and fn.size == f["bins"]
            d = f.get("data")
            if d is not None:
                d = np.ascontiguousarray(d, dtype=np.uint8)
                assert d.size == source_bytes(layout, f), "IXF data size mismatch"
            keep += [nx, fn, d]
            arr[i] = _lib.IxfView(f["bins"], f["stride"], f["seg_len"], f["seed"],
                                  d.ctypes.data if d is not None else None, nx.ctypes.data, fn.ctypes.data, int(f.get("src_stride", 0)))
        ws = int(window_size) if window_size is not None else k
        keep.append(arr)
        return _lib.HixfView(len(ixfs), arr, n_user_bins, k, s, t, 1 if use_syncmer else 0, scaling, ws), keep

    def _adopt(self, h, ixfs, n_user_bins, k, s, t, device, use_syncmer, window_size):
        self._h = h
        self.use_syncmer = bool(use_syncmer)
        self.window_size = int(window_size) if window_size is not None else k
        self.device = device
        self.k, self.s, self.t = k, s, t
        self.n_ixf = len(ixfs)
        self.n_user_bins = n_user_bins
        self.shapes = [(f["bins"], f["stride"], f["seg_len"]) for f in ixfs]
        self._view_keep = None           # paged(): the view later passes upload from

    @classmethod
    def paged(cls, ixfs, n_user_bins, budget_bytes, k=22, s=12, t=5, device=0, use_syncmer=True, scaling=1, window_size=None, arith=0, layout=0):
        """taxor_gpu_index_create_paged: an index whose slab holds the root and at most two groups of subtrees, at most budget_bytes.
        load_pass(0) comes before the first search; the arrays of `ixfs` stay referenced (later passes upload from them)"""
        view, keep = cls._view(ixfs, n_user_bins, k, s, t, use_syncmer, scaling, window_size, layout)
        view.ixf_arith = int(arith)
        view.ixf_layout = int(layout)
        h = C.c_void_p()
        check(_lib.lib().taxor_gpu_index_create_paged(C.byref(view), device, int(budget_bytes), C.byref(h)))
        g = cls.__new__(cls)
        g._adopt(h, ixfs, n_user_bins, k, s, t, device, use_syncmer, window_size)
        g._view_keep = (view, keep)
        return g

    @property
    def passes(self):
        """number of passes of a paged index, 0 for an ordinary one"""
        return int(_lib.lib().taxor_gpu_index_passes(self._h))

    def load_pass(self, p):
        """make group p the searched one (the next pass, or 0); every search of the pass before must have ended"""
        view = self._view_keep[0] if self._view_keep else _lib.HixfView(self.n_ixf, None, self.n_user_bins)      # an ordinary index: the library refuses
        check(_lib.lib().taxor_gpu_index_load_pass(self._h, C.byref(view), int(p)))

    def close(self):
        if getattr(self, "_h", None):
            _lib.lib().taxor_gpu_index_destroy(self._h)      # (joins an upload in flight before the view's arrays go)
            self._h = None
        self._view_keep = None

    __del__ = close

    @property
    def data_bytes(self):
        return int(_lib.lib().taxor_gpu_index_data_bytes(self._h))

    @property
    def leaf_runs(self):
        return int(_lib.lib().taxor_gpu_index_leaf_runs(self._h))

    @property
    def depth(self):
        return int(_lib.lib().taxor_gpu_index_depth(self._h))

    def gather_ceiling(self, ixf=0, want_bytes=32 << 30, reps=3, span=1):
        """random whole-row reads of IXF `ixf` (or of up to `span` equally shaped IXFs from it on), nothing else
        -> (GB/s requested, bytes read per row[, IXFs covered])"""
        g, rb, used = C.c_double(), C.c_uint64(), C.c_uint64()
        check(_lib.lib().taxor_gpu_gather_ceiling_span(self._h, ixf, int(span), int(want_bytes), int(reps), C.byref(g), C.byref(rb),
                                                       C.byref(used)))
        return (g.value, int(rb.value)) if span == 1 else (g.value, int(rb.value), int(used.value))

    def gather_pattern(self, ixf, pattern, nt, want_bytes=8 << 30, reps=3):
        """known-size launches in the query kernel's access shapes (0 = whole rows, 1 = one 16-B load per row)
        -> (GB/s requested, requested bytes per launch, requests per launch)"""
        g, b, r = C.c_double(), C.c_uint64(), C.c_uint64()
        check(_lib.lib().taxor_gpu_gather_pattern(self._h, ixf, int(pattern), 1 if nt else 0, int(want_bytes), int(reps), C.byref(g),
                                                  C.byref(b), C.byref(r)))
        return g.value, int(b.value), int(r.value)

    def fill_random(self, ixf, seed):
        check(_lib.lib().taxor_gpu_index_fill_random(self._h, ixf, seed))

    def upload_bin(self, ixf, bin_, column):
        col = np.ascontiguousarray(column, dtype=np.uint8)
        check(_lib.lib().taxor_gpu_index_upload_bin(self._h, ixf, bin_, _p(col), col.size))

    def build_ixf(self, ixf, bin_keys, seed0=1):
        """GPU construction of IXF `ixf` in place from {bin: uint64 keys}; returns (seed, peeling rounds)."""
        bins = self.shapes[ixf][0]
        off = np.zeros(bins + 1, dtype=np.uint64)
        parts = []
        for b in range(bins):
            k = np.ascontiguousarray(bin_keys.get(b, np.zeros(0, np.uint64)), dtype=np.uint64)
            parts.append(k)
            off[b + 1] = off[b] + np.uint64(k.size)
        keys = np.concatenate(parts) if parts else np.zeros(0, np.uint64)
        seed, rounds = C.c_uint64(), C.c_uint32()
        check(_lib.lib().taxor_gpu_index_build_ixf(self._h, ixf, _p(keys) if keys.size else None, _p(off), int(seed0),
                                                   C.byref(seed), C.byref(rounds)))
        return int(seed.value), int(rounds.value)

    def build_hixf(self, leaf_keys, seed0=1):
        """GPU construction of the whole hierarchy: leaf_keys = {(ixf, bin): uint64 keys} for leaf bins only; merged
        bins receive the union of their child IXF on the device.  Returns the number of peeling rounds of the slowest IXF."""
        parts, sizes = [], []
        for i, (bins, _, _) in enumerate(self.shapes):
            for b in range(bins):
                k = np.ascontiguousarray(leaf_keys.get((i, b), np.zeros(0, np.uint64)), dtype=np.uint64)
                parts.append(k)
                sizes.append(k.size)
        off = np.zeros(len(sizes) + 1, dtype=np.uint64)
        np.cumsum(np.array(sizes, dtype=np.uint64), out=off[1:])
        keys = np.concatenate(parts) if parts else np.zeros(0, np.uint64)
        rounds = C.c_uint32()
        check(_lib.lib().taxor_gpu_index_build_hixf(self._h, _p(keys) if keys.size else None, _p(off), int(seed0), C.byref(rounds)))
        return int(rounds.value)

    def build_hixf_synth(self, bin_counts, salt=1, seed0=1):
        """GPU construction of the whole hierarchy from SYNTHETIC keys generated on the device: technical bin g (index bin
        order: all bins of IXF 0, then IXF 1, ...) receives the keys synth_key(i, salt) for i in [off[g], off[g+1]), off =
        cumulative bin_counts (merged bins: 0).  Nothing crosses PCIe; a checker regenerates the keys with
        synth.synth_keys_host.  Returns the run's figures (taxor_build_stats) as a dict."""
        L = _lib.lib()
        cnt = np.ascontiguousarray(bin_counts, dtype=np.uint64)
        assert cnt.size == sum(b for b, _, _ in self.shapes)
        off = np.zeros(cnt.size + 1, dtype=np.uint64)
        np.cumsum(cnt, out=off[1:])
        total = int(off[-1])
        d_keys = C.c_void_p()
        check(L.taxor_gpu_malloc(self.device, total * 8, C.byref(d_keys)))
        try:
            check(L.taxor_gpu_synth_keys(self.device, d_keys, 0, total, int(salt)))
            st = _lib.BuildStats()
            check(L.taxor_gpu_index_build_hixf_ex(self._h, d_keys, 1, _p(off), int(seed0), C.byref(st)))
        finally:
            L.taxor_gpu_free(d_keys)
        return {k: getattr(st, k) for k, _ in _lib.BuildStats._fields_ if k != "reserved"}, off

    def build_hixf_host_keys(self, keys, off, seed0=1):
        """GPU construction of the whole hierarchy from keys in HOST memory (what a binding has): keys = uint64 array, off[total_bins + 1]
        per technical bin in index bin order (merged bins: empty).  Returns the run's figures (upload inside seconds_total)."""
        k = np.ascontiguousarray(keys, dtype=np.uint64)
        o = np.ascontiguousarray(off, dtype=np.uint64)
        st = _lib.BuildStats()
        check(_lib.lib().taxor_gpu_index_build_hixf_ex(self._h, _p(k) if k.size else None, 0, _p(o), int(seed0), C.byref(st)))
        return {kk: getattr(st, kk) for kk, _ in _lib.BuildStats._fields_ if kk != "reserved"}

    def build_hixf_stream(self, keys, off, budget_bytes, seed0=1):
        """taxor_gpu_index_build_hixf_stream: the whole hierarchy from keys in HOST memory with at most budget_bytes of them on the
        device at a time (keys, off as for build_hixf_host_keys).  Byte-identical to build_hixf on the same keys and seed0."""
        k = np.ascontiguousarray(keys, dtype=np.uint64)
        o = np.ascontiguousarray(off, dtype=np.uint64)
        st = _lib.BuildStats()
        check(_lib.lib().taxor_gpu_index_build_hixf_stream(self._h, _p(k) if k.size else None, _p(o), int(seed0), int(budget_bytes), C.byref(st)))
        return {kk: getattr(st, kk) for kk, _ in _lib.BuildStats._fields_ if not kk.startswith("reserved")}

    def build_ixf_bins(self, ixf, bin0, bin1, keys, off, seed, flags=0):
        """taxor_gpu_index_build_ixf_bins: bins [bin0, bin1) of one IXF under `seed` (keys in host memory, off[bins + 1] for the
        IXF's bins; keys may be None when only the offsets are to be judged) -> True when every bin of the range peeled"""
        o = np.ascontiguousarray(off, dtype=np.uint64)
        k = None if keys is None else np.ascontiguousarray(keys, dtype=np.uint64)
        ok = C.c_int(0)
        check(_lib.lib().taxor_gpu_index_build_ixf_bins(self._h, ixf, int(bin0), int(bin1), _p(k) if k is not None and k.size else None, 0, _p(o),
                                                        int(seed), int(flags), C.byref(ok)))
        return bool(ok.value)

    def ixf_seed(self, ixf):
        return int(_lib.lib().taxor_gpu_index_ixf_seed(self._h, ixf))

    def root_plane(self):
        """the root's 2-bit plane as the searches see it (derived now if it is stale) -> uint8[rows, plane_stride], or None when the
        root has none"""
        rows, ps = C.c_uint64(), C.c_uint32()
        check(_lib.lib().taxor_gpu_index_root_plane(self._h, None, 0, C.byref(rows), C.byref(ps)))
        if not ps.value:
            return None
        out = np.empty((int(rows.value), int(ps.value)), dtype=np.uint8)
        check(_lib.lib().taxor_gpu_index_root_plane(self._h, _p(out), out.size, C.byref(rows), C.byref(ps)))
        return out

    def download_ixf(self, ixf, out=None):
        bins, stride, seg = self.shapes[ixf]
        if out is None:
            out = np.empty(3 * seg * stride, dtype=np.uint8)
        assert out.dtype == np.uint8 and out.size == 3 * seg * stride and out.flags.c_contiguous
        check(_lib.lib().taxor_gpu_index_download_ixf(self._h, ixf, _p(out), out.size))
        return out

    def census(self, tile_iters=0, max_blocks=0, runs=1) -> "CensusTable":
        """nonzero fingerprint bytes per bin of the resident index (taxor_gpu_census_*, csrc/census.hip): one streaming pass.
        tile_iters / max_blocks: the work list's cut and the grid, 0 = the defaults (neither changes a word); runs > 1 repeats the
        pass on the same object and keeps every run's words (CensusTable.all_runs) and the last one's time"""
        L = _lib.lib()
        h = C.c_void_p()
        check(L.taxor_gpu_census_create(self._h, C.byref(h)))
        try:
            words = []
            for _ in range(max(1, int(runs))):
                r = _lib.CensusResults()
                check(L.taxor_gpu_census_run(h, int(tile_iters), int(max_blocks), C.byref(r)))
                words.append(np.ctypeslib.as_array(r.nonzero, (int(r.n_bins),)).copy() if r.n_bins else np.zeros(0, np.uint64))
            first = np.ctypeslib.as_array(r.bin_first, (int(r.n_ixf) + 1,)).copy()
            t = CensusTable(words[-1], first, float(r.seconds_kernel), int(r.bytes_read), int(r.n_tiles), int(r.launches))
            t.all_runs = words
            return t
        finally:
            L.taxor_gpu_census_destroy(h)


class Searcher:
    """One GPU-side agent: syncmers -> dedup -> threshold -> HIXF query -> per-read tuples."""

    def __init__(self, index: GpuIndex, error_rate=0.04, percentage=-1.0, ratio=None, sub_batch_reads=0,
                 sub_batch_bases=0, time_kernels=False, prune=True, group_always=False, small_path=True, split_always=False,
                 force_tree_stall=False, screen=True):
        self.index = index
        flags = ((0 if prune else _lib.SEARCH_NO_PRUNE) | (_lib.SEARCH_GROUP_ALWAYS if group_always else 0)
                 | (0 if small_path else _lib.SEARCH_NO_SMALL_PATH) | (_lib.SEARCH_SPLIT_ALWAYS if split_always else 0)
                 | (_lib.SEARCH_FORCE_TREE_STALL if force_tree_stall else 0) | (0 if screen else _lib.SEARCH_NO_SCREEN))
        prm = _lib.SearchParams(0.0, sub_batch_reads, sub_batch_bases, 1 if time_kernels else 0, _lib.THR_PERCENTAGE, error_rate, flags)
        if ratio is not None:          # explicit (size_t)(n * ratio), whatever the index
            prm.ratio = float(ratio)
        else:                          # the reference's choice: percentage / syncmer / k-mer / FracMinHash model
            view = _lib.HixfView(0, None, index.n_user_bins, index.k, index.s, index.t, 1 if index.use_syncmer else 0, 1,
                                 index.window_size)
            if _lib.lib().taxor_threshold_select(C.byref(view), float(error_rate), float(percentage), C.byref(prm)) != 0:
                raise ValueError(f"no threshold model for k={index.k}, error_rate={error_rate}")
        self.ratio, self.model = prm.ratio, int(prm.model)
        h = C.c_void_p()
        check(_lib.lib().taxor_gpu_searcher_create(index._h, C.byref(prm), C.byref(h)))
        self._h = h

    def close(self):
        if getattr(self, "_h", None):
            _lib.lib().taxor_gpu_searcher_destroy(self._h)
            self._h = None

    __del__ = close

    @staticmethod
    def _batch(bases, offsets):
        b = np.ascontiguousarray(bases, dtype=np.uint8)
        o = np.ascontiguousarray(offsets, dtype=np.uint64)
        return b, o

    # --- the drop-in batch call ---------------------------------------------------------------------------
    def search_batch(self, bases, offsets, copy=True) -> SearchResults:
        b, o = self._batch(bases, offsets)
        res = _lib.Results()
        check(_lib.lib().taxor_gpu_search_batch(self._h, _p(b), _p(o), o.size - 1, C.byref(res)))
        return _results(res, copy)

    def search_batch_begin(self, bases, offsets):
        """enqueue the drop-in call; keep the arrays alive until search_batch_end()"""
        b, o = self._batch(bases, offsets)
        self._inflight = (b, o)
        check(_lib.lib().taxor_gpu_search_batch_begin(self._h, _p(b), _p(o), o.size - 1))

    def search_segments(self, segments) -> SearchResults:
        """one batch over reads that live in several (bases, offsets) buffers, in the order given"""
        keep = [self._batch(b, o) for b, o in segments]
        arr = (_lib.ReadSegment * len(keep))()
        for i, (b, o) in enumerate(keep):
            arr[i] = _lib.ReadSegment(b.ctypes.data, o.ctypes.data, o.size - 1)
        check(_lib.lib().taxor_gpu_search_segments_begin(self._h, arr, len(keep)))
        res = _lib.Results()
        check(_lib.lib().taxor_gpu_search_batch_end(self._h, C.byref(res)))
        return _results(res)

    def search_fastx(self, raw: bytes, kind) -> FastxResults:
        """one batch straight from file bytes: whole records of one kind, '>' (FASTA) or '@' (four-line FASTQ); the device
        finds the records (taxor_gpu_search_fastx_begin)"""
        buf = np.frombuffer(bytes(raw), dtype=np.uint8)
        k = kind if isinstance(kind, int) else ord(kind)
        sc = _lib.FastxScan()
        check(_lib.lib().taxor_gpu_search_fastx_begin(self._h, _p(buf) if buf.size else None, buf.size, k, C.byref(sc)))
        if sc.status:
            return FastxResults(int(sc.status))
        n = int(sc.n_reads)
        arr = lambda p: np.ctypeslib.as_array(p, shape=(n,)).copy() if n else np.zeros(0, np.uint64)
        id_off, id_len, read_len = arr(sc.id_off), arr(sc.id_len), arr(sc.read_len)
        res = _lib.Results()
        check(_lib.lib().taxor_gpu_search_batch_end(self._h, C.byref(res)))
        ids = [buf[int(a):int(a + l)].tobytes() for a, l in zip(id_off, id_len)]
        return FastxResults(0, _results(res), ids, read_len)

    @staticmethod
    def _nibble_segments(segments):
        """[(seq4 bytes, byte_off, read_len, reverse or None), ...] -> (taxor_nibble_segment array, what must stay alive)"""
        keep = []
        arr = (_lib.NibbleSegment * max(1, len(segments)))()
        for i, (seq4, boff, rlen, rev) in enumerate(segments):
            q = np.ascontiguousarray(np.frombuffer(bytes(seq4), dtype=np.uint8) if isinstance(seq4, (bytes, bytearray)) else seq4, dtype=np.uint8)
            o = np.ascontiguousarray(boff, dtype=np.uint64)
            n = np.ascontiguousarray(rlen, dtype=np.uint32)
            v = None if rev is None else np.ascontiguousarray(rev, dtype=np.uint8)
            assert o.size == n.size and (v is None or v.size == n.size)
            keep += [q, o, n, v]
            arr[i] = _lib.NibbleSegment(q.ctypes.data if q.size else None, o.ctypes.data if o.size else None, n.ctypes.data if n.size else None,
                                        None if v is None else v.ctypes.data, n.size)
        return arr, keep

    def search_nibbles(self, segments) -> SearchResults:
        """one batch over reads stored at 4 bits per base (a BAM record's SEQ field): segments = [(seq4, byte_off, read_len,
        reverse or None), ...] (taxor_gpu_search_nibbles_begin + _batch_end)"""
        arr, keep = self._nibble_segments(segments)
        check(_lib.lib().taxor_gpu_search_nibbles_begin(self._h, arr, len(segments)))
        res = _lib.Results()
        check(_lib.lib().taxor_gpu_search_batch_end(self._h, C.byref(res)))
        del keep
        return _results(res)

    def pack_nibbles(self, segments, timed=False):
        """k_pack_nibbles alone (taxor_gpu_pack_nibbles) -> (word_off uint64[n+1], words uint32[]) in k_pack_dna4's layout
        [, the kernel's HIP-event milliseconds]"""
        arr, keep = self._nibble_segments(segments)
        wo, ws, ms = C.POINTER(C.c_uint64)(), C.POINTER(C.c_uint32)(), C.c_float(0)
        check(_lib.lib().taxor_gpu_pack_nibbles(self._h, arr, len(segments), C.byref(wo), C.byref(ws), C.byref(ms) if timed else None))
        n = sum(int(a.n_reads) for a in arr[:len(segments)])
        woff = np.ctypeslib.as_array(wo, shape=(n + 1,)).copy()
        tot = int(woff[n])
        words = np.ctypeslib.as_array(ws, shape=(tot,)).copy() if tot else np.zeros(0, np.uint32)
        del keep
        return (woff, words, float(ms.value)) if timed else (woff, words)

    def search_batch_end(self) -> SearchResults:
        res = _lib.Results()
        check(_lib.lib().taxor_gpu_search_batch_end(self._h, C.byref(res)))
        self._inflight = None
        return _results(res)

    # --- paged index: per-pass results and their merge -------------------------------------------------------
    def result_keys(self, n_tuples):
        """DFS keys of the last results' tuples (taxor_gpu_results_keys)"""
        kp = C.POINTER(C.c_uint32)()
        check(_lib.lib().taxor_gpu_results_keys(self._h, C.byref(kp)))
        return np.ctypeslib.as_array(kp, shape=(n_tuples,)).copy() if n_tuples else np.zeros(0, np.uint32)

    def search_pass(self, bases, offsets) -> PassResults:
        """search_batch + the tuples' keys: one pass's share of a batch on a paged index"""
        r = self.search_batch(bases, offsets)
        return PassResults(r, self.result_keys(r.user_bin.size))

    def merge_prior(self, priors) -> SearchResults:
        """after the LAST pass's batch: merge the earlier passes' PassResults of the same reads into the searcher's device CSR
        (taxor_gpu_search_merge_prior) and fetch the complete results"""
        arr = (_lib.Prior * max(1, len(priors)))()
        keep = []
        for i, p in enumerate(priors):
            ro = np.ascontiguousarray(p.results.read_off, dtype=np.uint64)
            ub = np.ascontiguousarray(p.results.user_bin, dtype=np.int64)
            ct = np.ascontiguousarray(p.results.count, dtype=np.uint32)
            ky = np.ascontiguousarray(p.key, dtype=np.uint32)
            keep += [ro, ub, ct, ky]
            arr[i] = _lib.Prior(ro.size - 1, ub.size, ro.ctypes.data, ub.ctypes.data, ct.ctypes.data, ky.ctypes.data)
        check(_lib.lib().taxor_gpu_search_merge_prior(self._h, arr, len(priors)))
        return self.fetch()

    # --- saved hash lists: capture and replay ----------------------------------------------------------------
    def capture(self, on=True):
        """taxor_gpu_search_capture: while on, every batch also leaves its hash lists on the host (take_saved)"""
        check(_lib.lib().taxor_gpu_search_capture(self._h, 1 if on else 0))

    def capture_positions(self, on=True):
        """taxor_gpu_search_capture_positions: while on (capture must be on, a syncmer index), every saved batch also carries
        SavedBatch.positions -- for each hash the first base at which its read shows the hashed k-mer, on either strand"""
        check(_lib.lib().taxor_gpu_search_capture_positions(self._h, 1 if on else 0))

    def take_saved(self) -> "SavedBatch":
        """the saved batch of the last batch that ran with capture on (taxor_gpu_search_take_saved)"""
        h = C.c_void_p()
        check(_lib.lib().taxor_gpu_search_take_saved(self._h, C.byref(h)))
        return SavedBatch(h)

    def search_saved(self, saved: "SavedBatch") -> SearchResults:
        """the batch again from its saved hash lists (taxor_gpu_search_saved_begin + _batch_end): nothing is packed or hashed"""
        check(_lib.lib().taxor_gpu_search_saved_begin(self._h, saved._h))
        res = _lib.Results()
        check(_lib.lib().taxor_gpu_search_batch_end(self._h, C.byref(res)))
        return _results(res)

    def search_saved_pass(self, saved: "SavedBatch") -> PassResults:
        """search_saved + the tuples' keys: one pass's share of a batch on a paged index"""
        r = self.search_saved(saved)
        return PassResults(r, self.result_keys(r.user_bin.size))

    # --- phases -------------------------------------------------------------------------------------------
    def upload(self, bases, offsets):
        b, o = self._batch(bases, offsets)
        check(_lib.lib().taxor_gpu_batch_upload(self._h, _p(b), _p(o), o.size - 1))

    def upload_timed(self, bases, offsets):
        """upload() -> HIP-event milliseconds of its packing kernel, k_pack_dna4 (taxor_gpu_pack_dna4_timed)"""
        b, o = self._batch(bases, offsets)
        ms = C.c_float(0)
        check(_lib.lib().taxor_gpu_pack_dna4_timed(self._h, _p(b), _p(o), o.size - 1, C.byref(ms)))
        return float(ms.value)

    def run(self):
        check(_lib.lib().taxor_gpu_batch_run(self._h))

    def sync(self):
        check(_lib.lib().taxor_gpu_batch_sync(self._h))

    def fetch(self) -> SearchResults:
        res = _lib.Results()
        check(_lib.lib().taxor_gpu_batch_fetch(self._h, C.byref(res)))
        return _results(res)

    def stats(self):
        st = _lib.RunStats()
        check(_lib.lib().taxor_gpu_batch_stats(self._h, C.byref(st)))
        out = {f: getattr(st, f) for f, _ in _lib.RunStats._fields_}
        for f in ("level_ms", "level_requested_bytes", "level_row_reads", "level_sparse_loads"):
            out[f] = list(out[f])
        return out

    def phase_profile(self):
        """per-phase cycle sums of k_syncmers [0..7] and k_query_level [8..15] since the last call (needs a searcher
        created under TAXOR_PROFILE_PHASES=1)"""
        out = np.zeros(16, dtype=np.uint64)
        check(_lib.lib().taxor_gpu_phase_profile(self._h, _p(out)))
        return out

    def result_sizes(self):
        a, b = C.c_uint64(), C.c_uint64()
        check(_lib.lib().taxor_gpu_batch_result_sizes(self._h, C.byref(a), C.byref(b)))
        return int(a.value), int(b.value)

    def export_device(self, read_off_ptr=None, user_bin_ptr=None, count_ptr=None, n_hashes_ptr=None):
        """D2D copy of the last run's results into caller-owned device buffers (raw device pointers)."""
        check(_lib.lib().taxor_gpu_batch_export_device(self._h, read_off_ptr, user_bin_ptr, count_ptr, n_hashes_ptr))

    # --- stage entry points ---------------------------------------------------------------------------------
    def seq_to_syncmers(self, bases, offsets):
        """hashing::seq_to_syncmers for a batch -> (hash_off uint64[n+1], hashes uint64[])"""
        b, o = self._batch(bases, offsets)
        ho, hs = C.POINTER(C.c_uint64)(), C.POINTER(C.c_uint64)()
        n = o.size - 1
        check(_lib.lib().taxor_gpu_syncmers(self._h, _p(b), _p(o), n, C.byref(ho), C.byref(hs)))
        hoff = np.ctypeslib.as_array(ho, shape=(n + 1,)).copy()
        tot = int(hoff[n])
        hashes = np.ctypeslib.as_array(hs, shape=(tot,)).copy() if tot else np.zeros(0, np.uint64)
        return hoff, hashes

    def ixf_bulk_count(self, ixf, hashes):
        h = np.ascontiguousarray(hashes, dtype=np.uint64)
        out = np.zeros(self.index.shapes[ixf][0], dtype=np.uint32)
        check(_lib.lib().taxor_gpu_ixf_bulk_count(self._h, ixf, _p(h), h.size, _p(out)))
        return out

    def bulk_contains(self, hashes, thr):
        h = np.ascontiguousarray(hashes, dtype=np.uint64)
        res = _lib.Results()
        check(_lib.lib().taxor_gpu_bulk_contains(self._h, _p(h), h.size, int(thr), C.byref(res)))
        r = _results(res)
        return r.user_bin, r.count


class SavedBatch:
    """A batch's saved hash lists (taxor_gpu_saved): owned by this object, freed by close().  The arrays are VIEWS of the library's
    own host memory (the C ABI's read-only pointers), valid until close()."""

    PARAMS = ("use_syncmer", "kmer_size", "syncmer_size", "t_syncmer", "scaling", "model", "window_size", "error_rate", "ratio")

    def __init__(self, h):
        self._h = h
        v = _lib.SavedView()
        check(_lib.lib().taxor_gpu_saved_view_get(h, C.byref(v)))
        n, t, ns = int(v.n_reads), int(v.total_hashes), int(v.n_sub_batches)
        arr = lambda p, m, dt: np.ctypeslib.as_array(p, shape=(m,)) if m else np.zeros(0, dt)
        self.n_reads, self.total_hashes, self.n_sub_batches = n, t, ns
        self.read_len = arr(v.read_len, n, np.uint32)
        self.n_hashes = arr(v.n_hashes, n, np.uint32)
        self.threshold = arr(v.threshold, n, np.uint64)
        self.hash_off = np.ctypeslib.as_array(v.hash_off, shape=(n + 1,))
        self.hashes = arr(v.hashes, t, np.uint64)
        self.sub_first = np.ctypeslib.as_array(v.sub_first, shape=(ns + 1,))
        self.order = arr(v.order, n, np.uint32)
        self.params = {f: getattr(v, f) for f in self.PARAMS}
        # taxor_gpu_saved_positions: every hash's position in its read, parallel to `hashes`; None when captured without positions
        pp = C.POINTER(C.c_uint32)()
        check(_lib.lib().taxor_gpu_saved_positions(h, C.byref(pp)))
        self.positions = arr(pp, t, np.uint32) if pp else None
        self.positions_seconds = float(_lib.lib().taxor_gpu_saved_positions_seconds(h))

    @property
    def nbytes(self):
        return int(_lib.lib().taxor_gpu_saved_bytes(self._h))

    def close(self):
        if getattr(self, "_h", None):
            for f in ("read_len", "n_hashes", "threshold", "hash_off", "hashes", "sub_first", "order", "positions"):
                setattr(self, f, None)
            _lib.lib().taxor_gpu_saved_free(self._h)
            self._h = None

    __del__ = close


def saved_bytes_bound(bases, use_syncmer=True, k=22, s=12, t=5):
    """taxor_saved_bytes_bound (host only): host bytes the saved hash lists of `bases` bases of query may need"""
    return int(_lib.lib().taxor_saved_bytes_bound(int(bases), 1 if use_syncmer else 0, int(k), int(s), int(t)))


def saved_store_fits(bound_bytes, available_bytes):
    """taxor_saved_store_fits (host only): True = keep the lists and replay, False = re-read the query every pass"""
    return bool(_lib.lib().taxor_saved_store_fits(int(bound_bytes), int(available_bytes)))


def hll_slot(h, precision=12):
    """taxor_hll_slot (host only): (register index, rho) of one hash -- the function the device uses"""
    i, rho = C.c_uint32(), C.c_uint8()
    _lib.lib().taxor_hll_slot(int(h) & (2**64 - 1), int(precision), C.byref(i), C.byref(rho))
    return int(i.value), int(rho.value)


def hll_estimate(registers, precision=12):
    """taxor_hll_estimate (host only): the distinct count a sketch's 2^precision byte registers stand for"""
    r = np.ascontiguousarray(registers, dtype=np.uint8)
    assert r.size == 1 << int(precision)
    return float(_lib.lib().taxor_hll_estimate(_p(r), int(precision)))


def census_keys_est(nonzero):
    """taxor_census_keys_est (host only): the keys a bin's column of `nonzero` nonzero bytes stands for, llround(nonzero * 256 / 255)"""
    return int(_lib.lib().taxor_census_keys_est(int(nonzero)))


def census_capacity(seg_len):
    """taxor_census_capacity (host only): the largest n with taxor_ixf_seg_len(n) <= seg_len"""
    return int(_lib.lib().taxor_census_capacity(int(seg_len)))


def census_peeled(nonzero, seg_len):
    """taxor_census_peeled (host only): False when the column holds more nonzero bytes than its IXF has room for keys"""
    return bool(_lib.lib().taxor_census_peeled(int(nonzero), int(seg_len)))


def _census_text(fn, *args):
    buf = C.create_string_buffer(4096)
    n = int(fn(*args, buf, len(buf)))
    assert n < len(buf)
    return buf.value.decode()


def census_ref_line(accession, name, taxid, ref_len, leaf_bins, index_hashes):
    """one line of `taxor census --output-file`; index_hashes None = NA"""
    enc = lambda s: None if s is None else s.encode()
    return _census_text(_lib.lib().taxor_census_ref_line, enc(accession), enc(name), enc(taxid), int(ref_len), int(leaf_bins),
                        int(index_hashes or 0), 1 if index_hashes is None else 0)


def census_ixf_line(ixf, bins, leaf_bins, seg_len, stride, max_bin_keys):
    """one line of `taxor census --ixf-file`; max_bin_keys None = NA"""
    return _census_text(_lib.lib().taxor_census_ixf_line, int(ixf), int(bins), int(leaf_bins), int(seg_len), int(stride), int(max_bin_keys or 0),
                        1 if max_bin_keys is None else 0)


def census_breadth_columns(distinct, hash_matches, index_hashes):
    """the four columns `taxor search --coverage-breadth` appends, each led by its tab; index_hashes None = NA"""
    return _census_text(_lib.lib().taxor_census_breadth_columns, int(distinct), int(hash_matches), int(index_hashes or 0), 1 if index_hashes is None else 0)


@dataclass
class CensusTable:
    """GpuIndex.census(): the nonzero fingerprint bytes of every bin, in index bin order"""
    nonzero: np.ndarray        # uint64[n_bins]: all bins of IXF 0, then IXF 1, ...
    bin_first: np.ndarray      # uint64[n_ixf + 1]
    seconds_kernel: float      # HIP-event time of the pass
    bytes_read: int            # fingerprint bytes of the index, each read once
    n_tiles: int
    launches: int
    all_runs: list = None

    def of_ixf(self, x):
        return self.nonzero[int(self.bin_first[x]):int(self.bin_first[x + 1])]

    def keys_est(self):
        """llround(nonzero * 256 / 255) per bin (census_format.h), whether the bin is a peeled filter or not"""
        return np.array([census_keys_est(v) for v in self.nonzero], dtype=np.uint64)


@dataclass
class CoverageTable:
    """Coverage.results(): per user bin the surviving tuples, their counts summed, and the sketch of the distinct matched hashes"""
    precision: int
    reads: np.ndarray          # uint64[n_user_bins]
    hash_matches: np.ndarray   # uint64[n_user_bins]
    registers: np.ndarray      # uint8[n_user_bins, 2^precision]
    seconds_kernels: float
    probes: int

    def distinct(self, b):
        """DISTINCT_HASHES of `taxor search --coverage-file`: the rounded estimate, at least 1 where anything matched"""
        d = int(np.floor(hll_estimate(self.registers[b], self.precision) + 0.5))      # llround: halves away from zero
        return max(d, 1) if self.hash_matches[b] else d


class Coverage:
    """Distinct matched hashes per user bin over a whole run (taxor_amd/csrc/coverage.hip).  `ixfs` is the list the GpuIndex was made
    from (only bins and fname_idx are read).  add_batch follows a batch that ran with Searcher.capture() on and takes its
    SavedBatch, which stays the caller's."""

    def __init__(self, index: GpuIndex, ixfs, precision=0):
        view, keep = GpuIndex._view([dict(f, data=None) for f in ixfs], index.n_user_bins, index.k, index.s, index.t, index.use_syncmer, 1,
                                    index.window_size)
        self._L = _lib.lib()
        self._h = C.c_void_p()
        self.index = index
        check(self._L.taxor_gpu_coverage_create(index._h, C.byref(view), int(precision), C.byref(self._h)))
        del keep

    def add_batch(self, searcher: Searcher, saved: "SavedBatch"):
        check(self._L.taxor_gpu_coverage_add_batch(self._h, searcher._h, saved._h if saved is not None else None))

    def results(self) -> CoverageTable:
        res = _lib.CoverageResults()
        check(self._L.taxor_gpu_coverage_results(self._h, C.byref(res)))
        n, p = int(res.n_user_bins), int(res.precision)
        arr = lambda ptr, m, dt: np.ctypeslib.as_array(ptr, shape=(m,)).copy() if m else np.zeros(0, dt)
        return CoverageTable(p, arr(res.reads, n, np.uint64), arr(res.hash_matches, n, np.uint64),
                             arr(res.registers, n << p, np.uint8).reshape(n, 1 << p), float(res.seconds_kernels), int(res.probes))

    def close(self):
        if getattr(self, "_h", None):
            self._L.taxor_gpu_coverage_destroy(self._h)
            self._h = C.c_void_p()

    __del__ = close

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


class Lineage:
    """The taxonomy of an index as a tree (taxor_lineage_*, host only; taxor_amd/csrc/lineage.h): built from a list of species dicts
    {organism_name, accession_id, taxid, taxnames_string, taxid_string, user_bin, seq_len}, the form hixf_file.py uses.  Node numbers
    are dense in byte-wise order of the id strings; parent -1 is ROOT."""

    def __init__(self, species, n_user_bins):
        L = _lib.lib()
        sp = (_lib.Species * max(1, len(species)))()
        for i, x in enumerate(species):
            sp[i] = _lib.Species(x["organism_name"].encode(), x["accession_id"].encode(), x["taxid"].encode(), x["taxnames_string"].encode(),
                                 x["taxid_string"].encode(), x["user_bin"], x["seq_len"])
        meta = _lib.HixfMeta(0, 1, 0, len(species), sp, 0, None)
        self._h = C.c_void_p()
        check(L.taxor_lineage_create(C.byref(meta), int(n_user_bins), C.byref(self._h)))
        v = _lib.LineageView()
        check(L.taxor_lineage_get_view(self._h, C.byref(v)))
        nb, nn = int(v.n_user_bins), int(v.n_nodes)
        arr = lambda ptr, m, dt: np.ctypeslib.as_array(ptr, shape=(m,)).copy() if m else np.zeros(0, dt)
        self.n_user_bins, self.n_nodes, self.max_depth = nb, nn, int(v.max_depth)
        self.bin_species = arr(v.bin_species, nb, np.uint32)
        self.path_off = np.ctypeslib.as_array(v.path_off, shape=(nb + 1,)).copy()
        self.path = arr(v.path, int(self.path_off[nb]), np.int32)
        self.parent = arr(v.parent, nn, np.int32)
        self.depth = arr(v.depth, nn, np.uint32)
        self.ids = [v.id[i].decode("utf-8", "replace") for i in range(nn)]
        self.names = [v.name[i].decode("utf-8", "replace") for i in range(nn)]
        self.ranks = [v.rank[i].decode("latin-1") for i in range(nn)]

    def path_of(self, b):
        return [int(x) for x in self.path[int(self.path_off[b]):int(self.path_off[b + 1])]]

    def close(self):
        if getattr(self, "_h", None):
            _lib.lib().taxor_lineage_free(self._h)
            self._h = C.c_void_p()

    __del__ = close


@dataclass
class LcaCalls:
    """per read of one add: node (a node number, _lib.LCA_ROOT or _lib.LCA_UNCLASSIFIED), the maximum count, the surviving tuples, and
    (add_batch only) QHASH_COUNT"""
    first_read: int
    node: np.ndarray        # int32[n_reads]
    best: np.ndarray        # uint32[n_reads]
    n_refs: np.ndarray      # uint32[n_reads]
    n_hashes: np.ndarray    # uint32[n_reads] or None


@dataclass
class LcaTallies:
    """Lca.results(): per node, then ROOT at [n_nodes] and UNCLASSIFIED at [n_nodes + 1]"""
    n_nodes: int
    direct_reads: np.ndarray   # uint64[n_nodes + 2]
    direct_bases: np.ndarray   # uint64[n_nodes + 2]
    n_reads: int
    seconds_kernel: float


class Lca:
    """Per-read lowest common ancestor and per-taxon tallies over a whole run (taxor_amd/csrc/lca.hip).  add_batch follows a batch on
    a Searcher of the same index; add_csr takes host arrays."""

    def __init__(self, index: GpuIndex, lineage: Lineage):
        self._L = _lib.lib()
        self._h = C.c_void_p()
        self.index, self.lineage = index, lineage
        check(self._L.taxor_gpu_lca_create(index._h, lineage._h, C.byref(self._h)))

    @staticmethod
    def _calls(c):
        n = int(c.n_reads)
        arr = lambda ptr, dt: np.ctypeslib.as_array(ptr, shape=(n,)).copy() if n else np.zeros(0, dt)
        return LcaCalls(int(c.first_read), arr(c.node, np.int32), arr(c.best, np.uint32), arr(c.n_refs, np.uint32),
                        arr(c.n_hashes, np.uint32) if c.n_hashes else None)

    def add_batch(self, searcher: Searcher, first_read=0) -> LcaCalls:
        c = _lib.LcaCalls()
        check(self._L.taxor_gpu_lca_add_batch(self._h, searcher._h, int(first_read), C.byref(c)))
        return self._calls(c)

    def add_csr(self, read_off, user_bin, count, query_len) -> LcaCalls:
        ro = np.ascontiguousarray(read_off, dtype=np.uint64)
        ub = np.ascontiguousarray(user_bin, dtype=np.int64)
        ct = np.ascontiguousarray(count, dtype=np.uint32)
        ql = np.ascontiguousarray(query_len, dtype=np.uint64)
        assert ro.size >= 1 and ql.size == ro.size - 1 and ub.size == ct.size and int(ro[-1]) <= ub.size
        c = _lib.LcaCalls()
        check(self._L.taxor_gpu_lca_add_csr(self._h, ro.size - 1, _p(ro), _p(ub) if ub.size else None, _p(ct) if ct.size else None,
                                            _p(ql) if ql.size else None, C.byref(c)))
        return self._calls(c)

    def results(self) -> LcaTallies:
        res = _lib.LcaResults()
        check(self._L.taxor_gpu_lca_results(self._h, C.byref(res)))
        n = int(res.n_nodes)
        return LcaTallies(n, np.ctypeslib.as_array(res.direct_reads, shape=(n + 2,)).copy(), np.ctypeslib.as_array(res.direct_bases, shape=(n + 2,)).copy(),
                          int(res.n_reads), float(res.seconds_kernel))

    def close(self):
        if getattr(self, "_h", None):
            self._L.taxor_gpu_lca_destroy(self._h)
            self._h = C.c_void_p()

    __del__ = close

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


@dataclass
class ConfidenceCalls:
    """per read of one add: the confident call and its depth, the call without a threshold and its depth D, support at the confident
    depth (support[0] for a read the threshold made unclassified), support[D], support[0], and LcaCalls' best / n_refs / n_hashes"""
    first_read: int
    node: np.ndarray          # int32[n_reads]
    depth: np.ndarray         # uint32[n_reads]
    lca_node: np.ndarray      # int32[n_reads]
    lca_depth: np.ndarray     # uint32[n_reads]
    support: np.ndarray       # uint32[n_reads]
    lca_support: np.ndarray   # uint32[n_reads]
    any_support: np.ndarray   # uint32[n_reads]
    best: np.ndarray          # uint32[n_reads]
    n_refs: np.ndarray        # uint32[n_reads]
    n_hashes: np.ndarray      # uint32[n_reads]
    seconds_kernels: float
    probes: int
    tuple_steps: int
    tuple_steps_full: int


class Confidence:
    """Hash support behind each LCA call and the call a threshold on it leaves (taxor_amd/csrc/confidence.hip).  `ixfs` is the list
    the GpuIndex was made from (only bins and fname_idx are read).  add_batch follows a batch that ran with Searcher.capture() on and
    takes its SavedBatch, which stays the caller's; add_csr takes host arrays.  The arrays returned are copies."""

    WORDS = ("node", "depth", "lca_node", "lca_depth", "support", "lca_support", "any_support", "best", "n_refs", "n_hashes")

    def __init__(self, index: GpuIndex, ixfs, lineage: Lineage, confidence=0.0):
        view, keep = GpuIndex._view([dict(f, data=None) for f in ixfs], index.n_user_bins, index.k, index.s, index.t, index.use_syncmer, 1,
                                    index.window_size)
        self._L = _lib.lib()
        self._h = C.c_void_p()
        self.index, self.lineage, self.confidence = index, lineage, float(confidence)
        check(self._L.taxor_gpu_confidence_create(index._h, C.byref(view), lineage._h, float(confidence), C.byref(self._h)))
        del keep

    @classmethod
    def _calls(cls, c):
        n = int(c.n_reads)
        arr = lambda ptr, dt: np.ctypeslib.as_array(ptr, shape=(n,)).copy() if n else np.zeros(0, dt)
        words = [arr(getattr(c, f), np.int32 if f in ("node", "lca_node") else np.uint32) for f in cls.WORDS]
        return ConfidenceCalls(int(c.first_read), *words, float(c.seconds_kernels), int(c.probes), int(c.tuple_steps), int(c.tuple_steps_full))

    def add_batch(self, searcher: Searcher, saved: "SavedBatch", first_read=0) -> ConfidenceCalls:
        c = _lib.ConfidenceCalls()
        check(self._L.taxor_gpu_confidence_add_batch(self._h, searcher._h, saved._h if saved is not None else None, int(first_read), C.byref(c)))
        return self._calls(c)

    def add_csr(self, read_off, user_bin, count, query_len, hash_off, hashes) -> ConfidenceCalls:
        ro = np.ascontiguousarray(read_off, dtype=np.uint64)
        ub = np.ascontiguousarray(user_bin, dtype=np.int64)
        ct = np.ascontiguousarray(count, dtype=np.uint32)
        ql = np.ascontiguousarray(query_len, dtype=np.uint64)
        ho = np.ascontiguousarray(hash_off, dtype=np.uint64)
        hs = np.ascontiguousarray(hashes, dtype=np.uint64)
        assert ro.size >= 1 and ql.size == ro.size - 1 and ho.size == ro.size and ub.size == ct.size and int(ro[-1]) <= ub.size and int(ho[-1]) <= hs.size
        c = _lib.ConfidenceCalls()
        check(self._L.taxor_gpu_confidence_add_csr(self._h, ro.size - 1, _p(ro), _p(ub) if ub.size else None, _p(ct) if ct.size else None,
                                                   _p(ql) if ql.size else None, _p(ho), _p(hs) if hs.size else None, C.byref(c)))
        return self._calls(c)

    def results(self) -> LcaTallies:
        res = _lib.LcaResults()
        check(self._L.taxor_gpu_confidence_results(self._h, C.byref(res)))
        n = int(res.n_nodes)
        return LcaTallies(n, np.ctypeslib.as_array(res.direct_reads, shape=(n + 2,)).copy(), np.ctypeslib.as_array(res.direct_bases, shape=(n + 2,)).copy(),
                          int(res.n_reads), float(res.seconds_kernel))

    def close(self):
        if getattr(self, "_h", None):
            self._L.taxor_gpu_confidence_destroy(self._h)
            self._h = C.c_void_p()

    __del__ = close

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


@dataclass
class HitmapBatch:
    """Hitmap.add_batch(): read r's mapped tuples are [map_off[r], map_off[r + 1]) of tuple / user_bin / count / hits"""
    segments: int
    map_off: np.ndarray     # uint64[n_reads + 1]
    tuple: np.ndarray       # uint64[n_mapped] index in the batch CSR
    user_bin: np.ndarray    # int64[n_mapped]
    count: np.ndarray       # uint32[n_mapped]
    hits: np.ndarray        # uint32[n_mapped, segments]
    n_hashes: np.ndarray    # uint32[n_reads]
    seconds_kernels: float
    probes: int


class Hitmap:
    """Where along a read each reference matched (taxor_amd/csrc/hitmap.hip).  `ixfs` is the list the GpuIndex was made from (only bins
    and fname_idx are read).  add_batch follows a batch that ran with Searcher.capture() on and takes its SavedBatch, which stays the
    caller's; the arrays it returns are copies."""

    def __init__(self, index: GpuIndex, ixfs, segments=16):
        view, keep = GpuIndex._view([dict(f, data=None) for f in ixfs], index.n_user_bins, index.k, index.s, index.t, index.use_syncmer, 1,
                                    index.window_size)
        self._L = _lib.lib()
        self._h = C.c_void_p()
        self.index, self.segments = index, int(segments)
        check(self._L.taxor_gpu_hitmap_create(index._h, C.byref(view), int(segments), C.byref(self._h)))
        del keep

    def add_batch(self, searcher: Searcher, saved: "SavedBatch") -> HitmapBatch:
        b = _lib.HitmapBatch()
        check(self._L.taxor_gpu_hitmap_add_batch(self._h, searcher._h, saved._h if saved is not None else None, C.byref(b)))
        n, m, S = int(b.n_reads), int(b.n_mapped), int(b.segments)
        arr = lambda ptr, k, dt: np.ctypeslib.as_array(ptr, shape=(k,)).copy() if k else np.zeros(0, dt)
        return HitmapBatch(S, arr(b.map_off, n + 1, np.uint64), arr(b.tuple, m, np.uint64), arr(b.user_bin, m, np.int64), arr(b.count, m, np.uint32),
                           arr(b.hits, m * S, np.uint32).reshape(m, S), arr(b.n_hashes, n, np.uint32), float(b.seconds_kernels), int(b.probes))

    def close(self):
        if getattr(self, "_h", None):
            self._L.taxor_gpu_hitmap_destroy(self._h)
            self._h = C.c_void_p()

    __del__ = close

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


@dataclass
class BreakpointBatch:
    """Breakpoints.add_batch() / add_csr(): per read the twelve words of include/taxor_gpu_tools.h (all 0 for a read that is not
    examined), the user bins of A, B and best, and every read's hash count.  reported = examined and gain >= min_gain"""
    min_gain: int
    examined: np.ndarray      # bool[n_reads]
    gain: np.ndarray          # uint32[n_reads]
    break_hash: np.ndarray    # uint32[n_reads] p*
    tuple_a: np.ndarray       # uint64[n_reads] index in the batch CSR
    tuple_b: np.ndarray
    tuple_best: np.ndarray
    pre_a: np.ndarray         # uint32[n_reads]
    suf_b: np.ndarray
    pre_b: np.ndarray
    suf_a: np.ndarray
    single: np.ndarray
    n_candidates: np.ndarray  # M
    n: np.ndarray             # the hash count of an examined read
    n_hashes: np.ndarray      # of every read
    bin_a: np.ndarray         # int64[n_reads]
    bin_b: np.ndarray
    bin_best: np.ndarray
    n_examined: int
    n_reported: int
    seconds_kernels: float
    lookups: int

    @property
    def reported(self):
        return self.examined & (self.gain >= self.min_gain)


class Breakpoints:
    """Where a read switches reference (taxor_amd/csrc/breakpoint.hip).  `ixfs` is the list the GpuIndex was made from (only bins and
    fname_idx are read).  add_batch follows a batch that ran with Searcher.capture() on and takes its SavedBatch, which stays the
    caller's; add_csr takes host arrays.  The arrays returned are copies."""

    WORDS = (("gain", np.uint32), ("break_hash", np.uint32), ("tuple_a", np.uint64), ("tuple_b", np.uint64), ("tuple_best", np.uint64), ("pre_a", np.uint32),
             ("suf_b", np.uint32), ("pre_b", np.uint32), ("suf_a", np.uint32), ("single", np.uint32), ("n_candidates", np.uint32), ("n", np.uint32),
             ("n_hashes", np.uint32), ("bin_a", np.int64), ("bin_b", np.int64), ("bin_best", np.int64))

    def __init__(self, index: GpuIndex, ixfs, min_gain=1):
        view, keep = GpuIndex._view([dict(f, data=None) for f in ixfs], index.n_user_bins, index.k, index.s, index.t, index.use_syncmer, 1,
                                    index.window_size)
        self._L = _lib.lib()
        self._h = C.c_void_p()
        self.index, self.min_gain = index, int(min_gain)
        check(self._L.taxor_gpu_breakpoint_create(index._h, C.byref(view), int(min_gain), C.byref(self._h)))
        del keep

    @classmethod
    def _batch(cls, b):
        n = int(b.n_reads)
        arr = lambda ptr, dt: np.ctypeslib.as_array(ptr, shape=(n,)).copy() if n else np.zeros(0, dt)
        return BreakpointBatch(int(b.min_gain), arr(b.examined, np.uint8).astype(bool), *[arr(getattr(b, f), dt) for f, dt in cls.WORDS], int(b.n_examined),
                               int(b.n_reported), float(b.seconds_kernels), int(b.lookups))

    def add_batch(self, searcher: Searcher, saved: "SavedBatch") -> BreakpointBatch:
        b = _lib.BreakpointBatch()
        check(self._L.taxor_gpu_breakpoint_add_batch(self._h, searcher._h, saved._h if saved is not None else None, C.byref(b)))
        return self._batch(b)

    def add_csr(self, read_off, user_bin, count, hash_off, hashes) -> BreakpointBatch:
        ro = np.ascontiguousarray(read_off, dtype=np.uint64)
        ub = np.ascontiguousarray(user_bin, dtype=np.int64)
        ct = np.ascontiguousarray(count, dtype=np.uint32)
        ho = np.ascontiguousarray(hash_off, dtype=np.uint64)
        hs = np.ascontiguousarray(hashes, dtype=np.uint64)
        assert ro.size >= 1 and ho.size == ro.size and ub.size == ct.size and int(ro[-1]) <= ub.size and int(ho[-1]) <= hs.size
        b = _lib.BreakpointBatch()
        check(self._L.taxor_gpu_breakpoint_add_csr(self._h, ro.size - 1, _p(ro), _p(ub) if ub.size else None, _p(ct) if ct.size else None, _p(ho),
                                                   _p(hs) if hs.size else None, C.byref(b)))
        return self._batch(b)

    def close(self):
        if getattr(self, "_h", None):
            self._L.taxor_gpu_breakpoint_destroy(self._h)
            self._h = C.c_void_p()

    __del__ = close

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


@dataclass
class SegmentsBatch:
    """Segments.add_batch() / add_csr(): per read the words of include/taxor_gpu_tools.h (all 0 for a read that is not examined), every
    read's hash count, and the segments of the reported reads (n_segments >= 2) in list order: read r's are [seg_off[r], seg_off[r+1])"""
    switch_cost: int
    examined: np.ndarray      # bool[n_reads]
    n_candidates: np.ndarray  # uint32[n_reads] M
    n: np.ndarray             # the hash count of an examined read
    n_hashes: np.ndarray      # of every read
    n_segments: np.ndarray    # K: 0 not examined, 1 examined and unbroken
    path_hits: np.ndarray
    path_switches: np.ndarray
    single: np.ndarray
    tuple_best: np.ndarray    # uint64[n_reads] index in the batch CSR
    bin_best: np.ndarray      # int64[n_reads]
    seg_off: np.ndarray       # uint64[n_reads + 1]
    seg_start: np.ndarray     # uint32 per segment
    seg_end: np.ndarray
    seg_tuple: np.ndarray     # uint64
    seg_bin: np.ndarray       # int64
    seg_hits: np.ndarray      # uint32
    seg_best_hits: np.ndarray
    n_examined: int
    n_reported: int
    seconds_kernels: float
    lookups: int
    n_groups: int = 0         # groups of reads the scratch budget cut the examined reads into

    @property
    def reported(self):
        return self.examined & (self.n_segments >= 2)


class Segments:
    """Paint a read with its references (taxor_amd/csrc/segments.hip): the optimal segmentation of its ordered hash list among all its
    candidates, `switch_cost` hits per switch.  `ixfs` is the list the GpuIndex was made from (only bins and fname_idx are read).
    add_batch follows a batch that ran with Searcher.capture() on and takes its SavedBatch, which stays the caller's; add_csr takes host
    arrays.  The arrays returned are copies."""

    WORDS = (("n_candidates", np.uint32), ("n", np.uint32), ("n_hashes", np.uint32), ("n_segments", np.uint32), ("path_hits", np.uint32),
             ("path_switches", np.uint32), ("single", np.uint32), ("tuple_best", np.uint64), ("bin_best", np.int64))
    SEG_WORDS = (("seg_start", np.uint32), ("seg_end", np.uint32), ("seg_tuple", np.uint64), ("seg_bin", np.int64), ("seg_hits", np.uint32),
                 ("seg_best_hits", np.uint32))

    def __init__(self, index: GpuIndex, ixfs, switch_cost=16):
        view, keep = GpuIndex._view([dict(f, data=None) for f in ixfs], index.n_user_bins, index.k, index.s, index.t, index.use_syncmer, 1,
                                    index.window_size)
        self._L = _lib.lib()
        self._h = C.c_void_p()
        self.index, self.switch_cost = index, int(switch_cost)
        check(self._L.taxor_gpu_segments_create(index._h, C.byref(view), int(switch_cost), C.byref(self._h)))
        del keep

    @classmethod
    def _batch(cls, b):
        n = int(b.n_reads)
        arr = lambda ptr, dt, m: np.ctypeslib.as_array(ptr, shape=(m,)).copy() if m else np.zeros(0, dt)
        seg_off = np.ctypeslib.as_array(b.seg_off, shape=(n + 1,)).copy()
        ns = int(seg_off[n])
        return SegmentsBatch(int(b.switch_cost), arr(b.examined, np.uint8, n).astype(bool), *[arr(getattr(b, f), dt, n) for f, dt in cls.WORDS], seg_off,
                             *[arr(getattr(b, f), dt, ns) for f, dt in cls.SEG_WORDS], int(b.n_examined), int(b.n_reported), float(b.seconds_kernels),
                             int(b.lookups), int(b.n_groups))

    def add_batch(self, searcher: Searcher, saved: "SavedBatch") -> SegmentsBatch:
        b = _lib.SegmentsBatch()
        check(self._L.taxor_gpu_segments_add_batch(self._h, searcher._h, saved._h if saved is not None else None, C.byref(b)))
        return self._batch(b)

    def add_csr(self, read_off, user_bin, count, hash_off, hashes) -> SegmentsBatch:
        ro = np.ascontiguousarray(read_off, dtype=np.uint64)
        ub = np.ascontiguousarray(user_bin, dtype=np.int64)
        ct = np.ascontiguousarray(count, dtype=np.uint32)
        ho = np.ascontiguousarray(hash_off, dtype=np.uint64)
        hs = np.ascontiguousarray(hashes, dtype=np.uint64)
        assert ro.size >= 1 and ho.size == ro.size and ub.size == ct.size and int(ro[-1]) <= ub.size and int(ho[-1]) <= hs.size
        b = _lib.SegmentsBatch()
        check(self._L.taxor_gpu_segments_add_csr(self._h, ro.size - 1, _p(ro), _p(ub) if ub.size else None, _p(ct) if ct.size else None, _p(ho),
                                                 _p(hs) if hs.size else None, C.byref(b)))
        return self._batch(b)

    def close(self):
        if getattr(self, "_h", None):
            self._L.taxor_gpu_segments_destroy(self._h)
            self._h = C.c_void_p()

    __del__ = close

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


@dataclass
class ExclusiveBatch:
    """Exclusive.add_batch() / add_csr(): per read the words of include/taxor_gpu_tools.h (all 0 for a read that is not examined), every
    read's hash count, and per candidate of an examined read -- cand_off[r] .. cand_off[r + 1], in CSR order -- its tuple, user bin,
    count, hits and exclusive hits"""
    precision: int
    examined: np.ndarray      # bool[n_reads]
    n_candidates: np.ndarray  # uint32[n_reads] M
    n: np.ndarray             # the hash count of an examined read
    matched: np.ndarray
    shared: np.ndarray
    n_hashes: np.ndarray      # of every read
    cand_off: np.ndarray      # uint64[n_reads + 1]
    cand_tuple: np.ndarray    # uint64[n_cand] index in the batch CSR
    cand_bin: np.ndarray      # int64[n_cand]
    cand_count: np.ndarray    # uint32[n_cand]
    cand_hits: np.ndarray
    cand_excl: np.ndarray
    n_examined: int
    seconds_kernels: float
    probes: int


@dataclass
class ExclusiveTable:
    """Exclusive.results(): per user bin the four sums of the whole run and the sketch of the hashes that were exclusive to it"""
    precision: int
    cand_reads: np.ndarray       # uint64[n_user_bins]
    hits: np.ndarray
    exclusive_hits: np.ndarray
    exclusive_reads: np.ndarray
    registers: np.ndarray        # uint8[n_user_bins, 2^precision]
    seconds_kernels: float
    probes: int

    def distinct(self, b):
        """DISTINCT_EXCLUSIVE of `taxor search --exclusive-file`: the rounded estimate, at least 1 where a hash was exclusive"""
        d = int(np.floor(hll_estimate(self.registers[b], self.precision) + 0.5))      # llround: halves away from zero
        return max(d, 1) if self.exclusive_hits[b] else d


class Exclusive:
    """Hashes only one reference explains (taxor_amd/csrc/exclusive.hip).  `ixfs` is the list the GpuIndex was made from (only bins and
    fname_idx are read).  add_batch follows a batch that ran with Searcher.capture() on and takes its SavedBatch, which stays the
    caller's; add_csr takes host arrays; results gives the run's sums.  The arrays returned are copies."""

    READ_WORDS = (("n_candidates", np.uint32), ("n", np.uint32), ("matched", np.uint32), ("shared", np.uint32), ("n_hashes", np.uint32))
    CAND_WORDS = (("cand_tuple", np.uint64), ("cand_bin", np.int64), ("cand_count", np.uint32), ("cand_hits", np.uint32), ("cand_excl", np.uint32))

    def __init__(self, index: GpuIndex, ixfs, precision=0):
        view, keep = GpuIndex._view([dict(f, data=None) for f in ixfs], index.n_user_bins, index.k, index.s, index.t, index.use_syncmer, 1,
                                    index.window_size)
        self._L = _lib.lib()
        self._h = C.c_void_p()
        self.index = index
        check(self._L.taxor_gpu_exclusive_create(index._h, C.byref(view), int(precision), C.byref(self._h)))
        del keep

    @classmethod
    def _batch(cls, b):
        n, m = int(b.n_reads), int(b.n_cand)
        arr = lambda ptr, k, dt: np.ctypeslib.as_array(ptr, shape=(k,)).copy() if k else np.zeros(0, dt)
        return ExclusiveBatch(int(b.precision), arr(b.examined, n, np.uint8).astype(bool), *[arr(getattr(b, f), n, dt) for f, dt in cls.READ_WORDS],
                              np.ctypeslib.as_array(b.cand_off, shape=(n + 1,)).copy(), *[arr(getattr(b, f), m, dt) for f, dt in cls.CAND_WORDS],
                              int(b.n_examined), float(b.seconds_kernels), int(b.probes))

    def add_batch(self, searcher: Searcher, saved: "SavedBatch") -> ExclusiveBatch:
        b = _lib.ExclusiveBatch()
        check(self._L.taxor_gpu_exclusive_add_batch(self._h, searcher._h, saved._h if saved is not None else None, C.byref(b)))
        return self._batch(b)

    def add_csr(self, read_off, user_bin, count, hash_off, hashes) -> ExclusiveBatch:
        ro = np.ascontiguousarray(read_off, dtype=np.uint64)
        ub = np.ascontiguousarray(user_bin, dtype=np.int64)
        ct = np.ascontiguousarray(count, dtype=np.uint32)
        ho = np.ascontiguousarray(hash_off, dtype=np.uint64)
        hs = np.ascontiguousarray(hashes, dtype=np.uint64)
        assert ro.size >= 1 and ho.size == ro.size and ub.size == ct.size and int(ro[-1]) <= ub.size and int(ho[-1]) <= hs.size
        b = _lib.ExclusiveBatch()
        check(self._L.taxor_gpu_exclusive_add_csr(self._h, ro.size - 1, _p(ro), _p(ub) if ub.size else None, _p(ct) if ct.size else None, _p(ho),
                                                  _p(hs) if hs.size else None, C.byref(b)))
        return self._batch(b)

    def results(self) -> ExclusiveTable:
        res = _lib.ExclusiveResults()
        check(self._L.taxor_gpu_exclusive_results(self._h, C.byref(res)))
        n, p = int(res.n_user_bins), int(res.precision)
        arr = lambda ptr, m, dt: np.ctypeslib.as_array(ptr, shape=(m,)).copy() if m else np.zeros(0, dt)
        return ExclusiveTable(p, arr(res.cand_reads, n, np.uint64), arr(res.hits, n, np.uint64), arr(res.exclusive_hits, n, np.uint64),
                              arr(res.exclusive_reads, n, np.uint64), arr(res.registers, n << p, np.uint8).reshape(n, 1 << p), float(res.seconds_kernels),
                              int(res.probes))

    def close(self):
        if getattr(self, "_h", None):
            self._L.taxor_gpu_exclusive_destroy(self._h)
            self._h = C.c_void_p()

    __del__ = close

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


class Comm:
    """Several GPUs of one node driven by this one process (the C++ host's `taxor search --gpus N` shape): the index is
    replicated (one upload + ncclBroadcast), every device classifies its own batch, results are gathered on devices[0].
    transport: "rccl" (RCCL over xGMI, one rank per device) or "host" (same calls staged through host memory)."""

    def __init__(self, devices, transport="rccl"):
        self.devices = [int(d) for d in devices]
        self.transport = transport
        arr = (C.c_int * len(self.devices))(*self.devices)
        h = C.c_void_p()
        check(_lib.lib().taxor_gpu_comm_create(arr, len(self.devices), _lib.COMM_RCCL if transport == "rccl" else _lib.COMM_HOST, C.byref(h)))
        self._h = h

    def close(self):
        if getattr(self, "_h", None):
            _lib.lib().taxor_gpu_comm_destroy(self._h)
            self._h = None

    __del__ = close

    def replicate_index(self, ixfs, n_user_bins, k=22, s=12, t=5, use_syncmer=True, scaling=1, window_size=None, layout=0):
        """-> [GpuIndex on devices[0], GpuIndex on devices[1], ...]; layout as in GpuIndex"""
        view, keep = GpuIndex._view(ixfs, n_user_bins, k, s, t, use_syncmer, scaling, window_size, layout)
        view.ixf_layout = int(layout)
        out = (C.c_void_p * len(self.devices))()
        check(_lib.lib().taxor_gpu_index_create_replicated(self._h, C.byref(view), out))
        del keep
        idx = []
        for d, h in zip(self.devices, out):
            g = GpuIndex.__new__(GpuIndex)
            g._adopt(C.c_void_p(h), ixfs, n_user_bins, k, s, t, d, use_syncmer, window_size)
            idx.append(g)
        return idx

    def set_self_exchange(self, on=True):
        """test hook: rank 0's own results go through ncclSend/ncclRecv to itself (one-GPU boxes execute the exchange code)"""
        check(_lib.lib().taxor_gpu_comm_set_self_exchange(self._h, 1 if on else 0))

    def gather(self, searchers) -> SearchResults:
        """per-read results of one round (searcher i ran its batch on devices[i]) as one CSR in device order"""
        assert len(searchers) == len(self.devices)
        arr = (C.c_void_p * len(searchers))(*[s._h for s in searchers])
        res = _lib.Results()
        check(_lib.lib().taxor_gpu_gather_results(self._h, arr, C.byref(res)))
        return _results(res)

    def info(self):
        st = _lib.CommStats()
        check(_lib.lib().taxor_gpu_comm_info(self._h, C.byref(st)))
        return {f: getattr(st, f) for f, _ in _lib.CommStats._fields_}


def read_bam(path):
    """The reads of a BAM file as `taxor search` selects them (SAMv1 section 4.2; secondary and supplementary records left out):
    (ids [bytes], seq4 uint8[], byte_off uint64[], read_len uint32[], reverse uint8[]) -- the SEQ fields back to back, what
    Searcher.search_nibbles / pack_nibbles take.  Plain Python over gzip; for tests and small files."""
    import gzip
    import struct
    with gzip.open(path, "rb") as f:
        raw = f.read()
    if raw[:4] != b"BAM\1":
        raise ValueError(f"{path}: not BAM")
    l_text, = struct.unpack_from("<i", raw, 4)
    p = 8 + l_text
    n_ref, = struct.unpack_from("<i", raw, p)
    p += 4
    for _ in range(n_ref):
        l_name, = struct.unpack_from("<i", raw, p)
        p += 4 + l_name + 4
    ids, seq, boff, rlen, rev = [], bytearray(), [], [], []
    while p < len(raw):
        block_size, = struct.unpack_from("<I", raw, p)
        l_read_name, = struct.unpack_from("<B", raw, p + 12)
        n_cigar, flag, l_seq = struct.unpack_from("<HHi", raw, p + 16)
        name_at = p + 36
        if not flag & 0x900:
            ids.append(raw[name_at:name_at + l_read_name - 1])
            at = name_at + l_read_name + 4 * n_cigar
            boff.append(len(seq))
            rlen.append(l_seq)
            rev.append(1 if flag & 0x10 else 0)
            seq += raw[at:at + (l_seq + 1) // 2]
        p += 4 + block_size
    return (ids, np.frombuffer(bytes(seq), dtype=np.uint8), np.array(boff, dtype=np.uint64), np.array(rlen, dtype=np.uint32),
            np.array(rev, dtype=np.uint8))
