"""The read-side selectors (k_syncmers<11>, k_syncmers<0>, k_syncmers_wave<11>, k_minimisers) over the whole domain that
taxor_gpu_index_create admits, at the lengths where their tiles, capacities and dedup strategies change.

Syncmer indexes: every (k, s) with 2 <= k <= 32, 1 <= s <= 16, s < k, w = k-s+1 <= 32, at t in {1, w//2 (the build default,
taxor_build.cpp:510), w}, and t = 1..w for every pair of the w = 11 fast path.  The GPU answer must equal the CPU oracle and, where
oracle/_ref/ holds libtaxor_ref_syncmer.so (the reference's own selector, see tests/test_syncmer_ref_cpu.py), wyhash of the
reference's selection for k <= 31 (k = 32 is the documented divergence).  Minimiser indexes: k = 1..32 x (w-k+1) in
{1, 2, 11, 64, 511, 512} against the oracle.  Whole path: about thirty configurations spread over the domain, search of a
planted hierarchy, tuples identical to the oracle, for a small call and for a batch above SMALL_MAX_READS.

Every read length comes from the kernels' own constants, read out of taxor_amd/csrc (kernels.hip, kernels.h, api.hip)."""
import os
import re
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

from oracle import oracle as orc
from taxor_amd import GpuIndex, Searcher, synth

pytestmark = pytest.mark.gpu

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "taxor_amd", "csrc")


def _constants():
    """`static constexpr <int type> NAME = EXPR;` of kernels.hip / kernels.h, EXPR over earlier names, + SMALL_MAX_READS"""
    env = {}
    for f in ("kernels.h", "kernels.hip"):
        src = open(os.path.join(CSRC, f)).read()
        for name, expr in re.findall(r"static constexpr (?:int|uint32_t) (\w+) = ([^;]+);", src):
            try:
                env[name] = int(eval(re.sub(r"(\d)u\b", r"\1", expr), {}, dict(env)))
            except Exception:
                pass
    api = open(os.path.join(CSRC, "api.hip")).read()
    env["SMALL_MAX_READS"] = int(re.search(r"SMALL_MAX_READS = (\d+)", api).group(1))
    kern = open(os.path.join(CSRC, "kernels.hip")).read()
    env["SY_PASS"] = int(re.search(r"\(n_sel \+ (\d+)u\) / (\d+)u", kern).group(2))     # candidates per LDS dedup pass
    return env


K = _constants()
BLK, SY_T, WV_T, MN_T = K["BLK"], K["SY_T"], K["WV_T"], K["MN_T"]
SY_LDS_CAND, SY_PASS = K["SY_LDS_CAND"], K["SY_PASS"]
SYNC_WAVE_CAND, SYNC_LDS_DEDUP_MAX, SMALL_MAX_READS = K["SYNC_WAVE_CAND"], K["SYNC_LDS_DEDUP_MAX"], K["SMALL_MAX_READS"]
REF = orc.ref_syncmer_lib()
POOL = ThreadPoolExecutor(8)


def test_kernel_constants_read():
    assert (BLK, SY_T, WV_T, MN_T) == (256, 2048, 512, 1024)
    assert (SY_LDS_CAND, SY_PASS, SYNC_WAVE_CAND, SYNC_LDS_DEDUP_MAX, SMALL_MAX_READS) == (2048, 1536, 512, 66816, 16384)


def _domain():
    return [(k, s) for k in range(2, 33) for s in range(1, 17) if s < k and k - s + 1 <= 32]


def _fast_path(k, s):
    """syncmers_wave_applies / launch_syncmers (kernels.hip): w == 11 and s <= 13 take k_syncmers<11> and k_syncmers_wave<11>"""
    return k - s + 1 == 11 and s <= 13


def _cfgs(k):
    out = []
    for k_, s in _domain():
        if k_ != k:
            continue
        w = k - s + 1
        ts = range(1, w + 1) if _fast_path(k, s) else sorted({1, w // 2, w} - {0})
        out += [(k, s, t) for t in ts]
    return out


def _round_up(x, m):
    return (x + m - 1) // m * m


def _wave_cross(gap):
    """first nwin whose candidate capacity (layout_batch: round_up(nwin/gap + 2, 16)) exceeds SYNC_WAVE_CAND"""
    n = max(0, (SYNC_WAVE_CAND - 3) * gap)
    while _round_up(n // gap + 2, 16) <= SYNC_WAVE_CAND:
        n += 1
    return n


def _wyhash(x):
    """orc_wyhash_u64 over a uint64 array (lo64 ^ hi64 of x * 0x9E3779B97F4A7C15)"""
    x = np.asarray(x, dtype=np.uint64)
    m32, c, s32 = np.uint64(0xFFFFFFFF), np.uint64(0x9E3779B97F4A7C15), np.uint64(32)
    a_lo, a_hi, b_lo, b_hi = x & m32, x >> s32, c & m32, c >> s32
    ll, lh, hl, hh = a_lo * b_lo, a_lo * b_hi, a_hi * b_lo, a_hi * b_hi
    mid = (ll >> s32) + (lh & m32) + (hl & m32)
    return ((ll & m32) | (mid << s32)) ^ (hh + (lh >> s32) + (hl >> s32) + (mid >> s32))


def test_wyhash_restatement():
    v = np.random.default_rng(3).integers(0, 2**64, size=500, dtype=np.uint64)
    assert _wyhash(v).tolist() == [orc.wyhash(int(x)) for x in v]


class _Reads:
    def __init__(self, seed):
        self.rng = np.random.default_rng(seed)
        self.acgt = np.frombuffer(b"ACGT", np.uint8)

    def rnd(self, n):
        return bytes(self.rng.choice(self.acgt, size=max(int(n), 0)))

    def lowc(self, n):
        """tie-heavy: random runs, homopolymers and short repeat units"""
        parts, tot = [], 0
        while tot < n:
            c = self.rng.random()
            if c < 0.3:
                p = self.rnd(self.rng.integers(3, 60))
            elif c < 0.6:
                p = bytes([int(self.rng.choice(self.acgt))]) * int(self.rng.integers(5, 120))
            else:
                p = self.rnd(self.rng.integers(2, 9)) * int(self.rng.integers(3, 50))
            parts.append(p)
            tot += len(p)
        return b"".join(parts)[:max(int(n), 0)]


def _sync_reads(k, s, t):
    """(name, read) at the edges of the selector's tiles, capacities and dedup strategies for this (k, s, t)"""
    w = k - s + 1
    gap = max(1, min(t, w - t + 1))                 # layout_batch: minimum distance between two open syncmers
    R = _Reads(k * 10007 + s * 101 + t)
    L = lambda nwin: nwin + k - 1
    out = [(f"nwin={n}", R.rnd(L(n))) for n in (0, 1, 2)]
    out += [(f"nwin=SY_T{d:+d}", R.rnd(L(SY_T + d))) for d in (-1, 0, 1)]
    out += [("nwin=2*SY_T tie-heavy", R.lowc(L(2 * SY_T))), ("nwin=SY_T+1 tie-heavy", R.lowc(L(SY_T + 1))),
            ("nwin=2*SY_T+1", R.rnd(L(2 * SY_T + 1)))]
    if _fast_path(k, s):
        out += [(f"nwin=WV_T*{m}{d:+d}", R.rnd(L(m * WV_T + d))) for m in (1, 2) for d in (-1, 0, 1)]
        out += [("nwin=WV_T+1 tie-heavy", R.lowc(L(WV_T + 1)))]
    x = _wave_cross(gap)                            # wave kernel <-> block kernel
    out += [(f"nwin=wave_cross{d:+d}", R.rnd(L(x + d))) for d in (-1, 0)]
    out += [("nwin=wave_cross-1 tie-heavy", R.lowc(L(x - 1)))]
    for name, n in (("BLK", BLK), ("SY_PASS", SY_PASS), ("SY_LDS_CAND", SY_LDS_CAND)):   # selections ~ nwin / w on random reads
        out += [(f"n_sel~{name}*{f}", R.rnd(L(int(n * w * f)))) for f in (0.95, 1.05)]
    if gap == 1:                                    # slots past SYNC_LDS_DEDUP_MAX: the global dedup table is allocated
        out += [("slots>SYNC_LDS_DEDUP_MAX", R.rnd(L(SYNC_LDS_DEDUP_MAX + 64)))]
    out += [("homopolymer", b"A" * L(SY_T + 37)), ("(AT)n", b"AT" * 1500), ("TTAGGG", b"TTAGGG" * 500),
            ("unit*n", R.rnd(97) * 40), ("tie-heavy 6k", R.lowc(6000))]
    return out


def _cat(reads):
    bases = np.frombuffer(b"".join(reads), dtype=np.uint8) if reads else np.zeros(0, np.uint8)
    return bases, np.cumsum([0] + [len(r) for r in reads]).astype(np.uint64)


def _dummy_index(k, s, t, use_syncmer=True, window_size=None):
    bins, stride, seg = 64, 64, 16
    return GpuIndex([dict(bins=bins, stride=stride, seg_len=seg, seed=1, next_ixf=np.zeros(bins, np.int64), fname_idx=np.arange(bins),
                          data=np.zeros(3 * seg * stride, np.uint8))], bins, k, s, t, use_syncmer=use_syncmer, window_size=window_size)


def _gpu_select(idx, reads, sub):
    sr = Searcher(idx, ratio=0.5, sub_batch_reads=sub)
    try:
        hoff, hashes = sr.seq_to_syncmers(*_cat(reads))
    finally:
        sr.close()
    return [hashes[int(hoff[i]):int(hoff[i + 1])] for i in range(len(reads))]


def _first_diff(a, b):
    a, b = list(a), list(b)
    return next((j for j in range(min(len(a), len(b))) if a[j] != b[j]), min(len(a), len(b)))


@pytest.mark.parametrize("k", range(2, 33))
def test_syncmer_domain(k):
    for k_, s, t in _cfgs(k):
        named = _sync_reads(k, s, t)
        reads = [r for _, r in named]
        want = list(POOL.map(lambda r: orc.seq_to_syncmers(r, k, s, t), reads))
        if REF is not None and k <= 31:
            ref = list(POOL.map(lambda r: orc.ref_seq_to_syncmers(r, k, s, t), reads))
            for (name, r), a, b in zip(named, want, ref):
                assert a.tolist() == _wyhash(b).tolist(), f"oracle vs reference k={k} s={s} t={t} {name} (len {len(r)})"
        idx = _dummy_index(k, s, t)
        try:
            for sub in (0, 5):
                got = _gpu_select(idx, reads, sub)
                for (name, r), g, wv in zip(named, got, want):
                    if g.size != wv.size or not np.array_equal(g, wv):
                        j = _first_diff(g, wv)
                        raise AssertionError(f"k={k} s={s} t={t} sub_batch_reads={sub} read '{name}' (len {len(r)}): "
                                             f"GPU {g.size} vs oracle {wv.size} hashes, first difference at selection {j}")
        finally:
            idx.close()


def test_syncmer_global_dedup_table():
    """reads with more selected syncmers than SYNC_LDS_DEDUP_MAX: the kernel dedups them in the per-block global table
    (generic and fast path, a narrow and a wide window)"""
    for k, s, t in ((3, 1, 1), (22, 12, 5), (12, 9, 2), (21, 16, 2)):
        w = k - s + 1
        R = _Reads(k * 31 + s)
        n = int(SYNC_LDS_DEDUP_MAX * w * 1.15) + k
        reads = [R.rnd(n), R.rnd(3000)]
        want = list(POOL.map(lambda r: orc.seq_to_syncmers(r, k, s, t), reads))
        assert want[0].size > SYNC_LDS_DEDUP_MAX or k == 3, (k, s, t, want[0].size)   # k = 3: only 32 distinct k-mers exist
        idx = _dummy_index(k, s, t)
        try:
            for sub in (0, 1):
                got = _gpu_select(idx, reads, sub)
                for i, (g, wv) in enumerate(zip(got, want)):
                    assert np.array_equal(g, wv), (k, s, t, sub, i, g.size, wv.size, _first_diff(g, wv))
        finally:
            idx.close()


# ------------------------------------------------------------------------------------------------ minimisers
def _mini_reads(k, w):
    R = _Reads(k * 7919 + w)
    L = lambda nwin: nwin + w - 1                   # windows of w bases, MN_T of them per tile
    out = [(n, R.rnd(n)) for n in (k - 1, k, w - 1, w, w + 1)]
    out += [(f"nwin=MN_T*{m}{d:+d}", R.rnd(L(m * MN_T + d))) for m in (1, 2) for d in (-1, 0, 1)]
    out += [("tie-heavy MN_T+1", R.lowc(L(MN_T + 1))), ("homopolymer", b"C" * L(MN_T + 5)), ("(AT)n", b"AT" * 900),
            ("TTAGGG", b"TTAGGG" * 300), ("tie-heavy", R.lowc(3000)), ("IUPAC", b"ACGTNRYKMSWBDHVNacgtnn" * 20)]
    return [(str(a), b) for a, b in out if len(b) > 0] + [("empty", b"")]


@pytest.mark.parametrize("k", range(1, 33))
def test_minimiser_domain(k):
    for span in (1, 2, 11, 64, 511, 512):
        w = k + span - 1
        named = _mini_reads(k, w)
        reads = [r for _, r in named]
        want = list(POOL.map(lambda r: orc.minimiser_hash(orc.dna4_normalise(r), k, w), reads))
        idx = _dummy_index(k, 0, 0, use_syncmer=False, window_size=w)
        try:
            for sub in (0, 3):
                got = _gpu_select(idx, reads, sub)
                for (name, r), g, wv in zip(named, got, want):
                    assert g.size == wv.size and np.array_equal(g, wv), \
                        f"k={k} w={w} sub={sub} read '{name}' (len {len(r)}): GPU {g.size} vs oracle {wv.size}, first at {_first_diff(g, wv)}"
        finally:
            idx.close()


# ------------------------------------------------------------------------------------------------ whole path
WHOLE = [(5, 1, 2), (7, 1, 7), (9, 2, 4), (11, 3, 1), (13, 3, 11), (12, 4, 4), (14, 2, 7), (15, 5, 5), (16, 8, 4), (17, 6, 6),
         (18, 3, 8), (19, 7, 7), (20, 10, 5), (21, 9, 6), (22, 12, 5), (22, 12, 1), (22, 12, 11), (23, 13, 5), (24, 16, 4),
         (25, 10, 8), (26, 14, 6), (27, 8, 10), (28, 14, 7), (29, 16, 7), (30, 12, 9), (30, 16, 1), (31, 16, 8), (31, 11, 10),
         (32, 1, 1), (32, 1, 16), (32, 1, 32), (32, 16, 8), (32, 12, 21)]
BIG = {(22, 12, 5), (13, 3, 11), (32, 1, 16), (27, 8, 10)}


@pytest.mark.parametrize("kst", WHOLE, ids=[f"k{k}s{s}t{t}" for k, s, t in WHOLE])
def test_whole_path(kst):
    k, s, t = kst
    err = 0.04
    pct = -1.0 if orc.syncmer_match_ratio(k, err) >= 0 else 0.3     # no syncmer-model row (odd k, k outside 12..30): percentage
    g, go = synth.random_genomes(5, 6000, seed=k * 100 + s)
    planted = [orc.seq_to_syncmers(bytes(g[int(go[i]):int(go[i + 1])]), k, s, t) for i in range(5)]
    lay = synth.make_layout(planted, root_bins=64, child_bins=32, n_children=3, seed=k + 7 * s + 31 * t)
    host = synth.materialize_host(lay)
    idx = GpuIndex(host, lay["n_user_bins"], k, s, t)
    h = orc.Hixf(host, [f["next_ixf"] for f in host], [f["fname_idx"] for f in host])
    try:
        calls = [(300, 900, (0,))]                                        # a small call: the lanes path
        if kst in BIG:
            calls.append((SMALL_MAX_READS + 700, 150, (0, 4096)))         # above SMALL_MAX_READS: the sub-batch pipeline
        for n, rl, subs in calls:
            bases, offs, _ = synth.synth_reads(g, go, n, rl, error_rate=0.03, frac_random=0.1, seed=n + k)
            for sub in subs:
                sr = Searcher(idx, error_rate=err, percentage=pct, sub_batch_reads=sub)
                try:
                    res = sr.search_batch(bases, offs)
                finally:
                    sr.close()
                nh, off, ub, cnt, _ = h.search_batch(bases, offs, k=k, s=s, t=t, err=err, percentage=pct, threads=8)
                assert np.array_equal(res.n_hashes, nh), (kst, n, sub)
                assert np.array_equal(res.read_off, off) and np.array_equal(res.user_bin, ub) and np.array_equal(res.count, cnt), (kst, n, sub)
                assert ub.size > 0, (kst, n)
    finally:
        idx.close()
