"""The root's 2-bit plane and the screen of k_query_level<..., SCREEN> (kernels.hip, query_screen_range): large batches count the
first hashes of a read on a quarter-size copy of the root's rows that keeps fingerprint & 3, and only the runs whose 2-bit sum can
still reach the threshold are then counted exactly.  Whatever the screen does, the tuples are the CPU oracle's, bit for bit; a
searcher created with screen=False (TAXOR_SEARCH_NO_SCREEN) on the same index is the second check.

Single reads go through bulk_contains (a hash list and a threshold of the caller's choice: the level-synchronous launches of the
searcher itself, one root item), batches through search_batch.  Every index here is a few megabytes."""
import numpy as np
import pytest

from oracle import oracle as orc
from taxor_amd import GpuIndex, Searcher, synth

pytestmark = pytest.mark.gpu

Q_CAP = 1024          # kernels.hip: probes staged at once
N_KEYS = 1600         # keys per planted bin


def _keys(rng, n=N_KEYS):
    return np.unique(rng.integers(1, 2**63, size=n + 64, dtype=np.uint64))[:n]


def make_root(bins, seed, leaves=(), runs=(), merged=(), decoys2=(), filler_run=0):
    """A root of `bins` bins over one child per merged bin.  leaves: bins holding a key set each; runs: (first bin, length) split
    runs holding one key set each, dealt over their bins; merged: bins leading to a 64-bin child with the key set in its bin 5;
    decoys2: bins whose column answers every key of its set on the low two fingerprint bits and none on all eight; filler_run > 0:
    every bin not named otherwise belongs to a decoy split run of that length.  -> (host IXF list, n_user_bins, {name: keys})"""
    rng = np.random.default_rng(seed)
    fname = np.full(bins, -2, np.int64)
    nxt = np.zeros(bins, np.int64)
    bin_keys, sets, ub = {}, {}, 0
    for b in leaves:
        sets[("leaf", b)] = bin_keys[b] = _keys(rng)
        fname[b] = ub
        ub += 1
    for first, ln in runs:
        k = sets[("run", first)] = _keys(rng)
        for j in range(ln):
            bin_keys[first + j] = k[j::ln]
            fname[first + j] = ub
        ub += 1
    for b in decoys2:
        sets[("decoy2", b)] = bin_keys[b] = _keys(rng)
        fname[b] = ub
        ub += 1
    children = []
    for b in merged:
        sets[("merged", b)] = bin_keys[b] = _keys(rng)
        fname[b] = -1
        nxt[b] = 1 + len(children)
        children.append(b)
    b = 0
    while b < bins:                                    # everything else: decoys of their own, or decoy split runs
        if fname[b] != -2:
            b += 1
            continue
        e = b
        while e < bins and fname[e] == -2 and e - b < max(1, filler_run):
            fname[e] = ub
            e += 1
        ub += 1
        b = e
    seg = synth.seg_len_for(N_KEYS)
    sd, cols = synth.build_columns(bin_keys, seg, int(rng.integers(1, 2**62)))
    stride = (bins + 63) // 64 * 64
    data = rng.integers(0, 256, size=(3 * seg, stride), dtype=np.uint8)
    for bb, col in cols.items():
        data[:, bb] = col
    for bb in decoys2:
        data[:seg, bb] ^= 0x80                         # one of every key's three rows: the XOR misses on bit 7, the low bits still agree
    host = [dict(bins=bins, stride=stride, seg_len=seg, seed=sd, next_ixf=nxt, fname_idx=fname, data=data.reshape(-1))]
    for ci, mb in enumerate(children):
        csd, ccols = synth.build_columns({5: bin_keys[mb]}, seg, int(rng.integers(1, 2**62)))
        cdata = rng.integers(0, 256, size=(3 * seg, 64), dtype=np.uint8)
        cdata[:, 5] = ccols[5]
        host.append(dict(bins=64, stride=64, seg_len=seg, seed=csd, next_ixf=np.full(64, 1 + ci, np.int64),
                         fname_idx=np.arange(ub, ub + 64, dtype=np.int64), data=cdata.reshape(-1)))
        ub += 64
    host[0]["next_ixf"] = np.where(fname == -1, nxt, 0)
    return host, ub, sets


class Rig:
    """an index, the oracle over the same bytes, a screening and a non-screening searcher"""

    def __init__(self, host, n_ub, sets):
        self.host, self.sets = host, sets
        self.idx = GpuIndex(host, n_ub)
        self.orc = orc.Hixf(host, [f["next_ixf"] for f in host], [f["fname_idx"] for f in host])
        self.on = Searcher(self.idx, ratio=0.5, small_path=False)
        self.off = Searcher(self.idx, ratio=0.5, small_path=False, screen=False)

    def check(self, hashes, thr, screened=None):
        """one read of these hashes under this threshold -> the oracle's tuples; screened: whether the plane must (not) have been read"""
        eub, ecnt, _ = self.orc.bulk_contains(hashes, thr)
        for sr in (self.on, self.off):
            ub, cnt = sr.bulk_contains(hashes, thr)
            assert np.array_equal(ub, eub) and np.array_equal(cnt, ecnt), (len(hashes), thr, sr is self.on)
            loads = sr.stats()["screen_plane_loads"]
            assert sr is self.on or loads == 0
            if sr is self.on and screened is not None:
                assert (loads > 0) == screened, (len(hashes), thr, loads)
        return eub, ecnt

    def close(self):
        self.on.close()
        self.off.close()
        self.idx.close()


def _query(rng, keys, n_own, n_h):
    """n_h distinct hashes: n_own of the key set, the rest random"""
    own = keys[rng.permutation(keys.size)[:n_own]]
    rnd = rng.integers(1, 2**63, size=n_h - n_own, dtype=np.uint64) | np.uint64(1 << 63)      # (the key sets stay below 2^63)
    h = np.concatenate([own, rnd])
    return h[rng.permutation(h.size)]


def _std_spec(bins):
    """planted leaves in the first and the last unit, a merged bin and a leaf in one unit, a split run of two over a unit boundary, a 2-bit decoy"""
    return dict(leaves=(1, bins - 3, 41), runs=((15, 2),), merged=(40,), decoys2=(60,))


@pytest.fixture(scope="module")
def rigs():
    made = {}

    def get(name):
        if name not in made:
            if isinstance(name, int):
                made[name] = Rig(*make_root(name, 100 + name, **_std_spec(name)))
            elif name == "runs":       # 1024 bins: runs of 2, 3 and 17; over a unit boundary, over a 128-bin line boundary, onto the last bin
                made[name] = Rig(*make_root(1024, 7, leaves=(1, 1000), merged=(40,), runs=((15, 2), (127, 3), (200, 17), (1022, 2))))
            elif name == "many":       # one key set in a leaf of each of 40 units: more alive units than Q_MAXU = 32
                host, n_ub, sets = make_root(1024, 8, leaves=(1,))
                col = host[0]["data"].reshape(-1, 1024)[:, 1].copy()
                for u in range(1, 40):
                    host[0]["data"].reshape(-1, 1024)[:, 16 * u + 3] = col
                made[name] = Rig(host, n_ub, sets)
            elif name == "split":      # nothing but split runs of eight: the split-run rule gives this root no plane
                made[name] = Rig(*make_root(1024, 9, leaves=(1,), filler_run=8))
        return made[name]

    yield get
    for r in made.values():
        r.close()


@pytest.mark.parametrize("bins", [256, 512, 1024, 2048])
def test_root_widths(rigs, bins):
    """plane rows of 128 B, 256 B and 512 B; rows of 256 B have no plane and run unscreened"""
    rig = rigs(bins)
    plane = rig.idx.root_plane()
    assert (plane is None) == (bins < 512)
    if plane is not None:
        assert plane.shape[1] == bins // 4
    rng = np.random.default_rng(bins)
    for name, keys in rig.sets.items():
        h = _query(rng, keys, 500, 700)
        ub, _ = rig.check(h, 350, screened=bins >= 512)
        assert (ub.size == 0) == (name[0] == "decoy2"), name      # the decoy passes on two bits (500 >= 350) and fails on eight


@pytest.mark.parametrize("n_h", [0, 1, 3, 240, 241, Q_CAP, Q_CAP + 1, 3 * Q_CAP + 5])
def test_hash_counts(rigs, n_h):
    """probes staged at once and in tiles; tile boundaries of the byte counters; reads too short to screen"""
    rig = rigs(1024)
    rng = np.random.default_rng(1000 + n_h)
    for name in (("leaf", 1), ("leaf", 1021), ("merged", 40), ("run", 15), ("decoy2", 60)):
        h = _query(rng, rig.sets[name], min(N_KEYS, (n_h * 2 + 2) // 3), n_h)
        rig.check(h, n_h // 2, screened=True if n_h >= 240 else None)
        rig.check(h, (n_h * 2 + 2) // 3)


def test_thresholds(rigs):
    """both sides of every boundary: nothing pruned, one match, all hashes, more than all, the planted bin's own count"""
    rig = rigs(1024)
    rng = np.random.default_rng(5)
    n_h = 600
    for name in (("leaf", 1), ("leaf", 1021), ("leaf", 41), ("merged", 40), ("run", 15)):
        h = _query(rng, rig.sets[name], 400, n_h)
        ub, cnt = rig.check(h, 300, screened=True)
        assert ub.size >= 1
        c = int(cnt.max())                                       # the planted bin's exact count (400 and a few false positives)
        assert 400 <= c < 420
        for thr, screened in ((0, False), (1, False), (n_h, True), (n_h + 1, False), (c, True), (c + 1, True)):
            e, _ = rig.check(h, thr, screened=screened)
            if thr in (n_h, n_h + 1, c + 1):
                assert e.size == 0
            if thr == c:
                assert e.size >= 1
    h = _query(rng, rig.sets[("decoy2", 60)], 400, n_h)          # 2-bit count >= 400, exact count a handful
    ub, _ = rig.check(h, 300, screened=True)
    assert ub.size == 0
    assert rig.check(h, 1)[0].size > 0


def test_run_shapes(rigs):
    """split runs of 2, 3 and 17 bins, across a unit and a line boundary and onto the row's last bin; planted bins in units 0 and units - 1"""
    rig = rigs("runs")
    assert rig.idx.root_plane() is not None
    rng = np.random.default_rng(6)
    for name, keys in rig.sets.items():
        # (a run of 17 random bins collects up to ~17 / 256 of the foreign hashes as false positives: the misses keep clear of that)
        for n_own, n_h, thr in ((500, 700, 350), (500, 700, 620), (300, 1500, 800), (900, 1100, 880)):
            h = _query(rng, keys, n_own, n_h)
            ub, cnt = rig.check(h, thr, screened=True)
            assert (ub.size > 0) == (n_own >= thr), (name, n_own, thr, cnt)


def test_dense_fallback(rigs):
    """forty units stay alive after the screen: the item is counted on the rows from its first hash"""
    rig = rigs("many")
    assert rig.idx.root_plane() is not None
    rng = np.random.default_rng(7)
    h = _query(rng, rig.sets[("leaf", 1)], 600, 600)
    ub, cnt = rig.check(h, 300, screened=True)
    assert ub.size == 40 and int(cnt.min()) >= 600
    h = _query(rng, rig.sets[("leaf", 1)], 400, 700)
    assert rig.check(h, 380, screened=True)[0].size == 40


def test_split_run_rule(rigs):
    """a root made of split runs gets no plane, and searches it as before"""
    rig = rigs("split")
    assert rig.idx.root_plane() is None
    rng = np.random.default_rng(8)
    h = _query(rng, rig.sets[("leaf", 1)], 500, 700)
    assert rig.check(h, 350, screened=False)[0].size >= 1


def test_plane_content(rigs):
    rig = rigs(1024)
    rows = rig.idx.download_ixf(0).reshape(-1, 1024)
    two = (rows & 3).astype(np.uint32).reshape(rows.shape[0], 64, 16)
    words = (two << (2 * np.arange(16, dtype=np.uint32))[None, None, :]).sum(axis=2, dtype=np.uint32)
    plane = rig.idx.root_plane()
    assert plane.shape == (rows.shape[0], 256)
    assert np.array_equal(np.ascontiguousarray(plane).view("<u4"), words)


def test_stale_plane():
    """a root column rewritten (upload_bin) after a screened search: the next search sees the new column"""
    host, n_ub, sets = make_root(1024, 11, **_std_spec(1024))
    rig = Rig(host, n_ub, sets)
    try:
        rng = np.random.default_rng(1111)                        # (not the seed the root's own key sets came from)
        from taxor_amd import _lib
        seg = host[0]["seg_len"]
        col = np.zeros(3 * seg, np.uint8)
        for _ in range(16):                                      # a key set that peels under the root's seed
            fresh = _keys(rng)
            if _lib.lib().taxor_ixf_build_bin_arith(fresh.ctypes.data_as(_lib.C.c_void_p), fresh.size, host[0]["seed"], seg, 0,
                                                    col.ctypes.data_as(_lib.C.c_void_p)) == 0:
                break
        else:
            raise AssertionError("no key set peeled under the root's seed")
        h = _query(rng, fresh, 500, 700)
        assert rig.check(h, 350, screened=True)[0].size == 0
        rig.idx.upload_bin(0, 500, col)
        host[0]["data"].reshape(-1, 1024)[:, 500] = col
        rig.orc = orc.Hixf(host, [f["next_ixf"] for f in host], [f["fname_idx"] for f in host])
        ub, cnt = rig.check(h, 350, screened=True)
        assert ub.size == 1 and int(cnt[0]) >= 500
        assert np.array_equal(rig.idx.root_plane()[:, 125] & 3, col & 3)          # bin 500: word 31, bits 8-9 -> byte 125, bits 0-1
    finally:
        rig.close()


def test_routing():
    """the pipeline of large batches (a sub-batch of 4096 reads and more: queues grouped by IXF, level-synchronous launches) screens
    its root items, in sub-batches of any size; a call of 256 reads on a default searcher takes the small path, which never does"""
    g, go = synth.random_genomes(6, 20000, seed=21)
    dummy = GpuIndex([dict(bins=64, stride=64, seg_len=16, seed=1, next_ixf=np.zeros(64, np.int64), fname_idx=np.arange(64),
                           data=np.zeros(3 * 16 * 64, np.uint8))], 64)
    hs = Searcher(dummy, ratio=0.5)
    hoff, hashes = hs.seq_to_syncmers(g, go)
    hs.close()
    dummy.close()
    lay = synth.make_layout([hashes[int(hoff[i]):int(hoff[i + 1])] for i in range(6)], root_bins=1024, child_bins=32, n_children=3, seed=22)
    host = synth.materialize_host(lay)
    idx = GpuIndex(host, lay["n_user_bins"])
    assert idx.root_plane() is not None
    h = orc.Hixf(host, [f["next_ixf"] for f in host], [f["fname_idx"] for f in host])
    bases, offs, _ = synth.synth_reads(g, go, 4300, 2000, error_rate=0.02, frac_random=0.1, seed=23)
    nh, off, ub, cnt, _ = h.search_batch(bases, offs, percentage=0.6, threads=8)
    assert ub.size > 0
    try:
        for kw, n, want in ((dict(small_path=False), 4300, True), (dict(small_path=False, screen=False), 4300, False), (dict(), 256, False),
                            (dict(small_path=False, sub_batch_reads=97), 256, True)):
            sr = Searcher(idx, percentage=0.6, **kw)
            res = sr.search_batch(bases[:int(offs[n])], offs[:n + 1])
            t = int(off[n])
            assert np.array_equal(res.n_hashes, nh[:n]) and np.array_equal(res.read_off, off[:n + 1])
            assert np.array_equal(res.user_bin, ub[:t]) and np.array_equal(res.count, cnt[:t])
            assert (sr.stats()["screen_plane_loads"] > 0) == want, (kw, n)
            sr.close()
    finally:
        idx.close()
