"""resident vs paged search on a synthetic two-level index: per-phase HIP-event times, upload wait"""
import ctypes as C, json, sys, time
import numpy as np
sys.path.insert(0, ".")
from taxor_amd import GpuIndex, Searcher, _lib, synth
from taxor_amd.search import plan_passes

g, go = synth.random_genomes(18, 60000, seed=1)
bins = 64
dummy = GpuIndex([dict(bins=bins, stride=64, seg_len=16, seed=1, next_ixf=np.zeros(bins, np.int64), fname_idx=np.arange(bins), data=np.zeros(3 * 16 * 64, np.uint8))], bins)
hs = Searcher(dummy, ratio=0.5)
hoff, hashes = hs.seq_to_syncmers(g, go)
hs.close(); dummy.close()
planted = [hashes[int(hoff[i]):int(hoff[i + 1])] for i in range(18)]
lay = synth.make_layout(planted, root_bins=64, child_bins=128, n_children=8, child_max_elems=400000, seed=2, with_deep=False)
host = synth.materialize_host(lay)
n_ub = lay["n_user_bins"]
bases, offs, _ = synth.synth_reads(g, go, 60000, 2000, error_rate=0.02, frac_random=0.1, seed=3)
gbp = float(offs[-1]) / 1e9
sizes = sorted({int(3 * f["seg_len"] * f["stride"]) for f in host})
whole, _, _ = plan_passes(host, n_ub, 1 << 40)
out = dict(index_bytes=whole["index_bytes"], root_bytes=whole["root_bytes"], reads=60000, gbp=gbp, runs=[])

def phases(st):
    return dict(hashing_ms=st["syncmer_ms"], root_ms=st["level_ms"][0], child_ms=float(sum(st["level_ms"][1:])), finalize_ms=st["finalize_ms"], total_ms=st["total_ms"])

def add(a, b):
    return {k: a.get(k, 0.0) + b[k] for k in b}

for rep in range(3):
    idx = GpuIndex(host, n_ub)
    sr = Searcher(idx, time_kernels=True)
    sr.search_batch(bases, offs, copy=False)
    t0 = time.perf_counter(); ref = sr.search_batch(bases, offs); wall = time.perf_counter() - t0
    out["runs"].append(dict(kind="resident", rep=rep, passes=1, wall_s=wall, s_per_gbp=wall / gbp, **phases(sr.stats())))
    sr.close(); idx.close()
    seen = set()
    for budget in range(whole["root_bytes"], whole["index_bytes"], 4 << 20):
        try:
            plan, _, _ = plan_passes(host, n_ub, budget)
        except _lib.TaxorError:
            continue
        if plan["n_passes"] < 3 or plan["n_passes"] in seen:
            continue
        seen.add(plan["n_passes"])
        idx = GpuIndex.paged(host, n_ub, budget)
        sr = Searcher(idx, time_kernels=True)
        L = _lib.lib(); L.taxor_gpu_index_upload_wait_seconds.restype = C.c_double
        ph, prior = {}, []
        t0 = time.perf_counter()
        for p in range(idx.passes):
            idx.load_pass(p)
            if p + 1 < idx.passes:
                prior.append(sr.search_pass(bases, offs))
            else:
                sr.search_batch(bases, offs, copy=False)
            ph = add(ph, phases(sr.stats()))
        tm = time.perf_counter()
        got = sr.merge_prior(prior)
        wall = time.perf_counter() - t0
        same = bool(np.array_equal(got.read_off, ref.read_off) and np.array_equal(got.user_bin, ref.user_bin) and np.array_equal(got.count, ref.count))
        out["runs"].append(dict(kind="paged", rep=rep, passes=plan["n_passes"], budget=budget, slab_bytes=plan["slab_bytes"], wall_s=wall, s_per_gbp=wall / gbp,
                                merge_s=time.perf_counter() - tm, upload_wait_s=float(L.taxor_gpu_index_upload_wait_seconds(idx._h)), identical=same, **ph))
        sr.close(); idx.close()
print(json.dumps(out))
