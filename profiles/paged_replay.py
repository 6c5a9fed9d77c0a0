"""paged search on paged_search.py's 0.5-GB synthetic index, library level (reads in host memory, no file): every pass from bases
against pass 0 from bases with capture + later passes replayed from the saved hash lists; and pass 0 alone with capture off / on"""
import json, sys, time
import numpy as np
sys.path.insert(0, ".")
from taxor_amd import GpuIndex, Searcher, _lib, synth
from taxor_amd.search import PassResults, plan_passes

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
whole, _, _ = plan_passes(host, n_ub, 1 << 40)
out = dict(index_bytes=whole["index_bytes"], reads=60000, gbp=gbp, runs=[])

idx = GpuIndex(host, n_ub)
sr = Searcher(idx)
sr.search_batch(bases, offs, copy=False)
t0 = time.perf_counter(); ref = sr.search_batch(bases, offs); out["resident_wall_s"] = time.perf_counter() - t0
sr.close(); idx.close()

budgets = {}
for budget in range(whole["root_bytes"], whole["index_bytes"], 4 << 20):
    try:
        plan, _, _ = plan_passes(host, n_ub, budget)
    except _lib.TaxorError:
        continue
    if plan["n_passes"] >= 3 and plan["n_passes"] not in budgets:
        budgets[plan["n_passes"]] = budget

for rep in range(3):
    for passes, budget in budgets.items():
        for kind in ("bases", "replay"):
            idx = GpuIndex.paged(host, n_ub, budget)
            sr = Searcher(idx)
            prior, sv, pass_s = [], None, []
            t0 = time.perf_counter()
            for p in range(idx.passes):
                tp = time.perf_counter()
                idx.load_pass(p)
                if kind == "replay" and p == 0:
                    sr.capture(True)
                    r = sr.search_batch(bases, offs)
                    prior.append(PassResults(r, sr.result_keys(r.user_bin.size)))
                    sv = sr.take_saved()
                    sr.capture(False)
                elif kind == "replay":
                    if p + 1 < idx.passes:
                        prior.append(sr.search_saved_pass(sv))
                    else:
                        sr.search_saved(sv)
                elif p + 1 < idx.passes:
                    prior.append(sr.search_pass(bases, offs))
                else:
                    sr.search_batch(bases, offs, copy=False)
                pass_s.append(time.perf_counter() - tp)
            got = sr.merge_prior(prior)
            wall = time.perf_counter() - t0
            same = bool(np.array_equal(got.read_off, ref.read_off) and np.array_equal(got.user_bin, ref.user_bin) and np.array_equal(got.count, ref.count))
            out["runs"].append(dict(kind=kind, rep=rep, passes=passes, wall_s=wall, pass_s=pass_s, identical=same,
                                    saved_bytes=sv.nbytes if sv is not None else 0))
            if sv is not None:
                sv.close()
            sr.close(); idx.close()
print(json.dumps(out))
