#!/usr/bin/env python3
"""The index census (taxor_amd/csrc/census.hip; docs/EXPERIMENTS.md, "Index census") on one MI355X: wall time and
HIP-event time of one streaming pass over a resident index, the achieved GB/s (index bytes over event time) and, taken in the same
process, a device-to-device copy of a buffer far larger than the Infinity Cache as the streaming baseline (it reads AND writes every
byte: its GB/s counts both, so a pure read at the copy's rate of traffic would show the same figure).

Legs, each printed as it ends:
  (r) bench.py's index of the workload named (gtdb: 113 GB), random-filled: every bin comes out flagged -- throughput only
  (e) the same layout with every bin a real filter (synth.exact_fill_index, fill 0.95): throughput, and how many bins are flagged
  (s) a two-level index built from synthetic keys whose per-bin counts are known (synth.full_hierarchy_shapes, build_hixf_synth):
      the worst |keys_est - n| / sqrt(n / 255) over all its bins, leaf bins against their counts, merged bins against their unions
usage: python profiles/census_cli.py [workload=gtdb] [runs=5] [legs=res]"""
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

import bench  # noqa: E402
from taxor_amd import GpuIndex, synth  # noqa: E402
from taxor_amd.search import census_capacity  # noqa: E402

workload = sys.argv[1] if len(sys.argv) > 1 else "gtdb"
runs = int(sys.argv[2]) if len(sys.argv) > 2 else 5
legs = sys.argv[3] if len(sys.argv) > 3 else "res"


def copy_baseline(n_bytes=8 << 30, reps=5):
    a = torch.empty(n_bytes, dtype=torch.uint8, device="cuda:0").random_(0, 256)
    b = torch.empty_like(a)
    b.copy_(a)
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        b.copy_(a)
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1) * 1e-3)
    del a, b
    torch.cuda.empty_cache()
    t = statistics.median(ts)
    print(f"baseline: device-to-device copy of {n_bytes/1e9:.1f} GB, median of {reps}: {t*1e3:.2f} ms = {2*n_bytes/t/1e9:.0f} GB/s read + written "
          f"({n_bytes/t/1e9:.0f} GB/s copied)", flush=True)
    return 2 * n_bytes / t / 1e9


def measure(idx, name, base):
    idx.census()                                       # warm-up: code object, work list
    walls, evs, t = [], [], None
    for _ in range(runs):
        t0 = time.perf_counter()
        t = idx.census()
        walls.append(time.perf_counter() - t0)
        evs.append(t.seconds_kernel)
    ev, wall = statistics.median(evs), statistics.median(walls)
    print(f"{name}: {t.bytes_read/1e9:.2f} GB in {len(t.bin_first)-1} IXFs, {t.nonzero.size} bins, {t.n_tiles} tiles, {t.launches} launch(es); wall median {wall*1e3:.2f} ms "
          f"(create + cut + pass + fetch, min {min(walls)*1e3:.2f}), event median {ev*1e3:.3f} ms (min {min(evs)*1e3:.3f}, max {max(evs)*1e3:.3f}) = "
          f"{t.bytes_read/ev/1e9:.0f} GB/s = {t.bytes_read/ev/1e9/base:.3f} of the copy's traffic rate", flush=True)
    return t


def flagged(t, shapes):
    n = 0
    for x, f in enumerate(shapes):
        cap = census_capacity(f["seg_len"])
        n += int(np.count_nonzero(t.of_ixf(x) > cap))
    return n


base = copy_baseline()
if "r" in legs or "e" in legs:
    args = bench.parse_args(["--workload", workload, "--reads", "1024", "--batches", "1", "--read-len", "1000", "--family-size", "1"])
    wl, idx, lay, batches, info = bench.build_workload(args, 0, 0, 1)
    if "r" in legs:
        t = measure(idx, f"(r) {workload} random-filled", base)
        print(f"(r) flagged bins: {flagged(t, lay['ixfs'])} of {t.nonzero.size}", flush=True)
    idx.close()
    if "e" in legs:
        t0 = time.time()
        idx_e, st = synth.exact_fill_index(lay, device=0, fill_frac=0.95)
        print(f"(e) exact-fill index built: {idx_e.data_bytes/1e9:.2f} GB, {st['keys_inserted']/1e9:.2f} G insertions, {time.time()-t0:.1f} s", flush=True)
        t = measure(idx_e, f"(e) {workload} exact_fill", base)
        print(f"(e) flagged bins: {flagged(t, lay['ixfs'])} of {t.nonzero.size}", flush=True)
        idx_e.close()
if "s" in legs:
    nc, cb, kpb = 512, 128, 20000
    shapes, ub, counts = synth.full_hierarchy_shapes(nc, cb, kpb, slack=1.1)
    idx_s = GpuIndex(shapes, ub)
    t0 = time.time()
    st, off = idx_s.build_hixf_synth(counts, salt=7, seed0=3)
    print(f"(s) synthetic index built: {idx_s.data_bytes/1e9:.2f} GB, {int(off[-1])/1e9:.2f} G keys, {time.time()-t0:.1f} s", flush=True)
    t = measure(idx_s, "(s) synthetic two-level", base)
    n = counts.astype(np.float64).copy()
    n[:nc] = cb * kpb                                  # a merged root bin holds its child's union: distinct synthetic keys
    est = t.keys_est().astype(np.float64)
    built = n > 0
    z = np.abs(est[built] - n[built]) / np.sqrt(n[built] / 255.0)
    over = int(np.count_nonzero(t.nonzero[built].astype(np.float64) > n[built]))
    print(f"(s) {int(built.sum())} built bins ({nc} merged of {cb*kpb} keys, {nc*cb} leaf of {kpb}): worst |keys_est - n| / sqrt(n / 255) = {z.max():.2f}, "
          f"mean {z.mean():.2f}, bins with nonzero > n: {over}, flagged: {flagged(t, shapes)} (the root's {shapes[0]['bins']-nc} unbuilt bins keep what the allocation held)", flush=True)
    idx_s.close()
