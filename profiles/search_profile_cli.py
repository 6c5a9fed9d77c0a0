#!/usr/bin/env python3
"""Search to profile in one run against the two-step route, wall time on one MI355X.

A class-scale synthetic `.hixf` (bench.py's family workload, built on the GPU and written to disk) and a FASTA of synthetic reads;
three routes over the same files, alternating, `runs` times each after one warm-up round:
  (a) taxor search -> TSV, then taxor profile on it       (the route before the one-run mode; TAXOR_SP_PARENT_BIN=<taxor of the
                                                           parent commit> runs that binary instead of this tree's)
  (b) taxor search with the profile options AND --output-file
  (c) taxor search with the profile options, no TSV
Prints per route the median and the spread of the wall time, the stage seconds each command reports, the search-phase rate of (c)
next to the library's sustained host-fed rate on the same reads, and whether the three routes wrote the same three files.
usage: python profiles/search_profile_cli.py [workload=refseq] [n_reads=12000000] [read_len=1000] [runs=3]"""
import os
import re
import shutil
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: F401,E402

import bench  # noqa: E402
from taxor_amd import synth  # noqa: E402
from taxor_amd.hixf_file import store_hixf  # noqa: E402

workload = sys.argv[1] if len(sys.argv) > 1 else "refseq"
n_reads = int(sys.argv[2]) if len(sys.argv) > 2 else 12000000
read_len = int(sys.argv[3]) if len(sys.argv) > 3 else 1000
runs = int(sys.argv[4]) if len(sys.argv) > 4 else 3
TAXOR = os.path.join(ROOT, "taxor_amd", "taxor")
PARENT = os.environ.get("TAXOR_SP_PARENT_BIN", TAXOR)
per = max(131072, 131072 * 10000 // read_len)            # reads per generated batch: ~1.3 Gbp like bench.py's batches
# unrelated genomes (--family-size 1): four strains of bench.py's default families share nearly all their reads, explain one another
# and end in the explained-by cycle that `taxor profile` refuses -- on either route
FAMILY = ["--family-size", os.environ.get("TAXOR_SP_FAMILY", "1")]
args = bench.parse_args(["--workload", workload, "--reads", str(min(n_reads, per)), "--batches", "1", "--read-len", str(read_len)] + FAMILY)
wl, idx, lay, batches, info = bench.build_workload(args, 0, 0, 1)
need = idx.data_bytes * 1.05 + n_reads * (read_len + 900) * 2
base = next((d for d in (os.environ.get("TAXOR_E2E_TMP"), "/tmp", "/dev/shm") if d and os.path.isdir(d) and shutil.disk_usage(d).free > need), None)
if base is None:
    raise SystemExit(f"no scratch directory with {need/1e9:.0f} GB free")
tmp = tempfile.mkdtemp(prefix="taxor_sp_", dir=base)
t0 = time.time()
host = [dict(bins=f["bins"], stride=f["stride"], seg_len=f["seg_len"], seed=idx.ixf_seed(i), next_ixf=f["next_ixf"], fname_idx=f["fname_idx"], data=None)
        for i, f in enumerate(lay["ixfs"])]
species = [dict(organism_name=f"Organism {u}", accession_id=f"GCF_{u:09d}.1", taxid=str(1000 + u),
                taxnames_string=f"k__Bacteria;p__P{u % 7};c__C{u % 31};o__O{u % 101};f__F{u % 401};g__G{u // 4};s__Organism {u}",
                taxid_string=f"2;{10 + u % 7};{100 + u % 31};{200 + u % 101};{400 + u % 401};{100000 + u // 4};{1000000 + u}", user_bin=u,
                seq_len=info["genome_len"]) for u in range(lay["n_user_bins"])]
idx_path = os.path.join(tmp, f"{workload}.hixf")
store_hixf(idx_path, host, lay["n_user_bins"], species, data_of=idx.download_ixf)
del host
print(f"{workload}-class index written: {os.path.getsize(idx_path)/1e9:.2f} GB, {time.time()-t0:.1f}s", flush=True)
fa = os.path.join(tmp, "reads.fa")
g, go = info.get("genomes"), info.get("genome_off")
kept, done, b = [], 0, 0
t0 = time.time()
with open(fa, "wb") as f:
    while done < n_reads:
        n = min(per, n_reads - done)
        if b == 0:
            bb, oo = batches[0]
            if oo.size - 1 > n:
                bb, oo = bb[: int(oo[n])], oo[: n + 1]
            n = oo.size - 1
        else:
            bb, oo, _ = synth.synth_reads(g, go, n, read_len, error_rate=args.read_error, frac_random=0.1, seed=synth.DEFAULT_SEED + 1000 * b, threads=info["ncpu"])
        if len(kept) < 8:
            kept.append((np.ascontiguousarray(bb), np.ascontiguousarray(oo)))
        # ids whose byte-wise order is not the input order, with a description: ">read_<9 digits, scrambled> ch=1\n"
        rec = np.empty((n, 1 + 14 + 6 + read_len + 1), dtype=np.uint8)
        rec[:, 0] = ord(">")
        rec[:, 1:6] = np.frombuffer(b"read_", np.uint8)
        num = (np.arange(done, done + n, dtype=np.int64) * 7919) % 10**9          # 7919 and 10^9 are coprime: a bijection below 10^9 reads
        rec[:, 6:15] = (num[:, None] // 10 ** np.arange(8, -1, -1)) % 10 + 48
        rec[:, 15:20] = np.frombuffer(b" ch=1", np.uint8)
        rec[:, 20] = 10
        rec[:, 21:21 + read_len] = bb.reshape(n, read_len)
        rec[:, -1] = 10
        rec.tofile(f)
        done += n
        b += 1
sargs = bench.parse_args(["--workload", workload, "--sustained-reads", str(max(n_reads, 4 * per)), "--read-len", str(read_len)] + FAMILY)
_, sustained = bench.dropin_measurements(sargs, idx, kept[:8], read_len)
print(f"library sustained (host-fed, two searchers, {sustained['reads']} reads): {sustained['value']:.0f} Mbp/s", flush=True)
del kept
idx.close()
print(f"fasta {os.path.getsize(fa)/1e9:.2f} GB ({n_reads} reads of {read_len}) written in {time.time()-t0:.1f}s", flush=True)


def prof_args(d):
    os.makedirs(d, exist_ok=True)
    return ["--cami-report-file", os.path.join(d, "cami"), "--seq-abundance-file", os.path.join(d, "seq"), "--binning-file", os.path.join(d, "bin"),
            "--sample-id", "S"]


# every command under a time limit of its own: 60 s for start-up and the index, 45 s per million reads (the TSV route parses a
# million reads in about 1.1 s), the 10-kb set in proportion.  A command that runs into it ends the script.
LIMIT = 60 + 45 * max(1.0, n_reads * max(read_len, 1000) / 1e9)


def timed(cmd):
    t = time.time()
    try:
        cp = subprocess.run(cmd, capture_output=True, text=True, env=dict(os.environ, TAXOR_TUNING="1", TAXOR_CLI_TRACE="1"), timeout=LIMIT)
    except subprocess.TimeoutExpired:
        subprocess.run(["rm", "-rf", tmp])
        raise SystemExit(f"{' '.join(cmd[:3])} did not end within {LIMIT:.0f} s; nothing further is started")
    dt = time.time() - t
    if cp.returncode != 0:
        subprocess.run(["rm", "-rf", tmp])
        raise SystemExit(f"{' '.join(cmd[:3])} failed ({cp.returncode}): {cp.stderr[-1500:]}")
    return dt, cp


def search_rate(cp):
    m = re.search(r"search phase ([0-9.]+) s wall after the index was resident = ([0-9.]+) Mbp/s", cp.stderr)
    return (float(m.group(1)), float(m.group(2))) if m else (float("nan"), float("nan"))


def stage_line(cp, word):
    return next((l for l in cp.stderr.splitlines() if l.startswith(word)), "")


search = ["search", "--index-file", idx_path, "--query-file", fa, "--threads", "16"]
tsv = os.path.join(tmp, "out.tsv")
routes = {"a": [], "b": [], "c": []}
detail = {}
for rnd in range(runs + 1):                                 # round 0 warms the page cache and the driver; not counted
    ta, cpa = timed([PARENT] + search + ["--output-file", tsv])
    tp, cpp = timed([PARENT, "profile", "--search-file", tsv] + prof_args(os.path.join(tmp, "a")))
    tb, cpb = timed([TAXOR] + search + ["--output-file", os.path.join(tmp, "b.tsv")] + prof_args(os.path.join(tmp, "b")))
    tc, cpc = timed([TAXOR] + search + prof_args(os.path.join(tmp, "c")))
    if rnd == 0:
        continue
    routes["a"].append((ta + tp, ta, tp))
    routes["b"].append((tb,))
    routes["c"].append((tc,))
    detail = dict(a_search=search_rate(cpa), a_profile=stage_line(cpp, "taxor profile:"), b=search_rate(cpb), b_stage=stage_line(cpb, "taxor search (profile):"),
                  c=search_rate(cpc), c_stage=stage_line(cpc, "taxor search (profile):"))
    print(f"round {rnd}: (a) search {ta:.2f} + profile {tp:.2f} = {ta + tp:.2f} s   (b) {tb:.2f} s   (c) {tc:.2f} s", flush=True)


def med(xs):
    return f"median {statistics.median(xs):.2f} s (min {min(xs):.2f}, max {max(xs):.2f}, {len(xs)} runs)"


print(f"(a) search -> TSV -> profile : {med([x[0] for x in routes['a']])}; its search step alone {med([x[1] for x in routes['a']])}, its profile step {med([x[2] for x in routes['a']])}")
print(f"(b) one run with --output-file: {med([x[0] for x in routes['b']])}")
print(f"(c) one run, no TSV           : {med([x[0] for x in routes['c']])}")
print(f"search phase, last round: (a) {detail['a_search'][1]:.0f} Mbp/s in {detail['a_search'][0]:.2f} s, (b) {detail['b'][1]:.0f} Mbp/s, (c) {detail['c'][1]:.0f} Mbp/s in "
      f"{detail['c'][0]:.2f} s = {detail['c'][1] / sustained['value']:.3f} x library sustained ({sustained['value']:.0f} Mbp/s)")
print("stages (a):", detail["a_profile"])
print("stages (b):", detail["b_stage"])
print("stages (c):", detail["c_stage"])
same = all(open(os.path.join(tmp, r, k), "rb").read() == open(os.path.join(tmp, "a", k), "rb").read() for r in ("b", "c") for k in ("cami", "seq", "bin"))
same_tsv = open(tsv, "rb").read() == open(os.path.join(tmp, "b.tsv"), "rb").read() if os.path.getsize(tsv) < (8 << 30) else None
print(f"the three routes wrote identical profile files: {same}; (b)'s TSV identical to the plain search's: {same_tsv}")
subprocess.run(["rm", "-rf", tmp])
sys.exit(0 if same and same_tsv is not False else 1)
