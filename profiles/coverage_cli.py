#!/usr/bin/env python3
"""`taxor search --coverage-file` against the plain search, wall time and search phase on one MI355X (DESIGN.md section 10,
"Distinct-hash coverage"; docs/EXPERIMENTS.md, "Distinct-hash coverage").

A class-scale synthetic `.hixf` (bench.py's family workload, built on the GPU and written to disk) and a FASTA of synthetic reads;
two commands over the same files, alternating, `runs` times each after one warm-up round:
  (a) taxor search -> TSV                       (TAXOR_COV_PARENT_BIN=<taxor of the parent commit> runs that binary)
  (b) taxor search -> TSV and --coverage-file   (this tree's)
Prints per command the median and the spread of the wall time and of the search phase, the accumulation's own figures from (b)'s
trace line (seconds inside the accumulation, seconds of its kernel, lookups, gathers per second) next to the random-row gather
ceiling of the same index measured in this process (taxor_gpu_gather_ceiling over the child IXFs), and whether the TSVs are equal.
usage: python profiles/coverage_cli.py [workload=refseq] [n_reads=2000000] [read_len=1000] [runs=3]"""
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
n_reads = int(sys.argv[2]) if len(sys.argv) > 2 else 2000000
read_len = int(sys.argv[3]) if len(sys.argv) > 3 else 1000
runs = int(sys.argv[4]) if len(sys.argv) > 4 else 3
TAXOR = os.path.join(ROOT, "taxor_amd", "taxor")
PARENT = os.environ.get("TAXOR_COV_PARENT_BIN", TAXOR)
per = max(131072, 131072 * 10000 // read_len)            # reads per generated batch: ~1.3 Gbp like bench.py's batches
args = bench.parse_args(["--workload", workload, "--reads", str(min(n_reads, per)), "--batches", "1", "--read-len", str(read_len), "--family-size", "1"])
wl, idx, lay, batches, info = bench.build_workload(args, 0, 0, 1)
need = idx.data_bytes * 1.05 + n_reads * (read_len + 900) * 2
base = next((d for d in (os.environ.get("TAXOR_E2E_TMP"), "/tmp", "/dev/shm") if d and os.path.isdir(d) and shutil.disk_usage(d).free > need), None)
if base is None:
    raise SystemExit(f"no scratch directory with {need/1e9:.0f} GB free")
tmp = tempfile.mkdtemp(prefix="taxor_cov_", dir=base)
t0 = time.time()
host = [dict(bins=f["bins"], stride=f["stride"], seg_len=f["seg_len"], seed=idx.ixf_seed(i), next_ixf=f["next_ixf"], fname_idx=f["fname_idx"], data=None)
        for i, f in enumerate(lay["ixfs"])]
species = [dict(organism_name=f"Organism {u}", accession_id=f"GCF_{u:09d}.1", taxid=str(1000 + u), taxnames_string=f"k__Bacteria;s__Organism {u}",
                taxid_string=f"2;{1000000 + u}", user_bin=u, seq_len=info["genome_len"]) for u in range(lay["n_user_bins"])]
idx_path = os.path.join(tmp, f"{workload}.hixf")
store_hixf(idx_path, host, lay["n_user_bins"], species, data_of=idx.download_ixf)
print(f"{workload}-class index written: {os.path.getsize(idx_path)/1e9:.2f} GB, {lay['n_user_bins']} user bins, {len(host)} IXFs, {time.time()-t0:.1f}s", flush=True)
# the ceiling the accumulation's gathers stand against: whole rows of the child IXFs at random row indices, nothing else
n_child = len(host) - 1
gbs, row_bytes, used = idx.gather_ceiling(ixf=1, want_bytes=8 << 30, reps=3, span=max(2, n_child))
print(f"gather ceiling over {used} child IXFs: {gbs:.0f} GB/s of {row_bytes}-B rows = {gbs / row_bytes:.2f} G rows/s", flush=True)
del host
fa = os.path.join(tmp, "reads.fa")
g, go = info.get("genomes"), info.get("genome_off")
done, b = 0, 0
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
        rec = np.empty((n, 1 + 14 + 1 + read_len + 1), dtype=np.uint8)
        rec[:, 0] = ord(">")
        rec[:, 1:6] = np.frombuffer(b"read_", np.uint8)
        rec[:, 6:15] = (np.arange(done, done + n, dtype=np.int64)[:, None] // 10 ** np.arange(8, -1, -1)) % 10 + 48
        rec[:, 15] = 10
        rec[:, 16:16 + read_len] = bb.reshape(n, read_len)
        rec[:, -1] = 10
        rec.tofile(f)
        done += n
        b += 1
idx.close()
print(f"fasta {os.path.getsize(fa)/1e9:.2f} GB ({n_reads} reads of {read_len})", flush=True)

# every command under a time limit of its own; one that runs into it ends the script
LIMIT = 90 + 45 * max(1.0, n_reads * max(read_len, 1000) / 1e9)


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
    m = re.search(r"search phase ([0-9.]+) s wall after the index was resident = ([0-9.]+) Mbp/s", cp.stderr)
    return dt, float(m.group(1)) if m else float("nan"), cp


search = ["search", "--index-file", idx_path, "--query-file", fa, "--threads", "16"]
tsv_a, tsv_b, cov = os.path.join(tmp, "a.tsv"), os.path.join(tmp, "b.tsv"), os.path.join(tmp, "cov.tsv")
wall = {"a": [], "b": []}
phase = {"a": [], "b": []}
line = ""
for rnd in range(runs + 1):                                 # round 0 warms the page cache and the driver; not counted
    ta, pa, _ = timed([PARENT] + search + ["--output-file", tsv_a])
    tb, pb, cpb = timed([TAXOR] + search + ["--output-file", tsv_b, "--coverage-file", cov])
    if rnd == 0:
        continue
    wall["a"].append(ta); wall["b"].append(tb); phase["a"].append(pa); phase["b"].append(pb)
    line = next((l for l in cpb.stderr.splitlines() if l.startswith("[trace] coverage:")), "")
    print(f"round {rnd}: (a) {ta:.2f} s wall, {pa:.3f} s search phase   (b) {tb:.2f} s wall, {pb:.3f} s search phase", flush=True)


def med(xs):
    return f"median {statistics.median(xs):.3f} s (min {min(xs):.3f}, max {max(xs):.3f}, {len(xs)} runs)"


gbp = n_reads * read_len / 1e9
print(f"{gbp:.2f} Gbp of {read_len}-base reads")
print(f"(a) plain search, wall        : {med(wall['a'])}")
print(f"(b) with --coverage-file, wall: {med(wall['b'])}   ratio of medians {statistics.median(wall['b']) / statistics.median(wall['a']):.3f}")
print(f"(a) plain search, search phase        : {med(phase['a'])}")
print(f"(b) with --coverage-file, search phase: {med(phase['b'])}   ratio of medians {statistics.median(phase['b']) / statistics.median(phase['a']):.3f}")
print("(b), last round:", line)
m = re.search(r"([0-9.]+) s in its kernel, (\d+) lookups", line)
if m:
    ks, lookups = float(m.group(1)), int(m.group(2))
    print(f"accumulation kernel: {ks / gbp * 1e3:.1f} ms per Gbp; {3 * lookups / ks / 1e9:.2f} G one-byte gathers/s against the ceiling's {gbs / row_bytes:.2f} G rows/s "
          f"= {3 * lookups / ks / 1e9 / (gbs / row_bytes):.2f} of it")
same = open(tsv_a, "rb").read() == open(tsv_b, "rb").read() if os.path.getsize(tsv_a) < (8 << 30) else None
print(f"TSV with the option identical to the plain search's: {same}; coverage file: {sum(1 for _ in open(cov)) - 1} references")
subprocess.run(["rm", "-rf", tmp])
sys.exit(0 if same is not False else 1)
