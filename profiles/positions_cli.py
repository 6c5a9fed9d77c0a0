#!/usr/bin/env python3
"""`taxor search --breakpoint-file` with and without `--base-positions`: search phase and the position kernel's own seconds on one
MI355X (docs/EXPERIMENTS.md, "Hash positions").

The 10-kb chimera workload of profiles/breakpoint_cli.py: a class-scale synthetic `.hixf` (bench.py's family workload, built on the GPU
and written to disk) and a FASTA of synthetic reads, every chimera_every-th read's second half replaced by the second half of the read
after it.  Two commands over the same files in turn, `runs` times each after one warm-up round, both this tree's binary:
  (b) taxor search -> TSV and --breakpoint-file                      the baseline: no launch, copy or allocation of the feature
  (q) taxor search -> TSV and --breakpoint-file --base-positions
Prints per command the median and the spread of the wall time and of the search phase, their ratio, the seconds between the event pairs
around k_hash_positions ([trace] positions), per Gbp and per million hashes, and whether the TSVs and the files' leading columns agree.
usage: python profiles/positions_cli.py [workload=refseq] [n_reads=150000] [read_len=10000] [runs=5] [chimera_every=10] [percentage=0.3]"""
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
n_reads = int(sys.argv[2]) if len(sys.argv) > 2 else 150000
read_len = int(sys.argv[3]) if len(sys.argv) > 3 else 10000
runs = int(sys.argv[4]) if len(sys.argv) > 4 else 5
chimera_every = int(sys.argv[5]) if len(sys.argv) > 5 else 10
percentage = sys.argv[6] if len(sys.argv) > 6 else "0.3"
TAXOR = os.path.join(ROOT, "taxor_amd", "taxor")
per = max(131072, 131072 * 10000 // read_len)            # reads per generated batch: ~1.3 Gbp like bench.py's batches
args = bench.parse_args(["--workload", workload, "--reads", str(min(n_reads, per)), "--batches", "1", "--read-len", str(read_len), "--family-size", "1"])
wl, idx, lay, batches, info = bench.build_workload(args, 0, 0, 1)
need = idx.data_bytes * 1.05 + n_reads * (read_len + 900) * 4
base = next((d for d in (os.environ.get("TAXOR_E2E_TMP"), "/tmp", "/dev/shm") if d and os.path.isdir(d) and shutil.disk_usage(d).free > need), None)
if base is None:
    raise SystemExit(f"no scratch directory with {need/1e9:.0f} GB free")
tmp = tempfile.mkdtemp(prefix="taxor_pos_", dir=base)
host = [dict(bins=f["bins"], stride=f["stride"], seg_len=f["seg_len"], seed=idx.ixf_seed(i), next_ixf=f["next_ixf"], fname_idx=f["fname_idx"], data=None)
        for i, f in enumerate(lay["ixfs"])]
species = [dict(organism_name=f"Organism {u}", accession_id=f"GCF_{u:09d}.1", taxid=str(1000 + u), taxnames_string=f"k__Bacteria;s__Organism {u}",
                taxid_string=f"2;{1000000 + u}", user_bin=u, seq_len=info["genome_len"]) for u in range(lay["n_user_bins"])]
idx_path = os.path.join(tmp, f"{workload}.hixf")
store_hixf(idx_path, host, lay["n_user_bins"], species, data_of=idx.download_ixf)
print(f"{workload}-class index written: {os.path.getsize(idx_path)/1e9:.2f} GB, {lay['n_user_bins']} user bins, {len(host)} IXFs", flush=True)
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
        if chimera_every > 0:                               # the second half of the read behind it: another genome, as a rule
            at = np.arange(0, n - 1, chimera_every)
            rec[at, 16 + read_len // 2:16 + read_len] = rec[at + 1, 16 + read_len // 2:16 + read_len]
        rec[:, -1] = 10
        rec.tofile(f)
        done += n
        b += 1
idx.close()
print(f"fasta {os.path.getsize(fa)/1e9:.2f} GB ({n_reads} reads of {read_len}; chimera_every {chimera_every}, percentage {percentage or '-'})", flush=True)

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


search = [TAXOR, "search", "--index-file", idx_path, "--query-file", fa, "--threads", "16"] + (["--percentage", percentage] if percentage else [])
tsv = {k: os.path.join(tmp, k + ".tsv") for k in "bq"}
bp = {k: os.path.join(tmp, "bp_" + k + ".tsv") for k in "bq"}
cmds = {"b": search + ["--output-file", tsv["b"], "--breakpoint-file", bp["b"]],
        "q": search + ["--output-file", tsv["q"], "--breakpoint-file", bp["q"], "--base-positions"]}
names = {"b": "(b) --breakpoint-file", "q": "(q) --breakpoint-file --base-positions"}
wall = {k: [] for k in cmds}
phase = {k: [] for k in cmds}
kernel, hashes, trace = [], 0, ""
for rnd in range(runs + 1):                                 # round 0 warms the page cache and the driver; not counted
    row = []
    for k, cmd in cmds.items():
        dt, ph, cp = timed(cmd)
        if rnd:
            wall[k].append(dt)
            phase[k].append(ph)
        row.append(f"({k}) {dt:.2f} s wall, {ph:.3f} s search phase")
        m = re.search(r"\[trace\] positions: (\d+) hashes placed, ([0-9.]+) s in k_hash_positions", cp.stderr)
        if m:
            trace = m.group(0)
            hashes = int(m.group(1))
            if rnd:
                kernel.append(float(m.group(2)))
    if rnd:
        print(f"round {rnd}: " + "   ".join(row), flush=True)


def med(xs, unit="s"):
    return f"median {statistics.median(xs):.3f} {unit} (min {min(xs):.3f}, max {max(xs):.3f}, {len(xs)} runs)"


gbp = n_reads * read_len / 1e9
print(f"{gbp:.2f} Gbp of {read_len}-base reads")
for k in cmds:
    print(f"{names[k]:42s} wall        : {med(wall[k])}")
for k in cmds:
    print(f"{names[k]:42s} search phase: {med(phase[k])}   / (b) {statistics.median(phase[k]) / statistics.median(phase['b']):.3f}")
print("(q), last round:", trace)
if kernel:
    km = statistics.median(kernel)
    print(f"(q) k_hash_positions (HIP event pairs): {med([x * 1e3 for x in kernel], 'ms')} = {km / gbp * 1e3:.2f} ms per Gbp, "
          f"{km / max(hashes, 1) * 1e9:.2f} ns per hash placed ({hashes} hashes, {hashes / n_reads:.0f} per read), "
          f"{km / statistics.median(phase['b']):.3f} of (b)'s search phase")
old = open(bp["b"]).read().splitlines()
new = open(bp["q"]).read().splitlines()
lead = len(old) == len(new) and all(n_.rsplit("\t", 2)[0] == o for o, n_ in zip(old, new))
same = open(tsv["b"], "rb").read() == open(tsv["q"], "rb").read()
print(f"the two TSVs are identical: {same}; breakpoint file: {len(old) - 1} lines, leading columns identical: {lead}")
subprocess.run(["rm", "-rf", tmp])
sys.exit(0 if same and lead else 1)
