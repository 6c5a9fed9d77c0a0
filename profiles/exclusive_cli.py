#!/usr/bin/env python3
"""`taxor search --exclusive-file` / `--exclusive-reads-file` against the plain search and against `--breakpoint-file`, wall time and
search phase on one MI355X (docs/EXPERIMENTS.md, "Exclusive hashes").

The workload of profiles/breakpoint_cli.py: a class-scale synthetic `.hixf` (bench.py's family workload, built on the GPU and written to
disk) and a FASTA of synthetic reads.  Four commands over the same files in turn, `runs` times each after one warm-up round:
  (p) taxor search -> TSV, the binary TAXOR_EXCLUSIVE_PARENT_BIN names (the parent commit's; this tree's if unset)
  (a) taxor search -> TSV, this tree's: the options off
  (b) taxor search -> TSV and --breakpoint-file, the binary of (p): the parent's figures on the same reads
  (x) taxor search -> TSV, --exclusive-file and --exclusive-reads-file
Prints per command the median and the spread of the wall time and of the search phase, the trace lines of (b) and (x) from the last
round, both options' kernel time per Gbp and per million lookups, lookups per read, lines written, the option's share of the search
phase, and whether the four TSVs are equal.  chimera_every and percentage as in profiles/breakpoint_cli.py.
usage: python profiles/exclusive_cli.py [workload=refseq] [n_reads=150000] [read_len=10000] [runs=5] [chimera_every=0] [percentage=]"""
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
chimera_every = int(sys.argv[5]) if len(sys.argv) > 5 else 0
percentage = sys.argv[6] if len(sys.argv) > 6 else ""
TAXOR = os.path.join(ROOT, "taxor_amd", "taxor")
PARENT = os.environ.get("TAXOR_EXCLUSIVE_PARENT_BIN", TAXOR)
per = max(131072, 131072 * 10000 // read_len)            # reads per generated batch: ~1.3 Gbp like bench.py's batches
args = bench.parse_args(["--workload", workload, "--reads", str(min(n_reads, per)), "--batches", "1", "--read-len", str(read_len), "--family-size", "1"])
wl, idx, lay, batches, info = bench.build_workload(args, 0, 0, 1)
need = idx.data_bytes * 1.05 + n_reads * (read_len + 900) * 4
base = next((d for d in (os.environ.get("TAXOR_E2E_TMP"), "/tmp", "/dev/shm") if d and os.path.isdir(d) and shutil.disk_usage(d).free > need), None)
if base is None:
    raise SystemExit(f"no scratch directory with {need/1e9:.0f} GB free")
tmp = tempfile.mkdtemp(prefix="taxor_ex_", dir=base)
t0 = time.time()
host = [dict(bins=f["bins"], stride=f["stride"], seg_len=f["seg_len"], seed=idx.ixf_seed(i), next_ixf=f["next_ixf"], fname_idx=f["fname_idx"], data=None)
        for i, f in enumerate(lay["ixfs"])]
species = [dict(organism_name=f"Organism {u}", accession_id=f"GCF_{u:09d}.1", taxid=str(1000 + u), taxnames_string=f"k__Bacteria;s__Organism {u}",
                taxid_string=f"2;{1000000 + u}", user_bin=u, seq_len=info["genome_len"]) for u in range(lay["n_user_bins"])]
idx_path = os.path.join(tmp, f"{workload}.hixf")
store_hixf(idx_path, host, lay["n_user_bins"], species, data_of=idx.download_ixf)
print(f"{workload}-class index written: {os.path.getsize(idx_path)/1e9:.2f} GB, {lay['n_user_bins']} user bins, {len(host)} IXFs, {time.time()-t0:.1f}s", flush=True)
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


search = ["search", "--index-file", idx_path, "--query-file", fa, "--threads", "16"] + (["--percentage", percentage] if percentage else [])
tsv = {k: os.path.join(tmp, k + ".tsv") for k in "pabx"}
bp, ex, exr = os.path.join(tmp, "bp.tsv"), os.path.join(tmp, "ex.tsv"), os.path.join(tmp, "exr.tsv")
cmds = {"p": [PARENT] + search + ["--output-file", tsv["p"]], "a": [TAXOR] + search + ["--output-file", tsv["a"]],
        "b": [PARENT] + search + ["--output-file", tsv["b"], "--breakpoint-file", bp],
        "x": [TAXOR] + search + ["--output-file", tsv["x"], "--exclusive-file", ex, "--exclusive-reads-file", exr]}
names = {"p": "(p) plain search, parent's binary", "a": "(a) plain search, this tree (options off)", "b": "(b) with --breakpoint-file, parent's binary",
         "x": "(x) with --exclusive-file and -reads-file"}
wall = {k: [] for k in cmds}
phase = {k: [] for k in cmds}
trace = {}
inside = {"breakpoint": [], "exclusive": []}                   # per round: seconds inside _add_batch, seconds in the kernels
for rnd in range(runs + 1):                                 # round 0 warms the page cache and the driver; not counted
    row = []
    for k, cmd in cmds.items():
        dt, ph, cp = timed(cmd)
        if rnd:
            wall[k].append(dt)
            phase[k].append(ph)
        row.append(f"({k}) {dt:.2f} s wall, {ph:.3f} s search phase")
        for tag in ("breakpoint", "exclusive"):
            line = next((l for l in cp.stderr.splitlines() if l.startswith(f"[trace] {tag}:")), None)
            if line:
                trace[tag] = line
                m = re.search(r"([0-9.]+) s inside the \w+ \(summed over workers\), ([0-9.]+) s in its kernels", line)
                if m and rnd:
                    inside[tag].append((float(m.group(1)), float(m.group(2))))
    if rnd:
        print(f"round {rnd}: " + "   ".join(row), flush=True)


def med(xs, unit="s"):
    return f"median {statistics.median(xs):.3f} {unit} (min {min(xs):.3f}, max {max(xs):.3f}, {len(xs)} runs)"


gbp = n_reads * read_len / 1e9
print(f"{gbp:.2f} Gbp of {read_len}-base reads")
for k in cmds:
    print(f"{names[k]:42s} wall        : {med(wall[k])}")
for k in cmds:
    print(f"{names[k]:42s} search phase: {med(phase[k])}   / (p) {statistics.median(phase[k]) / statistics.median(phase['p']):.3f}")
spread = max(phase["p"]) - min(phase["p"])
diff = statistics.median(phase["a"]) - statistics.median(phase["p"])
print(f"option off: (a) - (p) = {diff * 1e3:+.1f} ms of search phase; (p)'s own spread (max - min) is {spread * 1e3:.1f} ms: {'within' if abs(diff) <= spread else 'OUTSIDE'} it")
print("(b), last round:", trace.get("breakpoint", ""))
print("(x), last round:", trace.get("exclusive", ""))
lookups, kernels = {}, {}
for tag, k in (("breakpoint", "b"), ("exclusive", "x")):
    m = re.search(r"(\d+) lookups", trace.get(tag, ""))
    if not m or not inside[tag]:
        continue
    lookups[tag] = int(m.group(1))
    kernels[tag] = statistics.median([x[1] for x in inside[tag]])
    print(f"({k}) inside _add_batch: {med([x[0] * 1e3 for x in inside[tag]], 'ms')}")
    print(f"({k}) kernels (HIP events): {med([x[1] * 1e3 for x in inside[tag]], 'ms')} = {kernels[tag] / gbp * 1e3:.2f} ms per Gbp; "
          f"{lookups[tag]} lookups = {lookups[tag] / n_reads:.1f} per read" + (f", {kernels[tag] / lookups[tag] * 1e12:.1f} ps per lookup" if lookups[tag] else ""))
m = re.search(r"(\d+) lines from (\d+) examined reads of (\d+)", trace.get("breakpoint", ""))
if m:
    print(f"(b) {m.group(1)} lines written, {m.group(2)} of {m.group(3)} reads examined (two candidates or more)")
m = re.search(r"(\d+) user bins and (\d+) read lines from (\d+) examined reads of (\d+)", trace.get("exclusive", ""))
if m:
    print(f"(x) {m.group(1)} user bins and {m.group(2)} read lines written, {m.group(3)} of {m.group(4)} reads examined (one candidate or more)")
cost = statistics.median(phase["x"]) - statistics.median(phase["a"])
print(f"the options' cost: (x) - (a) = {cost * 1e3:+.1f} ms of search phase = {100 * cost / statistics.median(phase['x']):.1f} % of (x)'s; "
      f"(b) - (p) = {(statistics.median(phase['b']) - statistics.median(phase['p'])) * 1e3:+.1f} ms")
print(f"search phase per Gbp: " + ", ".join(f"({k}) {statistics.median(phase[k]) / gbp * 1e3:.1f} ms" for k in cmds))
same = all(open(tsv["p"], "rb").read() == open(tsv[k], "rb").read() for k in "abx") if os.path.getsize(tsv["p"]) < (8 << 30) else None
print(f"the four TSVs are identical: {same}; breakpoint file: {sum(1 for _ in open(bp)) - 1} lines; exclusive file: {sum(1 for _ in open(ex)) - 1} lines; "
      f"exclusive reads file: {sum(1 for _ in open(exr)) - 1} lines, {os.path.getsize(exr)/1e6:.2f} MB")
subprocess.run(["rm", "-rf", tmp])
sys.exit(0 if same is not False else 1)
