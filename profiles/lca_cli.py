#!/usr/bin/env python3
"""`taxor search --lca-file --report-file` against the plain search on one MI355X (docs/EXPERIMENTS.md,
"Per-read LCA and report").

A class-scale synthetic `.hixf` (bench.py's family workload, built on the GPU and written to disk; every user bin carries a
five-rank path: genera of 8, families of 64, phyla of 512 user bins) and a FASTA of synthetic reads; three commands over the same files,
in turn, `runs` times each after one warm-up round:
  (a) taxor search --output-file                           the parent commit's behaviour
  (b) taxor search --lca-file --report-file                no TSV: the tuples never leave the device
  (c) taxor search --output-file --lca-file --report-file  all three
Prints per command the median and the spread of the search phase's wall time and of the process's CPU seconds in it (the
`[trace] search phase` line: the accounting of profiles/cli_e2e_class.py), and from the `[trace] lca` line of (b) and (c) the seconds
inside the accumulation and in its kernel, set against the same run's GPU batches (the `search ... s (summed over workers)` figure:
host time from a batch's hand-over to its end on two workers -- an upper bound of the search kernels' time) and the search phase.
usage: python profiles/lca_cli.py [workload=refseq] [n_reads=150000] [read_len=10000] [runs=5]"""
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
TAXOR = os.path.join(ROOT, "taxor_amd", "taxor")
per = max(131072, 131072 * 10000 // read_len)            # reads per generated batch: ~1.3 Gbp like bench.py's batches
args = bench.parse_args(["--workload", workload, "--reads", str(min(n_reads, per)), "--batches", "1", "--read-len", str(read_len), "--family-size", "1"])
wl, idx, lay, batches, info = bench.build_workload(args, 0, 0, 1)
need = idx.data_bytes * 1.05 + n_reads * (read_len + 900) * 2
base = next((d for d in (os.environ.get("TAXOR_E2E_TMP"), "/tmp", "/dev/shm") if d and os.path.isdir(d) and shutil.disk_usage(d).free > need), None)
if base is None:
    raise SystemExit(f"no scratch directory with {need/1e9:.0f} GB free")
tmp = tempfile.mkdtemp(prefix="taxor_lca_", dir=base)
t0 = time.time()
host = [dict(bins=f["bins"], stride=f["stride"], seg_len=f["seg_len"], seed=idx.ixf_seed(i), next_ixf=f["next_ixf"], fname_idx=f["fname_idx"], data=None)
        for i, f in enumerate(lay["ixfs"])]
species = [dict(organism_name=f"Organism {u}", accession_id=f"GCF_{u:09d}.1", taxid=str(1000000 + u),
                taxnames_string=f"k__Bacteria;p__Phylum {u // 512};f__Family {u // 64};g__Genus {u // 8};s__Organism {u}",
                taxid_string=f"2;{4000000 + u // 512};{3000000 + u // 64};{2000000 + u // 8};{1000000 + u}", user_bin=u, seq_len=info["genome_len"])
           for u in range(lay["n_user_bins"])]
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
        rec[:, -1] = 10
        rec.tofile(f)
        done += n
        b += 1
idx.close()
print(f"fasta {os.path.getsize(fa)/1e9:.2f} GB ({n_reads} reads of {read_len})", flush=True)

# every command under a time limit of its own; one that runs into it ends the script
LIMIT = 90 + 45 * max(1.0, n_reads * max(read_len, 1000) / 1e9)


def timed(cmd):
    try:
        cp = subprocess.run(cmd, capture_output=True, text=True, env=dict(os.environ, TAXOR_TUNING="1", TAXOR_CLI_TRACE="1"), timeout=LIMIT)
    except subprocess.TimeoutExpired:
        subprocess.run(["rm", "-rf", tmp])
        raise SystemExit(f"{' '.join(cmd[:3])} did not end within {LIMIT:.0f} s; nothing further is started")
    if cp.returncode != 0:
        subprocess.run(["rm", "-rf", tmp])
        raise SystemExit(f"{' '.join(cmd[:3])} failed ({cp.returncode}): {cp.stderr[-1500:]}")
    m = re.search(r"\[trace\] search phase: ([0-9.]+) s wall, ([0-9.]+) s user \+ ([0-9.]+) s system CPU", cp.stderr)
    w = re.search(r"search ([0-9.]+) s, gather", cp.stderr)
    k = re.search(r"\[trace\] lca: .*?; ([0-9.]+) s inside the accumulation \(summed over workers\), ([0-9.]+) s in its kernel", cp.stderr)
    return dict(wall=float(m.group(1)), cpu=float(m.group(2)) + float(m.group(3)), batches=float(w.group(1)) if w else float("nan"),
                add=float(k.group(1)) if k else None, kernel=float(k.group(2)) if k else None,
                line=next((l for l in cp.stderr.splitlines() if l.startswith("[trace] lca:")), ""))


search = [TAXOR, "search", "--index-file", idx_path, "--query-file", fa, "--threads", "16"]
P = lambda n: os.path.join(tmp, n)
cmds = {"a": search + ["--output-file", P("a.tsv")],
        "b": search + ["--lca-file", P("b.calls"), "--report-file", P("b.report")],
        "c": search + ["--output-file", P("c.tsv"), "--lca-file", P("c.calls"), "--report-file", P("c.report")]}
names = {"a": "--output-file alone (the parent's behaviour)", "b": "--lca-file --report-file, no TSV", "c": "all three"}
res = {k: [] for k in cmds}
for rnd in range(runs + 1):                                 # round 0 warms the page cache and the driver; not counted
    for k, cmd in cmds.items():
        r = timed(cmd)
        if rnd:
            res[k].append(r)
    if rnd:
        print(f"round {rnd}: " + "   ".join(f"({k}) {res[k][-1]['wall']:.3f} s wall, {res[k][-1]['cpu']:.2f} CPU-s" for k in cmds), flush=True)


def med(xs):
    return f"median {statistics.median(xs):.3f} (min {min(xs):.3f}, max {max(xs):.3f}, {len(xs)} runs)"


gbp = n_reads * read_len / 1e9
print(f"{gbp:.2f} Gbp of {read_len}-base reads")
for k in cmds:
    print(f"({k}) {names[k]}\n      search phase, wall s   : {med([r['wall'] for r in res[k]])}\n      search phase, CPU s    : {med([r['cpu'] for r in res[k]])}")
for k in ("b", "c"):
    ks, ad, bt, wl_ = (statistics.median([r[f] for r in res[k]]) for f in ("kernel", "add", "batches", "wall"))
    print(f"({k}) lca kernel {ks * 1e3:.3f} ms (min {min(r['kernel'] for r in res[k]) * 1e3:.3f}, max {max(r['kernel'] for r in res[k]) * 1e3:.3f}) = {ks / gbp * 1e3:.3f} ms per Gbp; "
          f"{ad * 1e3:.1f} ms inside the accumulation; the run's GPU batches {bt:.3f} s summed over workers: kernel share {100 * ks / bt:.2f} %, "
          f"{100 * ks / wl_:.2f} % of the search phase's wall")
    print(f"({k}), last round: {res[k][-1]['line']}")
wa = statistics.median([r["wall"] for r in res["a"]])
ca = statistics.median([r["cpu"] for r in res["a"]])
for k in ("b", "c"):
    print(f"({k}) : (a)  search phase wall {statistics.median([r['wall'] for r in res[k]]) / wa:.3f}, CPU seconds {statistics.median([r['cpu'] for r in res[k]]) / ca:.3f}")
same_tsv = open(P("a.tsv"), "rb").read() == open(P("c.tsv"), "rb").read() if os.path.getsize(P("a.tsv")) < (8 << 30) else None
same_calls = open(P("b.calls"), "rb").read() == open(P("c.calls"), "rb").read() and open(P("b.report"), "rb").read() == open(P("c.report"), "rb").read()
print(f"TSV of (c) identical to (a)'s: {same_tsv}; calls and report of (b) identical to (c)'s: {same_calls}; report lines: {sum(1 for _ in open(P('b.report')))}")
print("report, first lines:\n" + "".join(open(P("b.report")).readlines()[:8]), end="")
subprocess.run(["rm", "-rf", tmp])
sys.exit(0 if same_tsv is not False and same_calls else 1)
