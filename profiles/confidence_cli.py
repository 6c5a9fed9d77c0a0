#!/usr/bin/env python3
"""`taxor search --lca-file --lca-confidence` against `--lca-file` alone on one MI355X (docs/EXPERIMENTS.md,
"LCA confidence").

The workload of profiles/lca_cli.py: a class-scale synthetic `.hixf` (bench.py's family workload, built on the GPU and written to disk;
every user bin carries a five-rank path) and a FASTA of synthetic reads; three commands over the same files, in turn, `runs` times each
after one warm-up round:
  (a) taxor search --lca-file                          the parent commit's behaviour
  (b) taxor search --lca-file --lca-confidence 0.1     capture on, the saved lists' round trip, the probe
  (h) taxor search --lca-file --hitmap-file            the sibling option that pays the same round trip
Prints per command the median and the spread of the search phase's wall time, and from the `[trace] confidence` line of (b) the seconds
inside taxor_gpu_confidence_add_batch (the round trip of the saved lists through host memory is in there, the kernels are a part of
it), the kernels' HIP-event time per Gbp, the lookups per read and the share of (64 hashes, tuple) steps the probe did not make.
usage: python profiles/confidence_cli.py [workload=refseq] [n_reads=150000] [read_len=10000] [runs=5] [confidence=0.1]"""
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
conf = sys.argv[5] if len(sys.argv) > 5 else "0.1"
TAXOR = os.path.join(ROOT, "taxor_amd", "taxor")
per = max(131072, 131072 * 10000 // read_len)            # reads per generated batch: ~1.3 Gbp like bench.py's batches
args = bench.parse_args(["--workload", workload, "--reads", str(min(n_reads, per)), "--batches", "1", "--read-len", str(read_len), "--family-size", "1"])
wl, idx, lay, batches, info = bench.build_workload(args, 0, 0, 1)
need = idx.data_bytes * 1.05 + n_reads * (read_len + 900) * 2
base = next((d for d in (os.environ.get("TAXOR_E2E_TMP"), "/tmp", "/dev/shm") if d and os.path.isdir(d) and shutil.disk_usage(d).free > need), None)
if base is None:
    raise SystemExit(f"no scratch directory with {need/1e9:.0f} GB free")
tmp = tempfile.mkdtemp(prefix="taxor_conf_", dir=base)
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
    m = re.search(r"\[trace\] search phase: ([0-9.]+) s wall", cp.stderr)
    k = re.search(r"\[trace\] confidence: .*?; ([0-9.]+) s inside the weighing \(summed over workers\), ([0-9.]+) s in its kernels, (\d+) \(hash, leaf bin\) lookups, (\d+) of (\d+)", cp.stderr)
    hm = re.search(r"\[trace\] hitmap: .*?; ([0-9.]+) s inside the locating \(summed over workers\), ([0-9.]+) s in its kernels", cp.stderr)
    return dict(wall=float(m.group(1)), add=float(k.group(1)) if k else None, kernel=float(k.group(2)) if k else None, lookups=int(k.group(3)) if k else None,
                steps=int(k.group(4)) if k else None, steps_full=int(k.group(5)) if k else None, hm_add=float(hm.group(1)) if hm else None,
                hm_kernel=float(hm.group(2)) if hm else None, line=next((l for l in cp.stderr.splitlines() if l.startswith("[trace] confidence:")), ""))


search = [TAXOR, "search", "--index-file", idx_path, "--query-file", fa, "--threads", "16"]
P = lambda n: os.path.join(tmp, n)
cmds = {"a": search + ["--lca-file", P("a.calls")],
        "b": search + ["--lca-file", P("b.calls"), "--lca-confidence", conf],
        "h": search + ["--lca-file", P("h.calls"), "--hitmap-file", P("h.hm")]}
names = {"a": "--lca-file alone (the parent's behaviour)", "b": f"--lca-file --lca-confidence {conf}", "h": "--lca-file --hitmap-file"}
res = {k: [] for k in cmds}
for rnd in range(runs + 1):                                 # round 0 warms the page cache and the driver; not counted
    for k, cmd in cmds.items():
        r = timed(cmd)
        if rnd:
            res[k].append(r)
    if rnd:
        print(f"round {rnd}: " + "   ".join(f"({k}) {res[k][-1]['wall']:.3f} s" for k in cmds), flush=True)


def med(xs):
    return f"median {statistics.median(xs):.3f} (min {min(xs):.3f}, max {max(xs):.3f}, {len(xs)} runs)"


gbp = n_reads * read_len / 1e9
print(f"{gbp:.2f} Gbp of {read_len}-base reads")
for k in cmds:
    print(f"({k}) {names[k]}\n      search phase, wall s   : {med([r['wall'] for r in res[k]])}")
wa = statistics.median([r["wall"] for r in res["a"]])
for k in ("b", "h"):
    print(f"({k}) : (a)  search phase wall {statistics.median([r['wall'] for r in res[k]]) / wa:.3f}")
ks, ad = (statistics.median([r[f] for r in res["b"]]) for f in ("kernel", "add"))
last = res["b"][-1]
print(f"(b) kernels {ks * 1e3:.3f} ms = {ks / gbp * 1e3:.3f} ms per Gbp; {ad * 1e3:.1f} ms inside _add_batch summed over workers = {ad / gbp * 1e3:.1f} ms per Gbp "
      f"(the saved lists' round trip through host memory and the probe; the kernels are {100 * ks / ad:.1f} % of it)")
print(f"(b) {last['lookups'] / n_reads:.1f} lookups per read; {last['steps']} of {last['steps_full']} (64 hashes, tuple) steps made: "
      f"{100 * (1 - last['steps'] / max(1, last['steps_full'])):.1f} % saved by the exit at D and by skipping tuples no lane needs")
print(f"(h) hit map: {statistics.median([r['hm_add'] for r in res['h']]) * 1e3:.1f} ms inside _add_batch, {statistics.median([r['hm_kernel'] for r in res['h']]) * 1e3:.3f} ms in its kernels")
print(f"(b), last round: {last['line']}")
u = lambda p: sum(1 for l in open(p) if l.startswith("U\t"))
print(f"unclassified reads: (a) {u(P('a.calls'))}, (b) {u(P('b.calls'))}; calls of (h) identical to (a)'s: {open(P('a.calls'), 'rb').read() == open(P('h.calls'), 'rb').read()}")
subprocess.run(["rm", "-rf", tmp])
