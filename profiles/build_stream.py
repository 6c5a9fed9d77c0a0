"""`taxor build` beyond device memory: on profiles/build_cli.py's input (300 genomes of 7 Mb, plain FASTA)
  * the unforced build of this tree against another binary (--other: the parent commit's `taxor`), alternating, after a warm-up:
    wall time and construction seconds, median and range -- the resident path must not have moved;
  * the build forced through the host store (--device-key-budget, default 256 MiB: the root in more than 8 bin ranges) against the
    resident one, alternating: the ratio of the construction phases, and the share of the key uploads hidden behind peeling.
Prints one JSON object.  Usage: python profiles/build_stream.py [--other path/to/taxor] [--runs 3] [--budget 256] [--dir /tmp/x]"""
import argparse
import json
import multiprocessing as mp
import os
import re
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from profiles.build_cli import fasta, genome  # noqa: E402

TAXOR = os.path.join(ROOT, "taxor_amd", "taxor")


def write_one(args):
    i, length, d = args
    with open(os.path.join(d, f"GCF_{i:09d}.1_SYN{i}_genomic.fna"), "wb") as f:
        f.write(fasta(genome(i, length)))


def build(exe, tsv, d, out, threads, *extra):
    t0 = time.time()
    cp = subprocess.run([exe, "build", "--input-file", tsv, "--input-sequence-dir", d, "--output-filename", out, "--use-syncmer", "--kmer-size", "22",
                         "--syncmer-size", "12", "--threads", str(threads), *extra], capture_output=True, text=True)
    wall = time.time() - t0
    if cp.returncode != 0:
        raise SystemExit(cp.stdout + cp.stderr)
    line = cp.stderr.strip().splitlines()[-1]
    r = dict(wall_s=wall, summary=line)
    for name in ("read+key", "layout", "construction", "store", "total"):
        r[name] = float(re.search(re.escape(name) + r" ([0-9.]+)", line).group(1))
    m = re.search(r"path (\w+): (\d+) waves, (\d+) groups, (\d+) bin ranges, (\d+) restarts, key uploads ([0-9.]+) s of which ([0-9.]+) s", line)
    if m:
        r.update(path=m.group(1), waves=int(m.group(2)), groups=int(m.group(3)), ranges=int(m.group(4)), restarts=int(m.group(5)),
                 upload_s=float(m.group(6)), upload_waited_s=float(m.group(7)))
    return r


def spread(runs, key):
    v = [r[key] for r in runs]
    return dict(median=statistics.median(v), min=min(v), max=max(v))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--genomes", type=int, default=300)
    ap.add_argument("--length", type=int, default=7_000_000)
    ap.add_argument("--dir", default=None)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--budget", type=int, default=256)
    ap.add_argument("--other", default=None)
    a = ap.parse_args()
    work = a.dir or tempfile.mkdtemp(prefix="taxor_build_stream_")
    d = os.path.join(work, "plain")
    os.makedirs(d, exist_ok=True)
    with mp.Pool(a.threads) as pool:
        pool.map(write_one, [(i, a.length, d) for i in range(a.genomes)])
    tsv = os.path.join(work, "tax.tsv")
    with open(tsv, "w") as f:
        for i in range(a.genomes):
            f.write(f"GCF_{i:09d}.1\t{i + 1}\tsyn/GCF_{i:09d}.1_SYN{i}\tSynthetic {i}\n")
    out = os.path.join(work, "x.hixf")
    res = dict(genomes=a.genomes, bases=a.genomes * a.length, runs=a.runs, budget_mib=a.budget)
    build(TAXOR, tsv, d, out, a.threads)                                   # warm-up: page cache, the driver
    if a.other:
        build(a.other, tsv, d, out, a.threads)
        this, other = [], []
        for _ in range(a.runs):
            other.append(build(a.other, tsv, d, out, a.threads))
            this.append(build(TAXOR, tsv, d, out, a.threads))
        res["unforced"] = dict(this={k: spread(this, k) for k in ("wall_s", "construction", "total")},
                               other={k: spread(other, k) for k in ("wall_s", "construction", "total")}, summary=this[-1]["summary"])
    resident, stream = [], []
    ref = os.path.join(work, "resident.hixf")
    build(TAXOR, tsv, d, ref, a.threads)
    build(TAXOR, tsv, d, out, a.threads, "--device-key-budget", str(a.budget))
    res["stream_file_identical"] = open(ref, "rb").read() == open(out, "rb").read()
    for _ in range(a.runs):
        resident.append(build(TAXOR, tsv, d, out, a.threads))
        stream.append(build(TAXOR, tsv, d, out, a.threads, "--device-key-budget", str(a.budget)))
    up, waited = statistics.median(r["upload_s"] for r in stream), statistics.median(r["upload_waited_s"] for r in stream)
    res["forced"] = dict(resident={k: spread(resident, k) for k in ("wall_s", "read+key", "layout", "construction", "total")},
                         stream={k: spread(stream, k) for k in ("wall_s", "read+key", "layout", "construction", "total")},
                         waves=stream[-1]["waves"], groups=stream[-1]["groups"], ranges=stream[-1]["ranges"], restarts=stream[-1]["restarts"],
                         construction_ratio_resident_over_stream=statistics.median(r["construction"] for r in resident) / statistics.median(r["construction"] for r in stream),
                         upload_s=up, upload_waited_s=waited, upload_share_hidden=(1 - waited / up) if up else None, summary=stream[-1]["summary"])
    print(json.dumps(res))


if __name__ == "__main__":
    main()
