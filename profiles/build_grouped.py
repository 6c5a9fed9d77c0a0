"""`taxor build --group-similar` against the build without the switch, on one family workload ("Similarity-aware
layout"): writes families of related genomes (default 256 families of 8, 100 kb each) in an order that interleaves the families,
builds the index both ways, searches the same reads against both, and times the pairs kernel alone on one full window.  Reports
  * wall time of both builds and the phases of their summary lines (sketches, pairs and clustering against the whole build),
  * index bytes, IXFs, depth and the root's seg_len of both,
  * search phase time per Gbp and tuples reported for both,
  * the pairs kernel's time at W = 4096, m = 1024.
Prints one JSON object.  Usage: python profiles/build_grouped.py [--families 256] [--family-size 8] [--length 100000] [--reads 20000]
[--dir /tmp/x] [--threads 16] [--tmax 0]"""
import argparse
import json
import os
import re
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from taxor_amd import synth  # noqa: E402
from taxor_amd.genome_keys import keys_sketch, sketch_pairs  # noqa: E402
from taxor_amd.hixf_file import HixfFile  # noqa: E402

TAXOR = os.path.join(ROOT, "taxor_amd", "taxor")


def build(tsv, d, out, threads, extra):
    t0 = time.time()
    cp = subprocess.run([TAXOR, "build", "--input-file", tsv, "--input-sequence-dir", d, "--output-filename", out, "--use-syncmer",
                         "--kmer-size", "22", "--syncmer-size", "12", "--threads", str(threads)] + extra, capture_output=True, text=True)
    wall = time.time() - t0
    if cp.returncode != 0:
        return dict(wall_s=wall, error=(cp.stdout + cp.stderr).strip().splitlines()[-1])
    line = cp.stderr.strip().splitlines()[-1]
    hf = HixfFile(out)
    root = hf.ixfs[0]
    res = dict(wall_s=wall, summary=line, file_bytes=os.path.getsize(out), ixfs=len(hf.ixfs), root_bins=int(root["bins"]),
               root_seg_len=int(root["seg_len"]), fingerprint_bytes=int(sum(3 * f["seg_len"] * f["stride"] for f in hf.ixfs)))
    hf.close()
    return res


def search(index, reads, out, threads, gbp):
    cp = subprocess.run([TAXOR, "search", "--index-file", index, "--query-file", reads, "--output-file", out, "--threads", str(threads)],
                        capture_output=True, text=True, env=dict(os.environ, TAXOR_TUNING="1", TAXOR_CLI_TRACE="1"))   # (the trace prints the search phase line)
    if cp.returncode != 0:
        raise SystemExit(cp.stdout + cp.stderr)
    m = re.search(r"search phase ([0-9.]+) s wall after the index was resident", cp.stderr)
    with open(out) as f:
        tuples = sum(1 for _ in f) - 1
    return dict(search_phase_s=float(m.group(1)) if m else None, search_phase_s_per_gbp=float(m.group(1)) / gbp if m else None, tuples=tuples)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--families", type=int, default=256)
    ap.add_argument("--family-size", type=int, default=8)
    ap.add_argument("--length", type=int, default=100_000)
    ap.add_argument("--reads", type=int, default=20000)
    ap.add_argument("--dir", default=None)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--tmax", type=int, default=0, help="force one t_max (0: the build chooses)")
    a = ap.parse_args()
    work = a.dir or tempfile.mkdtemp(prefix="taxor_grouped_profile_")
    d = os.path.join(work, "genomes")
    os.makedirs(d, exist_ok=True)
    n = a.families * a.family_size
    g, go, _ = synth.family_genomes(a.families, a.family_size, a.length)
    tsv = os.path.join(work, "tax.tsv")
    with open(tsv, "w") as f:
        for i in range(n):                                   # file i: member i // families of family i % families
            src = (i % a.families) * a.family_size + i // a.families
            seq = bytes(g[int(go[src]):int(go[src + 1])])
            with open(os.path.join(d, f"GCF_{i:09d}.1_SYN{i}_genomic.fna"), "wb") as out:
                out.write(b">chromosome\n" + seq + b"\n")
            f.write(f"GCF_{i:09d}.1\t{i + 1}\tsyn/GCF_{i:09d}.1_SYN{i}\tSynthetic {i}\n")
    bases, offs, _ = synth.synth_reads(g, go, a.reads, 5000, error_rate=0.04, frac_random=0.1, seed=9)
    fa = os.path.join(work, "reads.fa")
    with open(fa, "wb") as f:
        for i in range(a.reads):
            f.write(b">read_%d\n" % i + bytes(bases[int(offs[i]):int(offs[i + 1])]) + b"\n")
    gbp = float(offs[-1]) / 1e9
    res = dict(genomes=n, families=a.families, bases=n * a.length, reads=a.reads, read_gbp=gbp)
    for name, extra in (("plain", []), ("grouped", ["--group-similar"])):
        idx = os.path.join(work, name + ".hixf")
        res["build_" + name] = build(tsv, d, idx, a.threads, extra + (["--tmax", str(a.tmax)] if a.tmax else []))
        if "error" not in res["build_" + name]:
            res["search_" + name] = search(idx, fa, os.path.join(work, name + ".tsv"), a.threads, gbp)
    # the pairs kernel on one full window: 4096 bins of 5000 random keys, m = 1024 (truncated sketches, the expensive case)
    rng = np.random.default_rng(1)
    W, m, per = 4096, 1024, 5000
    keys = rng.integers(0, 2**64, W * per, dtype=np.uint64)
    off = (np.arange(W + 1) * per).astype(np.uint64)
    t0 = time.time()
    sk, ln = keys_sketch(keys, off, m)
    t_sketch = time.time() - t0
    times = [sketch_pairs(sk, ln, np.diff(off), want_ms=True)[2] for _ in range(3)]
    res["pairs_kernel"] = dict(window=W, sketch_size=m, pairs=W * W, kernel_ms=times, sketch_call_s=t_sketch)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
