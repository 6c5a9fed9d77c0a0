"""`taxor build` rates (DESIGN.md "taxor build"): writes synthetic genomes (default 2.1 Gbp: 300 genomes of 7 Mb) as plain FASTA and
as .gz, then reports
  * the device keyer alone on genomes resident in host memory: HIP-event time of packing + selection + set insertion (Gbp/s), and
    its _finish (gather, segmented sort),
  * `taxor build` end to end on both file sets: wall time and the phases of its summary line, and the keyer's share of the wall.
Prints one JSON object.  Usage: python profiles/build_cli.py [--genomes 300] [--length 7000000] [--dir /tmp/x] [--threads 16]"""
import argparse
import gzip
import json
import multiprocessing as mp
import os
import re
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from taxor_amd.genome_keys import GenomeKeyer  # noqa: E402

TAXOR = os.path.join(ROOT, "taxor_amd", "taxor")


def genome(i, length):
    rng = np.random.default_rng(1000 + i)
    return np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, length, dtype=np.uint8)].tobytes()


def fasta(seq):
    return b">chromosome\n" + b"\n".join(seq[p:p + 80] for p in range(0, len(seq), 80)) + b"\n"


def write_one(args):
    i, length, d_plain, d_gz = args
    text = fasta(genome(i, length))
    stem = f"GCF_{i:09d}.1_SYN{i}_genomic.fna"
    with open(os.path.join(d_plain, stem), "wb") as f:
        f.write(text)
    with gzip.open(os.path.join(d_gz, stem + ".gz"), "wb", compresslevel=1) as f:
        f.write(text)
    return len(text)


def build(tsv, d, out, threads):
    t0 = time.time()
    cp = subprocess.run([TAXOR, "build", "--input-file", tsv, "--input-sequence-dir", d, "--output-filename", out, "--use-syncmer",
                         "--kmer-size", "22", "--syncmer-size", "12", "--threads", str(threads)], capture_output=True, text=True)
    wall = time.time() - t0
    if cp.returncode != 0:
        raise SystemExit(cp.stdout + cp.stderr)
    line = cp.stderr.strip().splitlines()[-1]
    nums = dict((k, float(v)) for v, k in re.findall(r"([0-9.]+) \(?(genomes|bases|distinct keys|IXFs|index bytes)", line))
    sec = dict((k.strip(), float(v)) for k, v in re.findall(r"([a-z+ ]+?) ([0-9.]+)[,)]", line.split("seconds:")[1]))
    return dict(wall_s=wall, summary=line, seconds=sec, **{k.replace(" ", "_"): v for k, v in nums.items()})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--genomes", type=int, default=300)
    ap.add_argument("--length", type=int, default=7_000_000)
    ap.add_argument("--dir", default=None)
    ap.add_argument("--threads", type=int, default=16)
    a = ap.parse_args()
    work = a.dir or tempfile.mkdtemp(prefix="taxor_build_profile_")
    d_plain, d_gz = os.path.join(work, "plain"), os.path.join(work, "gz")
    os.makedirs(d_plain, exist_ok=True)
    os.makedirs(d_gz, exist_ok=True)
    t0 = time.time()
    with mp.Pool(a.threads) as pool:
        pool.map(write_one, [(i, a.length, d_plain, d_gz) for i in range(a.genomes)])
    t_write = time.time() - t0
    tsv = os.path.join(work, "tax.tsv")
    with open(tsv, "w") as f:
        for i in range(a.genomes):
            f.write(f"GCF_{i:09d}.1\t{i + 1}\tsyn/GCF_{i:09d}.1_SYN{i}\tSynthetic {i}\n")
    res = dict(genomes=a.genomes, bases=a.genomes * a.length, write_s=t_write)
    # the keyer alone, genomes resident in host memory, calls of ~256 Mbp
    kr = GenomeKeyer(a.genomes, k=22, s=12, t=5)
    per = max(1, (256 << 20) // a.length)
    t0 = time.time()
    for i0 in range(0, a.genomes, per):
        ids = list(range(i0, min(a.genomes, i0 + per)))
        seqs = [genome(i, a.length) for i in ids]
        kr.add(b"".join(seqs), np.cumsum([0] + [len(x) for x in seqs]).astype(np.uint64), ids)
    off, keys = kr.finish()
    st = kr.stats()
    kr.close()
    res["keyer"] = dict(device_s=st["seconds_device"], device_gbp_s=st["bases"] / st["seconds_device"] / 1e9, add_s=st["seconds_add"],
                        finish_s=st["seconds_finish"], keys=int(st["keys"]), tiles=int(st["tiles"]), wall_s=time.time() - t0,
                        bases_per_key=st["bases"] / max(1, st["keys"]))
    for kind, d in (("plain", d_plain), ("gz", d_gz)):
        r = build(tsv, d, os.path.join(work, f"{kind}.hixf"), a.threads)
        r["keyer_device_share_of_wall"] = st["seconds_device"] / r["wall_s"]
        res["build_" + kind] = r
    print(json.dumps(res))


if __name__ == "__main__":
    main()
