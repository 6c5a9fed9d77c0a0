#!/usr/bin/env python3
"""`taxor search` on ONE set of 10-kb reads written three ways -- plain FASTQ, bgzip-style .fastq.gz, unaligned BAM -- against the
RefSeq-class synthetic index (bench.py's workload, written to disk as cli_e2e_class.py does).  Per format, medians of three runs:
the search phase's seconds per Gbp, the process CPU-seconds per Gbp (both from the CLI's own trace line), the bytes of sequence
that cross to the device per base, and the reader's own rate (`taxor reads --summary-only`: inflate + record walk or parse, no GPU).
Beside them the packing kernels' HIP-event time per Gbp on one batch of the same reads through the library (k_pack_dna4:
taxor_gpu_pack_dna4_timed, k_pack_nibbles: taxor_gpu_pack_nibbles).  Qualities are random over 40 values, so that neither
compressed file shrinks to nothing.  The comparison that matters is BAM against .fastq.gz: what a BAM user does today.
usage: python profiles/bam_cli.py [n_reads=1000000] [out.json]"""
import json
import os
import re
import shutil
import statistics
import struct
import subprocess
import sys
import tempfile
import zlib
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: F401,E402

import bench  # noqa: E402
from taxor_amd import Searcher, synth  # noqa: E402
from taxor_amd.hixf_file import store_hixf  # noqa: E402

n_reads = int(sys.argv[1]) if len(sys.argv) > 1 else 1000000
out_json = sys.argv[2] if len(sys.argv) > 2 else None
TAXOR = os.path.join(ROOT, "taxor_amd", "taxor")
THREADS = 16
EOF_BLOCK = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")


def bgzf_block(data):
    co = zlib.compressobj(1, zlib.DEFLATED, -15)
    c = co.compress(data) + co.flush()
    return (struct.pack("<BBBBIBBH", 0x1F, 0x8B, 8, 4, 0, 0, 0xFF, 6) + b"BC" + struct.pack("<HH", 2, 18 + len(c) + 8 - 1) + c +
            struct.pack("<II", zlib.crc32(data) & 0xFFFFFFFF, len(data)))


class BgzfWriter:
    """bytes in, 60000-byte blocks deflated on THREADS threads (zlib releases the GIL), the end-of-file block at close"""

    def __init__(self, path):
        self.f = open(path, "wb")
        self.ex = ThreadPoolExecutor(THREADS)

    def add(self, chunk):
        mv = memoryview(chunk)
        for blk in self.ex.map(bgzf_block, (bytes(mv[a:a + 60000]) for a in range(0, len(mv), 60000))):
            self.f.write(blk)

    def close(self):
        self.f.write(EOF_BLOCK)
        self.f.close()
        self.ex.shutdown()


args = bench.parse_args(["--workload", "refseq", "--reads", str(min(n_reads, 131072)), "--batches", "1"])
wl, idx, lay, batches, info = bench.build_workload(args, 0, 0, 1)
read_len = info["read_len"]
tmp = tempfile.mkdtemp(prefix="taxor_bam_", dir=os.environ.get("TAXOR_E2E_TMP", "/tmp"))
host = [dict(bins=f["bins"], stride=f["stride"], seg_len=f["seg_len"], seed=idx.ixf_seed(i), next_ixf=f["next_ixf"], fname_idx=f["fname_idx"], data=None)
        for i, f in enumerate(lay["ixfs"])]
species = [dict(organism_name=f"Organism {u}", accession_id=f"GCF_{u:09d}.1", taxid=str(1000 + u), taxnames_string=f"k__Bacteria;s__Organism {u}",
                taxid_string=f"2;{1000 + u}", user_bin=u, seq_len=info["genome_len"]) for u in range(lay["n_user_bins"])]
idx_path = os.path.join(tmp, "refseq.hixf")
store_hixf(idx_path, host, lay["n_user_bins"], species, data_of=idx.download_ixf)
print(f"index written: {os.path.getsize(idx_path) / 1e9:.2f} GB", flush=True)

# the reads, 16384 at a time: every record of a format has the same length (fixed-width ids), so a batch is one 2-D array
g, go = info["genomes"], info["genome_off"]
code = np.zeros(256, np.uint8)
for i, ch in enumerate(b"=ACMGRSVTWYHKDBN"):
    code[ch] = i
comp = np.array([((n & 1) << 3) | ((n & 2) << 1) | ((n & 4) >> 1) | ((n & 8) >> 3) for n in range(16)], np.uint8)


def batches_of_reads():
    done, b = 0, 0
    while done < n_reads:
        n = min(16384, n_reads - done)
        bb, _, _ = synth.synth_reads(g, go, n, read_len, error_rate=args.read_error, frac_random=0.1, seed=synth.DEFAULT_SEED + 1000 * b, threads=THREADS)
        yield done, bb.reshape(n, read_len)
        done += n
        b += 1


def ids_of(first, n):
    num = np.arange(first, first + n, dtype=np.int64)
    out = np.empty((n, 14), np.uint8)
    out[:, :5] = np.frombuffer(b"read_", np.uint8)
    out[:, 5:] = (num[:, None] // 10 ** np.arange(8, -1, -1)) % 10 + 48
    return out


def fastq_chunk(first, seq, qual):
    n = seq.shape[0]
    rec = np.empty((n, 1 + 14 + 1 + read_len + 3 + read_len + 1), np.uint8)
    rec[:, 0] = ord("@")
    rec[:, 1:15] = ids_of(first, n)
    rec[:, 15] = 10
    rec[:, 16:16 + read_len] = seq
    rec[:, 16 + read_len:19 + read_len] = np.frombuffer(b"\n+\n", np.uint8)
    rec[:, 19 + read_len:19 + 2 * read_len] = qual + 33
    rec[:, -1] = 10
    return rec.tobytes()


def bam_chunk(first, seq, qual):
    """unaligned records (flag 4); every third stored reverse-complemented (flag 0x10 | 4), as an aligner's output would hold them"""
    n = seq.shape[0]
    c = code[seq]
    rev = (np.arange(first, first + n) % 3) == 1
    c[rev] = comp[c[rev][:, ::-1]]
    nb = (read_len + 1) // 2
    if read_len & 1:
        c = np.concatenate([c, np.zeros((n, 1), np.uint8)], axis=1)
    body = 32 + 15 + nb + read_len
    rec = np.zeros((n, 4 + body), np.uint8)
    fixed = struct.pack("<IiiBBHHHiiii", body, -1, -1, 15, 0, 4680, 0, 4, read_len, -1, -1, 0)
    rec[:, :36] = np.frombuffer(fixed, np.uint8)
    rec[rev, 18] = 0x14
    rec[:, 36:50] = ids_of(first, n)
    rec[:, 51:51 + nb] = (c[:, 0::2] << 4) | c[:, 1::2]
    rec[:, 51 + nb:] = qual          # (QUAL is stored in the read's stored direction; its values do not matter here)
    return rec.tobytes()


fq, gz, bam = (os.path.join(tmp, x) for x in ("reads.fastq", "reads.fastq.gz", "reads.bam"))
qrng = np.random.default_rng(7)
first_batch = None
wz, wb = BgzfWriter(gz), BgzfWriter(bam)
wb.add(b"BAM\1" + struct.pack("<i", 0) + struct.pack("<i", 0))
with open(fq, "wb") as f:
    for first, seq in batches_of_reads():
        qual = qrng.integers(32, 72, seq.shape, dtype=np.uint8)      # (phred 32..71: no quality line begins with @ or +)
        if first_batch is None:
            first_batch = seq.copy()
        text = fastq_chunk(first, seq, qual)
        f.write(text)
        wz.add(text)
        wb.add(bam_chunk(first, seq, qual))
wz.close()
wb.close()

# the packing kernels by themselves, HIP events, on the first batch of these reads: ASCII through k_pack_dna4, the same reads as
# 4-bit codes (every third reversed, as in the file) through k_pack_nibbles; five calls each, medians
nb0 = first_batch.shape[0]
offs0 = np.arange(nb0 + 1, dtype=np.uint64) * np.uint64(read_len)
c0 = code[first_batch]
rev0 = (np.arange(nb0) % 3) == 1
c0[rev0] = comp[c0[rev0][:, ::-1]]
if read_len & 1:
    c0 = np.concatenate([c0, np.zeros((nb0, 1), np.uint8)], axis=1)
seq4 = np.ascontiguousarray((c0[:, 0::2] << 4) | c0[:, 1::2]).reshape(-1)
boff0 = np.arange(nb0, dtype=np.uint64) * np.uint64((read_len + 1) // 2)
sr = Searcher(idx, error_rate=args.error_rate)
ms_dna4 = statistics.median(sr.upload_timed(first_batch.reshape(-1), offs0) for _ in range(5))
ms_nib = statistics.median(sr.pack_nibbles([(seq4, boff0, np.full(nb0, read_len, np.uint32), rev0.astype(np.uint8))], timed=True)[2] for _ in range(5))
sr.close()
idx.close()
gbp0 = nb0 * read_len / 1e9
print(f"packing kernels on {nb0} reads: k_pack_dna4 {ms_dna4:.3f} ms = {ms_dna4 / gbp0:.2f} ms per Gbp, k_pack_nibbles {ms_nib:.3f} ms = {ms_nib / gbp0:.2f} ms per Gbp", flush=True)
gbp = n_reads * read_len / 1e9
print(f"{n_reads} reads of {read_len} = {gbp:.2f} Gbp: fastq {os.path.getsize(fq) / 1e9:.2f} GB, fastq.gz {os.path.getsize(gz) / 1e9:.2f} GB, "
      f"bam {os.path.getsize(bam) / 1e9:.2f} GB", flush=True)

PHASE = re.compile(r"search phase: ([0-9.]+) s wall, ([0-9.]+) s user \+ ([0-9.]+) s system")
env = dict(os.environ, TAXOR_TUNING="1", TAXOR_CLI_TRACE="1", TAXOR_CLI_CLEAN_EXIT="1")
result = dict(n_reads=n_reads, read_len=read_len, gbp=gbp, index_gb=os.path.getsize(idx_path) / 1e9, formats={},
              pack_kernel_ms_per_gbp=dict(k_pack_dna4=ms_dna4 / gbp0, k_pack_nibbles=ms_nib / gbp0, reads=nb0))
tsv = {}
for name, q, h2d in (("fastq", fq, 1.0), ("fastq.gz", gz, 1.0), ("bam", bam, ((read_len + 1) // 2) / read_len)):
    runs = []
    out = os.path.join(tmp, name + ".tsv")
    for rep in range(3):
        cp = subprocess.run([TAXOR, "search", "--index-file", idx_path, "--query-file", q, "--output-file", out, "--threads", str(THREADS)],
                            capture_output=True, text=True, env=env, timeout=1200)
        m = PHASE.search(cp.stderr)
        if cp.returncode != 0 or not m:
            raise SystemExit(f"{name}: rc {cp.returncode}\n{cp.stderr[-3000:]}")
        runs.append(dict(search_s_per_gbp=float(m.group(1)) / gbp, cpu_s_per_gbp=(float(m.group(2)) + float(m.group(3))) / gbp))
        print(name, rep, runs[-1], flush=True)
    tsv[name] = open(out, "rb").read()
    # the reader by itself: inflate and record walk (or parse) on the same threads, nothing printed, no GPU
    cp = subprocess.run([TAXOR, "reads", "--query-file", q, "--threads", str(THREADS), "--summary-only"], capture_output=True, text=True, timeout=1200)
    m = re.search(r"batches, ([0-9.]+) s", cp.stderr)
    if cp.returncode != 0 or not m:
        raise SystemExit(f"{name}: reads rc {cp.returncode}\n{cp.stderr[-2000:]}")
    reader_s = float(m.group(1))
    result["formats"][name] = dict(runs=runs, search_s_per_gbp=statistics.median(r["search_s_per_gbp"] for r in runs),
                                   cpu_s_per_gbp=statistics.median(r["cpu_s_per_gbp"] for r in runs), h2d_sequence_bytes_per_base=h2d,
                                   reader_s_per_gbp=reader_s / gbp, file_gb=os.path.getsize(q) / 1e9)
result["tsv_identical"] = tsv["fastq"] == tsv["fastq.gz"] == tsv["bam"]
result["bam_over_fastq_gz"] = result["formats"]["bam"]["search_s_per_gbp"] / result["formats"]["fastq.gz"]["search_s_per_gbp"]
line = json.dumps(result)
print(line)
if out_json:
    os.makedirs(os.path.dirname(os.path.abspath(out_json)), exist_ok=True)
    with open(out_json, "w") as f:
        f.write(line + "\n")
shutil.rmtree(tmp, ignore_errors=True)
