"""`taxor build --device-key-budget`: 48 synthetic genomes of 20-60 kb built once with every key resident and once in waves through the
host store with the root in bin ranges -- the two .hixf files are byte-identical and `taxor search` answers the same over both; a
genome whose keys may exceed the budget is refused by its file's name."""
import os
import re
import subprocess

import numpy as np
import pytest

from taxor_amd import synth

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TAXOR = os.path.join(ROOT, "taxor_amd", "taxor")
N = 48


def write_inputs(tmp_path):
    g, go = synth.random_genomes(N, 60000, seed=21)
    rng = np.random.default_rng(22)
    lens = rng.integers(20000, 60001, size=N)
    genomes = [bytes(g[int(go[i]):int(go[i]) + int(lens[i])]) for i in range(N)]
    big, _ = synth.random_genomes(1, 700000, seed=23)
    d = tmp_path / "g"
    d.mkdir()
    lines = []
    for i, seq in enumerate(genomes + [bytes(big)]):
        acc = f"GCF_{200000 + i:09d}.1"
        stem = f"{acc}_ASM{i}v1_genomic"
        recs = [seq] if i % 3 else [seq[:len(seq) // 2], seq[len(seq) // 2:]]
        (d / (stem + ".fna")).write_bytes(b"".join(b">r%d\n" % j + b"".join(r[p:p + 80] + b"\n" for p in range(0, len(r), 80)) for j, r in enumerate(recs)))
        lines.append("\t".join([acc, str(7000 + i), f"ftp://host/genomes/{acc}/{stem}", f"Organism {i}", f"k__B;s__Organism {i}", f"2;{7000 + i}"]))
    tsv, tsv_big = tmp_path / "tax.tsv", tmp_path / "tax_big.tsv"
    tsv.write_text("\n".join(lines[:N]) + "\n")
    tsv_big.write_text("\n".join(lines) + "\n")
    bases, offs, _ = synth.synth_reads(np.frombuffer(b"".join(genomes), np.uint8), np.cumsum([0] + [len(x) for x in genomes]).astype(np.uint64), 200, 1500,
                                       error_rate=0.0, frac_random=0.1, seed=9)
    fa = tmp_path / "reads.fa"
    fa.write_bytes(b"".join(b">read_%d\n" % i + bytes(bases[int(offs[i]):int(offs[i + 1])]) + b"\n" for i in range(200)))
    return tsv, tsv_big, d, fa, str(d / f"GCF_{200000 + N:09d}.1_ASM{N}v1_genomic.fna")


def build(tsv, d, out, *extra):
    return subprocess.run([TAXOR, "build", "--input-file", str(tsv), "--input-sequence-dir", str(d), "--output-filename", str(out), "--threads", "4", *extra],
                          capture_output=True, text=True, timeout=600)


def path_line(cp):
    m = re.search(r"path (\w+): (\d+) waves, (\d+) groups, (\d+) bin ranges, (\d+) restarts", cp.stderr)
    assert cp.returncode == 0 and m, cp.stdout + cp.stderr
    return (m.group(1),) + tuple(int(x) for x in m.groups()[1:])


def search(index, fa, out):
    cp = subprocess.run([TAXOR, "search", "--index-file", str(index), "--query-file", str(fa), "--output-file", str(out), "--threads", "4"],
                        capture_output=True, text=True, timeout=300)
    assert cp.returncode == 0, cp.stderr
    return out.read_bytes()


@pytest.mark.parametrize("extra,budget,min_waves,min_groups", [
    (["--use-syncmer", "--kmer-size", "22", "--syncmer-size", "12"], 1, 3, 1),
    (["--scaling", "10"], 1, 3, 1),                                              # minimisers, FracMinHash down-sampling
    (["--use-syncmer", "--kmer-size", "22", "--syncmer-size", "12", "--tmax", "16"], 2, 2, 2),   # a merged level: children in groups
], ids=["syncmer-k22-s12", "minimiser-scaling10", "syncmer-tmax16"])
def test_stream_build_is_byte_identical(tmp_path, extra, budget, min_waves, min_groups):
    tsv, tsv_big, d, fa, big_path = write_inputs(tmp_path)
    a, b = tmp_path / "resident.hixf", tmp_path / "stream.hixf"
    assert path_line(build(tsv, d, a, *extra))[:2] == ("resident", 1)
    cp = build(tsv, d, b, *extra, "--device-key-budget", str(budget))
    kind, waves, groups, ranges, _ = path_line(cp)
    assert cp.stdout == "checking input ... done!\nparsing taxonomy input files ... done!\ncreating HIXF layout ... done!\nbuilding HIXF index ... done!\n"
    assert cp.stderr.startswith(f"taxor build: {N} genomes")
    assert kind == "stream" and waves >= min_waves and ranges >= 2 and groups >= min_groups - 1, cp.stderr
    assert a.read_bytes() == b.read_bytes()
    ta, tb = search(a, fa, tmp_path / "a.tsv"), search(b, fa, tmp_path / "b.tsv")
    assert ta == tb and ta.count(b"\n") > 200
    # one genome of 700 kb: up to 140 001 syncmer keys (700 001 minimisers), more than 1 MiB holds
    cp = build(tsv_big, d, tmp_path / "big.hixf", *extra, "--device-key-budget", "1")
    assert cp.returncode == 255 and cp.stderr.startswith(f"[TAXOR BUILD ERROR] the distinct keys of {big_path} alone"), cp.stderr
    assert not (tmp_path / "big.hixf").exists()
