"""`taxor build` end to end on the device: 150 synthetic genomes (one 20x the others, so it is split) as GCF_..._genomic.fna and
.fna.gz over two --input-sequence-dirs, some multi-record and multi-line, built with a forced t_max of 64 (a merged level), then
checked against the oracle's keys: metadata, tree, geometry, every key in its leaf run and in every merged bin above it, `taxor
search` output byte-identical to the oracle-derived text, and a byte-identical rebuild."""
import gzip
import os
import subprocess

import numpy as np
import pytest

from oracle import oracle as orc
from taxor_amd import synth
from taxor_amd.hixf_file import HixfFile
from tests.test_hixf_file_cpu import HEADER, expected_lines

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TAXOR = os.path.join(ROOT, "taxor_amd", "taxor")
N = 150


def write_inputs(tmp_path):
    g, go = synth.random_genomes(N - 1, 6000, seed=11)
    big, _ = synth.random_genomes(1, 120000, seed=12)
    genomes = [bytes(big)] + [bytes(g[int(go[i]):int(go[i + 1])]) for i in range(N - 1)]
    dirs = [tmp_path / "d1", tmp_path / "d2"]
    for d in dirs:
        d.mkdir()
    lines, paths, records = [], [], []
    for i, seq in enumerate(genomes):
        acc = f"GCF_{100000 + i:09d}.1"
        stem = f"{acc}_ASM{i}v1_genomic"
        recs = [seq] if i % 3 else [seq[:len(seq) // 3], seq[len(seq) // 3:2 * len(seq) // 3], seq[2 * len(seq) // 3:]]
        width = (60, 80, 1 << 20)[i % 3]
        text = b"".join(b">r%d some description\n" % j + b"".join(r[p:p + width] + b"\n" for p in range(0, len(r), width)) for j, r in enumerate(recs))
        d = dirs[i % 2]
        if i % 4 == 1:
            path = d / (stem + ".fna.gz")
            with gzip.open(path, "wb") as f:
                f.write(text)
        else:
            path = d / (stem + ".fna")
            path.write_bytes(text)
        paths.append(str(path))
        records.append(recs)
        lines.append("\t".join([acc, str(5000 + i), f"ftp://host/genomes/{acc}/{stem}", f"Organism {i}", f"k__B;s__Organism {i}", f"2;{5000 + i}"]))
    (tmp_path / "d2" / "notes.txt").write_text("not a genome\n")
    tsv = tmp_path / "tax.tsv"
    tsv.write_text("\n".join(lines) + "\n")
    return tsv, dirs, paths, records


def build(tsv, dirs, out, *extra):
    cp = subprocess.run([TAXOR, "build", "--input-file", str(tsv), "--input-sequence-dir", ",".join(map(str, dirs)), "--output-filename", str(out),
                         "--threads", "4", *extra], capture_output=True, text=True, timeout=600)
    assert cp.returncode == 0, cp.stdout + cp.stderr
    assert cp.stdout == "checking input ... done!\nparsing taxonomy input files ... done!\ncreating HIXF layout ... done!\nbuilding HIXF index ... done!\n"
    assert cp.stderr.startswith("taxor build: 150 genomes"), cp.stderr
    return cp


def oracle_sets(records, k, s, t, scaling, w=None):
    out = []
    for recs in records:
        parts = [orc.minimiser_hash(r, k, w) if w else orc.seq_to_syncmers(r, k, s, t) for r in recs]
        u = np.unique(np.concatenate(parts))
        if scaling > 1:
            lim = float(2**64 - 1) / scaling
            u = u[np.array([float(orc.wyhash(int(x))) <= lim for x in u], dtype=bool)]
        out.append(u)
    return out


def check_index(hf, sets, paths, records, k, s, t, use_syncmer, w, scaling):
    assert (hf.k, hf.use_syncmer, hf.window_size, hf.scaling) == (k, use_syncmer, w, scaling)
    if use_syncmer:
        assert (hf.s, hf.t) == (s, t)
    assert [x["accession_id"] for x in hf.species] == [f"GCF_{100000 + i:09d}.1" for i in range(N)]
    assert [x["user_bin"] for x in hf.species] == list(range(N))
    assert [x["seq_len"] for x in hf.species] == [sum(len(r) for r in recs) for recs in records]
    assert [x["organism_name"] for x in hf.species] == [f"Organism {i}" for i in range(N)]
    assert hf.filenames == paths
    ixfs = hf.ixfs
    h = orc.Hixf(ixfs, [f["next_ixf"] for f in ixfs], [f["fname_idx"] for f in ixfs])
    parent = {}
    for i, f in enumerate(ixfs):
        for b in range(f["bins"]):
            if f["fname_idx"][b] < 0:
                parent[int(f["next_ixf"][b])] = (i, b)
    below = {}

    def under(i):
        if i not in below:
            f = ixfs[i]
            below[i] = sorted({int(u) for u in f["fname_idx"] if u >= 0} |
                              {u for b in range(f["bins"]) if f["fname_idx"][b] < 0 for u in under(int(f["next_ixf"][b]))})
        return below[i]

    depth = 1
    for i, f in enumerate(ixfs):
        sizes = []
        for b in range(f["bins"]):
            u = int(f["fname_idx"][b])
            if u < 0:
                sizes.append(np.unique(np.concatenate([sets[x] for x in under(int(f["next_ixf"][b]))])).size)
            else:
                run = np.flatnonzero(f["fname_idx"] == u)
                p, j, n = run.size, b - run[0], sets[u].size
                sizes.append(n * (j + 1) // p - n * j // p)
        assert f["seg_len"] == orc.ixf_seg_len(max(sizes + [1])), f"IXF {i}"
        assert f["stride"] == (f["bins"] + 63) // 64 * 64
        d, x = 1, i
        while x in parent:
            x, d = parent[x][0], d + 1
        depth = max(depth, d)
    splits = merged = 0
    for u in range(N):
        i = next(i for i, f in enumerate(ixfs) if (f["fname_idx"] == u).any())
        run = np.flatnonzero(ixfs[i]["fname_idx"] == u)
        assert np.array_equal(run, np.arange(run[0], run[0] + run.size))
        splits += run.size > 1
        keys, p = sets[u], run.size
        cnt = h.ixf_bulk_count(i, keys)
        for j in range(p):                                   # part j of the sorted keys sits in the run's j-th bin
            part = keys[keys.size * j // p:keys.size * (j + 1) // p]
            assert h.ixf_bulk_count(i, part)[run[j]] == part.size
        assert cnt[run].sum() >= keys.size
        x = i
        while x in parent:                                   # and in every merged bin above it
            x, b = parent[x]
            assert h.ixf_bulk_count(x, keys)[b] == keys.size
            merged += 1
    return depth, splits, merged


def test_build_syncmers_end_to_end(tmp_path):
    tsv, dirs, paths, records = write_inputs(tmp_path)
    out = tmp_path / "idx.hixf"
    build(tsv, dirs, out, "--use-syncmer", "--kmer-size", "22", "--syncmer-size", "12", "--tmax", "64")
    sets = oracle_sets(records, 22, 12, 5, 1)
    hf = HixfFile(out)
    depth, splits, merged = check_index(hf, sets, paths, records, 22, 12, 5, True, 20, 1)
    assert depth >= 2 and splits >= 1 and merged >= 1
    # taxor search on the built index == the oracle on the same file
    g = np.frombuffer(b"".join(b"".join(r) for r in records), np.uint8)
    go = np.cumsum([0] + [sum(len(x) for x in r) for r in records]).astype(np.uint64)
    bases, offs, origin = synth.synth_reads(g, go, 300, 1500, error_rate=0.0, frac_random=0.1, seed=9)
    reads = [bytes(bases[int(offs[i]):int(offs[i + 1])]) for i in range(300)]
    ids = [f"read_{i}" for i in range(300)]
    fa = tmp_path / "reads.fa"
    fa.write_bytes(b"".join(b">" + i.encode() + b"\n" + r + b"\n" for i, r in zip(ids, reads)))
    res = tmp_path / "out.tsv"
    cp = subprocess.run([TAXOR, "search", "--index-file", str(out), "--query-file", str(fa), "--output-file", str(res), "--threads", "4"],
                        capture_output=True, text=True, timeout=300)
    assert cp.returncode == 0, cp.stderr
    h = orc.Hixf(hf.ixfs, [f["next_ixf"] for f in hf.ixfs], [f["fname_idx"] for f in hf.ixfs])
    B = np.frombuffer(b"".join(reads), dtype=np.uint8)
    O = np.cumsum([0] + [len(r) for r in reads]).astype(np.uint64)
    nh, off, ub, cnt, _ = h.search_batch(B, O, threads=4)
    want = HEADER
    for i, rid in enumerate(ids):
        tup = [(int(a), int(b)) for a, b in zip(ub[int(off[i]):int(off[i + 1])], cnt[int(off[i]):int(off[i + 1])])]
        want += expected_lines(hf.species, rid, len(reads[i]), int(nh[i]), tup)
    text = open(res).read()
    assert text == want
    hits = 0
    for i, rid in enumerate(ids):                            # error-free reads report their source genome
        if origin[i] >= 0 and len(reads[i]) >= 1000:
            acc = f"GCF_{100000 + int(origin[i]):09d}.1"
            hits += any(l.split("\t")[1] == acc for l in text.splitlines() if l.startswith(rid + "\t"))
    assert hits == sum(1 for i in range(300) if origin[i] >= 0)
    hf.close()
    # a second build is byte-identical
    out2 = tmp_path / "idx2.hixf"
    build(tsv, dirs, out2, "--use-syncmer", "--kmer-size=22", "--syncmer-size=12", "--tmax=64")
    assert out.read_bytes() == out2.read_bytes()


BUILD_ROWS = [
    ([], 20, 0, 0, 20, 1),
    (["--use-syncmer", "--kmer-size", "22", "--syncmer-size", "12", "--scaling", "10"], 22, 12, 5, 20, 10),
    (["--use-syncmer", "--kmer-size", "30", "--syncmer-size", "16"], 30, 16, 7, 20, 1),
    (["--use-syncmer", "--kmer-size", "2", "--syncmer-size", "1"], 2, 1, 1, 20, 1),
    (["--kmer-size", "32", "--window-size", "96"], 32, 0, 0, 96, 1),
    (["--kmer-size", "1", "--window-size", "1"], 1, 0, 0, 1, 1),
    # most 6-kb genomes keep zero or one key: user bins without keys go through layout, build and check_index
    (["--use-syncmer", "--kmer-size", "22", "--syncmer-size", "12", "--scaling", "1000"], 22, 12, 5, 20, 1000),
]


# the first two rows keep the ids they had before the s and t columns
BUILD_IDS = ["extra0-20-20-1", "extra1-22-20-10", "syncmer-k30-s16", "syncmer-k2-s1", "minimiser-k32-w96", "minimiser-k1-w1",
             "syncmer-k22-s12-scaling1000"]


@pytest.mark.parametrize("extra,k,s,t,w,scaling", BUILD_ROWS, ids=BUILD_IDS)
def test_build_minimisers_and_scaling(tmp_path, extra, k, s, t, w, scaling):
    tsv, dirs, paths, records = write_inputs(tmp_path)
    out = tmp_path / "idx.hixf"
    build(tsv, dirs, out, "--tmax", "64", *extra)
    use_syncmer = "--use-syncmer" in extra
    sets = oracle_sets(records, k, s, t, scaling, None if use_syncmer else w)
    if scaling == 1000:
        assert sum(x.size == 0 for x in sets) > N // 3
    hf = HixfFile(out)
    depth, splits, merged = check_index(hf, sets, paths, records, k, s, t, use_syncmer, w, scaling)
    assert depth >= 2 and merged >= 1
    hf.close()
    out2 = tmp_path / "idx2.hixf"
    build(tsv, dirs, out2, "--tmax", "64", *extra)
    assert out.read_bytes() == out2.read_bytes()
