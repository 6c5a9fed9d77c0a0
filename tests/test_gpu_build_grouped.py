"""`taxor build --group-similar` end to end: 16 families of 8 related genomes, written in an order that interleaves the families,
built with a forced t_max of 16.  With the switch every family lies under at most two root bins, the root's merged bins hold
fewer keys and its seg_len does not grow; the grouped index is as correct as the ungrouped one (test_gpu_build_cli.py's checks),
builds are repeatable on both routes, and without the switch the tree is the one the unranked layout gives."""
import functools
import os
import subprocess

import numpy as np
import pytest

from oracle import oracle as orc
from taxor_amd import synth
from taxor_amd.genome_keys import build_layout
from taxor_amd.hixf_file import HixfFile
from tests import test_gpu_build_cli as bc
from tests.test_hixf_file_cpu import HEADER, expected_lines

pytestmark = pytest.mark.gpu
TAXOR = bc.TAXOR
N_FAM, FAM_SIZE, LENGTH = 16, 8, 6000
N = N_FAM * FAM_SIZE
K, S, T = 22, 12, 5
SCHEME = ["--use-syncmer", "--kmer-size", str(K), "--syncmer-size", str(S), "--tmax", "16"]


@functools.lru_cache(maxsize=None)
def genomes():
    """file i holds member i // 16 of family i % 16 -> (sequences in file order, family of each file, oracle key sets)"""
    g, go, fam = synth.family_genomes(N_FAM, FAM_SIZE, LENGTH)
    seqs, family = [], []
    for i in range(N):
        src = (i % N_FAM) * FAM_SIZE + i // N_FAM
        seqs.append(bytes(g[int(go[src]):int(go[src + 1])]))
        family.append(int(fam[src]))
    sets = bc.oracle_sets([[s] for s in seqs], K, S, T, 1)
    return seqs, np.array(family), sets


def write_inputs(tmp_path):
    seqs, _, _ = genomes()
    d = tmp_path / "genomes"
    d.mkdir()
    lines, paths = [], []
    for i, seq in enumerate(seqs):
        acc = f"GCF_{100000 + i:09d}.1"
        stem = f"{acc}_ASM{i}v1_genomic"
        path = d / (stem + ".fna")
        path.write_bytes(b">chr\n" + seq + b"\n")
        paths.append(str(path))
        lines.append("\t".join([acc, str(5000 + i), f"ftp://host/genomes/{acc}/{stem}", f"Organism {i}", f"k__B;s__Organism {i}", f"2;{5000 + i}"]))
    tsv = tmp_path / "tax.tsv"
    tsv.write_text("\n".join(lines) + "\n")
    return tsv, d, paths


def build(tsv, d, out, *extra):
    cp = subprocess.run([TAXOR, "build", "--input-file", str(tsv), "--input-sequence-dir", str(d), "--output-filename", str(out), "--threads", "4",
                         *SCHEME, *extra], capture_output=True, text=True, timeout=600)
    assert cp.returncode == 0, cp.stdout + cp.stderr
    assert cp.stderr.startswith(f"taxor build: {N} genomes"), cp.stderr
    return cp


def jaccard(a, b):
    inter = np.intersect1d(a, b, assume_unique=True).size
    return inter / (a.size + b.size - inter)


def test_premise_families_are_connected_and_apart():
    """the oracle's key sets: every family is connected under exact Jaccard >= 0.2 (twice the default threshold), no two genomes of
    different families reach 0.05, and every sketch of 1024 values is complete"""
    _, family, sets = genomes()
    assert max(s.size for s in sets) <= 1024
    J = np.array([[jaccard(sets[a], sets[b]) for b in range(N)] for a in range(N)])
    for f in range(N_FAM):
        mem = np.flatnonzero(family == f)
        seen, todo = {int(mem[0])}, [int(mem[0])]
        while todo:
            x = todo.pop()
            for y in mem:
                if int(y) not in seen and J[x, y] >= 0.2:
                    seen.add(int(y))
                    todo.append(int(y))
        assert len(seen) == FAM_SIZE, f"family {f}"
    other = family[:, None] != family[None, :]
    assert J[other].max() < 0.05


def root_bin_of(hf):
    """user bin -> the root bin it lies in or under; and the user bins under each merged root bin"""
    ixfs = hf.ixfs

    def under(i):
        f = ixfs[i]
        out = {int(u) for u in f["fname_idx"] if u >= 0}
        for b in range(f["bins"]):
            if f["fname_idx"][b] < 0:
                out |= under(int(f["next_ixf"][b]))
        return out

    where, merged = np.full(N, -1), {}
    root = ixfs[0]
    for b in range(root["bins"]):
        if root["fname_idx"][b] >= 0:
            where[int(root["fname_idx"][b])] = b
        else:
            merged[b] = sorted(under(int(root["next_ixf"][b])))
            where[merged[b]] = b
    assert (where >= 0).all()
    return where, merged


def union_sum(merged, sets):
    return sum(np.unique(np.concatenate([sets[u] for u in ub])).size for ub in merged.values())


def check(hf, paths, monkeypatch):
    seqs, _, sets = genomes()
    monkeypatch.setattr(bc, "N", N)
    return bc.check_index(hf, sets, paths, [[s] for s in seqs], K, S, T, True, 20, 1)


def test_grouped_build_end_to_end(tmp_path, monkeypatch):
    seqs, family, sets = genomes()
    tsv, d, paths = write_inputs(tmp_path)
    plain, grouped = tmp_path / "plain.hixf", tmp_path / "grouped.hixf"
    build(tsv, d, plain)
    cp = build(tsv, d, grouped, "--group-similar")
    assert "similar genomes grouped: 16 clusters of more than one genome" in cp.stderr, cp.stderr
    hp, hg = HixfFile(plain), HixfFile(grouped)
    # ---- the grouping
    where_g, merged_g = root_bin_of(hg)
    where_p, merged_p = root_bin_of(hp)
    assert max(np.unique(where_g[family == f]).size for f in range(N_FAM)) <= 2
    assert max(np.unique(where_p[family == f]).size for f in range(N_FAM)) > 2          # (what the switch is for)
    assert union_sum(merged_g, sets) < union_sum(merged_p, sets)
    assert hg.ixfs[0]["seg_len"] <= hp.ixfs[0]["seg_len"]
    # ---- the grouped index is correct: metadata, geometry, every key in its leaf run and in every merged bin above it
    depth, _, merged = check(hg, paths, monkeypatch)
    assert depth >= 2 and merged >= 1
    # ---- without the switch: the tree of the unranked layout over the exact counts
    check(hp, paths, monkeypatch)
    lay = build_layout([s.size for s in sets], 16)
    assert len(hp.ixfs) == len(lay["ixfs"])
    for f, want in zip(hp.ixfs, lay["ixfs"]):
        assert f["bins"] == want["bins"]
        assert np.array_equal(f["next_ixf"], want["next_ixf"]) and np.array_equal(f["fname_idx"], want["fname_idx"])
    # ---- taxor search on the grouped index == the oracle on the same file
    g = np.frombuffer(b"".join(seqs), np.uint8)
    go = (np.arange(N + 1) * LENGTH).astype(np.uint64)
    n_reads = 200
    bases, offs, origin = synth.synth_reads(g, go, n_reads, 1500, error_rate=0.0, frac_random=0.1, seed=9)
    reads = [bytes(bases[int(offs[i]):int(offs[i + 1])]) for i in range(n_reads)]
    ids = [f"read_{i}" for i in range(n_reads)]
    fa = tmp_path / "reads.fa"
    fa.write_bytes(b"".join(b">" + i.encode() + b"\n" + r + b"\n" for i, r in zip(ids, reads)))
    res = tmp_path / "out.tsv"
    cp = subprocess.run([TAXOR, "search", "--index-file", str(grouped), "--query-file", str(fa), "--output-file", str(res), "--threads", "4"],
                        capture_output=True, text=True, timeout=300)
    assert cp.returncode == 0, cp.stderr
    h = orc.Hixf(hg.ixfs, [f["next_ixf"] for f in hg.ixfs], [f["fname_idx"] for f in hg.ixfs])
    B = np.frombuffer(b"".join(reads), dtype=np.uint8)
    O = np.cumsum([0] + [len(r) for r in reads]).astype(np.uint64)
    nh, off, ub, cnt, _ = h.search_batch(B, O, threads=4)
    want = HEADER
    for i, rid in enumerate(ids):
        tup = [(int(a), int(b)) for a, b in zip(ub[int(off[i]):int(off[i + 1])], cnt[int(off[i]):int(off[i + 1])])]
        want += expected_lines(hg.species, rid, len(reads[i]), int(nh[i]), tup)
    assert open(res).read() == want
    hp.close()
    hg.close()
    # ---- determinism and routes
    again, streamed = tmp_path / "again.hixf", tmp_path / "streamed.hixf"
    build(tsv, d, again, "--group-similar")
    assert again.read_bytes() == grouped.read_bytes()
    cp = build(tsv, d, streamed, "--group-similar", "--device-key-budget", "1")
    assert "path stream" in cp.stderr, cp.stderr
    assert streamed.read_bytes() == grouped.read_bytes()


def test_four_similarity_windows(tmp_path, monkeypatch):
    _, family, sets = genomes()
    tsv, d, paths = write_inputs(tmp_path)
    out = tmp_path / "w32.hixf"
    build(tsv, d, out, "--group-similar", "--similarity-window", "32")
    hf = HixfFile(out)
    check(hf, paths, monkeypatch)
    where, _ = root_bin_of(hf)
    # the windows: runs of 32 in descending key count, ties on the index
    counts = np.array([s.size for s in sets])
    p = np.lexsort((np.arange(N), -counts))
    window = np.empty(N, np.int64)
    window[p] = np.arange(N) // 32
    shared_a_window = 0
    for f in range(N_FAM):
        for w in range(4):
            mem = np.flatnonzero((family == f) & (window == w))
            shared_a_window += mem.size > 1
            assert np.unique(where[mem]).size <= 2, (f, w)
    assert shared_a_window >= N_FAM
    hf.close()


@pytest.mark.parametrize("option,value", [("--sketch-size", "8"), ("--similarity-threshold", "0"), ("--similarity-window", "1")])
def test_refusals_come_before_any_device_work(tmp_path, option, value):
    # no device is visible to the process: a HIP call would fail with another message, and nothing of the input is looked at yet
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1")
    cp = subprocess.run([TAXOR, "build", "--input-file", str(tmp_path / "absent.tsv"), "--output-filename", str(tmp_path / "x.hixf"), *SCHEME,
                         "--group-similar", option, value], capture_output=True, text=True, timeout=60, env=env)
    assert cp.returncode != 0
    assert cp.stdout == ""
    assert cp.stderr.startswith("[TAXOR BUILD ERROR] ") and option in cp.stderr and "range" in cp.stderr, cp.stderr
    assert not (tmp_path / "x.hixf").exists()
