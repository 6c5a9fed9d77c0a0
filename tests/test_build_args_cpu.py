"""`taxor build` on a box without a GPU: every error path the reference's sanity checks have (taxor_build.cpp:51-166,268-293)
answers with its "[TAXOR BUILD ERROR] ..." line and exit status -1 before any HIP call, and the layout function
(taxor_build_layout, host only) holds its invariants."""
import os
import subprocess

import numpy as np
import pytest

from taxor_amd.genome_keys import build_layout

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TAXOR = os.path.join(ROOT, "taxor_amd", "taxor")


def run(*args, cwd=None):
    p = subprocess.run([TAXOR, "build", *map(str, args)], capture_output=True, text=True, cwd=cwd, timeout=60)
    return p.returncode, p.stdout, p.stderr


def tsv(tmp_path, lines, name="tax.tsv"):
    p = tmp_path / name
    p.write_text("".join("\t".join(l) + "\n" for l in lines))
    return p


def test_missing_input_file():
    rc, _, err = run("--kmer-size", 20)
    assert rc == 255 and err == "[TAXOR BUILD ERROR] Option --input-file is required but not set.\n"


def test_nonexistent_file_and_dir(tmp_path):
    rc, out, err = run("--input-file", tmp_path / "nope.tsv")
    assert rc == 255 and out == "checking input ... "
    assert err == f"[TAXOR BUILD ERROR] Please check the given input file(s). \nThe following input file does not exist: {tmp_path / 'nope.tsv'}\n"
    t = tsv(tmp_path, [["GCF_000000001.1", "5", "a/GCF_000000001.1_x"]])
    rc, _, err = run(f"--input-file={t}", f"--input-sequence-dir={tmp_path / 'nodir'}")
    assert rc == 255
    assert err == f"[TAXOR BUILD ERROR] Please check the given input folder(s). \nThe following input folder does not exist: {tmp_path / 'nodir'}\n"


def test_tsv_line_with_two_fields(tmp_path):
    t = tsv(tmp_path, [["GCF_000000001.1", "5", "a/GCF_000000001.1_x"], ["GCF_000000002.1", "6"]])
    rc, _, err = run("--input-file", t, "--input-sequence-dir", tmp_path)
    assert rc == 255 and err == f"[TAXOR BUILD ERROR] Error parsing the taxonomy file: {t}\n"


def test_species_without_genome_file(tmp_path):
    (tmp_path / "g").mkdir()
    (tmp_path / "g" / "GCF_000000001.1_ASM1v1_genomic.fna").write_text(">r\nACGT\n")
    t = tsv(tmp_path, [["GCF_000000001.1", "5", "a/GCF_000000001.1_ASM1v1"], ["GCF_000000002.1", "6", "a/GCF_000000002.1_ASM2v1"]])
    rc, out, err = run("--input-file", t, "--input-sequence-dir", tmp_path / "g", "--output-filename", tmp_path / "x.hixf")
    assert rc == 255
    assert out == "checking input ... done!\nparsing taxonomy input files ... done!\ncreating HIXF layout ... "
    assert err == "[TAXOR BUILD ERROR] Could not find a genome file for GCF_000000002.1\n"
    assert not (tmp_path / "x.hixf").exists()


@pytest.mark.parametrize("args,msg", [
    (["--use-syncmer", "--kmer-size", "31"], "The chosen k-mer size is too large for the syncmer scheme. Please choose a k-mer size <= 30 or use the minimizer scheme"),
    (["--scaling", "5"], "Validation failed for option --scaling: Value 5 is not in range [10,1000]."),
    (["--scaling=5"], "Validation failed for option --scaling: Value 5 is not in range [10,1000]."),
    (["--threads", "33"], "Validation failed for option --threads: Value 33 is not in range [1,32]."),
    (["--kmer-size=65"], "Validation failed for option --kmer-size: Value 65 is not in range [1,64]."),
    (["--syncmer-size", "27"], "Validation failed for option --syncmer-size: Value 27 is not in range [1,26]."),
    (["--window-size", "0"], "Validation failed for option --window-size: Value 0 is not in range [1,96]."),
])
def test_option_checks(tmp_path, args, msg):
    t = tsv(tmp_path, [["GCF_000000001.1", "5", "a/GCF_000000001.1_x"]])
    rc, _, err = run("--input-file", t, *args)
    assert rc == 255 and err == f"[TAXOR BUILD ERROR] {msg}\n"


def _runs(L, n):
    """every user bin -> list of (ixf, first bin, bins) runs; checks each IXF's arrays"""
    runs = {}
    for i, f in enumerate(L["ixfs"]):
        fn, nx = f["fname_idx"], f["next_ixf"]
        assert f["bins"] == fn.size == nx.size and f["bins"] <= L["t_max"]
        b = 0
        while b < f["bins"]:
            if fn[b] < 0:
                assert nx[b] > i                       # children are numbered after their parents
                b += 1
                continue
            assert nx[b] == i
            u, e = fn[b], b
            while e < f["bins"] and fn[e] == u:
                e += 1
            assert list(f["part"][b:e]) == list(range(e - b)) and set(f["parts"][b:e]) == {e - b}
            runs.setdefault(int(u), []).append((i, b, e - b))
            b = e
    assert sorted(runs) == list(range(n))
    assert all(len(r) == 1 for r in runs.values()), "one leaf run per user bin"
    return runs


@pytest.mark.parametrize("n,t_max", [(1, 64), (10, 64), (64, 64), (65, 64), (150, 64), (700, 64), (300, 128), (2000, 0)])
def test_layout_invariants(n, t_max):
    rng = np.random.default_rng(n)
    counts = rng.integers(1, 100000, size=n).astype(np.uint64)
    L = build_layout(counts, t_max)
    runs = _runs(L, n)
    if t_max:
        assert L["t_max"] == t_max
    for u, [(i, b, m)] in runs.items():
        assert m <= counts[u]                            # no empty technical bin: every part holds a key
    # every merged bin's child exists and is reached once
    kids = [int(c) for i, f in enumerate(L["ixfs"]) for c, x in zip(f["next_ixf"], f["fname_idx"]) if x < 0]
    assert sorted(kids) == list(range(1, len(L["ixfs"])))
    if n > L["t_max"]:
        assert L["depth"] >= 2 and len(L["ixfs"]) >= 2
    else:
        assert L["depth"] == 1 and len(L["ixfs"]) == 1
    L2 = build_layout(counts, t_max)
    for a, b in zip(L["ixfs"], L2["ixfs"]):
        for key in ("next_ixf", "fname_idx", "part", "parts"):
            assert np.array_equal(a[key], b[key])
    assert (L["t_max"], L["depth"], L["bytes_per_hash"]) == (L2["t_max"], L2["depth"], L2["bytes_per_hash"])


def test_layout_splits_a_dominant_bin():
    counts = np.array([1000] * 20 + [200000] + [1000] * 20, dtype=np.uint64)
    runs = _runs(build_layout(counts, 64), 41)
    assert runs[20][0][2] > 1 and all(r[0][2] == 1 for u, r in runs.items() if u != 20)
    counts = np.array([20000] + [1000] * 149, dtype=np.uint64)       # n > t_max: the large bin is split at the root
    L = build_layout(counts, 64)
    runs = _runs(L, 150)
    assert runs[0][0][0] == 0 and runs[0][0][2] > 1 and L["depth"] >= 2


def test_layout_default_t_max_candidates():
    assert build_layout(np.full(10, 5000, np.uint64))["t_max"] == 64
    L = build_layout(np.full(5000, 5000, np.uint64))
    assert L["t_max"] in {64, 128, 256, 512, 1024, 2048, 4096} and L["depth"] >= 2
