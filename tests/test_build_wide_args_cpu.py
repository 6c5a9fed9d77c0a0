"""`taxor build --use-syncmer` with syncmer sizes above 16, on a box without a GPU: the argument checks let every size of the
reference's documented range [1,26] below the k-mer size through, and still refuse s >= k and the range's end by name."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TAXOR = os.path.join(ROOT, "taxor_amd", "taxor")


def run(*args):
    p = subprocess.run([TAXOR, "build", *map(str, args)], capture_output=True, text=True, timeout=60)
    return p.returncode, p.stdout, p.stderr


@pytest.fixture
def inputs(tmp_path):
    """a taxonomy of two species with the genome file of the first only: a build that passes its argument checks stops at the
    genome lookup, before any device call"""
    (tmp_path / "g").mkdir()
    (tmp_path / "g" / "GCF_000000001.1_ASM1v1_genomic.fna").write_text(">r\nACGT\n")
    t = tmp_path / "tax.tsv"
    t.write_text("GCF_000000001.1\t5\ta/GCF_000000001.1_ASM1v1\nGCF_000000002.1\t6\ta/GCF_000000002.1_ASM2v1\n")
    return ["--input-file", t, "--input-sequence-dir", tmp_path / "g", "--output-filename", tmp_path / "x.hixf"]


@pytest.mark.parametrize("k,s", [(28, 20), (18, 17), (24, 17), (30, 26), (27, 26)])
def test_wide_syncmer_sizes_pass_the_checks(inputs, k, s):
    rc, out, err = run(*inputs, "--use-syncmer", "--kmer-size", k, "--syncmer-size", s)
    assert out == "checking input ... done!\nparsing taxonomy input files ... done!\ncreating HIXF layout ... ", (out, err)
    assert rc == 255 and err == "[TAXOR BUILD ERROR] Could not find a genome file for GCF_000000002.1\n"
    assert "syncmer size" not in err


@pytest.mark.parametrize("k,s", [(20, 20), (20, 21), (17, 17), (12, 16)])
def test_syncmer_size_not_below_kmer_size_is_refused_by_name(inputs, k, s):
    rc, out, err = run(*inputs, "--use-syncmer", "--kmer-size", k, "--syncmer-size", s)
    assert rc == 255 and out == "checking input ... "
    assert err.startswith(f"[TAXOR BUILD ERROR] syncmer size {s} with k-mer size {k}: "), err
    assert "16" not in err.split(": ", 1)[1]            # the message names no s <= 16 limit any more


def test_reference_range_and_kmer_limit_stay(inputs):
    rc, _, err = run(*inputs, "--use-syncmer", "--kmer-size", 30, "--syncmer-size", 27)
    assert rc == 255 and err == "[TAXOR BUILD ERROR] Validation failed for option --syncmer-size: Value 27 is not in range [1,26].\n"
    rc, _, err = run(*inputs, "--use-syncmer", "--kmer-size", 31, "--syncmer-size", 20)
    assert rc == 255 and err == ("[TAXOR BUILD ERROR] The chosen k-mer size is too large for the syncmer scheme. "
                                 "Please choose a k-mer size <= 30 or use the minimizer scheme\n")


def test_help_names_the_range():
    p = subprocess.run([TAXOR, "build", "--advanced-help"], capture_output=True, text=True, timeout=60)
    line = next(l for l in p.stdout.splitlines() if l.lstrip().startswith("--syncmer-size"))
    assert p.returncode == 0 and "[1,26]" in line and "below --kmer-size" in line
