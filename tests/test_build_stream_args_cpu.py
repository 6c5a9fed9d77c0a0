"""`taxor build` beyond device memory on a box without a GPU: --device-key-budget's parsing and range, the advanced help, and the
two refusals that numbers alone decide -- a genome whose keys may exceed the budget, by its file's name, and a key store larger than
the host memory, with the figure handed in -- all before any HIP call."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TAXOR = os.path.join(ROOT, "taxor_amd", "taxor")


def run(*args):
    p = subprocess.run([TAXOR, "build", *map(str, args)], capture_output=True, text=True, timeout=60)
    return p.returncode, p.stdout, p.stderr


@pytest.mark.parametrize("args,msg", [
    (["--device-key-budget", "0"], "Validation failed for option --device-key-budget: Value 0 is not in range [1,16777216]."),
    (["--device-key-budget=16777217"], "Validation failed for option --device-key-budget: Value 16777217 is not in range [1,16777216]."),
    (["--device-key-budget", "-3"], "Validation failed for option --device-key-budget: Value -3 is not in range [1,16777216]."),
    (["--device-key-budget", "12MiB"], "Value parse failed for --device-key-budget: Argument 12MiB could not be parsed as type int32."),
    (["--device-key-budget"], "Missing value for option --device-key-budget"),
    (["--host-memory-mib", "0"], "Validation failed for option --host-memory-mib: Value 0 is not in range [1,1073741824]."),
])
def test_option_parsing_and_range(tmp_path, args, msg):
    t = tmp_path / "tax.tsv"
    t.write_text("GCF_000000001.1\t5\ta/GCF_000000001.1_x\n")
    rc, _, err = run("--input-file", t, *args)
    assert rc == 255 and err == f"[TAXOR BUILD ERROR] {msg}\n"


def test_advanced_help_lists_the_hidden_options():
    rc, out, err = run("--advanced-help")
    assert rc == 0 and err == ""
    lines = out.splitlines()
    tmax = next(i for i, l in enumerate(lines) if l.lstrip().startswith("--tmax "))
    budget = next(i for i, l in enumerate(lines) if l.lstrip().startswith("--device-key-budget <MiB>"))
    assert budget > tmax and all(not l.lstrip().startswith("--") for l in lines[tmax + 1:budget])       # beside --tmax
    assert "[1,16777216]" in out and "--host-memory-mib <MiB>" in out


def genomes(tmp_path, sizes):
    d = tmp_path / "g"
    d.mkdir()
    lines = []
    for i, n in enumerate(sizes):
        acc = f"GCF_{i + 1:09d}.1"
        (d / f"{acc}_ASM{i}v1_genomic.fna").write_bytes(b">r\n" + b"ACGT" * (n // 4) + b"\n")
        lines.append(f"{acc}\t{5 + i}\ta/{acc}_ASM{i}v1\n")
    t = tmp_path / "tax.tsv"
    t.write_text("".join(lines))
    return t, d


def test_host_memory_refusal_names_both_figures(tmp_path):
    """three genomes of 400 kB: up to 80 001 syncmer keys each, 640 kB -- within a budget of 1 MiB one by one, beyond it together, so
    the keys go to a host store of up to 1.83 MiB; 1 MiB of host memory does not hold it"""
    t, d = genomes(tmp_path, [400000] * 3)
    rc, out, err = run("--input-file", t, "--input-sequence-dir", d, "--output-filename", tmp_path / "x.hixf", "--use-syncmer", "--kmer-size", 22,
                       "--syncmer-size", 12, "--device-key-budget", 1, "--host-memory-mib", 1)
    assert rc == 255 and out.endswith("creating HIXF layout ... ")
    assert err == ("[TAXOR BUILD ERROR] the distinct keys of these genomes may need 1 MiB of host memory, 1 MiB are available; "
                   "keys on disk are not supported\n")
    assert not (tmp_path / "x.hixf").exists()


def test_host_memory_refusal_rounds_down_but_compares_bytes(tmp_path):
    t, d = genomes(tmp_path, [400000] * 6)
    rc, _, err = run("--input-file", t, "--input-sequence-dir", d, "--output-filename", tmp_path / "x.hixf", "--use-syncmer", "--kmer-size", 22,
                     "--syncmer-size", 12, "--device-key-budget", 1, "--host-memory-mib", 3)
    assert rc == 255 and "may need 3 MiB of host memory, 3 MiB are available" in err


def test_a_genome_beyond_the_budget_is_refused_by_name(tmp_path):
    """minimisers: up to one key per base; 200 kB of bases are 1.5 MiB of keys"""
    t, d = genomes(tmp_path, [50000, 200000, 50000])
    rc, _, err = run("--input-file", t, "--input-sequence-dir", d, "--output-filename", tmp_path / "x.hixf", "--device-key-budget", 1)
    path = d / "GCF_000000002.1_ASM1v1_genomic.fna"
    assert rc == 255
    assert err == f"[TAXOR BUILD ERROR] the distinct keys of {path} alone (up to 1 MiB) may exceed the device key budget of 1 MiB\n"
