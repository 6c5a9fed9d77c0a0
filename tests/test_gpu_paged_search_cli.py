"""`taxor search --device-index-budget`: an index searched in resident passes from its .hixf (the file's fingerprints are read through
the loader's source, group by group, on the upload thread) writes what the resident search writes, byte for byte: the TSV, at two
batch sizes, and the three profile files of search-to-profile in one run.  The two refusals exit non-zero with their messages."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from taxor_amd import _lib, synth

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TAXOR = os.path.join(ROOT, "taxor_amd", "taxor")
N_GENOMES, GENOME_LEN, N_READS = 40, 60000, 400


def run(args, timeout=300, **kw):
    return subprocess.run([TAXOR] + [str(a) for a in args], capture_output=True, text=True, timeout=timeout, **kw)


def plan_of(path, budget):
    """(passes, or None when the plan refuses) of the file's hierarchy under `budget` bytes -- host arithmetic only"""
    L = _lib.lib()
    h = C.c_void_p()
    _lib.check(L.taxor_hixf_load(str(path).encode(), C.byref(h)))
    plan = _lib.PassPlan()
    rc = L.taxor_index_plan_passes(L.taxor_hixf_get_view(h), int(budget), C.byref(plan), None, None)
    L.taxor_hixf_free(h)
    return plan.n_passes if rc == 0 else None


@pytest.fixture(scope="module")
def world(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("paged_cli")
    g, go = synth.random_genomes(N_GENOMES, GENOME_LEN, seed=31)
    gdir = tmp / "genomes"
    gdir.mkdir()
    lines = []
    for i in range(N_GENOMES):
        acc = f"GCF_{800000 + (i * 7) % N_GENOMES:09d}.1"
        stem = f"{acc}_ASM{i}v1_genomic"
        (gdir / (stem + ".fna")).write_bytes(b">chr1\n" + bytes(g[int(go[i]):int(go[i + 1])]) + b"\n")
        names = f"k__Bacteria;p__P{i % 2};c__C{i % 3};o__O{i % 5};f__F{i % 7};g__G{i};s__G{i} species{i}"
        ids = f"2;{20 + i % 2};{30 + i % 3};{40 + i % 5};{500 + i % 7};{6000 + i};{70000 + i}"
        lines.append("\t".join([acc, str(70000 + i), f"ftp://host/genomes/{acc}/{stem}", f"G{i} species{i}", names, ids]))
    tax = tmp / "tax.tsv"
    tax.write_text("\n".join(lines) + "\n")
    idx = tmp / "idx.hixf"
    # --tmax 6: a root of at most six bins, every one of them a merged bin over a subtree two levels deep
    cp = run(["build", "--input-file", tax, "--input-sequence-dir", gdir, "--output-filename", idx, "--threads", "4", "--use-syncmer",
              "--kmer-size", "22", "--syncmer-size", "12", "--tmax", "6"], timeout=600)
    assert cp.returncode == 0, cp.stdout + cp.stderr
    rng = np.random.default_rng(32)
    acgt = np.frombuffer(b"ACGT", np.uint8)
    recs = []
    for i in range(N_READS):
        n = int(rng.integers(1000, 3001))
        if i % 10 == 9:
            seq = acgt[rng.integers(0, 4, n)]
        else:
            j = int(rng.integers(0, N_GENOMES))
            a = int(go[j]) + int(rng.integers(0, GENOME_LEN - n + 1))
            seq = g[a:a + n]
        recs.append(b"@read_%d ch=%d\n" % ((i * 7919) % N_READS, i % 512) + bytes(seq) + b"\n+\n" + b"I" * n + b"\n")
    fq = tmp / "reads.fq"
    fq.write_bytes(b"".join(recs))
    budget = next((m for m in range(1, 64) if (plan_of(idx, m << 20) or 0) >= 3), None)
    assert budget is not None, "no budget of whole MiB gives this index three passes"
    plain = tmp / "plain.tsv"
    cp = run(["search", "--index-file", idx, "--query-file", fq, "--output-file", plain, "--threads", "4"])
    assert cp.returncode == 0, cp.stdout + cp.stderr
    assert plain.read_bytes().count(b"\n") > N_READS // 2
    return dict(tmp=tmp, idx=idx, fq=fq, plain=plain, budget=budget, passes=plan_of(idx, budget << 20))


def test_paged_tsv_is_byte_identical(world):
    w = world
    out = w["tmp"] / "paged.tsv"
    cp = run(["search", "--index-file", w["idx"], "--query-file", w["fq"], "--output-file", out, "--threads", "4", "--device-index-budget", w["budget"]])
    assert cp.returncode == 0, cp.stdout + cp.stderr
    assert f"searched in {w['passes']} resident passes" in cp.stderr and "--device-index-budget" in cp.stderr
    assert out.read_bytes() == w["plain"].read_bytes()


def test_paged_tsv_with_several_batches_per_pass(world):
    w = world
    out = w["tmp"] / "paged_small.tsv"
    cp = run(["search", "--index-file", w["idx"], "--query-file", w["fq"], "--output-file", out, "--threads", "4", "--device-index-budget", w["budget"],
              "--batch-reads", "96"])
    assert cp.returncode == 0, cp.stdout + cp.stderr
    assert out.read_bytes() == w["plain"].read_bytes()


def test_paged_profile_files_are_byte_identical(world):
    w = world

    def prof(d, extra):
        os.makedirs(str(d), exist_ok=True)
        cp = run(["search", "--index-file", w["idx"], "--query-file", w["fq"], "--threads", "4", "--cami-report-file", d / "cami", "--seq-abundance-file", d / "seq",
                  "--binning-file", d / "bin", "--sample-id", "S"] + extra)
        assert cp.returncode == 0, cp.stdout + cp.stderr
        return {k: (d / k).read_bytes() for k in ("cami", "seq", "bin")}

    a = prof(w["tmp"] / "prof_resident", [])
    b = prof(w["tmp"] / "prof_paged", ["--device-index-budget", w["budget"], "--batch-reads", "150"])
    assert a == b and len(a["bin"]) > 0


def test_paging_refuses_standard_input_and_several_devices(world):
    w = world
    cp = run(["search", "--index-file", w["idx"], "--query-file", "/dev/stdin", "--output-file", w["tmp"] / "x.tsv", "--device-index-budget", w["budget"]],
             input=open(w["fq"]).read())                 # a pipe
    assert cp.returncode != 0 and "cannot be read again" in cp.stderr
    cp = run(["search", "--index-file", w["idx"], "--query-file", w["fq"], "--output-file", w["tmp"] / "y.tsv", "--device-index-budget", w["budget"], "--gpus", "2",
              "--gather", "host"])
    assert cp.returncode != 0 and "ONE device" in cp.stderr and "--gpus" in cp.stderr
