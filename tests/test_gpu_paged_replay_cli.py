"""`taxor search --device-index-budget --paged-replay`: the query file is read in the first pass only, the later passes replay the
reads' saved hash lists.  Plain FASTQ, .fastq.gz and BAM against a three-pass budget, several batches per pass: the TSV is the resident
run's and the re-reading runs' (the default, and --paged-reread) byte for byte, the three profile files are the resident run's, and
stderr says what the run did with the query.  Replay is opt-in: re-reading stays the default until the command line has been measured."""
import gzip
import os

import pytest

from tests.test_gpu_bam import run
from tests.test_gpu_bam import world as bam_world  # noqa: F401  (the paged test's index, 200 reads as BAM and as FASTQ)

pytestmark = pytest.mark.gpu
BATCH = 64


@pytest.fixture(scope="module")
def world(bam_world):  # noqa: F811
    w = dict(bam_world)
    gz = w["tmp"] / "reads.fastq.gz"
    with gzip.open(gz, "wb", compresslevel=1) as f:
        f.write(w["fq"].read_bytes())
    w["gz"] = gz
    w["n_reads"] = w["fq"].read_bytes().count(b"\n") // 4
    return w


def _search(w, query, out, extra):
    cp = run(["search", "--index-file", w["idx"], "--query-file", query, "--output-file", out, "--threads", "4"] + extra)
    assert cp.returncode == 0, cp.stdout + cp.stderr
    return cp.stderr


@pytest.mark.parametrize("kind", ["fq", "gz", "bam"])
def test_replayed_passes_write_the_resident_tsv(world, kind):
    w = world
    paged = ["--device-index-budget", w["budget"], "--batch-reads", BATCH]
    replay, reread = w["tmp"] / f"replay_{kind}.tsv", w["tmp"] / f"reread_{kind}.tsv"
    err = _search(w, w[kind], replay, paged + ["--paged-replay"])
    n_batches = (w["n_reads"] + BATCH - 1) // BATCH
    passes_line = f"searched in {w['passes']} resident passes over the query (--device-index-budget {w['budget']} MiB)\n"
    assert w["passes"] >= 3 and n_batches >= 3
    assert passes_line in err
    line = next(ln for ln in err.splitlines() if "saved hash lists" in ln)
    assert f"passes 1 to {w['passes'] - 1} replay {n_batches} batches from " in line and "read again" not in err
    assert int(line.split(" batches from ")[1].split(" bytes")[0]) > 8 * 100 * w["n_reads"] // 11 // 4            # 8 B per hash, reads of 300+ bases
    assert err.index(passes_line) < err.index(line)
    assert replay.read_bytes() == w["plain"].read_bytes()
    err2 = _search(w, w[kind], reread, paged + ["--paged-reread"])
    assert passes_line in err2 and "taxor search: the query is read again in every pass (--paged-reread)\n" in err2 and "saved hash lists" not in err2
    assert reread.read_bytes() == w["plain"].read_bytes()
    default = w["tmp"] / f"default_{kind}.tsv"
    err3 = _search(w, w[kind], default, paged)                       # the default re-reads, and names the option that does not
    assert passes_line in err3 and "taxor search: the query is read again in every pass (the default; --paged-replay" in err3 and "saved hash lists" not in err3
    assert default.read_bytes() == w["plain"].read_bytes()
    err4 = _search(w, w[kind], default, paged + ["--paged-replay", "--paged-reread"])          # said aloud, re-reading wins
    assert "read again in every pass (--paged-reread)" in err4 and "saved hash lists" not in err4


@pytest.mark.parametrize("kind", ["fq", "gz", "bam"])
def test_replayed_passes_write_the_resident_profile_files(world, kind):
    w = world

    def prof(d, extra):
        os.makedirs(str(d), exist_ok=True)
        cp = run(["search", "--index-file", w["idx"], "--query-file", w[kind], "--threads", "4", "--cami-report-file", d / "cami", "--seq-abundance-file", d / "seq",
                  "--binning-file", d / "bin", "--sample-id", "S"] + extra)
        assert cp.returncode == 0, cp.stdout + cp.stderr
        return {k: (d / k).read_bytes() for k in ("cami", "seq", "bin")}, cp.stderr

    a, _ = prof(w["tmp"] / f"prof_resident_{kind}", [])
    b, err = prof(w["tmp"] / f"prof_replay_{kind}", ["--device-index-budget", w["budget"], "--batch-reads", BATCH, "--paged-replay"])
    assert "bytes of saved hash lists" in err and a == b and len(a["bin"]) > 0
