"""`taxor search` writing the profile itself (search to profile in one run), end to end.

An index of 40 genomes of 8 kb in ten families of four related strains is built with `taxor build`; 3000 reads of 1-3 kb (1 %
substitutions, 5 % random reads, ids with a description, in an order that is not sorted) are classified.  The yardstick is this
tree's own two-step route, `taxor search` -> TSV -> `taxor profile`; the fused command must write the same three files byte for
byte -- without a TSV, with one (which is then the plain search's), at two batch sizes, under --min-abundance 0 --em-steps 1 -- and
refuse a query in which a read id occurs twice."""
import os
import re
import subprocess

import numpy as np
import pytest

from taxor_amd import synth

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TAXOR = os.path.join(ROOT, "taxor_amd", "taxor")
N_FAMILIES, FAMILY, GENOME_LEN, N_READS, SHARED = 10, 4, 8000, 3000, 3500
EM_LINE = re.compile(r"^Number of EM steps needed: (\d+)$", re.M)


def run(args, timeout=300):
    return subprocess.run([TAXOR] + [str(a) for a in args], capture_output=True, text=True, timeout=timeout)


def make_genomes():
    """ten families of four strains (taxor_amd/synth.py): the first SHARED bases of a strain are its family's ancestor with 0.1-0.4 %
    substitutions, the rest is the strain's own.  A read from the shared part reaches several strains (several TSV lines), one from
    the rest a single strain -- and no strain shares 95 % of its reads with a sibling, which the profile would take for an
    explained reference (four mutually explained strains are a cycle it refuses)"""
    g, go, fam = synth.family_genomes(N_FAMILIES, FAMILY, GENOME_LEN, seed=21, ladder=(0.001, 0.002, 0.003, 0.004))
    own, _ = synth.random_genomes(N_FAMILIES * FAMILY, GENOME_LEN - SHARED, seed=23)
    g = g.copy()
    for i in range(N_FAMILIES * FAMILY):
        g[int(go[i]) + SHARED:int(go[i + 1])] = own[i * (GENOME_LEN - SHARED):(i + 1) * (GENOME_LEN - SHARED)]
    return g, go, fam


def make_reads(g, go, seed):
    """(id line, sequence) in input order"""
    rng = np.random.default_rng(seed)
    acgt = np.frombuffer(b"ACGT", np.uint8)
    out = []
    for i in range(N_READS):
        n = int(rng.integers(1000, 3001))
        if rng.random() < 0.05:
            seq = acgt[rng.integers(0, 4, n)]
        else:
            j = int(rng.integers(0, go.size - 1))
            a = int(go[j]) + int(rng.integers(0, GENOME_LEN - n + 1))
            seq = g[a:a + n].copy()
            pos = np.flatnonzero(rng.random(n) < 0.01)                # 1 % substitutions, always another base
            code = np.searchsorted(acgt, seq[pos])
            seq[pos] = acgt[(code + rng.integers(1, 4, pos.size)) & 3]
        out.append((f"read_{(i * 7919) % N_READS} runid=ab{i} ch={i % 512}", bytes(seq)))
    return out


def write_fasta(path, reads):
    path.write_bytes(b"".join(b">" + i.encode() + b"\n" + s + b"\n" for i, s in reads))


@pytest.fixture(scope="module")
def world(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("search_profile")
    g, go, fam = make_genomes()
    gdir = tmp / "genomes"
    gdir.mkdir()
    lines = []
    for i in range(N_FAMILIES * FAMILY):
        f = int(fam[i])
        acc = f"GCF_{900000 + (i * 13) % 40:09d}.1"                   # accession order differs from user bin order
        stem = f"{acc}_ASM{i}v1_genomic"
        (gdir / (stem + ".fna")).write_bytes(b">chr1 strain\n" + bytes(g[int(go[i]):int(go[i + 1])]) + b"\n")
        names = f"k__Bacteria;p__Phylum{f % 2};c__Class{f % 3};o__Order{f % 5};f__Family{f};g__Genus{f};s__Genus{f} species{i}"
        ids = f"2;{20 + f % 2};{30 + f % 3};{40 + f % 5};{500 + f};{6000 + f};{70000 + i}"
        lines.append("\t".join([acc, str(70000 + i), f"ftp://host/genomes/{acc}/{stem}", f"Genus{f} species{i}", names, ids]))
    tax = tmp / "tax.tsv"
    tax.write_text("\n".join(lines) + "\n")
    idx = tmp / "idx.hixf"
    cp = run(["build", "--input-file", tax, "--input-sequence-dir", gdir, "--output-filename", idx, "--threads", "4", "--use-syncmer",
              "--kmer-size", "22", "--syncmer-size", "12"], timeout=600)
    assert cp.returncode == 0, cp.stdout + cp.stderr
    reads = make_reads(g, go, seed=22)
    assert [i for i, _ in reads] != sorted(i for i, _ in reads) and min(len(s) for _, s in reads) >= 1000      # none shorter than k
    fa = tmp / "reads.fa"
    write_fasta(fa, reads)
    # ---- the yardstick: search -> TSV -> profile
    tsv = tmp / "plain.tsv"
    cp = run(["search", "--index-file", idx, "--query-file", fa, "--output-file", tsv, "--threads", "4", "--batch-reads", "512"])
    assert cp.returncode == 0, cp.stdout + cp.stderr
    w = dict(tmp=tmp, idx=idx, fa=fa, tsv=tsv, reads=reads)
    w["yard"] = profile_of(w, tsv, tmp / "yard")
    w["yard_min0"] = profile_of(w, tsv, tmp / "yard_min0", ["--min-abundance", "0", "--em-steps", "1"])
    return w


def files_of(d):
    return {k: open(os.path.join(str(d), k), "rb").read() for k in ("cami", "seq", "bin")}


def profile_args(d):
    os.makedirs(str(d), exist_ok=True)
    return ["--cami-report-file", os.path.join(str(d), "cami"), "--seq-abundance-file", os.path.join(str(d), "seq"), "--binning-file",
            os.path.join(str(d), "bin"), "--sample-id", "SAMPLE"]


def profile_of(w, tsv, d, extra=()):
    cp = run(["profile", "--search-file", tsv] + profile_args(d) + list(extra))
    assert cp.returncode == 0, cp.stderr
    return dict(files=files_of(d), em_line=EM_LINE.search(cp.stdout).group(0))


def fused(w, d, extra=(), batch="512", query=None):
    cp = run(["search", "--index-file", w["idx"], "--query-file", query or w["fa"], "--threads", "4", "--batch-reads", batch] + profile_args(d) + list(extra))
    return cp


def check_fused(cp, d, yard):
    assert cp.returncode == 0, cp.stdout + cp.stderr
    assert EM_LINE.search(cp.stdout).group(0) == yard["em_line"]
    assert "taxor search (profile): 3000 reads" in cp.stderr, cp.stderr            # the stage timing line
    got = files_of(d)
    for k in ("cami", "seq", "bin"):
        assert got[k] == yard["files"][k], (k, got[k].decode()[:800], yard["files"][k].decode()[:800])


def test_yardstick_exercises_the_pipeline(world):
    """the two-step route's own outputs: enough multi-line reads, '-' reads, binning entries, species rows and EM steps for the
    comparison to mean something"""
    per_read, miss = {}, 0
    for line in open(world["tsv"], "rb").read().split(b"\n")[1:]:
        if line:
            f = line.split(b"\t")
            per_read[f[0]] = per_read.get(f[0], 0) + 1
            miss += f[1] == b"-"
    multi = sum(1 for n in per_read.values() if n >= 2)
    y = world["yard"]
    binning = [l for l in y["files"]["bin"].split(b"\n") if l and not l.startswith(b"@")]
    species = [l for l in y["files"]["cami"].split(b"\n") if l.split(b"\t")[1:2] == [b"species"]]
    steps = int(y["em_line"].rsplit(" ", 1)[1])
    print(f"reads {len(per_read)}, two or more lines {multi}, '-' reads {miss}, binning entries {len(binning)}, species rows {len(species)}, EM steps {steps}")
    assert len(per_read) == N_READS
    assert multi >= 100 and miss >= 50 and len(binning) >= 2000 and len(species) >= 5 and steps >= 2


def test_fused_without_tsv_is_byte_identical(world):
    d = world["tmp"] / "fused"
    cp = fused(world, d)
    check_fused(cp, d, world["yard"])
    assert sorted(os.listdir(str(d))) == ["bin", "cami", "seq"]                    # and no TSV anywhere


def test_fused_with_tsv_writes_the_plain_tsv_too(world):
    d = world["tmp"] / "fused_tsv"
    out = world["tmp"] / "fused.tsv"
    cp = fused(world, d, ["--output-file", str(out)])
    check_fused(cp, d, world["yard"])
    assert out.read_bytes() == world["tsv"].read_bytes()


def test_batch_size_does_not_change_the_files(world):
    d = world["tmp"] / "fused_big"
    cp = fused(world, d, batch="100000")
    check_fused(cp, d, world["yard"])


def test_min_abundance_and_em_steps_match_the_yardstick(world):
    d = world["tmp"] / "fused_min0"
    cp = fused(world, d, ["--min-abundance", "0", "--em-steps", "1"])
    check_fused(cp, d, world["yard_min0"])
    assert world["yard_min0"]["files"]["cami"] != world["yard"]["files"]["cami"]  # the options do something


def test_duplicate_read_id_is_refused_by_name(world):
    reads = list(world["reads"][:700])
    reads[650] = ("read_" + reads[3][0].split(" ")[0][5:] + " another=description", reads[650][1])   # the same id before its first space
    fa = world["tmp"] / "dup.fa"
    write_fasta(fa, reads)
    d = world["tmp"] / "dup"
    cp = fused(world, d, query=fa)
    assert cp.returncode == 255, (cp.returncode, cp.stderr)
    assert "[TAXOR SEARCH ERROR] read id " + reads[3][0].split(" ")[0] + " occurs twice" in cp.stderr, cp.stderr
    assert not os.path.exists(os.path.join(str(d), "cami")) and not os.path.exists(os.path.join(str(d), "bin"))
