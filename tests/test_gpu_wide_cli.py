"""`taxor build --use-syncmer --kmer-size 28 --syncmer-size 20` and `taxor search` on the built index: six genomes of 120 kb, the
index's keys are the oracle's, the search TSV equals the oracle-derived text byte for byte -- parsed on the host and with
--device-parse -- and a build streamed through the host key store (--device-key-budget 1) writes the same file byte for byte."""
import os
import re
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
N, K, S, T = 6, 28, 20, 4                  # t = (k - s + 1) / 2 in integer division (taxor_build.cpp:509-510)
SCHEME = ["--use-syncmer", "--kmer-size", str(K), "--syncmer-size", str(S)]


@pytest.fixture(scope="module")
def world(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("wide_cli")
    g, go = synth.random_genomes(N, 120000, seed=41)
    genomes = [bytes(g[int(go[i]):int(go[i + 1])]) for i in range(N)]
    d = tmp / "g"
    d.mkdir()
    lines, records = [], []
    for i, seq in enumerate(genomes):
        acc = f"GCF_{300000 + i:09d}.1"
        stem = f"{acc}_ASM{i}v1_genomic"
        recs = [seq] if i % 2 else [seq[:len(seq) // 2], seq[len(seq) // 2:]]
        (d / (stem + ".fna")).write_bytes(b"".join(b">r%d\n" % j + b"".join(r[p:p + 80] + b"\n" for p in range(0, len(r), 80)) for j, r in enumerate(recs)))
        records.append(recs)
        lines.append("\t".join([acc, str(9000 + i), f"ftp://host/genomes/{acc}/{stem}", f"Organism {i}", f"k__B;s__Organism {i}", f"2;{9000 + i}"]))
    tsv = tmp / "tax.tsv"
    tsv.write_text("\n".join(lines) + "\n")
    bases, offs, origin = synth.synth_reads(g, go, 200, 1500, error_rate=0.0, frac_random=0.1, seed=42)
    reads = [bytes(bases[int(offs[i]):int(offs[i + 1])]) for i in range(200)]
    ids = [f"read_{i}" for i in range(200)]
    fa = tmp / "reads.fa"
    fa.write_bytes(b"".join(b">" + i.encode() + b"\n" + r + b"\n" for i, r in zip(ids, reads)))
    out = tmp / "resident.hixf"
    cp = build(tsv, d, out)
    assert path_line(cp)[:2] == ("resident", 1)
    return dict(tmp=tmp, tsv=tsv, d=d, fa=fa, index=out, records=records, reads=reads, ids=ids, origin=origin)


def build(tsv, d, out, *extra):
    cp = subprocess.run([TAXOR, "build", "--input-file", str(tsv), "--input-sequence-dir", str(d), "--output-filename", str(out), "--threads", "4",
                         *SCHEME, *extra], capture_output=True, text=True, timeout=600)
    assert cp.returncode == 0, cp.stdout + cp.stderr
    assert cp.stdout == "checking input ... done!\nparsing taxonomy input files ... done!\ncreating HIXF layout ... done!\nbuilding HIXF index ... done!\n"
    return cp


def path_line(cp):
    m = re.search(r"path (\w+): (\d+) waves, (\d+) groups, (\d+) bin ranges, (\d+) restarts", cp.stderr)
    assert m, cp.stderr
    return (m.group(1),) + tuple(int(x) for x in m.groups()[1:])


def search(w, out, *extra):
    cp = subprocess.run([TAXOR, "search", "--index-file", str(w["index"]), "--query-file", str(w["fa"]), "--output-file", str(out), "--threads", "4", *extra],
                        capture_output=True, text=True, timeout=300)
    assert cp.returncode == 0, cp.stderr
    return open(out).read()


def expected_text(w):
    if "want" not in w:
        hf = HixfFile(w["index"])
        assert (hf.k, hf.s, hf.t, hf.use_syncmer, hf.scaling) == (K, S, T, True, 1)
        h = orc.Hixf(hf.ixfs, [f["next_ixf"] for f in hf.ixfs], [f["fname_idx"] for f in hf.ixfs])
        # every genome's oracle keys are found in its user bin's run
        for u, recs in enumerate(w["records"]):
            keys = np.unique(np.concatenate([orc.seq_to_syncmers(r, K, S, T) for r in recs]))
            i = next(i for i, f in enumerate(hf.ixfs) if (f["fname_idx"] == u).any())
            run = np.flatnonzero(hf.ixfs[i]["fname_idx"] == u)
            assert keys.size > 10000 and h.ixf_bulk_count(i, keys)[run].sum() >= keys.size, u
        B = np.frombuffer(b"".join(w["reads"]), dtype=np.uint8)
        O = np.cumsum([0] + [len(r) for r in w["reads"]]).astype(np.uint64)
        nh, off, ub, cnt, _ = h.search_batch(B, O, k=K, s=S, t=T, threads=4)
        want = HEADER
        for i, rid in enumerate(w["ids"]):
            tup = [(int(a), int(b)) for a, b in zip(ub[int(off[i]):int(off[i + 1])], cnt[int(off[i]):int(off[i + 1])])]
            want += expected_lines(hf.species, rid, len(w["reads"][i]), int(nh[i]), tup)
        hf.close()
        assert ub.size >= sum(1 for o in w["origin"] if o >= 0)            # error-free reads report their source genome
        w["want"] = want
    return w["want"]


def test_build_then_search_equals_the_oracle(world):
    assert search(world, world["tmp"] / "host.tsv") == expected_text(world)


def test_device_parse_gives_the_same_text(world):
    assert search(world, world["tmp"] / "device.tsv", "--device-parse") == expected_text(world)


def test_streamed_build_is_byte_identical(world):
    out = world["tmp"] / "stream.hixf"
    cp = build(world["tsv"], world["d"], out, "--device-key-budget", "1")
    kind, waves, _, _, _ = path_line(cp)
    assert kind == "stream" and waves >= 2, cp.stderr
    assert out.read_bytes() == world["index"].read_bytes()


def test_profile_feed_equals_profile_of_the_tsv(world):
    """search results fed to the profile on the device (no TSV in between) write the files `taxor profile` writes from the TSV"""
    tsv = world["tmp"] / "for_profile.tsv"
    search(world, tsv)

    def args(d):
        os.makedirs(str(d), exist_ok=True)
        return ["--cami-report-file", os.path.join(str(d), "cami"), "--seq-abundance-file", os.path.join(str(d), "seq"), "--binning-file",
                os.path.join(str(d), "bin"), "--sample-id", "SAMPLE"]

    a, b = world["tmp"] / "prof_tsv", world["tmp"] / "prof_fused"
    cp = subprocess.run([TAXOR, "profile", "--search-file", str(tsv)] + args(a), capture_output=True, text=True, timeout=300)
    assert cp.returncode == 0, cp.stderr
    cp = subprocess.run([TAXOR, "search", "--index-file", str(world["index"]), "--query-file", str(world["fa"]), "--threads", "4"] + args(b),
                        capture_output=True, text=True, timeout=300)
    assert cp.returncode == 0, cp.stdout + cp.stderr
    for k in ("cami", "seq", "bin"):
        got, want = open(os.path.join(str(b), k), "rb").read(), open(os.path.join(str(a), k), "rb").read()
        assert got == want and len(want) > 0, k
    assert open(os.path.join(str(a), "bin")).read().count("\n") > 100
