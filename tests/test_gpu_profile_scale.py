"""`taxor profile` past one grid pass and past one parser range (taxor_amd/csrc/profile.hip, profile_cmd.h).

The read kernels launch at most 2048 blocks of four waves, one read per wave: 8192 reads a pass, and a wave reaches a second read
only from the 8193rd on.  k_pf_accept takes one reference per thread, 2048 x 256 = 524 288 a pass.  The parser cuts the search file
into min(hardware threads, 16, bytes / 1 MiB + 1) ranges.  tests/test_gpu_profile.py stays below all three; here

1. the stages run over 17 677 reads (two full passes and a partial third) against the restatement of test_gpu_profile.py, once
   more with 5000 reads on one triple of references, whose six pair keys are then incremented from waves of every pass;
2. round 2's boundary cases lie on reference ids of the first pass of k_pf_accept, of its second pass and on the last id;
3. golden search files, padded in the two places the reference never reads until they span 2 and 16 ranges, give the golden
   outputs byte for byte."""
import os

import pytest

from tests import test_gpu_profile as tp
from tests.profile_padding import MIB, nominal_ranges, padded, reads_across

pytestmark = pytest.mark.gpu

PASS_READS = 2048 * 4                 # P_GRID_CAP blocks of PW waves
PASS_REFS = 2048 * 256                # P_GRID_CAP blocks of PB threads


# ---- 1. the read kernels' grid-stride loops -----------------------------------------------------------------------------------
def kinds_by_pass(off, ref):
    """{kind: set of passes (read index // 8192) in which a read of that kind lies}, from the CSR alone"""
    seen = {"multi": set(), "wide": set(), "miss": set()}
    for r in range(len(off) - 1):
        m = off[r + 1] - off[r]
        if m >= 2:
            seen["multi"].add(r // PASS_READS)
        if m >= 63:
            seen["wide"].add(r // PASS_READS)
        if m == 1 and ref[off[r]] < 0:
            seen["miss"].add(r // PASS_READS)
    return seen


@pytest.mark.parametrize("seed,contended", [(21, False), (22, False), (21, True)], ids=["seed21", "seed22", "seed21-contended"])
def test_stages_across_grid_passes(seed, contended):
    """test_stages_against_restatement's mix, ten times the multi-match reads, among enough single-match reads for 2 * 8192 + 1293
    reads: each of the first 1293 waves takes three reads, the others two, the last pass is partial.  Reads with several matches,
    with 63 or more, and '-' reads lie in every pass, so a kernel that left its loop after one read, returned where it should go
    on to the next read, or reset the EM's per-wave sums per read cannot give the restatement's survivors, counts and totals.
    Contended: 5000 more reads that all hold references 10, 20 and 30 (in three rotations), shuffled among the others -- each of
    the six ordered pairs is one key of the pair table, incremented at least 5000 times from waves in all passes.  Each of the
    three has about 337 unique reads (16 831 single-match reads over 50 references), more than 5 % of its reads, so none of
    them explains another; the restatement says so before the device is asked.
    The random part decides round 2 with a wide margin on every reference (about 337 unique reads or none), so k_pf_hist could
    lose most of its counts there unseen.  The contended variant therefore also holds a reference x that no other read names,
    with exactly three unique reads and 100 reads shared with y (50 unique reads): x passes round 2 only if all three are
    counted, and they do not all lie in the first pass."""
    sizes = [2] * 400 + [3] * 200 + [63, 64, 65, 300] * 6
    triple = (10, 20, 30)
    extra = []
    if contended:
        unused = sorted(set(range(50, 4990)) - set(tp.random_csr(seed, 5000, sizes, 16831, 100)[1]))
        x, y = unused[:2]
        extra = [[triple[(i + j) % 3] for j in range(3)] for i in range(5000)] + [[x]] * 3 + [[x, y]] * 100 + [[y]] * 50
    csr = tp.random_csr(seed, 5000, sizes, 16831, 100, extra)
    off, ref = csr[0], csr[1]
    n_reads = len(off) - 1
    assert n_reads == 2 * PASS_READS + 1293 + len(extra) and 2 * PASS_READS < n_reads < 3 * PASS_READS
    assert kinds_by_pass(off, ref) == {k: {0, 1, 2} for k in ("multi", "wide", "miss")}
    if contended:
        of_x = [r for r in range(n_reads) if x in ref[off[r]:off[r + 1]]]
        alone = [r for r in of_x if off[r + 1] - off[r] == 1]
        assert len(of_x) == 103 and len(alone) == 3 and {r // PASS_READS for r in alone} != {0}
    got, want = tp.check_against_restatement(csr, 5000, 6)
    assert len(want["expl"]) >= 1 and len(want["iter_ref_nts"]) >= 2 and want["un_nts"] > 0
    if contended:
        assert not any(r in want["expl"] for r in triple)
        assert all(want["pairs"][(a, b)] >= 5000 for a in triple for b in triple if a != b)
        assert all(want["alive2"][i] for r in of_x for i in range(off[r], off[r + 1]))      # x is accepted: 3 / 103 >= 0.01


# ---- 2. k_pf_accept's loop ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("swapped", [False, True], ids=["accepted-first", "rejected-first"])
def test_accept_beyond_one_grid_pass(swapped):
    """524 288 + 300 references, one more than a pass of k_pf_accept by 300.  test_round2_boundaries' construction -- u unique
    reads, amb reads shared with a partner of 50 unique reads -- with the accepted case (3, 297) and the rejected case (3, 298) on
    a pair of ids in each region: 0 and 255 (the first block of the first pass), 524 288 and 524 288 + 137 (the second pass),
    F - 2 and F - 1 (its end).  The second parameter exchanges the two cases, so every one of the six ids carries both."""
    F = PASS_REFS + 300
    pairs = [(0, 255), (PASS_REFS, PASS_REFS + 137), (F - 2, F - 1)]
    partner = [17, 18, PASS_REFS + 1, PASS_REFS + 299 - 20, F - 40, F - 41]
    cases = []                                                     # (reference, partner, amb, accepted)
    for k, (x, y) in enumerate(pairs):
        if swapped:
            x, y = y, x
        cases += [(x, partner[2 * k], 297, True), (y, partner[2 * k + 1], 298, False)]
    assert len({c[0] for c in cases} | {c[1] for c in cases}) == 12
    assert sum(c[0] < 256 for c in cases) == 2 and sum(c[0] >= PASS_REFS for c in cases) == 4 and any(c[0] == F - 1 for c in cases)
    off, ref, shared = [0], [], {}
    for x, y, amb, _ in cases:
        for L in [[x]] * 3 + [[x, y]] * amb + [[y]] * 50:
            if len(L) == 2:
                shared.setdefault(x, []).append(len(ref))          # the position of x's match in a shared read
            ref += L
            off.append(len(ref))
    n = len(off) - 1
    csr = (off, ref, [1000000] * len(ref), [60] * len(ref), [2000] * n, [100] * n)
    got, want = tp.check_against_restatement(csr, F, 2)
    for x, y, amb, accepted in cases:
        assert len(shared[x]) == amb and all(ref[i] == x for i in shared[x])
        assert all(got["alive_round2"][i] == (1 if accepted else 0) for i in shared[x]), (x, accepted)


# ---- 3. the parser's ranges ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("target,n_ranges", [(MIB + MIB // 2, 2), (15 * MIB + MIB // 2, 16)], ids=["2-ranges", "16-ranges"])
@pytest.mark.parametrize("name", ["many", "round2", "names", "ties"])
def test_golden_case_padded_across_parser_ranges(tmp_path, name, target, n_ranges):
    """The reference's parser (taxor_profile.cpp:110-160) never reads REFERENCE_NAME and cuts QUERY_NAME at its first space, so
    padded() changes the size of a search file and nothing the reference writes: the golden outputs of the unpadded file are
    the expectation.  This was confirmed once with the reference's own taxor_profile.cpp, in the build of
    tests/golden/make_profile_golden.py, on the eight padded files of this test: it wrote the golden .cami, .seq and .bin and the
    same EM step count for each.  In all four cases the order of the lines matters (the erased match of a read is its last with
    a prior, the first line of an accession fixes its taxonomy); `names` repeats read ids and carries descriptions of its own.
    Preconditions, from the padded bytes alone: the size gives the intended number of ranges, and for that number and every
    smaller one down to 2 some read has lines on both sides of a range start.  The parser takes no more ranges than the host
    has hardware threads, so `16-ranges` is parsed in 16 ranges only on a host with at least 16 of them (a smaller host parses
    the same file in as many ranges as it has threads, which the precondition covers); two are required."""
    case = next(c for c in tp.CASES if c["name"] == name)
    assert len(os.sched_getaffinity(0)) >= 2, "the parser takes one range per hardware thread: this test needs at least two CPUs"
    data = padded(open(os.path.join(tp.GOLDEN, case["tsv"]), "rb").read(), target, seed=f"{name}/{n_ranges}")
    assert nominal_ranges(len(data)) == n_ranges, len(data)
    for n in range(2, n_ranges + 1):
        assert reads_across(data, n), n
    tsv = tmp_path / "padded.tsv"
    tsv.write_bytes(data)
    cp = tp.run_cli(tsv, str(tmp_path / "o"), case["sample_id"], case["args"])
    assert cp.returncode == 0, cp.stderr
    assert cp.stdout.strip().splitlines() == [case["em_steps_line"]], cp.stdout
    for kind in ("bin", "seq", "cami"):
        got = open(tmp_path / "o" / kind, "rb").read()
        want = open(os.path.join(tp.GOLDEN, f"{name}.{kind}"), "rb").read()
        assert got == want, (name, kind, got.decode()[:600], want.decode()[:600])
