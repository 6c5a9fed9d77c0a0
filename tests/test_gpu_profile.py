"""`taxor profile` on the device (taxor_amd/csrc/profile.hip, profile_cmd.h).

1. Every case of tests/golden/profile/ (tests/golden/make_profile_golden.py: what the reference's own taxor_profile.cpp writes
   for seeded search TSVs) comes out byte for byte: CAMI profile, sequence abundances, binning file, the EM step count.
2. A second run writes the same files.
3. The two inputs the reference leaves undefined are refused by name.
4. Through the ctypes binding, on seeded random CSRs: the survivor sets of the three rounds, the pair table, the found taxa and
   every iteration's ref_nts equal a plain-Python restatement of src/main/taxor_profile.cpp (restate(), below).

Mutants of the new code and the test that fails on them: `>` for `>=` in the best-match rule (k_pf_em) -- the golden case `ties`
and test_stages_against_restatement (ties under the uniform prior); the FIRST instead of the LAST match with a prior erased -- the
golden cases `many`, `ties` and the per-iteration ref_nts of test_stages_against_restatement; `>` for `>=` in round 2's ratio test or
`> 3` for `>= 3` unique reads (k_pf_accept) -- test_round2_boundaries.  Double instead of float in that ratio changes a result only
beyond 145 000 unique reads on one reference (see test_round2_boundaries) and has no test here.  Every input of this file fits
one pass of the kernels' grid-stride loops (8192 reads, 524 288 references) and one range of the parser, so four more pass it
and fail in tests/test_gpu_profile_scale.py: `acc_all = 0` moved inside the loop of k_pf_em, `return` for `continue` in
k_pf_filter -- every parameter of test_stages_across_grid_passes; `break` for the loop step of k_pf_hist -- only its parameter
seed21-contended, through the planted reference with exactly three unique reads (the random CSR alone decides round 2 too far
from its edge to notice lost counts); in profile_command `first` not advanced, so that every range starts at line 0 --
test_golden_case_padded_across_parser_ranges (and the four refusals of tests/test_profile_args_cpu.py that name a line of a
later range).  The failures as seen are in docs/EXPERIMENTS.md section 14."""
import json
import math
import os
import random
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TAXOR = os.path.join(ROOT, "taxor_amd", "taxor")
GOLDEN = os.path.join(ROOT, "tests", "golden", "profile")
CASES = json.load(open(os.path.join(GOLDEN, "cases.json")))
HEADER = "#QUERY_NAME\tACCESSION\tREFERENCE_NAME\tTAXID\tREF_LEN\tQUERY_LEN\tQHASH_COUNT\tQHASH_MATCH\tTAX_STR\tTAX_ID_STR\n"


def run_cli(tsv, out_dir, sample_id, extra=()):
    os.makedirs(out_dir, exist_ok=True)
    cmd = [TAXOR, "profile", "--search-file", str(tsv), "--cami-report-file", os.path.join(out_dir, "cami"), "--seq-abundance-file",
           os.path.join(out_dir, "seq"), "--binning-file", os.path.join(out_dir, "bin"), "--sample-id", sample_id] + list(extra)
    return subprocess.run(cmd, capture_output=True, text=True, timeout=120)


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_golden_case_is_byte_identical(tmp_path, case):
    cp = run_cli(os.path.join(GOLDEN, case["tsv"]), str(tmp_path), case["sample_id"], case["args"])
    assert cp.returncode == 0, cp.stderr
    assert cp.stdout.strip().splitlines() == [case["em_steps_line"]], cp.stdout          # no other chatter on stdout
    for kind in ("bin", "seq", "cami"):
        got = open(os.path.join(str(tmp_path), kind), "rb").read()
        want = open(os.path.join(GOLDEN, f"{case['name']}.{kind}"), "rb").read()
        assert got == want, (case["name"], kind, got.decode()[:600], want.decode()[:600])


def test_second_run_is_identical_and_empty_seq_file_is_not_written(tmp_path):
    case = next(c for c in CASES if c["name"] == "many")
    tsv = os.path.join(GOLDEN, case["tsv"])
    a, b = run_cli(tsv, str(tmp_path / "a"), "S"), run_cli(tsv, str(tmp_path / "b"), "S")
    assert a.returncode == 0 and b.returncode == 0, (a.stderr, b.stderr)
    for kind in ("bin", "seq", "cami"):
        assert open(tmp_path / "a" / kind, "rb").read() == open(tmp_path / "b" / kind, "rb").read()
    os.makedirs(tmp_path / "c")
    cp = subprocess.run([TAXOR, "profile", "--search-file", tsv, "--cami-report-file", str(tmp_path / "c" / "cami"), "--binning-file",
                         str(tmp_path / "c" / "bin"), "--sample-id", "S", "--seq-abundance-file", ""], capture_output=True, text=True, timeout=120)
    assert cp.returncode == 0, cp.stderr
    assert sorted(os.listdir(tmp_path / "c")) == ["bin", "cami"]
    assert open(tmp_path / "c" / "cami", "rb").read() == open(tmp_path / "a" / "cami", "rb").read()


def line(read, acc, qlen=3000, count=250, match=100):
    return f"{read}\t{acc}\tn\t1{acc}\t1000000\t{qlen}\t{count}\t{match}\tk__B;s__{acc}\t2;1{acc}\n"


def test_explained_by_cycle_is_refused(tmp_path):
    """three references in the same 40 reads: B and C are explained by A, A by B; C's chain runs into the pair A <-> B and the
    reference's `while (found)` never ends"""
    tsv = tmp_path / "cycle.tsv"
    tsv.write_text(HEADER + "".join(line(f"r{i}", a) for i in range(40) for a in ("A", "B", "C")))
    cp = run_cli(tsv, str(tmp_path / "o"), "S")
    assert cp.returncode == 255, (cp.returncode, cp.stderr)
    assert cp.stderr.startswith("[TAXOR PROFILE ERROR] ") and "cycle" in cp.stderr, cp.stderr


def test_multi_match_read_without_prior_is_refused(tmp_path):
    """A <-> B and A2 <-> B2 explain each other (equal counts, all but one read shared), so none of the four has a prior; the
    read [A, A2] is renamed to [B, B2] and the reference erases a default-constructed iterator in it"""
    text = HEADER
    for i in range(40):
        text += line(f"r{i}", "A") + line(f"r{i}", "B") + line(f"s{i}", "A2") + line(f"s{i}", "B2")
    text += line("t1", "A") + line("t1", "A2") + line("t2", "B") + line("t2", "B2")
    tsv = tmp_path / "noprior.tsv"
    tsv.write_text(text)
    cp = run_cli(tsv, str(tmp_path / "o"), "S")
    assert cp.returncode == 255, (cp.returncode, cp.stderr)
    assert cp.stderr.startswith("[TAXOR PROFILE ERROR] ") and "prior" in cp.stderr, cp.stderr


# ---- src/main/taxor_profile.cpp restated over the CSR (match positions stay, an alive list per read) ---------------------------
def restate(off, ref, ref_len, hm, qlen, hc, F, em_steps):
    R, M = len(off) - 1, len(ref)
    ref = list(ref)
    alive = [1] * M

    def rd(r):
        return [i for i in range(off[r], off[r + 1]) if alive[i]]

    def keep_only(flag):                                           # remove_matches_to_nonunique_refs (:186-229)
        for r in range(R):
            L = rd(r)
            if len(L) > 1 and any(flag[ref[i]] for i in L):
                for i in L:
                    if not flag[ref[i]]:
                        alive[i] = 0

    flag = [0] * F
    for r in range(R):
        L = rd(r)
        if len(L) == 1 and ref[L[0]] >= 0:
            flag[ref[L[0]]] = 1
    keep_only(flag)
    out = dict(alive1=alive[:])
    uniq, amb = [0] * F, [0] * F
    for r in range(R):
        L = rd(r)
        if len(L) == 1:
            if ref[L[0]] >= 0:
                uniq[ref[L[0]]] += 1
        else:
            for i in L:
                amb[ref[i]] += 1
    keep_only([u >= 3 and np.float32(u) / np.float32(u + a) >= np.float32(0.01) for u, a in zip(uniq, amb)])
    out["alive2"] = alive[:]
    uniq, all_, first, pairs = [0] * F, [0] * F, [None] * F, {}
    for r in range(R):
        L = rd(r)
        if len(L) == 1:
            if ref[L[0]] >= 0:
                x = ref[L[0]]
                uniq[x] += 1
                all_[x] += 1
                first[x] = L[0] if first[x] is None else first[x]
        else:
            for i in L:
                all_[ref[i]] += 1
                first[ref[i]] = i if first[ref[i]] is None else first[ref[i]]
            for i in L:
                for j in L:
                    if ref[i] != ref[j]:
                        pairs[(ref[i], ref[j])] = pairs.get((ref[i], ref[j]), 0) + 1
    out["pairs"] = pairs
    expl = {}
    for (a, b) in sorted(pairs):                                   # :351-383, the first insert wins
        if uniq[a] > uniq[b] or all_[a] > all_[b]:
            if all_[a] - pairs[(a, b)] < int(0.05 * float(all_[a])):
                expl.setdefault(a, b)
        elif all_[b] - pairs[(b, a)] < int(0.05 * float(all_[b])):
            expl.setdefault(b, a)
    found, passes = True, 0
    while found:                                                   # :385-399
        found, passes = False, passes + 1
        assert passes < 1000, "explained-by cycle: not an input for this test"
        for x in sorted(expl):
            if expl[x] in expl and x != expl[expl[x]]:
                expl[x] = expl[expl[x]]
                found = True
    taxa_len = {x: ref_len[first[x]] for x in range(F) if all_[x] > 0}
    for r in range(R):                                             # :405-451
        L = rd(r)
        if len(L) < 2:
            continue
        ids = {ref[i] for i in L}
        for i in L:
            if ref[i] in expl:
                if expl[ref[i]] in ids:
                    alive[i] = 0
                else:
                    ref[i] = expl[ref[i]]
    taxa = sorted(x for x in taxa_len if x not in expl)
    out.update(alive3=alive[:], ref3=ref[:], taxa=taxa, taxa_len=taxa_len, expl=expl)
    prior = {x: math.log(1.0 / float(len(taxa))) for x in taxa}
    cond, step, iters, unclassified = -1.7976931348623157e308, 0, [], 0.0
    while step < em_steps:                                         # :650-731
        new_cond, nts, all_nts, un_nts, best_of = 0.0, {x: 0 for x in taxa}, 0, 0, {}
        for r in range(R):
            L = rd(r)
            if not L:
                continue
            best = []
            if len(L) == 1:
                if ref[L[0]] < 0:
                    best = [L[0]]
                elif ref[L[0]] in prior:
                    new_cond += 0.0 + prior[ref[L[0]]]
                    best = [L[0]]
            else:
                s = 0.0
                for i in L:
                    s += float(hm[i]) / float(hc[r])
                lik = {}
                for i in L:
                    lik.setdefault(ref[i], (math.log(float(hm[i])) - math.log(float(hc[r]))) - math.log(s))
                mx, worst = -1.7976931348623157e308, None
                for i in L:
                    if ref[i] not in prior:
                        continue
                    post = lik[ref[i]] + prior[ref[i]]
                    new_cond += post
                    if post >= mx:
                        if post > mx:
                            mx, best = post, []
                        best.append(i)
                    worst = i                                      # min_post is never lowered (:709)
                assert worst is not None, "a multi-match read without a prior: not an input for this test"
                alive[worst] = 0
            best_of[r] = best
        for r, best in best_of.items():                            # update_log_prior_probabilities (:515-566)
            if not best:
                continue
            all_nts += qlen[r]
            if ref[best[0]] < 0:
                un_nts += qlen[r]
                continue
            for i in best:
                nts[ref[i]] += qlen[r]
        for x in taxa:
            prior[x] = math.log(float(nts[x]) + 0.000000000001) - math.log(float(all_nts))
        unclassified = math.log(float(un_nts) + 0.000000000001) - math.log(float(all_nts))
        iters.append([nts.get(x, 0) for x in range(F)])
        best_at = {i for b in best_of.values() for i in b}
        out["best"] = [1 if i in best_at else 0 for i in range(M)]
        if new_cond - cond < abs(math.log(0.0001)):
            break
        cond, step = new_cond, step + 1
    out.update(iter_ref_nts=iters, steps=step, alive=alive[:], prior=prior, unclassified=unclassified, all_nts=all_nts, un_nts=un_nts)
    return out


def random_csr(seed, F, sizes, n_single, n_miss, extra=()):
    """reads of the given match counts among n_single single-match reads and n_miss '-' reads, shuffled; a planted pair: reference
    1 shares all but one of its reads with reference 0 (explained, erased where 0 is in the read, renamed where it is not).
    extra: further reads, as lists of reference ids, that go into the shuffle with the others"""
    rng = random.Random(seed)
    reads = [rng.sample(range(F), m) if m <= F else [rng.randrange(F) for _ in range(m)] for m in sizes]
    reads += [[rng.randrange(min(F, 50))] for _ in range(n_single)] + [[-1] for _ in range(n_miss)]
    if F > 100:
        reads += [[F - 1, F - 2] if i % 2 else [F - 2, F - 1, F - 3] for i in range(120)] + [[F - 1, F - 4], [F - 5, F - 1, F - 1]]
    reads += [list(L) for L in extra]
    rng.shuffle(reads)
    off, ref, hm, qlen, hc = [0], [], [], [], []
    for L in reads:
        q = rng.randrange(500, 9000)
        c = q // 10
        ties = rng.random() < 0.3
        for x in L:
            ref.append(x)
            hm.append(c // 2 if ties else rng.randrange(c // 4, c) + 1)
        off.append(len(ref))
        qlen.append(q)
        hc.append(0 if L == [-1] else c)
    ref_len = [1000000 + 1000 * (x % 97) if x >= 0 else 0 for x in ref]
    return off, ref, ref_len, hm, qlen, hc


def check_against_restatement(csr, F, em_steps):
    from taxor_amd.profile import run_profile

    off, ref, ref_len, hm, qlen, hc = csr
    want = restate(off, ref, ref_len, hm, qlen, hc, F, em_steps)
    got = run_profile(off, ref, ref_len, hm, qlen, hc, F, em_steps=em_steps)
    assert got["alive_round1"].tolist() == want["alive1"]
    assert got["alive_round2"].tolist() == want["alive2"]
    assert got["alive_round3"].tolist() == want["alive3"]
    a3 = np.array(want["alive3"], bool)
    assert got["ref"][a3].tolist() == np.array(want["ref3"])[a3].tolist()
    pairs = {(int(k) >> 32, int(k) & 0xFFFFFFFF): int(c) for k, c in zip(got["pair_key"], got["pair_count"])}
    assert pairs == want["pairs"]
    assert {x: int(got["explained_by"][x]) for x in range(F) if got["explained_by"][x] >= 0} == want["expl"]
    assert np.flatnonzero(got["has_prior"]).tolist() == want["taxa"]
    assert {x: int(got["taxa_len"][x]) for x in want["taxa_len"]} == want["taxa_len"]
    assert got["em_steps_needed"] == want["steps"] and got["em_iterations"] == len(want["iter_ref_nts"])
    assert got["iter_ref_nts"].tolist() == want["iter_ref_nts"]
    assert got["alive"].tolist() == want["alive"]
    assert got["best"].tolist() == want["best"]
    assert (got["all_nts"], got["unclassified_nts"]) == (want["all_nts"], want["un_nts"])
    assert [got["log_prior"][x] for x in want["taxa"]] == [want["prior"][x] for x in want["taxa"]]      # bit for bit
    assert got["log_unclassified"] == want["unclassified"]
    return got, want


def test_stages_against_restatement():
    """5000 references; reads of 1, 2, 63, 64, 65 and 300 matches (either side of a wave), 1293 reads in all (not a multiple of
    the four reads a block takes per pass), ties in the match counts, a planted explained reference"""
    sizes = [2] * 40 + [3] * 20 + [63, 64, 65, 300, 63, 64, 65, 300]
    got, want = check_against_restatement(random_csr(11, 5000, sizes, 1093, 10), 5000, 6)
    assert len(want["expl"]) >= 1 and got["em_iterations"] >= 2
    assert any(sum(1 for i in range(1, 5000) if row[i]) > 3 for row in want["iter_ref_nts"])


def test_one_reference():
    """a single reference: every read is unique or a miss, the pair table stays empty, one EM step"""
    got, _ = check_against_restatement(random_csr(12, 1, [], 37, 6), 1, 5)
    assert got["pair_key"].size == 0 and got["has_prior"].tolist() == [1]


def test_pair_table_at_its_sizing_bound():
    """no two reads share a reference, so every ordered pair inside a read is a key of its own: the table holds exactly
    sum m (m - 1) keys, the number it was sized from"""
    rng = random.Random(5)
    sizes = [2, 3, 5, 64, 65, 7, 2, 130, 3, 4, 66]
    off, ref, nxt = [0], [], 0
    for m in sizes:
        ids = list(range(nxt, nxt + m))
        rng.shuffle(ids)
        ref += ids
        nxt += m
        off.append(len(ref))
    F = nxt
    qlen = [1000 + 7 * i for i in range(len(sizes))]
    hc = [q // 10 for q in qlen]
    hm = [hc[r] // 2 + (i % 5) for r in range(len(sizes)) for i in range(sizes[r])]
    csr = (off, ref, [2000000] * len(ref), hm, qlen, hc)
    got, want = check_against_restatement(csr, F, 3)
    bound = sum(m * (m - 1) for m in sizes)
    assert got["pair_key"].size == bound == len(want["pairs"]) and set(got["pair_count"].tolist()) == {1}
    assert got["pair_slots"] >= 2 * bound and got["pair_slots"] < 4 * bound + 64


@pytest.mark.parametrize("u,amb,accepted", [(3, 297, True), (3, 298, False), (2, 0, False), (4, 396, True), (4, 397, False)])
def test_round2_boundaries(u, amb, accepted):
    """unique >= 3 and (float)unique / (float)(unique + ambiguous) >= 0.01f at their edges: 3 / 300 and 4 / 400 round to 0.01f
    itself and pass, one more ambiguous mapping fails, two unique reads fail whatever the ratio.  (Single against double precision
    differs only where the quotient lies within half a float ulp below 0.01f: more than 145 000 unique reads on one reference.)"""
    # reference 0: u unique reads and amb reads shared with reference 1, which has 50 unique reads and is accepted
    reads = [[0]] * u + [[0, 1]] * amb + [[1]] * 50
    off, ref = [0], []
    for L in reads:
        ref += L
        off.append(len(ref))
    n = len(reads)
    csr = (off, ref, [1000000] * len(ref), [60] * len(ref), [2000] * n, [100] * n)
    got, want = check_against_restatement(csr, 2, 2)
    shared = [i for r in range(u, u + amb) for i in range(off[r], off[r + 1]) if ref[i] == 0]
    assert all(got["alive_round2"][i] == (1 if accepted else 0) for i in shared)
