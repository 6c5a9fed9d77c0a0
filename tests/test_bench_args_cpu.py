"""bench.py's command line and --dump-outputs writer, without a GPU: a plain run measures the headline alone (every extra leg is
behind --full), --steps is validated, and an output larger than the cap is written as a seeded sample of whole reads."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import bench  # noqa: E402

EXTRAS = ("no_unpruned", "no_ceiling", "no_e04", "no_dropin", "no_cpu_baseline", "no_layouts")


def test_plain_run_switches_every_extra_off():
    a = bench.parse_args(["--gpus", "1", "--steps", "5", "--warmup", "2"])
    assert not a.full and a.steps == 5 and a.warmup == 2 and a.traffic == "none"
    assert all(getattr(a, f) for f in EXTRAS)


def test_full_run_keeps_todays_defaults_and_switches():
    a = bench.parse_args(["--full"])
    assert a.full and a.traffic == "live" and not any(getattr(a, f) for f in EXTRAS)
    b = bench.parse_args(["--full", "--no-layouts", "--traffic", "none"])
    assert b.no_layouts and b.traffic == "none" and not b.no_unpruned


@pytest.mark.parametrize("argv", [["--steps", "0"], ["--warmup", "-1"]])
def test_steps_must_be_timed(argv, capsys):
    with pytest.raises(SystemExit):
        bench.parse_args(argv)


def _csr(n, seed):
    rng = np.random.default_rng(seed)
    per = rng.integers(0, 9, n)
    off = np.zeros(n + 1, np.int64)
    np.cumsum(per, out=off[1:])
    return off, rng.integers(0, 5000, int(off[-1])), rng.integers(1, 900, int(off[-1])).astype(np.uint32), rng.integers(0, 1000, n).astype(np.uint32)


def _load(d):
    return {n: np.load(os.path.join(d, f"{n}.npy")) for n in ("read_index", "read_off", "user_bin", "count", "n_hashes")}


def test_dump_writes_the_whole_csr_as_float64(tmp_path):
    off, ub, cnt, nh = _csr(300, 1)
    bench.dump_search_outputs(str(tmp_path), off, ub, cnt, nh)
    o = _load(tmp_path)
    assert all(a.dtype == np.float64 for a in o.values())
    assert np.array_equal(o["read_index"], np.arange(300)) and np.array_equal(o["read_off"], off)
    assert np.array_equal(o["user_bin"], ub) and np.array_equal(o["count"], cnt) and np.array_equal(o["n_hashes"], nh)


def test_dump_over_the_cap_is_a_fixed_sample_of_whole_reads(tmp_path, monkeypatch):
    off, ub, cnt, nh = _csr(5000, 2)
    monkeypatch.setattr(bench, "DUMP_CAP_BYTES", 64 << 10)
    bench.dump_search_outputs(str(tmp_path / "a"), off, ub, cnt, nh)
    bench.dump_search_outputs(str(tmp_path / "b"), off, ub, cnt, nh)
    a, b = _load(tmp_path / "a"), _load(tmp_path / "b")
    assert sum(x.nbytes for x in a.values()) <= 64 << 10
    for n in a:
        assert np.array_equal(a[n], b[n]), n
    ids = a["read_index"].astype(np.int64)
    assert 0 < ids.size < 5000 and np.all(np.diff(ids) > 0)
    for j, r in enumerate(ids[:200]):              # every sampled read carries all of its own tuples
        lo, hi = int(a["read_off"][j]), int(a["read_off"][j + 1])
        assert np.array_equal(a["user_bin"][lo:hi], ub[off[r]:off[r + 1]]) and np.array_equal(a["count"][lo:hi], cnt[off[r]:off[r + 1]])
        assert a["n_hashes"][j] == nh[r]
