"""`taxor search --device-parse` on the command line: the switch is in the usage text and is accepted together with the other
options before any HIP call is made, so all of this runs without a device."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TAXOR = os.path.join(ROOT, "taxor_amd", "taxor")


def run(args):
    env = dict(os.environ, HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="")        # nothing below may need a device
    return subprocess.run([TAXOR, "search"] + args, capture_output=True, text=True, timeout=60, env=env)


def inputs(tmp_path):
    """an index file and a query file that EXIST (the index is empty: every case below ends when it is opened, or before)"""
    idx, q = tmp_path / "idx.hixf", tmp_path / "reads.fa"
    idx.write_bytes(b"")
    q.write_text(">r1\nACGT\n")
    return ["--index-file", str(idx), "--query-file", str(q)]


def test_usage_names_the_switch():
    for flag in ("--help", "--advanced-help"):
        cp = run([flag])
        assert cp.returncode == 0
        assert "--device-parse" in cp.stdout + cp.stderr


OTHERS = [[], ["--threads", "4", "--batch-reads", "16"], ["--gpu-list", "0,0"], ["--gpus", "2", "--gather", "none"], ["--sequential"],
          ["--percentage", "0.5", "--error-rate", "0.02"], ["--group-reads", "64"]]


@pytest.mark.parametrize("others", OTHERS, ids=[" ".join(o) or "alone" for o in OTHERS])
@pytest.mark.parametrize("first", [True, False])
def test_accepted_with_the_other_options_before_any_device_call(tmp_path, others, first):
    """the command gets past its command line and its input check and fails at the index file, which is empty"""
    sw = ["--device-parse"]
    a = inputs(tmp_path) + ["--output-file", str(tmp_path / "o.tsv")]
    cp = run(sw + a + others if first else a + others + sw)
    assert cp.returncode == 255, (cp.returncode, cp.stdout, cp.stderr)
    assert cp.stdout.startswith("checking input ... done!"), (cp.stdout, cp.stderr)
    assert "Unknown option" not in cp.stderr and "Validation failed" not in cp.stderr and "Missing value" not in cp.stderr, cp.stderr
    assert "hip" not in cp.stderr.lower(), cp.stderr


def test_accepted_with_the_profile_options(tmp_path):
    prof = ["--cami-report-file", str(tmp_path / "cami"), "--binning-file", str(tmp_path / "bin"), "--sample-id", "s"]
    cp = run(inputs(tmp_path) + prof + ["--device-parse"])
    assert cp.returncode == 255 and cp.stdout.startswith("checking input ... done!"), (cp.stdout, cp.stderr)
    assert "Unknown option" not in cp.stderr and "required but not set" not in cp.stderr, cp.stderr


def test_the_switch_takes_no_value(tmp_path):
    cp = run(inputs(tmp_path) + ["--device-parse", "yes"])
    assert cp.returncode == 255 and "Unknown option yes" in cp.stderr, cp.stderr

