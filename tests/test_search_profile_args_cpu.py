"""`taxor search` with the options of `taxor profile` (search to profile in one run) checks them before the
first HIP call, so all of this runs without a device: every partial set of the three required options, the ranges and parses of
--min-abundance and --em-steps in `taxor profile`'s own words, the refusal of several index files and of several devices.  Without
the new options the command demands what it always did."""
import itertools
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TAXOR = os.path.join(ROOT, "taxor_amd", "taxor")
REQUIRED = ["--cami-report-file", "--binning-file", "--sample-id"]


def run(sub, args):
    env = dict(os.environ, HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="")        # nothing below may need a device
    return subprocess.run([TAXOR, sub] + args, capture_output=True, text=True, timeout=60, env=env)


def inputs(tmp_path):
    """an index file and a query file that EXIST (their content is never read: every case below ends before that)"""
    idx, q = tmp_path / "idx.hixf", tmp_path / "reads.fa"
    idx.write_bytes(b"")
    q.write_text(">r1\nACGT\n")
    return ["--index-file", str(idx), "--query-file", str(q)]


def profile_args(tmp_path, keep=REQUIRED):
    a = {"--cami-report-file": str(tmp_path / "cami"), "--binning-file": str(tmp_path / "bin"), "--sample-id": "s"}
    return [x for k in keep for x in (k, a[k])]


def refused(cp, needle, prefix="[TAXOR SEARCH ERROR] "):
    assert cp.returncode == 255, (cp.returncode, cp.stdout, cp.stderr)                # exit(-1)
    assert cp.stderr.startswith(prefix), cp.stderr
    assert needle in cp.stderr, cp.stderr
    assert "checking input" not in cp.stdout, cp.stdout                                # refused before the files are looked at
    assert "hip" not in cp.stderr.lower(), cp.stderr                                   # and before any device call


PARTIAL = [list(c) for n in (1, 2) for c in itertools.combinations(REQUIRED, n)]


@pytest.mark.parametrize("given", PARTIAL, ids=["+".join(o.strip("-") for o in g) for g in PARTIAL])
def test_partial_set_of_required_options(tmp_path, given):
    missing = next(o for o in REQUIRED if o not in given)                            # reported in the profile's order
    cp = run("search", inputs(tmp_path) + profile_args(tmp_path, given))
    refused(cp, f"Option {missing} is required but not set.")
    assert not (tmp_path / "cami").exists() and not (tmp_path / "bin").exists()


@pytest.mark.parametrize("opt", ["--seq-abundance-file", "--min-abundance", "--em-steps"])
def test_an_optional_profile_option_alone_demands_the_three(tmp_path, opt):
    value = {"--seq-abundance-file": str(tmp_path / "seq"), "--min-abundance": "0.01", "--em-steps": "5"}[opt]
    refused(run("search", inputs(tmp_path) + [opt, value]), "Option --cami-report-file is required but not set.")


def profile_message(tmp_path, opt, value):
    """what `taxor profile` itself says about the value"""
    tsv = tmp_path / "search.tsv"
    tsv.write_text("#h\n")
    cp = run("profile", ["--search-file", str(tsv)] + profile_args(tmp_path) + [opt, value])
    assert cp.returncode == 255 and cp.stderr.startswith("[TAXOR PROFILE ERROR] "), cp.stderr
    return cp.stderr[len("[TAXOR PROFILE ERROR] "):]


@pytest.mark.parametrize("opt,value,needle", [("--min-abundance", "-0.1", "Validation failed for option --min-abundance"),
                                              ("--min-abundance", "1.5", "Validation failed for option --min-abundance"),
                                              ("--em-steps", "0", "Validation failed for option --em-steps"),
                                              ("--em-steps", "1001", "Validation failed for option --em-steps"),
                                              ("--min-abundance", "abc", "Value parse failed for --min-abundance"),
                                              ("--em-steps", "12x", "Value parse failed for --em-steps")])
def test_range_and_parse_errors_match_taxor_profile(tmp_path, opt, value, needle):
    cp = run("search", inputs(tmp_path) + profile_args(tmp_path) + [opt, value])
    refused(cp, needle)
    assert cp.stderr[len("[TAXOR SEARCH ERROR] "):] == profile_message(tmp_path, opt, value)


def test_missing_value(tmp_path):
    refused(run("search", inputs(tmp_path) + profile_args(tmp_path) + ["--em-steps"]), "Missing value for option --em-steps")


def test_two_index_files_are_refused_with_the_profile_options(tmp_path):
    a = inputs(tmp_path)
    a[1] = a[1] + "," + a[1]
    cp = run("search", a + profile_args(tmp_path))
    refused(cp, "--index-file")
    assert "ONE index file" in cp.stderr


@pytest.mark.parametrize("extra,named", [(["--gpus", "2"], "--gpus"), (["--gpu-list", "0,1"], "--gpu-list"), (["--gpus=3"], "--gpus")])
def test_several_devices_are_refused_with_the_profile_options(tmp_path, extra, named):
    cp = run("search", inputs(tmp_path) + extra + profile_args(tmp_path))
    refused(cp, f"Validation failed for option {named}")
    assert "ONE device" in cp.stderr


def test_output_file_is_optional_with_the_profile_options(tmp_path):
    """the command gets past its command line and fails at the index file, which is empty"""
    cp = run("search", inputs(tmp_path) + profile_args(tmp_path))
    assert cp.returncode == 255 and cp.stdout.startswith("checking input ... done!"), (cp.stdout, cp.stderr)
    assert "cannot open output file" not in cp.stderr and "required but not set" not in cp.stderr, cp.stderr


def test_without_the_new_options_the_demands_are_the_old_ones(tmp_path):
    a = inputs(tmp_path)
    refused(run("search", a[2:]), "Option --index-file is required but not set.")
    # no --output-file: the report cannot be opened, as before (after the input check, which passes)
    cp = run("search", a)
    assert cp.returncode == 255 and "cannot open output file" in cp.stderr, (cp.stdout, cp.stderr)
    assert cp.stdout.startswith("checking input ... done!")
    # --gpus 2 and two index files are accepted without the profile options: both runs get to the index file
    cp = run("search", a + ["--gpus", "2", "--output-file", str(tmp_path / "o.tsv")])
    assert "Validation failed" not in cp.stderr and cp.stdout.startswith("checking input ... done!"), (cp.stdout, cp.stderr)


def test_help_names_the_new_options_and_the_duplicate_id_limit():
    for flag in ("--help", "--advanced-help"):
        cp = run("search", [flag])
        assert cp.returncode == 0
        text = cp.stdout + cp.stderr
        for opt in REQUIRED + ["--seq-abundance-file", "--min-abundance", "--em-steps"]:
            assert opt in text
        assert "must occur once" in text
