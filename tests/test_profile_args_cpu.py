"""`taxor profile` checks its command line and opens the search file before the first HIP call (taxor_amd/csrc/profile_cmd.h), so
all of this runs without a device: every required option missing, every range violated, a search file that is not there.  Errors
carry the reference's prefix and its exit status -1 (src/main/taxor_profile.cpp:874-878).  Parse and merge errors come before the
first HIP call too: the last four tests take them from a search file of 16 parser ranges, where the line number in the message is
the sum of the newlines the earlier ranges counted."""
import os
import subprocess

import pytest

from tests import profile_padding as scale

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TAXOR = os.path.join(ROOT, "taxor_amd", "taxor")
HEADER = "#QUERY_NAME\tACCESSION\tREFERENCE_NAME\tTAXID\tREF_LEN\tQUERY_LEN\tQHASH_COUNT\tQHASH_MATCH\tTAX_STR\tTAX_ID_STR\n"


def run(args):
    env = dict(os.environ, HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="")        # nothing below may need a device
    return subprocess.run([TAXOR, "profile"] + args, capture_output=True, text=True, timeout=60, env=env)


def full_args(tmp_path, **override):
    tsv = tmp_path / "search.tsv"
    tsv.write_text(HEADER + "r1\tA\tn\t1\t1000\t500\t40\t30\tk__B;s__S\t2;10\n")
    a = {"--search-file": str(tsv), "--cami-report-file": str(tmp_path / "cami"), "--binning-file": str(tmp_path / "bin"),
         "--sample-id": "s"}
    a.update(override)
    return [x for k, v in a.items() if v is not None for x in (k, v)]


def refused(cp, needle):
    assert cp.returncode == 255, (cp.returncode, cp.stderr)
    assert cp.stderr.startswith("[TAXOR PROFILE ERROR] "), cp.stderr
    assert needle in cp.stderr, cp.stderr
    assert "not provided by this build" not in cp.stderr


@pytest.mark.parametrize("opt", ["--search-file", "--cami-report-file", "--binning-file", "--sample-id"])
def test_required_option_missing(tmp_path, opt):
    refused(run(full_args(tmp_path, **{opt: None})), f"Option {opt} is required but not set.")


@pytest.mark.parametrize("opt,value", [("--min-abundance", "-0.1"), ("--min-abundance", "1.5"), ("--em-steps", "0"), ("--em-steps", "1001")])
def test_value_out_of_range(tmp_path, opt, value):
    refused(run(full_args(tmp_path, **{opt: value})), f"Validation failed for option {opt}")


@pytest.mark.parametrize("opt,value", [("--min-abundance", "abc"), ("--em-steps", "12x")])
def test_value_does_not_parse(tmp_path, opt, value):
    refused(run(full_args(tmp_path, **{opt: value})), f"Value parse failed for {opt}")


def test_unknown_option_and_missing_value(tmp_path):
    refused(run(full_args(tmp_path) + ["--threads", "4"]), "Unknown option --threads")
    refused(run(full_args(tmp_path) + ["--em-steps"]), "Missing value for option --em-steps")


def test_search_file_that_does_not_exist(tmp_path):
    refused(run(full_args(tmp_path, **{"--search-file": str(tmp_path / "nothing.tsv")})), "Could not open search results file")
    assert not (tmp_path / "cami").exists() and not (tmp_path / "bin").exists()


def test_malformed_and_undefined_lines_are_named(tmp_path):
    bad = tmp_path / "bad.tsv"
    bad.write_text(HEADER + "r1\tA\tn\t1\tlong\t500\t40\t30\tk__B;s__S\t2;10\n")
    refused(run(full_args(tmp_path, **{"--search-file": str(bad)})), "line 2 of the search file")
    # a '-' line followed by a match of the same read: a '-' among several matches, which the reference leaves undefined
    bad.write_text(HEADER + "r1\t-\t-\t-\t-\t500\nr1 x\tA\tn\t1\t1000\t500\t40\t30\tk__B;s__S\t2;10\n")
    refused(run(full_args(tmp_path, **{"--search-file": str(bad)})), "has a match after its '-' line")


def test_help_exits_zero():
    cp = run(["--help"])
    assert cp.returncode == 0, cp.stderr
    for opt in ("--search-file", "--cami-report-file", "--seq-abundance-file", "--binning-file", "--sample-id", "--min-abundance", "--em-steps",
                "--gpu"):
        assert opt in cp.stdout
    assert "--debug" not in cp.stdout and "--output-verbose-statistics" not in cp.stdout      # hidden


def test_hidden_flags_are_accepted(tmp_path):
    # accepted: the run gets past the command line and fails later, at the search file
    cp = run(full_args(tmp_path, **{"--search-file": str(tmp_path / "nothing.tsv")}) + ["--debug", "--output-verbose-statistics"])
    refused(cp, "Could not open search results file")


# ---- refusals in a file of 16 parser ranges: the expected line number is counted from the bytes written -------------------------
@pytest.fixture(scope="module")
def big_lines():
    """tests/golden/profile/many.tsv padded to 15.5 MiB, as lines with their newlines"""
    raw = open(os.path.join(ROOT, "tests", "golden", "profile", "many.tsv"), "rb").read()
    return scale.padded(raw, 15 * scale.MIB + scale.MIB // 2, seed="refusals").splitlines(keepends=True)


def refused_at(tmp_path, lines, index, needle):
    """writes the lines; the command must refuse them naming lines[index] by its 1-based number.  Returns the range (of 16) that
    line starts in."""
    data = b"".join(lines)
    at = len(b"".join(lines[:index]))
    number = data[:at].count(b"\n") + 1
    assert scale.nominal_ranges(len(data)) == 16
    tsv = tmp_path / "big.tsv"
    tsv.write_bytes(data)
    cp = run(full_args(tmp_path, **{"--search-file": str(tsv)}))
    refused(cp, needle)
    assert cp.stderr.startswith(f"[TAXOR PROFILE ERROR] line {number} of the search file: "), (number, cp.stderr[:300])
    return sum(at >= c for c in scale.range_starts(data, 16)) - 1


def field_edit(line, fn):
    f = line.rstrip(b"\n").split(b"\t")
    return b"\t".join(fn(f)) + b"\n"


def line_in_range(lines, t):
    """index of a match line that starts in range t of 16"""
    data = b"".join(lines)
    starts = scale.range_starts(data, 16) + [len(data)]
    at = 0
    for i, ln in enumerate(lines):
        if i > 0 and starts[t] <= at < starts[t + 1] and ln.split(b"\t")[1] != b"-":
            return i
        at += len(ln)
    raise AssertionError(f"no match line starts in range {t}")


def test_number_that_does_not_parse_in_the_last_range(tmp_path, big_lines):
    lines = list(big_lines)
    i = line_in_range(lines, 15)
    lines[i] = field_edit(lines[i], lambda f: f[:7] + [b"x"] + f[8:])                   # QHASH_MATCH
    assert refused_at(tmp_path, lines, i, "must be numbers") == 15


def test_short_match_line_in_the_second_range(tmp_path, big_lines):
    lines = list(big_lines)
    i = line_in_range(lines, 1)
    lines[i] = field_edit(lines[i], lambda f: f[:5])
    assert refused_at(tmp_path, lines, i, "a match needs ten columns") == 1


def test_match_in_the_last_range_after_a_dash_line_in_the_first(tmp_path, big_lines):
    lines = list(big_lines)
    lines.insert(3, b"fresh_read\t-\t-\t-\t-\t4000\n")
    lines.append(field_edit(lines[line_in_range(lines, 15)], lambda f: [b"fresh_read later"] + f[1:5] + [b"4000"] + f[6:]))
    data = b"".join(lines)
    assert len(b"".join(lines[:4])) <= scale.range_starts(data, 16)[1]                    # the '-' line lies in the first range
    assert refused_at(tmp_path, lines, len(lines) - 1, "has a match after its '-' line") == 15


def test_query_len_that_changes_between_the_first_and_the_last_range(tmp_path, big_lines):
    lines = list(big_lines)
    first = lines[1].rstrip(b"\n").split(b"\t")                                          # the file's first read, in the first range
    assert first[1] != b"-"
    lines.append(b"\t".join(first[:5] + [str(int(first[5]) + 1).encode()] + first[6:]) + b"\n")
    assert refused_at(tmp_path, lines, len(lines) - 1, "changes its QUERY_LEN or QHASH_COUNT") == 15
