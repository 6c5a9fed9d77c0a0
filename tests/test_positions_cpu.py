"""The host side of hash positions, without a GPU:
1. the line formatters of `taxor search --base-positions` and the saved batch's position store -- saved_validate refuses a store of the
   wrong size by name -- as a stand-alone program under AddressSanitizer + UBSan (tests/sanitize/positions_check.cpp);
2. the new exports are declared in include/taxor_gpu_tools.h (which still compiles as C11, like the seam's header), link from plain C, and
   taxor_gpu_saved_view keeps its layout;
3. the command line refuses --base-positions without --breakpoint-file or --segments-file before any HIP call, and both help texts state
   the definition, the syncmer-only limit, the tie-rule caveat and the cost;
4. the restatement the GPU tests compare with (tests/positions_expect.py) is the first occurrence on either strand."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from oracle import oracle as orc
from tests import positions_expect as pe
from tests.test_sanitizers_cpu import SAN, _build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TAXOR = os.path.join(ROOT, "taxor_amd", "taxor")
NEW = ("taxor_gpu_search_capture_positions", "taxor_gpu_saved_positions", "taxor_gpu_saved_positions_seconds")


@pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")
def test_formatters_and_position_store_under_asan_ubsan(tmp_path):
    exe = _build(tmp_path, "positions_check", [os.path.join(SAN, "positions_check.cpp")], ["-fsanitize=address,undefined"])
    cp = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert cp.returncode == 0 and cp.stdout.startswith("ok "), cp.stdout + cp.stderr[-2000:]
    assert "ERROR" not in cp.stderr and "runtime error" not in cp.stderr, cp.stderr[-2000:]


def test_new_exports_link_from_c_and_the_view_keeps_its_layout(tmp_path):
    from tests.test_c_abi_header import declared
    tools = declared("taxor_gpu_tools.h")
    for n in NEW:
        assert n in tools and n not in declared("taxor_gpu.h"), n
    src = tmp_path / "abi.c"
    # the view: 3 counts, 7 pointers, 6 words, a 64-bit window and two doubles -- what existing callers lay out themselves
    src.write_text('#include "taxor_gpu.h"\n#include "taxor_gpu_tools.h"\n#include <stdio.h>\n#include <stddef.h>\ntypedef void (*fn)(void);\n'
                   "int (*const a)(taxor_gpu_searcher *, int) = &taxor_gpu_search_capture_positions;\n"
                   "int (*const b)(const taxor_gpu_saved *, const uint32_t **) = &taxor_gpu_saved_positions;\n"
                   "double (*const c)(const taxor_gpu_saved *) = &taxor_gpu_saved_positions_seconds;\n"
                   'int main(void) {\n    printf("%d %d %d\\n", a != 0 && b != 0 && c != 0, (int)sizeof(taxor_gpu_saved_view), (int)offsetof(taxor_gpu_saved_view, use_syncmer));\n    return 0;\n}\n')
    exe = tmp_path / "abi"
    lib_dir = os.path.join(ROOT, "taxor_amd")
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe), "-L", lib_dir,
                           "-ltaxor_gpu", f"-Wl,-rpath,{lib_dir}", "-Wl,--unresolved-symbols=ignore-in-shared-libs"])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0 and out.stdout.split() == ["1", str(3 * 8 + 7 * 8 + 6 * 4 + 8 + 2 * 8), str(3 * 8 + 7 * 8)], out.stdout + out.stderr


def _taxor(*args):
    return subprocess.run([TAXOR, "search", *args], capture_output=True, text=True, timeout=60)


def test_the_switch_alone_is_refused_before_any_device_call(tmp_path):
    cp = _taxor("--index-file", str(tmp_path / "none.hixf"), "--query-file", str(tmp_path / "none.fq"), "--output-file", str(tmp_path / "o.tsv"), "--base-positions")
    assert cp.returncode != 0 and "--base-positions" in cp.stderr and "needs one of them" in cp.stderr
    assert "hip" not in cp.stderr.lower()


@pytest.mark.parametrize("flag", ["--help", "--advanced-help"])
def test_help_states_the_definition_and_its_limits(flag):
    cp = _taxor(flag)
    text = " ".join((cp.stdout + cp.stderr).split())
    assert cp.returncode == 0 and "--base-positions" in text
    for words in ("first base at which the read shows", "either strand", "syncmer indexes only" if flag == "--help" else "minimiser or k-mer index", "tie rule",
                  "earlier occurrence", "2048"):
        assert words in text, words
    if flag == "--advanced-help":
        for words in ("pos[i] = min", "LEFT_END_BASE = pos[BREAK_HASH - 1] + k", "BREAK_BASE = pos[BREAK_HASH]", "BASE_START = pos[HASH_START]",
                      "BASE_END = pos[HASH_END - 1] + k", "swept P times", "need not increase"):
            assert words in text, words


def test_the_restatement_is_the_first_occurrence_on_either_strand():
    rng = np.random.default_rng(3)
    a = bytes(rng.choice(np.frombuffer(b"ACGT", np.uint8), 400))
    rc = a.translate(bytes.maketrans(b"ACGT", b"TGCA"))[::-1]
    k = 22
    fwd, rev = pe.kmer_hashes(a, k), pe.kmer_hashes(rc, k)
    assert fwd.size == 400 - k + 1 and np.array_equal(fwd, rev[::-1])                 # the canonical form: a k-mer and its reverse complement hash alike
    h = orc.seq_to_syncmers(a + rc)
    p = pe.positions(a + rc, h, k).astype(np.int64)
    assert h.size > 30 and (p != pe.SENTINEL).all() and (p + k <= len(a) + k - 1).all()   # nothing resolves into the second half proper
    assert [int(x) for x in fwd[p[p + k <= len(a)]]] == [int(x) for x in h[p + k <= len(a)]]
    assert pe.positions(a, np.array([12345], np.uint64), k).tolist() == [pe.SENTINEL]
    assert pe.positions(b"ACGT", np.zeros(0, np.uint64), k).size == 0 and pe.kmer_hashes(b"ACGTN" * 4 + b"A", k + 0).size == 0
    # IUPAC codes are mapped before the k-mer is formed (N -> A)
    assert np.array_equal(pe.kmer_hashes(b"N" * 30, k), pe.kmer_hashes(b"A" * 30, k))
