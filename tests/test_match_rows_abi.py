"""CPU checks of fseq_match_rows' boundary (include/fseq.h) and of what reports on the split walk (include/fseq_debug.h,
fseq_debug_match_split): the symbols, the header as C, the refusals that need no context (a context needs a device: the others
are in tests/test_gpu_match_rows.py), the knobs, the front end's options -- and the model of the split walk
(tests/match_split_model.py) pinned to the built host tool match_founder_sequences on sequences that are NOT the rows the
founders were made from, a byte outside the alphabet and a full 2-bit alphabet among them."""
import ctypes as C
import importlib
import os
import subprocess

import numpy as np
import pytest

import match_model as mm
import match_split_model as sm
from test_match_abi import _tool_report, report_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def build():
    return importlib.import_module("founder-sequences_amd.build")


@pytest.fixture(scope="module")
def pkg(build):
    build.build()
    return importlib.import_module("founder-sequences_amd")


def test_library_exports_the_entry_points(pkg):
    lib = pkg.load_library()
    for name in ("fseq_match_rows", "fseq_debug_match_split"):
        assert hasattr(lib, name) and name in pkg.EXPORTS
    assert "fseq_match_rows" not in pkg.DEBUG_EXPORTS and "fseq_debug_match_split" in pkg.DEBUG_EXPORTS
    assert lib.fseq_abi_version() == 5                       # (detected by symbol: no struct of the boundary changed)
    assert callable(pkg.SegmentationContext.match_rows) and callable(pkg.SegmentationContext.match_split)


def test_headers_compile_as_c(pkg, tmp_path):
    src = tmp_path / "t.c"
    src.write_text('#include <stdio.h>\n#include "fseq.h"\n#include "fseq_debug.h"\n'
                   'int main(void){ int (*f)(fseq_ctx *, uint32_t const *, uint8_t const *const *, uint32_t, uint8_t const *const *, uint32_t, uint64_t, fseq_match_summary *) = fseq_match_rows;\n'
                   'int (*g)(fseq_ctx *, fseq_match_split_info *) = fseq_debug_match_split;\n'
                   'printf("%zu %d %d\\n", sizeof(fseq_match_split_info), f != 0, g != 0); return 0; }\n')
    exe = tmp_path / "t"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe),
                    "-L", os.path.dirname(pkg.LIB_PATH), "-l:" + os.path.basename(pkg.LIB_PATH), "-Wl,-rpath," + os.path.dirname(pkg.LIB_PATH)], check=True)
    size, f, g = map(int, subprocess.run([str(exe)], capture_output=True, check=True).stdout.split())
    assert size == C.sizeof(pkg.MatchSplitInfo) == 4 * 4 + 2 * 8 and f and g


def test_null_arguments_fail_without_touching_a_device(pkg):
    lib = pkg.load_library()
    sm_ = pkg.MatchSummary()
    info = pkg.MatchSplitInfo()
    perm = (C.c_uint32 * 4)()
    rows = (C.c_void_p * 1)(C.cast(C.create_string_buffer(8), C.c_void_p))
    assert lib.fseq_match_rows(None, perm, None, 0, rows, 1, 0, C.byref(sm_)) == pkg.FSEQ_E_ARG
    assert lib.fseq_match_rows(None, None, rows, 1, rows, 1, 0, C.byref(sm_)) == pkg.FSEQ_E_ARG
    assert lib.fseq_debug_match_split(None, C.byref(info)) == pkg.FSEQ_E_ARG


def test_the_knobs_are_in_the_table_the_library_and_the_readme(pkg):
    lib = pkg.load_library()
    src = open(os.path.join(ROOT, "founder-sequences_amd", "csrc", "fseq_ctx.hpp")).read()
    readme = open(os.path.join(ROOT, "README.md")).read()
    for name, field in (("FSEQ_MATCH_SPLIT", "match_split"), ("FSEQ_MATCH_OVERLAP", "match_overlap")):
        assert lib.fseq_debug_set_tuning(None, name.encode(), b"2") == pkg.FSEQ_E_ARG
        assert '{"%s", nullptr, &Tuning::%s,' % (name, field) in src
        assert name.encode() + b"\0" in open(pkg.LIB_PATH, "rb").read()
        assert "`%s" % name in readme


def test_front_end_names_the_options_and_refuses_their_misuse(build, tmp_path):
    cli = build.build_cli()
    r = subprocess.run([cli, "--help"], capture_output=True, timeout=60)
    assert r.returncode == 0 and b"--match-sequences" in r.stdout and b"--output-sequence-matches" in r.stdout
    base = [cli, "--input", str(tmp_path / "missing.txt"), "--segment-length-bound", "5", "--output-founders", str(tmp_path / "f")]
    pair = ["--match-sequences", str(tmp_path / "q.txt"), "--output-sequence-matches", str(tmp_path / "m")]
    for extra, word in ((pair[:2], b"--match-sequences requires --output-sequence-matches"),
                        (pair[2:], b"--output-sequence-matches requires --match-sequences"),
                        (pair + ["--gpus", "2"], b"--match-sequences is not supported together with --gpus"),
                        (pair + ["--remove-identity-columns"], b"--match-sequences is not supported together with --remove-identity-columns")):
        r = subprocess.run(base + extra, capture_output=True, timeout=60)
        # refused before any input is read: the input does not exist, and the message is the option's
        assert r.returncode != 0 and word in r.stderr, r.stderr
        assert b"Loading the input" not in r.stderr and b"Unable to open" not in r.stderr
        assert not (tmp_path / "m").exists() and not (tmp_path / "f").exists()


def held_out(seed, m, n, K, sigma, take):
    """mosaic_case's founders, and of its rows the last `take` as queries (the others would be the input)"""
    msa, founders = mm.mosaic_case(seed, m, n, K, sigma)
    return msa[:-take], msa[-take:].copy(), founders


@pytest.mark.parametrize("min_len", [0, 7])
def test_models_are_the_host_tool_on_held_out_sequences(build, tmp_path, min_len):
    tool = dict(zip(build.AUX_TOOLS, build.build_aux()))["match_founder_sequences"]
    rest, queries, founders = held_out(31 + min_len, 15, 500, 5, 4, 6)
    assert len(np.unique(rest)) == 4 == len(np.unique(founders[founders != 0x7E]))       # a full 2-bit alphabet
    queries[2, 250] = ord("N")                               # a byte no sequence of the input and no founder has
    queries[3, 0] = ord("N")
    queries[4, -1] = ord("N")
    out, err = _tool_report(tool, tmp_path, queries, founders, min_len)
    whole = mm.match_rows(queries, founders, min_len)
    for G, overlap in ((1, 1), (3, 40), (7, 5), (500, 1)):
        got = sm.split_match(queries, founders, min_len, G, overlap)
        assert np.array_equal(got["pieces"], whole["pieces"]) and np.array_equal(got["sets"], whole["sets"])
        by_row = [[] for _ in queries]
        for p, idx in zip(got["pieces"], mm.sets_to_lists(got["sets"])):
            by_row[int(p["row"])].append((int(p["lb"]), int(p["rb"]), idx))
        assert report_of(by_row) == out
        last = sum(1 for s in queries if not (founders[:, -1] == s[-1]).any())
        assert err.count("not found in the founders") == got["uncovered_cells"] + last and got["uncovered_cells"] >= 3
        assert err.count("under the given limit") == got["short_pieces"]
