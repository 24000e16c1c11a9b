"""CPU checks of the device matcher's boundary (include/fseq.h, fseq_match_founders .. fseq_write_match): the symbols, the
struct layouts, the refusals that must not touch a device, the front end's option -- and the Python model the GPU tests
(tests/test_gpu_match.py) lean on, pinned to the built host tool match_founder_sequences, which is the yardstick."""
import ctypes as C
import importlib
import os
import subprocess

import numpy as np
import pytest

import match_model as mm
from test_aux_cli import _match_oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["fseq_match_founders", "fseq_match_founder_rows", "fseq_get_match", "fseq_write_match"]


@pytest.fixture(scope="module")
def build():
    return importlib.import_module("founder-sequences_amd.build")


@pytest.fixture(scope="module")
def pkg(build):
    build.build()
    return importlib.import_module("founder-sequences_amd")


def test_library_exports_the_entry_points(pkg):
    lib = pkg.load_library()
    for name in NAMES:
        assert hasattr(lib, name), name
        assert name in pkg.EXPORTS
    assert lib.fseq_abi_version() == 5


def test_struct_layouts_match_header(pkg, tmp_path):
    src = tmp_path / "t.c"
    src.write_text('#include <stdio.h>\n#include "fseq.h"\nint main(void){ printf("%zu %zu\\n", sizeof(fseq_match_piece), sizeof(fseq_match_summary)); return 0; }\n')
    exe = tmp_path / "t"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    piece, summary = map(int, subprocess.run([str(exe)], capture_output=True, check=True).stdout.split())
    assert piece == 24 == C.sizeof(pkg.MatchPiece) == pkg.MATCH_PIECE_DTYPE.itemsize
    assert summary == C.sizeof(pkg.MatchSummary) == 4 * 8 + 2 * 4 + 8


def test_null_arguments_fail_without_touching_a_device(pkg):
    lib = pkg.load_library()
    sm = pkg.MatchSummary()
    perm = (C.c_uint32 * 4)()
    rows = (C.c_void_p * 1)(C.cast(C.create_string_buffer(8), C.c_void_p))
    assert lib.fseq_match_founders(None, perm, 0, C.byref(sm)) == pkg.FSEQ_E_ARG
    assert lib.fseq_match_founder_rows(None, rows, 1, 0, C.byref(sm)) == pkg.FSEQ_E_ARG
    assert lib.fseq_get_match(None, None, None) == pkg.FSEQ_E_ARG
    assert lib.fseq_write_match(None, None) == pkg.FSEQ_E_ARG


def test_front_end_names_the_option_and_refuses_it_on_several_gpus(build, tmp_path):
    cli = build.build_cli()
    r = subprocess.run([cli, "--help"], capture_output=True, timeout=60)
    assert r.returncode == 0 and b"--output-matches" in r.stdout and b"--match-min-segment-length" in r.stdout
    # refused before any input is read: the input does not exist, and the message is the option's
    r = subprocess.run([cli, "--input", str(tmp_path / "missing.txt"), "--segment-length-bound", "5", "--output-founders", str(tmp_path / "f"),
                        "--output-matches", str(tmp_path / "m"), "--gpus", "2"], capture_output=True, timeout=60)
    assert r.returncode != 0
    assert b"--output-matches is not supported together with --gpus" in r.stderr
    assert b"Loading the input" not in r.stderr and b"Unable to open" not in r.stderr
    assert not (tmp_path / "m").exists()


def _tool_report(tool, tmp_path, seqs, founders, min_len):
    paths = []
    for i, s in enumerate(seqs):
        (tmp_path / ("s%d.txt" % i)).write_bytes(bytes(s))
        paths.append(str(tmp_path / ("s%d.txt" % i)))
    (tmp_path / "seqs.txt").write_text("\n".join(paths) + "\n")
    (tmp_path / "founders.txt").write_bytes(b"".join(bytes(f) + b"\n" for f in founders))
    r = subprocess.run([tool, "--sequences", str(tmp_path / "seqs.txt"), "--founders", str(tmp_path / "founders.txt"), "--founders-format", "text",
                        "--min-segment-length", str(min_len), "--single-threaded"], capture_output=True, timeout=120)
    assert r.returncode == 0, r.stderr
    return r.stdout.decode(), r.stderr.decode()


def report_of(pieces_by_row):
    lines = ["SEQUENCE_INDEX\tLB\tRB\tFOUNDER_INDICES"]
    for i, o in enumerate(pieces_by_row):
        lines += ["%d\t%d\t%d\t%s" % (i, lb, rb, ",".join(map(str, idx))) for lb, rb, idx in o]
    return "\n".join(lines) + "\n"


@pytest.mark.parametrize("min_len", [0, 7])
def test_model_is_the_host_tool(build, tmp_path, min_len):
    """match_row against the yardstick's stdout and its two kinds of error lines, on a small case with a foreign character,
    an uncovered cell in column 0, one in the last column and two adjacent ones."""
    tool = dict(zip(build.AUX_TOOLS, build.build_aux()))["match_founder_sequences"]
    msa, founders = mm.mosaic_case(5 + min_len, 9, 300, 5, 4)
    msa[3, 100] = ord("N")                                  # a character no founder has anywhere
    out, err = _tool_report(tool, tmp_path, msa, founders, min_len)
    got = [mm.match_row(bytes(s), [bytes(f) for f in founders], min_len) for s in msa]
    assert out == report_of([g[0] for g in got])
    uncovered, short = sum(g[1] for g in got), sum(g[2] for g in got)
    # (the tool reports an uncovered cell in the last column twice: once where it finds it, once at the end of the sequence)
    last = sum(1 for s in msa if not (founders[:, -1] == s[-1]).any())
    assert err.count("not found in the founders") == uncovered + last and uncovered >= 5 and last >= 1
    assert err.count("under the given limit") == short and (short >= 1) == (min_len != 0)
    for s, g in zip(msa, got):                              # and it is the restatement the aux tool's own test uses
        o, e = _match_oracle(bytes(s), [bytes(f) for f in founders], min_len)
        assert (o, e) == (g[0], g[1])


@pytest.mark.parametrize("seed,m,n,K,sigma", [(1, 7, 60, 3, 2), (2, 5, 40, 33, 4), (3, 4, 33, 70, 16), (4, 3, 1, 2, 2), (5, 1, 2, 1, 2), (6, 6, 50, 5, 40)])
def test_vectorised_models_are_the_model(seed, m, n, K, sigma):
    msa, founders = mm.mosaic_case(seed, m, n, K, sigma)
    fb = [bytes(f) for f in founders]
    for min_len in (0, 1, 7, n + 1):
        want = [mm.match_row(bytes(s), fb, min_len) for s in msa]
        got = mm.match_rows(msa, founders, min_len)
        flat = [(lb, rb, r, len(idx)) for r, w in enumerate(want) for lb, rb, idx in w[0]]
        assert [tuple(int(x) for x in p) for p in got["pieces"]] == flat
        assert mm.sets_to_lists(got["sets"]) == [idx for w in want for _, _, idx in w[0]]
        assert got["uncovered_cells"] == sum(w[1] for w in want) and got["short_pieces"] == sum(w[2] for w in want)
        assert got["max_pieces_per_row"] == max(len(w[0]) for w in want)
    for r, s in enumerate(msa):
        o, unc = mm.match_row_fast(s, founders, window=8)
        w = mm.match_row(bytes(s), fb, 0)
        assert [(lb, rb, list(map(int, idx))) for lb, rb, idx in o] == w[0] and unc == w[1]
