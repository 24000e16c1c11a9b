"""CPU checks of the hold-out boundary (include/fseq.h: fseq_create_without_rows, fseq_get_held_out, fseq_match_held_out;
include/fseq_debug.h: fseq_debug_held_out_columns, fseq_debug_row_split_plan): the plan of the split applied in numpy, the struct's
layout, the header as C99, the refusals that need no device (a context needs one: the others are in tests/test_gpu_hold_out.py), the
front end's refusals, and the plan's header as a program of its own under the host sanitizers."""
import ctypes as C
import importlib
import os
import subprocess

import numpy as np
import pytest

import hold_out_model as hm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROWS = list(range(1, 71)) + [255, 256, 257, 4097]


@pytest.fixture(scope="module")
def build():
    return importlib.import_module("founder-sequences_amd.build")


@pytest.fixture(scope="module")
def pkg(build):
    build.build()
    return importlib.import_module("founder-sequences_amd")


def test_library_exports_the_entry_points(pkg):
    lib = pkg.load_library()
    for name in ("fseq_create_without_rows", "fseq_get_held_out", "fseq_match_held_out", "fseq_debug_held_out_columns", "fseq_debug_row_split_plan"):
        assert hasattr(lib, name) and name in pkg.EXPORTS
        assert (name in pkg.DEBUG_EXPORTS) == name.startswith("fseq_debug_")
    assert lib.fseq_abi_version() == 5                       # (detected by symbol: no struct of the boundary changed)
    for name in ("without_rows", "held_out", "match_held_out", "held_out_columns"):
        assert callable(getattr(pkg.SegmentationContext, name))
    assert callable(pkg.row_split_plan_host)


@pytest.mark.parametrize("bits", [2, 4, 8])
def test_the_plan_applied_in_numpy_gives_the_packed_kept_rows(pkg, bits):
    """Word for word: the descriptors applied to the packed source columns are pack(codes[kept]), at every row count and held pattern;
    n_slow is the number of words whose rows span more than their window."""
    rng = np.random.default_rng(bits)
    seen = {}
    for m in ROWS:
        codes = rng.integers(0, 1 << bits, size=(m, 3), dtype=np.uint8)
        packed, _ = pkg.pack_columns(codes, bits)
        for name, held in hm.patterns(m, bits).items():
            kept, base, keep, n_slow = pkg.row_split_plan_host(m, bits, held)
            want_kept = hm.kept_rows(m, held)
            assert np.array_equal(kept, want_kept), (m, name)
            assert n_slow == hm.expected_slow(m, bits, held) == int((keep == 0).sum()), (m, name)
            want, _ = hm.split(codes, held, bits)
            for c in range(codes.shape[1]):
                words = hm.apply_plan(packed[c], bits, base, keep, kept)
                got = np.zeros(want.shape[1], dtype=np.uint8)
                got[:4 * len(words)] = words.astype("<u4").view(np.uint8)[:want.shape[1]]
                assert np.array_equal(got, want[c]), (m, name, c)
            seen.setdefault(name, []).append(n_slow)
    # the runs: per held rows inside a word and per + 1 between two words stay in the window; 2 per + 1 is a slow word; per + 1 inside
    # a word is one where the word has all its per rows (at the smallest m the word behind the run is a partial one and spans less)
    assert set(seen) >= {"first", "last", "borders", "every_other", "all_but_one", "run_per", "run_per_1", "run_per_1_inside", "run_2per_1", "unsorted"}
    assert max(seen["run_per"]) == 0 and max(seen["run_per_1"]) == 0 and min(seen["run_2per_1"]) >= 1 and seen["run_per_1_inside"][-1] == 1


def test_summary_layout_and_header_as_c99(pkg, tmp_path):
    assert C.sizeof(pkg.HoldOutSummary) == 24
    src = tmp_path / "t.c"
    src.write_text('#include <stdio.h>\n#include "fseq.h"\n#include "fseq_debug.h"\n'
                   'int main(void){\n'
                   'int (*a)(fseq_ctx *, uint32_t const *, uint32_t, fseq_params const *, fseq_ctx **, fseq_hold_out_summary *) = fseq_create_without_rows;\n'
                   'int (*b)(fseq_ctx *, uint32_t *, uint32_t *) = fseq_get_held_out;\n'
                   'int (*c)(fseq_ctx *, uint32_t const *, uint8_t const *const *, uint32_t, uint64_t, fseq_match_summary *) = fseq_match_held_out;\n'
                   'int (*d)(fseq_ctx *, uint64_t, uint64_t, uint8_t *, uint64_t *, uint32_t *) = fseq_debug_held_out_columns;\n'
                   'int (*e)(uint32_t, uint32_t, uint32_t const *, uint32_t, uint32_t *, uint32_t *, uint32_t *, uint32_t *, uint32_t *) = fseq_debug_row_split_plan;\n'
                   'printf("%zu %d\\n", sizeof(fseq_hold_out_summary), a != 0 && b != 0 && c != 0 && d != 0 && e != 0); return 0; }\n')
    exe = tmp_path / "t"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe),
                    "-L", os.path.dirname(pkg.LIB_PATH), "-l:" + os.path.basename(pkg.LIB_PATH), "-Wl,-rpath," + os.path.dirname(pkg.LIB_PATH)], check=True)
    size, ok = map(int, subprocess.run([str(exe)], capture_output=True, check=True).stdout.split())
    assert size == 24 and ok


def test_refusals_that_need_no_device(pkg):
    lib = pkg.load_library()
    p = pkg.Params(0, 0, 5, 0, 0, 0, 0)
    h = C.c_void_p(1)
    sm, ms = pkg.HoldOutSummary(), pkg.MatchSummary()
    held = (C.c_uint32 * 2)(1, 2)
    perm = (C.c_uint32 * 4)()
    assert lib.fseq_create_without_rows(None, held, 2, C.byref(p), C.byref(h), C.byref(sm)) == pkg.FSEQ_E_ARG and h.value is None
    assert lib.fseq_create_without_rows(None, held, 2, None, C.byref(h), C.byref(sm)) == pkg.FSEQ_E_ARG
    assert lib.fseq_create_without_rows(None, held, 2, C.byref(p), None, C.byref(sm)) == pkg.FSEQ_E_ARG
    assert lib.fseq_get_held_out(None, None, None) == pkg.FSEQ_E_ARG
    assert lib.fseq_match_held_out(None, perm, None, 0, 0, C.byref(ms)) == pkg.FSEQ_E_ARG
    ld, bits = C.c_uint64(), C.c_uint32()
    assert lib.fseq_debug_held_out_columns(None, 0, 0, None, C.byref(ld), C.byref(bits)) == pkg.FSEQ_E_ARG
    # the held list, as fseq_create_without_rows checks it before it touches a device: through the plan's entry, which takes m itself
    for m, bits_, rows in ((8, 2, []), (8, 2, list(range(8))), (8, 2, [3, 3]), (8, 2, [8]), (8, 2, [1, 0xFFFFFFFF]), (8, 3, [1]), (1, 2, [0])):
        with pytest.raises(pkg.FseqError) as e:
            pkg.row_split_plan_host(m, bits_, np.array(rows, dtype=np.uint32))
        assert e.value.code == pkg.FSEQ_E_ARG, (m, bits_, rows)
    nw, ns = C.c_uint32(), C.c_uint32()
    assert lib.fseq_debug_row_split_plan(8, 2, held, 2, None, None, None, None, C.byref(ns)) == pkg.FSEQ_E_ARG
    assert lib.fseq_debug_row_split_plan(8, 2, held, 2, None, None, None, C.byref(nw), C.byref(ns)) == pkg.FSEQ_OK and (nw.value, ns.value) == (1, 0)
    kept, base, keep, n_slow = pkg.row_split_plan_host(8, 2, [1, 2])
    assert kept.tolist() == [0, 3, 4, 5, 6, 7] and base.tolist() == [0] and keep.tolist() == [0b11111001] and n_slow == 0


def test_the_grammar_of_the_model():
    assert hm.parse_hold_out("3,10:12", 20) == [3, 10, 11, 12] and hm.parse_hold_out("5:5,0", 6) == [5, 0]
    for spec, m in (("", 5), ("a", 5), ("1,", 5), ("3:1", 5), ("1:2:3", 5), ("-1", 5), ("1,1", 5), ("0:2,2", 5), ("5", 5), ("0:4", 5)):
        with pytest.raises(hm.HoldOutError):
            hm.parse_hold_out(spec, m)


def test_front_end_names_the_options_and_refuses_their_misuse(build, tmp_path):
    cli = build.build_cli()
    r = subprocess.run([cli, "--help"], capture_output=True, timeout=60)
    assert r.returncode == 0 and b"--hold-out=LIST" in r.stdout and b"--output-held-out-matches=PATH" in r.stdout
    base = [cli, "--input", str(tmp_path / "missing.txt"), "--output-founders", str(tmp_path / "f")]
    L = ["--segment-length-bound", "5"]
    out = ["--output-held-out-matches", str(tmp_path / "m")]
    for extra, word in ((L + ["--hold-out=1,x"] + out, b"malformed"),
                        (L + ["--hold-out=3:1"] + out, b"malformed"),
                        (L + ["--hold-out=1,"] + out, b"malformed"),
                        (L + ["--hold-out=1,0:2"] + out, b"names a sequence twice"),
                        (L + out, b"--output-held-out-matches requires --hold-out"),
                        (L + ["--hold-out=1", "--gpus", "2"] + out, b"--hold-out is not supported together with --gpus"),
                        (L + ["--hold-out=1", "--remove-identity-columns"] + out, b"--hold-out is not supported together with --remove-identity-columns"),
                        (["--hold-out=1", "--scan-segment-lengths=5,10"] + out, b"needs a segment length to go on with")):
        r = subprocess.run(base + extra, capture_output=True, timeout=60)
        # refused before any input is read: the input does not exist, and the message is the option's
        assert r.returncode != 0 and word in r.stderr, (extra, r.stderr)
        assert b"Loading the input" not in r.stderr and b"Unable to open" not in r.stderr
        assert not (tmp_path / "m").exists() and not (tmp_path / "f").exists()
    # what takes the sequence count: refused once the input is read, before a device is opened
    (tmp_path / "in.fa").write_text(">a\nACGTACGTAC\n>b\nACGTTCGTAC\n>c\nACGAACGTAC\n")
    base = [cli, "--input", str(tmp_path / "in.fa"), "--input-format", "FASTA", "--output-founders", str(tmp_path / "f")] + L + out
    for spec, word in (("3", b"out of range"), ("0:2", b"leaves no sequence"), ("0,1:7", b"out of range")):
        r = subprocess.run(base + ["--hold-out=" + spec], capture_output=True, timeout=60)
        assert r.returncode != 0 and word in r.stderr, (spec, r.stderr)
        assert b"Generating a compressed alphabet" not in r.stderr and b"Unable to initialise" not in r.stderr
        assert not (tmp_path / "m").exists() and not (tmp_path / "f").exists()


def test_plan_under_the_sanitizers(tmp_path):
    """The header is host-only: tests/row_split_plan_sanitized.cpp includes it alone and runs the plan and the strips over these row
    counts and patterns as a program of its own under AddressSanitizer and UndefinedBehaviorSanitizer (nothing loaded into Python
    runs under either)."""
    here = os.path.dirname(os.path.abspath(__file__))
    exe = str(tmp_path / "row_split_plan_sanitized")
    subprocess.run(["g++", "-std=c++17", "-g", "-O1", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", os.path.join(os.path.dirname(here), "founder-sequences_amd", "csrc"), os.path.join(here, "row_split_plan_sanitized.cpp"), "-o", exe], check=True)
    p = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120)
    assert p.returncode == 0 and p.stdout.strip() == "ok", p.stderr[-3000:]
