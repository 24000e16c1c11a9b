"""CPU checks of the chunked input that drops the identity columns on the way (include/fseq.h, fseq_input_scan_identity ..
fseq_set_rows_streamed_without_identity_columns): the symbols, the headers as C, the refusals that must not touch a device, the
front end's --reduce-on-upload, and the range of a kept list inside a chunk (input_kept_range, csrc/fseq_input_kept_range.hpp)
against numpy's searchsorted and as a program under the host sanitizers.  The GPU side is tests/test_gpu_input_reduced.py."""
import ctypes as C
import importlib
import os
import subprocess

import numpy as np
import pytest

import input_reduced_model as rmodel

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["fseq_input_scan_identity", "fseq_input_reduce", "fseq_input_kept_columns", "fseq_input_columns_kept", "fseq_input_end_kept",
         "fseq_set_rows_streamed_without_identity_columns"]
DEBUG_NAMES = ["fseq_debug_input_kept_range", "fseq_debug_alphabet"]


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
        assert hasattr(lib, name) and name in pkg.EXPORTS and name not in pkg.DEBUG_EXPORTS, name
    for name in DEBUG_NAMES:
        assert hasattr(lib, name) and name in pkg.EXPORTS and name in pkg.DEBUG_EXPORTS, name
    assert lib.fseq_abi_version() == 5                       # (detected by symbol: no struct of the boundary changed)
    for name in ("input_scan_identity", "input_reduce", "input_kept_columns", "input_columns_kept", "input_end_kept", "set_sequences_without_identity_columns"):
        assert callable(getattr(pkg.SegmentationContext, name))


def test_headers_compile_as_c(tmp_path):
    src = tmp_path / "t.c"
    src.write_text('#include "fseq.h"\n#include "fseq_debug.h"\n'
                   'int main(void){ uint64_t a = 0, b = 0; uint32_t s = 0, w = 0; fseq_ctx *out = 0; fseq_identity_summary sm; fseq_params p = {0};\n'
                   ' return fseq_input_scan_identity(0, 0, 1, 0) + fseq_input_reduce(0, &p, &sm) + fseq_input_kept_columns(0, 0, 1, &a) + fseq_input_columns_kept(0, 0, 1, 0)\n'
                   ' + fseq_input_end_kept(0, &out) + fseq_set_rows_streamed_without_identity_columns(0, 0, 0, &p, &out, &sm) + fseq_debug_input_kept_range(0, 0, 0, 1, &a, &b)\n'
                   ' + fseq_debug_alphabet(0, &s, &w, 0); }\n')
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)], check=True)


def test_null_arguments_fail_without_touching_a_device(pkg):
    lib = pkg.load_library()
    rows = (C.c_void_p * 2)()
    count, sigma, bits = C.c_uint64(), C.c_uint32(), C.c_uint32()
    out = C.c_void_p(5)
    p = pkg.Params(0, 0, 10, 0, 0, 0, 0)
    sm = pkg.IdentitySummary()
    E = pkg.FSEQ_E_ARG
    assert lib.fseq_input_scan_identity(None, 0, 1, rows) == E
    assert lib.fseq_input_reduce(None, C.byref(p), C.byref(sm)) == E
    assert lib.fseq_input_kept_columns(None, 0, 1, C.byref(count)) == E
    assert lib.fseq_input_columns_kept(None, 0, 1, rows) == E
    assert lib.fseq_input_end_kept(None, C.byref(out)) == E
    assert lib.fseq_set_rows_streamed_without_identity_columns(None, rows, 0, C.byref(p), C.byref(out), C.byref(sm)) == E
    assert lib.fseq_debug_alphabet(None, C.byref(sigma), C.byref(bits), None) == E
    # a context that is not looked at: the other pointers are checked first
    h = C.c_void_p(0)
    assert lib.fseq_input_scan_identity(h, 0, 1, None) == E
    assert lib.fseq_input_reduce(h, None, C.byref(sm)) == E
    assert lib.fseq_input_kept_columns(h, 0, 1, None) == E
    assert lib.fseq_input_end_kept(h, None) == E
    assert lib.fseq_set_rows_streamed_without_identity_columns(h, None, 0, C.byref(p), C.byref(out), C.byref(sm)) == E
    assert lib.fseq_set_rows_streamed_without_identity_columns(h, rows, 0, None, C.byref(out), C.byref(sm)) == E
    assert lib.fseq_set_rows_streamed_without_identity_columns(h, rows, 0, C.byref(p), None, C.byref(sm)) == E


def test_front_end_lists_the_option_and_refuses_its_combinations(build, tmp_path):
    cli = build.build_cli()
    r = subprocess.run([cli, "--help"], capture_output=True, timeout=60)
    assert r.returncode == 0 and b"--reduce-on-upload" in r.stdout
    common = [cli, "--input", str(tmp_path / "missing.txt"), "--segment-length-bound", "5", "--output-founders", str(tmp_path / "f")]
    refusals = [
        (["--reduce-on-upload", "--remove-identity-columns"], b"--reduce-on-upload requires --upload-memory"),
        (["--reduce-on-upload", "--upload-memory", "4"], b"--reduce-on-upload requires --remove-identity-columns"),
        (["--reduce-on-upload"], b"--reduce-on-upload requires --upload-memory"),
        (["--reduce-on-upload", "--upload-memory", "4", "--remove-identity-columns", "--hold-out", "1", "--output-held-out-restored-matches", str(tmp_path / "h")],
         b"--reduce-on-upload is not supported together with --hold-out"),
        (["--reduce-on-upload", "--upload-memory", "4", "--remove-identity-columns", "--gpus", "2"], b"--reduce-on-upload is not supported together with --gpus > 1"),
    ]
    for extra, message in refusals:
        r = subprocess.run(common + extra, capture_output=True, timeout=60)
        # refused before any input is read and any device is looked for: the input does not exist, and the reason is one line
        assert r.returncode != 0 and message in r.stderr, (extra, r.stderr)
        assert r.stderr.count(b"\n") == 1 and b"Loading the input" not in r.stderr
        assert not (tmp_path / "f").exists() and not (tmp_path / "h").exists()
    # accepted with its two companions: the run then stops at the input, which is missing
    r = subprocess.run(common + ["--reduce-on-upload", "--upload-memory", "4", "--remove-identity-columns"], capture_output=True, timeout=60)
    assert r.returncode != 0 and b"Unable to open the input file" in r.stderr


def test_kept_range_equals_searchsorted(pkg):
    rng = np.random.default_rng(77)
    seen = set()
    for _ in range(300):
        n_src = int(rng.integers(1, 500))
        n = int(rng.integers(0, n_src + 1))
        kept = np.sort(rng.choice(n_src, size=n, replace=False)).astype(np.uint64)
        c0 = int(rng.integers(0, n_src + 2))
        ncols = int(rng.integers(0, n_src + 2))
        got = pkg.input_kept_range_host(kept, c0, ncols)
        assert got == rmodel.kept_range(kept, c0, ncols), (kept, c0, ncols)
        seen.add((n == 0, got[0] == got[1], got[0] == 0, got[1] == n))
    # empty lists, chunks without a kept column, chunks that begin in front of and end behind the list: all among the 300
    assert {x[0] for x in seen} == {x[1] for x in seen} == {x[2] for x in seen} == {x[3] for x in seen} == {True, False}
    # the tilings of a second pass: the ranges of consecutive chunks tile the list
    kept = np.sort(rng.choice(4097, size=700, replace=False)).astype(np.uint64)
    for width in (1, 15, 16, 64, 100, 4097):
        at = 0
        for c0 in range(0, 4097, width):
            k0, k1 = pkg.input_kept_range_host(kept, c0, min(width, 4097 - c0))
            assert k0 == at and (k0, k1) == rmodel.kept_range(kept, c0, min(width, 4097 - c0))
            at = k1
        assert at == len(kept)
    # refusals
    lib = pkg.load_library()
    a, b = C.c_uint64(), C.c_uint64()
    assert lib.fseq_debug_input_kept_range(None, 3, 0, 5, C.byref(a), C.byref(b)) == pkg.FSEQ_E_ARG
    assert lib.fseq_debug_input_kept_range(kept.ctypes.data, len(kept), 0, 5, None, C.byref(b)) == pkg.FSEQ_E_ARG
    assert lib.fseq_debug_input_kept_range(kept.ctypes.data, len(kept), 0, 5, C.byref(a), None) == pkg.FSEQ_E_ARG


def test_kept_range_under_the_sanitizers(tmp_path):
    """The header is host-only: tests/input_kept_range_sanitized.cpp includes it alone and runs random lists, every tiling and the
    corners on arrays of exactly the lengths given, as a program of its own under AddressSanitizer and UndefinedBehaviorSanitizer
    (nothing loaded into Python runs under either)."""
    here = os.path.dirname(os.path.abspath(__file__))
    exe = str(tmp_path / "input_kept_range_sanitized")
    subprocess.run(["g++", "-std=c++17", "-g", "-O1", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", os.path.join(os.path.dirname(here), "founder-sequences_amd", "csrc"), os.path.join(here, "input_kept_range_sanitized.cpp"), "-o", exe], check=True)
    p = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120)
    assert p.returncode == 0 and p.stdout.strip() == "ok", p.stderr[-3000:]
