"""CPU checks of the chunked input boundary (include/fseq.h, fseq_input_begin .. fseq_set_rows_streamed; include/fseq_debug.h,
fseq_debug_device_bytes): the symbols, the header as C, the refusals that must not touch a device, the front end's
--upload-memory -- and the numpy model (tests/input_model.py) the GPU tests (tests/test_gpu_input_stream.py) compare against."""
import ctypes as C
import importlib
import os
import subprocess

import numpy as np
import pytest

import input_model as model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["fseq_input_begin", "fseq_input_chunk_columns", "fseq_input_scan", "fseq_input_columns", "fseq_input_end", "fseq_set_rows_streamed"]


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
        assert name in pkg.EXPORTS and name not in pkg.DEBUG_EXPORTS
    for name in ("fseq_debug_device_bytes", "fseq_debug_packed_columns"):
        assert hasattr(lib, name) and name in pkg.EXPORTS and name in pkg.DEBUG_EXPORTS
    assert lib.fseq_abi_version() == 5                       # (detected by symbol: no struct of the boundary changed)


def test_headers_compile_as_c(tmp_path):
    src = tmp_path / "t.c"
    src.write_text('#include "fseq.h"\n#include "fseq_debug.h"\n'
                   'int main(void){ uint64_t a = 0, b = 0; return (int) fseq_input_chunk_columns(0) + fseq_input_begin(0, 0, 0, 0) * 0'
                   ' + 0 * fseq_debug_device_bytes(0, &a, &b, 0); }\n')
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)], check=True)


def test_null_arguments_fail_without_touching_a_device(pkg):
    lib = pkg.load_library()
    rows = (C.c_void_p * 2)()
    now, peak = C.c_uint64(), C.c_uint64()
    assert lib.fseq_input_begin(None, None, 0, 0) == pkg.FSEQ_E_ARG
    assert lib.fseq_input_chunk_columns(None) == 0
    assert lib.fseq_input_scan(None, 0, 1, rows) == pkg.FSEQ_E_ARG
    assert lib.fseq_input_columns(None, 0, 1, rows) == pkg.FSEQ_E_ARG
    assert lib.fseq_input_end(None) == pkg.FSEQ_E_ARG
    assert lib.fseq_set_rows_streamed(None, rows, 0) == pkg.FSEQ_E_ARG
    assert lib.fseq_debug_device_bytes(None, C.byref(now), C.byref(peak), 0) == pkg.FSEQ_E_ARG
    # a context that is not looked at: the row pointer is checked first
    h = C.c_void_p(0)
    assert lib.fseq_input_scan(h, 0, 1, None) == pkg.FSEQ_E_ARG
    assert lib.fseq_input_columns(h, 0, 1, None) == pkg.FSEQ_E_ARG
    assert lib.fseq_set_rows_streamed(h, None, 0) == pkg.FSEQ_E_ARG


def test_front_end_lists_the_option_and_refuses_what_is_out_of_scope(build, tmp_path):
    cli = build.build_cli()
    r = subprocess.run([cli, "--help"], capture_output=True, timeout=60)
    assert r.returncode == 0 and b"--upload-memory=MIB" in r.stdout
    common = [cli, "--input", str(tmp_path / "missing.txt"), "--segment-length-bound", "5", "--output-founders", str(tmp_path / "f")]
    refusals = [
        (["--upload-memory", "4", "--input-format", "FASTA"], b"--upload-memory is not supported together with --input-format=FASTA"),
        (["--upload-memory", "4", "--gpus", "2"], b"--upload-memory is not supported together with --gpus > 1"),
        (["--upload-memory", "0"], b"The upload memory must be a positive number of MiB."),
        (["--upload-memory=-1"], b"The upload memory must be a positive number of MiB."),
        (["--upload-memory", "x"], b"The upload memory must be a positive number of MiB."),
        (["--upload-memory", "4", "--output-segments", str(tmp_path / "s")], b"--upload-memory is not supported together with --output-segments under bipartite-matching or random"),
        (["--upload-memory", "4", "--output-segments", str(tmp_path / "s"), "--segment-joining", "random"],
         b"--upload-memory is not supported together with --output-segments under bipartite-matching or random"),
    ]
    for extra, message in refusals:
        r = subprocess.run(common + extra, capture_output=True, timeout=60)
        # refused before any input is read and any device is looked for: the input does not exist, and the message is the option's
        assert r.returncode != 0 and message in r.stderr, (extra, r.stderr)
        assert b"Loading the input" not in r.stderr
        assert not (tmp_path / "f").exists() and not (tmp_path / "s").exists()
    # accepted with greedy joining: the run then stops at the input, which is missing
    r = subprocess.run(common + ["--upload-memory", "4", "--output-segments", str(tmp_path / "s"), "--segment-joining", "greedy"], capture_output=True, timeout=60)
    assert r.returncode != 0 and b"Unable to open the input file" in r.stderr


def test_model_code_table(pkg):
    msa = np.frombuffer(b"TACG" b"GGAT" b"\xf0A\xf0C", dtype=np.uint8).reshape(3, 4)
    table, sigma, bits = model.code_table(msa)
    assert sigma == 5 and bits == 4
    assert [int(table[b]) for b in b"ACGT\xf0"] == [0, 1, 2, 3, 4] and (np.delete(table, list(b"ACGT\xf0")) == -1).all()
    # a supplied alphabet in any order: ascending codes, the unused byte keeps its code
    table, sigma, bits = model.code_table(msa, b"\xf0TN-GCA")
    assert sigma == 7 and bits == 4
    assert [int(table[b]) for b in b"-ACGNT\xf0"] == list(range(7))
    assert model.outside(msa, b"ACGT") == [0xF0] and model.outside(msa, b"ACGT\xf0") == []


@pytest.mark.parametrize("m,size", [(1, 1), (3, 4), (5, 2), (17, 5), (33, 16), (64, 17), (65, 256)])
def test_model_packed_columns(pkg, m, size):
    alpha = model.alphabet_bytes(size, m)
    assert len(alpha) == size and list(alpha) == sorted(set(alpha)) and (size == 1 or max(alpha) > 127)
    msa = model.mosaic(m, m, 300, alpha)
    assert set(np.unique(msa).tolist()) == set(alpha)
    packed, bits = model.packed_columns(pkg, msa)
    assert bits == (2 if size <= 4 else 4 if size <= 16 else 8)
    per = 8 // bits
    ld = ((m + per - 1) // per + 15) // 16 * 16
    assert packed.shape == (300, ld)
    table, _, _ = model.code_table(msa)
    for r in range(m):                                       # row r of a column: field r % per of byte r // per
        assert np.array_equal((packed[:, r // per] >> (bits * (r % per))) & ((1 << bits) - 1), table[msa[r]])
    # what lies behind row m - 1 is zero: the padding fields of the last byte in use, the padding bytes up to ld
    used = np.zeros((300, ld * per), dtype=np.uint8)
    used[:, :m] = table[msa].T
    again = np.zeros_like(packed)
    for j in range(per):
        again |= (used[:, j::per] << (bits * j)).astype(np.uint8)
    assert np.array_equal(again, packed) and not packed[:, (m + per - 1) // per:].any()
