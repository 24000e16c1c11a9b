"""CPU checks of the boundary of the segments file in source co-ordinates (include/fseq.h: fseq_get_segments_restored,
fseq_write_segments_restored; include/fseq_debug.h: fseq_debug_restored_bounds): the symbols, both headers as C99, the refusals
that need no device (a context needs one: the others are in tests/test_gpu_segments_restored.py) and the front end's grammar."""
import ctypes as C
import importlib
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("fseq_get_segments_restored", "fseq_write_segments_restored")
DEBUG_ENTRIES = ("fseq_debug_restored_bounds",)


@pytest.fixture(scope="module")
def build():
    return importlib.import_module("founder-sequences_amd.build")


@pytest.fixture(scope="module")
def pkg(build):
    build.build()
    return importlib.import_module("founder-sequences_amd")


def test_library_exports_the_entry_points(pkg):
    lib = pkg.load_library()
    for name in ENTRIES:
        assert hasattr(lib, name) and name in pkg.EXPORTS and name not in pkg.DEBUG_EXPORTS
    for name in DEBUG_ENTRIES:
        assert hasattr(lib, name) and name in pkg.EXPORTS and name in pkg.DEBUG_EXPORTS
    assert lib.fseq_abi_version() == 5                       # (detected by symbol: no struct of the boundary changed)
    for name in ("segments_restored", "write_segments_restored"):
        assert callable(getattr(pkg.SegmentationContext, name))
    assert callable(pkg.restored_bounds_host)


def test_headers_as_c99(pkg, tmp_path):
    src = tmp_path / "t.c"
    src.write_text('#include <stdio.h>\n#include "fseq.h"\n#include "fseq_debug.h"\n'
                   'int main(void){\n'
                   'int (*a)(fseq_ctx *, fseq_segment *) = fseq_get_segments_restored;\n'
                   'int (*b)(fseq_ctx *, int, char const *) = fseq_write_segments_restored;\n'
                   'int (*c)(uint64_t const *, uint64_t, uint64_t, uint64_t const *, uint64_t const *, uint64_t, uint64_t *, uint64_t *) = fseq_debug_restored_bounds;\n'
                   'uint64_t kept[3] = {1, 2, 5}, lb[2] = {0, 1}, rb[2] = {1, 3}, slb[2], srb[2];\n'
                   'int rc = c(kept, 3, 7, lb, rb, 2, slb, srb);\n'
                   'printf("%d %d %d %d %d %d %d\\n", FSEQ_ABI_VERSION, a != 0 && b != 0, rc, (int) slb[0], (int) srb[0], (int) slb[1], (int) srb[1]); return 0; }\n')
    exe = tmp_path / "t"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe),
                    "-L", os.path.dirname(pkg.LIB_PATH), "-l:" + os.path.basename(pkg.LIB_PATH), "-Wl,-rpath," + os.path.dirname(pkg.LIB_PATH)], check=True)
    out = list(map(int, subprocess.run([str(exe)], capture_output=True, check=True).stdout.split()))
    assert out == [5, 1, pkg.FSEQ_OK, 0, 2, 2, 7]


def test_null_arguments_fail_without_a_device(pkg, tmp_path):
    lib = pkg.load_library()
    seg = (C.c_uint64 * 6)()
    path = str(tmp_path / "s.txt")
    assert lib.fseq_get_segments_restored(None, seg) == pkg.FSEQ_E_ARG
    for joining in (pkg.JOIN_GREEDY, pkg.JOIN_BIPARTITE, pkg.JOIN_RANDOM, 3):
        assert lib.fseq_write_segments_restored(None, joining, path.encode()) == pkg.FSEQ_E_ARG
    assert not os.path.exists(path)
    kept, lb, rb, out = (C.c_uint64 * 2)(1, 3), (C.c_uint64 * 1)(0), (C.c_uint64 * 1)(2), (C.c_uint64 * 1)(7)
    bounds = lib.fseq_debug_restored_bounds
    assert bounds(kept, 2, 5, lb, rb, 1, out, out) == pkg.FSEQ_OK
    for args in ((None, 2, 5, lb, rb, 1, out, out), (kept, 2, 5, None, rb, 1, out, out), (kept, 2, 5, lb, None, 1, out, out),
                 (kept, 2, 5, lb, rb, 1, None, out), (kept, 2, 5, lb, rb, 1, out, None), (kept, 2, 5, lb, rb, 0, out, out)):
        assert bounds(*args) == pkg.FSEQ_E_ARG, args


def test_front_end_names_the_option_and_refuses_it_alone(build, tmp_path):
    cli = build.build_cli()
    r = subprocess.run([cli, "--help"], capture_output=True, timeout=60)
    assert r.returncode == 0 and b"--output-restored-segments=PATH" in r.stdout
    base = [cli, "--input", str(tmp_path / "missing.txt"), "--output-founders", str(tmp_path / "f"), "--segment-length-bound", "5"]
    N, R, E = ["--output-restored-segments", str(tmp_path / "r")], ["--remove-identity-columns"], ["--output-segments", str(tmp_path / "e")]
    refused = ((N, b"--output-restored-segments requires --remove-identity-columns"),
               (N + E, b"--output-restored-segments requires --remove-identity-columns"),
               (N + R + ["--gpus", "2"], b"--output-restored-segments is not supported together with --gpus > 1"),
               (N + ["--gpus", "2"], b"is not supported together with --gpus > 1"),
               # today's refusal stays: the reduced file under --upload-memory, with or without the new option beside it
               (R + E + ["--upload-memory=1"], b"--upload-memory is not supported together with --output-segments"),
               (N + R + E + ["--upload-memory=1"], b"--upload-memory is not supported together with --output-segments"))
    for extra, word in refused:
        r = subprocess.run(base + extra, capture_output=True, timeout=60)
        assert r.returncode != 0 and word in r.stderr, (extra, r.stderr)
        assert b"Loading the input" not in r.stderr and b"Unable to open" not in r.stderr
        assert not any((tmp_path / x).exists() for x in "fre")
    # admitted: the command line passes the checks of the options and fails on the input that does not exist
    for extra in (N + R, N + R + E, N + R + ["--upload-memory=1"], N + R + ["--segment-joining", "random", "--upload-memory=1"]):
        r = subprocess.run(base + extra, capture_output=True, timeout=60)
        assert r.returncode != 0 and b"not supported" not in r.stderr and b"requires" not in r.stderr, (extra, r.stderr)
        assert not (tmp_path / "r").exists()
