"""The restored block graph's entries (include/fseq.h: fseq_write_block_graph_restored, fseq_graph_thread_rows_restored,
fseq_graph_thread_held_out_restored) on the CPU: declared, exported and bound; the refusals that are decided before a device is
touched; the front end's new refusals, and that the old ones keep their words.  (A context cannot be made without a device: what
is refused of a context is in tests/test_gpu_block_graph_restored.py and tests/test_gpu_graph_thread_restored.py.)"""
import ctypes as C
import importlib
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("fseq_write_block_graph_restored", "fseq_graph_thread_rows_restored", "fseq_graph_thread_held_out_restored")


@pytest.fixture(scope="module")
def pkg():
    build = importlib.import_module("founder-sequences_amd.build")
    build.build()
    return importlib.import_module("founder-sequences_amd")


def test_new_symbols_are_declared_exported_and_bound(pkg):
    lib = pkg.load_library()
    vp = C.c_void_p
    for name in NEW:
        assert hasattr(lib, name) and name in pkg.EXPORTS and name not in pkg.DEBUG_EXPORTS, name
    assert lib.fseq_write_block_graph_restored.argtypes == [vp, C.c_uint32, C.c_int, C.c_char_p] == lib.fseq_write_block_graph.argtypes
    assert lib.fseq_graph_thread_rows_restored.argtypes == [vp, C.POINTER(vp), C.c_uint32, vp, vp, vp, vp, C.POINTER(pkg.GraphThreadSummary)]
    assert lib.fseq_graph_thread_rows_restored.argtypes == lib.fseq_graph_thread_rows.argtypes
    assert lib.fseq_graph_thread_held_out_restored.argtypes == [vp, vp, vp, vp, vp, C.POINTER(pkg.GraphThreadSummary)] == lib.fseq_graph_thread_held_out.argtypes
    assert lib.fseq_abi_version() == 5                       # (detected by symbol: no struct of the boundary changed)
    for name in ("write_block_graph_restored", "graph_thread_rows_restored", "graph_thread_held_out_restored"):
        assert callable(getattr(pkg.SegmentationContext, name)), name
    text = open(os.path.join(ROOT, "include", "fseq.h")).read()
    assert all(("int  %s(" % n) in text for n in NEW)


def test_the_header_compiles_as_c_and_links(pkg, tmp_path):
    src = tmp_path / "t.c"
    src.write_text('#include "fseq.h"\nint main(void){\n'
                   '  return 0 * (fseq_write_block_graph_restored(0, 0, -1, 0) + fseq_graph_thread_rows_restored(0, 0, 0, 0, 0, 0, 0, 0)\n'
                   '              + fseq_graph_thread_held_out_restored(0, 0, 0, 0, 0, 0));\n}\n')
    exe = tmp_path / "t"
    libdir = os.path.dirname(pkg.LIB_PATH)
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe),
                    "-L", libdir, "-lfseq_hip", "-Wl,-rpath," + libdir, "-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib"], check=True)
    assert subprocess.run([str(exe)]).returncode == 0


def test_refusals_before_a_device_is_touched(pkg, tmp_path):
    """No context: FSEQ_E_ARG from every entry, whatever the other arguments, and nothing is written through them."""
    lib = pkg.load_library()
    sm = pkg.GraphThreadSummary(7, 7, 7, 7, 7, 7, 7, 7.0)
    row = np.frombuffer(b"ACGT", dtype=np.uint8).copy()
    rows = (C.c_void_p * 1)(row.ctypes.data)
    nodes = np.full(4, 9, dtype=np.uint32)
    path = tmp_path / "g.gfa"
    assert lib.fseq_write_block_graph_restored(None, 1, 45, str(path).encode()) == pkg.FSEQ_E_ARG and not path.exists()
    assert lib.fseq_graph_thread_rows_restored(None, rows, 1, nodes.ctypes.data, None, None, None, C.byref(sm)) == pkg.FSEQ_E_ARG
    assert lib.fseq_graph_thread_rows_restored(None, None, 0, None, None, None, None, None) == pkg.FSEQ_E_ARG
    assert lib.fseq_graph_thread_held_out_restored(None, nodes.ctypes.data, None, None, None, C.byref(sm)) == pkg.FSEQ_E_ARG
    assert (sm.rows, sm.segments, sm.rows_on_graph) == (7, 7, 7) and (nodes == 9).all()


def test_front_end_refusals_and_usage(tmp_path):
    cli = importlib.import_module("founder-sequences_amd.build").build_cli()
    lst = str(tmp_path / "list.txt")
    (tmp_path / "list.txt").write_text("")
    base = [cli, "--input", lst, "--segment-length-bound", "5"]
    out = tmp_path / "t.txt"

    def refused(args, words):
        r = subprocess.run(base + args, capture_output=True, timeout=60)
        assert r.returncode != 0 and words in r.stderr, (args, r.stderr)
        assert not out.exists()

    # the new options' own
    refused(["--output-restored-graph", str(out)], b"--output-restored-graph requires --remove-identity-columns")
    refused(["--output-restored-graph", str(out), "--remove-identity-columns", "--gpus", "2"], b"--output-restored-graph is not supported together with --gpus > 1")
    for option, with_, needs in (("--output-held-out-restored-graph-threads", ["--hold-out", "0"], b"--hold-out"),
                                 ("--output-sequence-restored-graph-threads", ["--match-sequences", lst], b"--match-sequences")):
        words = option.encode() + b" requires " + needs + b" and --remove-identity-columns."
        refused([option, str(out)], words)
        refused(with_ + [option, str(out)], words)
        refused(["--remove-identity-columns", option, str(out)], words)
        refused(with_ + ["--remove-identity-columns", option, str(out), "--gpus", "2"], option.encode() + b" is not supported together with --gpus > 1")
    refused(["--hold-out", "0", "--remove-identity-columns", "--upload-memory", "1", "--reduce-on-upload", "--output-held-out-restored-graph-threads", str(out)],
            b"--reduce-on-upload is not supported together with --hold-out")
    # the earlier refusals keep their words
    refused(["--graph-paths"], b"--graph-paths requires --output-graph.")
    refused(["--graph-gap-character", "A"], b"--graph-gap-character requires --output-graph.")
    refused(["--output-restored-graph", str(out), "--remove-identity-columns", "--graph-gap-character", "AB"], b"The gap character of the graph must be one character")
    refused(["--output-graph", str(out), "--gpus", "2"], b"--output-graph is not supported together with --gpus > 1 (a rank holds its own columns and boundary states only).")
    refused(["--match-sequences", lst], b"--match-sequences requires --output-sequence-matches.")
    refused(["--match-sequences", lst, "--output-sequence-matches", str(out), "--remove-identity-columns"],
            b"--match-sequences is not supported together with --remove-identity-columns (the match would be in reduced co-ordinates).")
    refused(["--match-sequences", lst, "--output-sequence-matches", str(out), "--output-sequence-restored-graph-threads", str(out), "--remove-identity-columns"],
            b"--match-sequences is not supported together with --remove-identity-columns (the match would be in reduced co-ordinates).")
    refused(["--hold-out", "0", "--remove-identity-columns"],
            b"--hold-out is not supported together with --remove-identity-columns (the held-out sequences would have to lose the same columns).")
    refused(["--hold-out", "0", "--remove-identity-columns", "--output-held-out-matches", str(out), "--output-held-out-restored-graph-threads", str(out)],
            b"--hold-out is not supported together with --remove-identity-columns (the held-out sequences would have to lose the same columns).")
    for option, with_ in (("--output-held-out-graph-threads", ["--hold-out", "0"]), ("--output-sequence-graph-threads", ["--match-sequences", lst])):
        refused(with_ + [option, str(out), "--remove-identity-columns"], option.encode() + b" is not supported together with --remove-identity-columns (the sequences would be threaded in reduced co-ordinates).")
    # with their options the new ones pass the refusals (an empty list: nothing to segment, nothing written, success)
    for args in (["--remove-identity-columns", "--output-restored-graph", str(out), "--graph-paths", "--graph-gap-character", ""],
                 ["--remove-identity-columns", "--match-sequences", lst, "--output-sequence-restored-graph-threads", str(out)],
                 ["--remove-identity-columns", "--hold-out", "0", "--output-held-out-restored-graph-threads", str(out)],
                 ["--remove-identity-columns", "--upload-memory", "1", "--reduce-on-upload", "--output-restored-graph", str(out), "--match-sequences", lst,
                  "--output-sequence-restored-graph-threads", str(out)]):
        r = subprocess.run(base + args, capture_output=True, timeout=60)
        assert r.returncode == 0 and b"The input file contained no sequences." in r.stderr, (args, r.stderr)
    usage = subprocess.run([cli, "--help"], capture_output=True, timeout=60).stdout
    for option in (b"--output-restored-graph=PATH", b"--output-held-out-restored-graph-threads=PATH", b"--output-sequence-restored-graph-threads=PATH",
                   b"--output-graph=PATH", b"--output-held-out-graph-threads=PATH", b"--output-sequence-graph-threads=PATH"):
        assert option in usage, option
