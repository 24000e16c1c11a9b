"""The graph threading's entries (include/fseq.h: fseq_graph_thread_rows, fseq_graph_thread_held_out; include/fseq_debug.h:
fseq_debug_graph_thread) on the CPU: declared, exported and bound; the structs against the header; the refusals that are decided
before a device is touched; the front end's refusals.  (A context cannot be made without a device: what is refused of a context
is in tests/test_gpu_graph_thread.py.)"""
import ctypes as C
import importlib
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("fseq_graph_thread_rows", "fseq_graph_thread_held_out", "fseq_debug_graph_thread")


@pytest.fixture(scope="module")
def pkg():
    build = importlib.import_module("founder-sequences_amd.build")
    build.build()
    return importlib.import_module("founder-sequences_amd")


def test_new_symbols_are_declared_exported_and_bound(pkg):
    lib = pkg.load_library()
    for name in NEW:
        assert hasattr(lib, name) and name in pkg.EXPORTS, name
        assert (name in pkg.DEBUG_EXPORTS) == name.startswith("fseq_debug_"), name
        assert getattr(lib, name).argtypes is not None, name
    assert len(lib.fseq_graph_thread_rows.argtypes) == 8 and len(lib.fseq_graph_thread_held_out.argtypes) == 6
    assert lib.fseq_abi_version() == 5                       # (detected by symbol: no struct of the boundary changed)
    for name in ("graph_thread_rows", "graph_thread_held_out", "graph_thread_info"):
        assert callable(getattr(pkg.SegmentationContext, name)), name
    assert pkg.GRAPH_NONE == 0xFFFFFFFF
    for header, names in (("fseq.h", NEW[:2]), ("fseq_debug.h", NEW[2:])):
        text = open(os.path.join(ROOT, "include", header)).read()
        assert all(("int  %s(" % n) in text for n in names), header


def test_struct_layouts_match_header(pkg, tmp_path):
    assert pkg.GRAPH_THREAD_ROW_DTYPE.itemsize == 40 and pkg.GRAPH_THREAD_SEGMENT_DTYPE.itemsize == 16
    assert C.sizeof(pkg.GraphThreadSummary) == 64 and C.sizeof(pkg.GraphThreadInfo) == 32
    rf = list(pkg.GRAPH_THREAD_ROW_DTYPE.names)
    gf = list(pkg.GRAPH_THREAD_SEGMENT_DTYPE.names)
    sf = [k for k, _ in pkg.GraphThreadSummary._fields_]
    nf = [k for k, _ in pkg.GraphThreadInfo._fields_]
    assert rf == ["columns_matched", "longest_walk_columns", "segments_matched", "junctions_linked", "junctions_novel", "walks", "longest_walk_segments", "reserved"]
    assert gf == ["matched", "linked", "novel", "reserved"]
    assert sf == ["rows", "segments", "segments_matched", "junctions_linked", "junctions_novel", "walks", "rows_on_graph", "ms_device"]
    assert nf == ["key_bits", "table_slots", "candidates_verified", "candidates_rejected", "queries_out_of_alphabet"]
    src = tmp_path / "t.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "fseq.h"\n#include "fseq_debug.h"\nint main(void){\n'
                   '  printf("%zu %zu %zu %zu %u", sizeof(fseq_graph_thread_row), sizeof(fseq_graph_thread_segment), sizeof(fseq_graph_thread_summary),\n'
                   '         sizeof(fseq_graph_thread_info), (unsigned) FSEQ_GRAPH_NONE);\n'
                   + "".join('  printf(" %%zu", offsetof(fseq_graph_thread_row, %s));\n' % f for f in rf)
                   + "".join('  printf(" %%zu", offsetof(fseq_graph_thread_segment, %s));\n' % f for f in gf)
                   + "".join('  printf(" %%zu", offsetof(fseq_graph_thread_summary, %s));\n' % f for f in sf)
                   + "".join('  printf(" %%zu", offsetof(fseq_graph_thread_info, %s));\n' % f for f in nf)
                   + '  return 0 * (fseq_graph_thread_rows(0, 0, 0, 0, 0, 0, 0, 0) + fseq_graph_thread_held_out(0, 0, 0, 0, 0, 0) + fseq_debug_graph_thread(0, 0));\n}\n')
    exe = tmp_path / "t"
    libdir = os.path.dirname(pkg.LIB_PATH)
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe),
                    "-L", libdir, "-lfseq_hip", "-Wl,-rpath," + libdir, "-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib"], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], stdout=subprocess.PIPE, text=True, check=True).stdout.split()]
    want = ([40, 16, 64, 32, pkg.GRAPH_NONE] + [pkg.GRAPH_THREAD_ROW_DTYPE.fields[f][1] for f in rf] + [pkg.GRAPH_THREAD_SEGMENT_DTYPE.fields[f][1] for f in gf]
            + [getattr(pkg.GraphThreadSummary, f).offset for f in sf] + [getattr(pkg.GraphThreadInfo, f).offset for f in nf])
    assert got == want


def test_model_layouts_are_the_bindings(pkg):
    import graph_thread_model as tm
    assert tm.ROW_DTYPE == pkg.GRAPH_THREAD_ROW_DTYPE and tm.SEGMENT_DTYPE == pkg.GRAPH_THREAD_SEGMENT_DTYPE and tm.NONE == pkg.GRAPH_NONE


def test_refusals_before_a_device_is_touched(pkg):
    """No context: FSEQ_E_ARG from every entry, whatever the other arguments, and nothing is written through them."""
    lib = pkg.load_library()
    sm = pkg.GraphThreadSummary(7, 7, 7, 7, 7, 7, 7, 7.0)
    row = np.frombuffer(b"ACGT", dtype=np.uint8).copy()
    rows = (C.c_void_p * 1)(row.ctypes.data)
    nodes = np.full(4, 9, dtype=np.uint32)
    assert lib.fseq_graph_thread_rows(None, rows, 1, nodes.ctypes.data, None, None, None, C.byref(sm)) == pkg.FSEQ_E_ARG
    assert lib.fseq_graph_thread_rows(None, None, 0, None, None, None, None, None) == pkg.FSEQ_E_ARG
    assert lib.fseq_graph_thread_held_out(None, nodes.ctypes.data, None, None, None, C.byref(sm)) == pkg.FSEQ_E_ARG
    assert (sm.rows, sm.segments, sm.rows_on_graph) == (7, 7, 7) and (nodes == 9).all()
    info = pkg.GraphThreadInfo(3, 3, 3, 3, 3)
    assert lib.fseq_debug_graph_thread(None, C.byref(info)) == pkg.FSEQ_E_ARG and info.key_bits == 3


def test_front_end_refusals_and_usage(tmp_path):
    cli = importlib.import_module("founder-sequences_amd.build").build_cli()
    (tmp_path / "list.txt").write_text("")
    base = [cli, "--input", str(tmp_path / "list.txt"), "--segment-length-bound", "5"]
    out = tmp_path / "t.txt"
    for option, with_, needs in (("--output-held-out-graph-threads", ["--hold-out", "0"], b"--hold-out"),
                                 ("--output-sequence-graph-threads", ["--match-sequences", str(tmp_path / "list.txt")], b"--match-sequences")):
        r = subprocess.run(base + [option, str(out)], capture_output=True, timeout=60)
        assert r.returncode != 0 and option.encode() + b" requires " + needs + b"." in r.stderr, r.stderr
        r = subprocess.run(base + with_ + [option, str(out), "--gpus", "2"], capture_output=True, timeout=60)
        assert r.returncode != 0 and option.encode() + b" is not supported together with --gpus > 1" in r.stderr, r.stderr
        r = subprocess.run(base + with_ + [option, str(out), "--remove-identity-columns"], capture_output=True, timeout=60)
        assert r.returncode != 0 and option.encode() + b" is not supported together with --remove-identity-columns" in r.stderr, r.stderr
        assert not out.exists()
    # what --match-sequences said without an output, it still says
    r = subprocess.run(base + ["--match-sequences", str(tmp_path / "list.txt")], capture_output=True, timeout=60)
    assert r.returncode != 0 and b"--match-sequences requires --output-sequence-matches." in r.stderr
    usage = subprocess.run([cli, "--help"], capture_output=True, timeout=60).stdout
    assert b"--output-held-out-graph-threads=PATH" in usage and b"--output-sequence-graph-threads=PATH" in usage
