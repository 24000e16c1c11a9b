"""The nearest-node entries (include/fseq.h: fseq_graph_nearest_rows, fseq_graph_nearest_held_out; include/fseq_debug.h:
fseq_debug_graph_nearest_info, fseq_debug_graph_nearest_plan, fseq_debug_graph_nearest) on the CPU: declared, exported and bound;
the structs against the header, compiled as C99; the refusals that are decided before a device is touched; the batch cut against
a restatement in Python and as a program under the host sanitizers; the knob in the README's table; the front end's refusals.
(A context cannot be made without a device: what is refused of a context is in tests/test_gpu_graph_nearest.py.)"""
import ctypes as C
import importlib
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("fseq_graph_nearest_rows", "fseq_graph_nearest_held_out", "fseq_debug_graph_nearest_info", "fseq_debug_graph_nearest_plan", "fseq_debug_graph_nearest")


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
    assert len(lib.fseq_graph_nearest_rows.argtypes) == 11 and len(lib.fseq_graph_nearest_held_out.argtypes) == 9
    assert len(lib.fseq_debug_graph_nearest_plan.argtypes) == 9 and len(lib.fseq_debug_graph_nearest.argtypes) == 22
    assert lib.fseq_abi_version() == 5                       # (detected by symbol: no struct of the boundary changed)
    for name in ("graph_nearest_rows", "graph_nearest_held_out", "graph_nearest_info"):
        assert callable(getattr(pkg.SegmentationContext, name)), name
    assert callable(pkg.graph_nearest_plan_host) and callable(pkg.debug_graph_nearest)
    for header, names in (("fseq.h", NEW[:2]), ("fseq_debug.h", NEW[2:])):
        text = open(os.path.join(ROOT, "include", header)).read()
        assert all(("int  %s(" % n) in text for n in names), header
    text = open(os.path.join(ROOT, "include", "fseq.h")).read()
    for limit in ("identity-reduced", "sharded contexts and a host form"):
        assert limit in text[text.index("the NEAREST node"):text.index("int  fseq_graph_nearest_rows(")], limit


def test_struct_layouts_match_header(pkg, tmp_path):
    assert pkg.GRAPH_NEAREST_ROW_DTYPE.itemsize == 64 and pkg.GRAPH_NEAREST_SEGMENT_DTYPE.itemsize == 32
    assert C.sizeof(pkg.GraphNearestSummary) == 80 and C.sizeof(pkg.GraphNearestInfo) == 32
    rf = list(pkg.GRAPH_NEAREST_ROW_DTYPE.names)
    gf = list(pkg.GRAPH_NEAREST_SEGMENT_DTYPE.names)
    sf = [k for k, _ in pkg.GraphNearestSummary._fields_]
    nf = [k for k, _ in pkg.GraphNearestInfo._fields_]
    assert rf == ["columns_admitted", "longest_walk_columns", "mismatches_admitted", "mismatches", "segments_admitted", "segments_exact", "junctions_linked",
                  "junctions_novel", "walks", "longest_walk_segments", "max_distance", "reserved"]
    assert gf == ["mismatches", "admitted", "exact", "linked", "novel", "max_distance", "reserved"]
    assert sf == ["rows", "segments", "segments_admitted", "segments_exact", "junctions_linked", "junctions_novel", "walks", "rows_on_graph", "mismatches", "ms_device"]
    assert nf == ["batches", "packed_words", "query_words", "bits", "reserved"]
    src = tmp_path / "t.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "fseq.h"\n#include "fseq_debug.h"\nint main(void){\n'
                   '  printf("%zu %zu %zu %zu", sizeof(fseq_graph_nearest_row), sizeof(fseq_graph_nearest_segment), sizeof(fseq_graph_nearest_summary),\n'
                   '         sizeof(fseq_graph_nearest_info));\n'
                   + "".join('  printf(" %%zu", offsetof(fseq_graph_nearest_row, %s));\n' % f for f in rf)
                   + "".join('  printf(" %%zu", offsetof(fseq_graph_nearest_segment, %s));\n' % f for f in gf)
                   + "".join('  printf(" %%zu", offsetof(fseq_graph_nearest_summary, %s));\n' % f for f in sf)
                   + "".join('  printf(" %%zu", offsetof(fseq_graph_nearest_info, %s));\n' % f for f in nf)
                   + '  return 0 * (fseq_graph_nearest_rows(0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0) + fseq_graph_nearest_held_out(0, 0, 0, 0, 0, 0, 0, 0, 0)\n'
                     '              + fseq_debug_graph_nearest_info(0, 0) + fseq_debug_graph_nearest_plan(0, 0, 0, 0, 0, 0, 0, 0, 0)\n'
                     '              + fseq_debug_graph_nearest(0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0));\n}\n')
    exe = tmp_path / "t"
    libdir = os.path.dirname(pkg.LIB_PATH)
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe),
                    "-L", libdir, "-lfseq_hip", "-Wl,-rpath," + libdir, "-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib"], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], stdout=subprocess.PIPE, text=True, check=True).stdout.split()]
    want = ([64, 32, 80, 32] + [pkg.GRAPH_NEAREST_ROW_DTYPE.fields[f][1] for f in rf] + [pkg.GRAPH_NEAREST_SEGMENT_DTYPE.fields[f][1] for f in gf]
            + [getattr(pkg.GraphNearestSummary, f).offset for f in sf] + [getattr(pkg.GraphNearestInfo, f).offset for f in nf])
    assert got == want


def test_model_layouts_are_the_bindings(pkg):
    import graph_nearest_model as nm
    assert nm.ROW_DTYPE == pkg.GRAPH_NEAREST_ROW_DTYPE and nm.SEGMENT_DTYPE == pkg.GRAPH_NEAREST_SEGMENT_DTYPE and nm.NONE == pkg.GRAPH_NONE
    assert list(nm.SUMMARY) == [k for k, _ in pkg.GraphNearestSummary._fields_][:-1]


def test_refusals_before_a_device_is_touched(pkg):
    """No context: FSEQ_E_ARG from every entry, whatever the other arguments, and nothing is written through them."""
    lib = pkg.load_library()
    sm = pkg.GraphNearestSummary(7, 7, 7, 7, 7, 7, 7, 7, 7, 7.0)
    row = np.frombuffer(b"ACGT", dtype=np.uint8).copy()
    rows = (C.c_void_p * 1)(row.ctypes.data)
    out = np.full(4, 9, dtype=np.uint32)
    assert lib.fseq_graph_nearest_rows(None, rows, 1, 0, out.ctypes.data, out.ctypes.data, None, None, None, None, C.byref(sm)) == pkg.FSEQ_E_ARG
    assert lib.fseq_graph_nearest_rows(None, None, 0, 3, None, None, None, None, None, None, None) == pkg.FSEQ_E_ARG
    assert lib.fseq_graph_nearest_held_out(None, 1, out.ctypes.data, None, None, None, None, None, C.byref(sm)) == pkg.FSEQ_E_ARG
    assert (sm.rows, sm.segments, sm.mismatches) == (7, 7, 7) and (out == 9).all()
    info = pkg.GraphNearestInfo(3, 3, 3, 3, 3)
    assert lib.fseq_debug_graph_nearest_info(None, C.byref(info)) == pkg.FSEQ_E_ARG and info.batches == 3


def test_debug_entry_refuses_what_a_kernel_could_index_with(pkg):
    """Every refusal is decided on the host: the device number is one no machine has, so a call that got as far as the device
    would come back with FSEQ_E_HIP and not with FSEQ_E_ARG."""
    rng = np.random.default_rng(2)
    m, n, Q = 9, 40, 5
    codes = rng.integers(0, 4, size=(m, n))
    qcodes = rng.integers(0, 5, size=(Q, n))
    lb, rb = np.array([0, 16, 33]), np.array([16, 33, 40])
    count = np.array([2, 3, 1])
    rep = np.array([[0, 1, 0], [2, 3, 4], [8, 0, 0]])
    nowhere = 1 << 20

    def call(**kw):
        a = dict(codes=codes, bits=2, seg_lb=lb, seg_rb=rb, count=count, rep=rep, query_codes=qcodes, qbits=4, sigma=4, device=nowhere)
        a.update(kw)
        return pkg.debug_graph_nearest(**a)

    with pytest.raises(pkg.FseqError) as err:
        call()
    assert err.value.code == pkg.FSEQ_E_HIP                                     # the base case is in order: it reaches the device
    bad_rep = rep.copy()
    bad_rep[1, 2] = m
    unused_rep = rep.copy()
    unused_rep[0, 2] = m                                                         # behind count[0]: never read, not refused
    with pytest.raises(pkg.FseqError) as err:
        call(rep=unused_rep)
    assert err.value.code == pkg.FSEQ_E_HIP
    refused = {
        "rep >= m": dict(rep=bad_rep),
        "count > X": dict(count=np.array([2, 4, 1])),
        "count == 0": dict(count=np.array([2, 0, 1])),
        "a bound behind n": dict(seg_rb=np.array([16, 33, 41])),
        "bounds out of order": dict(seg_lb=np.array([0, 33, 33]), seg_rb=np.array([16, 16, 40])),
        "an empty segment": dict(seg_lb=np.array([0, 16, 40])),
        "bits": dict(bits=3),
        "qbits": dict(qbits=16),
        "qbits < bits": dict(codes=codes, bits=4, qbits=2, query_codes=qcodes % 4),
        "a code at 2^bits": dict(codes=np.where(codes == 3, 4, codes), sigma=5),
        "a code at sigma": dict(sigma=3),
        "a query code at 2^qbits": dict(query_codes=np.where(qcodes == 4, 16, qcodes)),
        "queries of another length": dict(query_codes=qcodes[:, :-1]),
        "no queries": dict(query_codes=qcodes[:0]),
    }
    for what, kw in refused.items():
        with pytest.raises(pkg.FseqError) as err:
            call(**kw)
        assert err.value.code == pkg.FSEQ_E_ARG, what
    # the C entry itself, on packed columns
    lib = pkg.load_library()
    cols, ld = pkg.pack_columns(codes.astype(np.uint8), 2)
    qcols, qld = pkg.pack_columns(qcodes.astype(np.uint8), 4)
    l64, r64, c32, r32 = lb.astype(np.uint64), rb.astype(np.uint64), count.astype(np.uint32), np.ascontiguousarray(rep, dtype=np.uint32)
    out = np.full((3, 3, Q), 9, dtype=np.uint32)

    def raw(m_=m, n_=n, bits=2, qbits=4, S=3, X=3, Q_=Q, ld_=ld, qld_=qld, rep_=r32, nodes=out[0].ctypes.data):
        return lib.fseq_debug_graph_nearest(nowhere, cols.ctypes.data, ld_, m_, n_, bits, l64.ctypes.data, r64.ctypes.data, c32.ctypes.data, rep_.ctypes.data, S, X,
                                            qcols.ctypes.data, qld_, Q_, qbits, 4, 0, nodes, out[1].ctypes.data, out[2].ctypes.data, None)

    assert raw() == pkg.FSEQ_E_HIP
    bad32 = r32.copy()
    bad32[2, 0] = m
    for kw in (dict(m_=8), dict(n_=39), dict(bits=1), dict(qbits=2, bits=4), dict(S=0), dict(X=2), dict(X=0), dict(Q_=0), dict(ld_=2), dict(qld_=2), dict(rep_=bad32),
               dict(nodes=None)):
        assert raw(**kw) == pkg.FSEQ_E_ARG, kw
    assert (out == 9).all()


def plan_in_python(lb, rb, count, bits, budget):
    cpw = 32 // bits
    nw = [-(-(int(r) - int(l)) // cpw) for l, r in zip(lb, rb)]
    words = [0]
    for w, c in zip(nw, count):
        words.append(words[-1] + w * int(c))
    first, s, S = [0], 0, len(lb)
    while s < S:
        e = s + 1
        while e < S and (words[e + 1] - words[s]) * 4 <= budget - budget % 4:
            e += 1
        first.append(e)
        s = e
    return words, first


def test_plan_against_a_restatement(pkg):
    rng = np.random.default_rng(5)
    for trial in range(60):
        S = int(rng.integers(1, 40))
        widths = rng.integers(1, [2, 40, 600][trial % 3] + 1, size=S)
        rb = np.cumsum(widths)
        lb = rb - widths
        count = rng.integers(1, 70, size=S)
        for bits in (2, 4, 8):
            for budget in (1, 4, 7, 64, 1000, 10 ** 5, 256 << 20):
                words, first = pkg.graph_nearest_plan_host(lb, rb, count, bits, budget)
                want_words, want_first = plan_in_python(lb, rb, count, bits, budget)
                assert words.tolist() == want_words and first.tolist() == want_first, (trial, bits, budget)
    words, first = pkg.graph_nearest_plan_host([0, 15, 31, 48], [15, 31, 48, 49], [2, 1, 3, 5], 2, 12)
    assert words.tolist() == [0, 2, 3, 9, 14] and first.tolist() == [0, 2, 3, 4]
    assert pkg.graph_nearest_plan_host([0], [5003], [3], 2)[1].tolist() == [0, 1] and pkg.GRAPH_NEAREST_BATCH_BYTES == 256 << 20
    for what, args, code in (("no segments", ([], [], [], 2, 8), pkg.FSEQ_E_ARG), ("bits", ([0], [4], [1], 3, 8), pkg.FSEQ_E_ARG), ("budget", ([0], [4], [1], 2, 0), pkg.FSEQ_E_ARG),
                             ("an empty segment", ([0, 4], [4, 4], [1, 1], 2, 8), pkg.FSEQ_E_ARG), ("no class", ([0], [4], [0], 2, 8), pkg.FSEQ_E_ARG),
                             ("2^32 - 1 columns", ([0], [2 ** 32 - 1], [1], 2, 8), pkg.FSEQ_E_UNSUPPORTED)):
        with pytest.raises(pkg.FseqError) as err:
            pkg.graph_nearest_plan_host(*args)
        assert err.value.code == code, what
    assert pkg.graph_nearest_plan_host([0], [2 ** 32 - 2], [1], 8, 8)[0].tolist() == [0, 2 ** 30]


def test_plan_under_the_sanitizers(tmp_path):
    """The header is host-only: tests/graph_nearest_plan_sanitized.cpp includes it alone and runs random segments and every refusal
    on arrays of exactly the lengths given, as a program of its own under AddressSanitizer and UndefinedBehaviorSanitizer (nothing
    loaded into Python runs under either)."""
    here = os.path.dirname(os.path.abspath(__file__))
    exe = str(tmp_path / "graph_nearest_plan_sanitized")
    subprocess.run(["g++", "-std=c++17", "-g", "-O1", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", os.path.join(os.path.dirname(here), "founder-sequences_amd", "csrc"), os.path.join(here, "graph_nearest_plan_sanitized.cpp"), "-o", exe], check=True)
    p = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120)
    assert p.returncode == 0 and p.stdout.strip() == "ok", p.stderr[-3000:]


def test_knob_is_in_the_readme_and_the_library():
    readme = open(os.path.join(ROOT, "README.md")).read()
    assert re.search(r"^\|\s*`FSEQ_GRAPH_NEAREST_BATCH(=[^`]*)?`\s*\|", readme, re.M), "the knob table has no row for FSEQ_GRAPH_NEAREST_BATCH"
    assert '"FSEQ_GRAPH_NEAREST_BATCH"' in open(os.path.join(ROOT, "founder-sequences_amd", "csrc", "fseq_ctx.hpp")).read()
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "fseq_graph_nearest_rows" in design and "fseq_graph_nearest_rows" in readme


def test_front_end_refusals_and_usage(tmp_path):
    cli = importlib.import_module("founder-sequences_amd.build").build_cli()
    (tmp_path / "list.txt").write_text("")
    base = [cli, "--input", str(tmp_path / "list.txt"), "--segment-length-bound", "5"]
    out = tmp_path / "t.txt"
    for option, with_, needs in (("--output-held-out-graph-nearest", ["--hold-out", "0"], b"--hold-out"),
                                 ("--output-sequence-graph-nearest", ["--match-sequences", str(tmp_path / "list.txt")], b"--match-sequences")):
        r = subprocess.run(base + [option, str(out)], capture_output=True, timeout=60)
        assert r.returncode != 0 and option.encode() + b" requires " + needs + b"." in r.stderr, r.stderr
        r = subprocess.run(base + with_ + [option, str(out), "--gpus", "2"], capture_output=True, timeout=60)
        assert r.returncode != 0 and option.encode() + b" is not supported together with --gpus > 1" in r.stderr, r.stderr
        r = subprocess.run(base + with_ + [option, str(out), "--remove-identity-columns"], capture_output=True, timeout=60)
        assert r.returncode != 0 and option.encode() + b" is not supported together with --remove-identity-columns" in r.stderr, r.stderr
        for bad in ("-1", "x", "4294967296", ""):
            r = subprocess.run(base + with_ + [option, str(out), "--graph-nearest-max-distance=" + bad], capture_output=True, timeout=60)
            assert r.returncode != 0 and b"--graph-nearest-max-distance must be a number" in r.stderr, (bad, r.stderr)
        assert not out.exists()
    # what --match-sequences said without an output, it still says
    r = subprocess.run(base + ["--match-sequences", str(tmp_path / "list.txt")], capture_output=True, timeout=60)
    assert r.returncode != 0 and b"--match-sequences requires --output-sequence-matches." in r.stderr
    usage = subprocess.run([cli, "--help"], capture_output=True, timeout=60).stdout
    assert b"--output-held-out-graph-nearest=PATH" in usage and b"--output-sequence-graph-nearest=PATH" in usage and b"--graph-nearest-max-distance=D" in usage
