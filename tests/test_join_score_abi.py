"""The score of a join (include/fseq.h: fseq_join_score, fseq_join_score_host; include/fseq_debug.h: fseq_debug_join_score_path,
fseq_debug_join_score) on the CPU: the host form on boundary states from the oracle against tests/join_score_model.py, which
counts on the raw rows' bytes; the definitions' properties; the structs against the header; the debug entry's refusals, which
need no device; the host form as a program of its own under the sanitizers."""
import ctypes as C
import importlib
import os
import subprocess

import numpy as np
import pytest

import fso
import join_score_model as jm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("fseq_join_score", "fseq_join_score_host", "fseq_debug_join_score_path", "fseq_debug_join_score")


@pytest.fixture(scope="module")
def pkg():
    build = importlib.import_module("founder-sequences_amd.build")
    build.build()
    return importlib.import_module("founder-sequences_amd")


# m, n, L, founders, recombination block, mutation rate, seed
CASES = [(8, 1000, 10, 3, 100, 5e-3, 0x5EED0001), (24, 400, 7, 4, 60, 1e-2, 11), (70, 500, 9, 6, 45, 8e-3, 21), (200, 1200, 15, 6, 150, 3e-3, 31)]
_segmented = {}


def segmented(case):
    """(msa, oracle result) of a case: computed once, shared, never written to."""
    if case not in _segmented:
        m, n, L, K, Brec, mu, seed = case
        msa = np.ascontiguousarray(fso.synth_msa(fso.synth_spec(seed, K, Brec, mu), m, n))
        res = fso.segment_long(msa, L, debug=True)
        assert res["status"] == 0 and len(res["reduced"]) >= 2
        msa.setflags(write=False)
        _segmented[case] = (msa, res)
    return _segmented[case]


def host_score(pkg, case, perm, want_support=True):
    msa, res = segmented(case)
    red = res["reduced"]
    return pkg.join_score_host(msa.shape[0], res["max_segment_size"], red["lb"], red["rb"], res["a"], res["d"], perm, want_support=want_support)


def doctored(m, S, X, seed):
    """Permutations no joiner makes: random rows; random rows with gaps (m, m + 7 and 0xFFFFFFFF); every slot the same row."""
    rng = np.random.default_rng(seed)
    rows = rng.integers(0, m, size=(S, X)).astype(np.uint32)
    gapped = rows.copy()
    gapped[rng.random((S, X)) < 0.2] = m
    gapped[rng.random((S, X)) < 0.05] = m + 7
    gapped[rng.random((S, X)) < 0.05] = 0xFFFFFFFF
    return {"random rows": rows, "gaps": gapped, "all slots equal": np.full((S, X), rng.integers(0, m), dtype=np.uint32)}


def test_new_symbols_are_declared_exported_and_bound(pkg):
    lib = pkg.load_library()
    for name in NEW:
        assert hasattr(lib, name) and name in pkg.EXPORTS, name
        assert (name in pkg.DEBUG_EXPORTS) == name.startswith("fseq_debug_"), name
    assert lib.fseq_abi_version() == 5                       # (detected by symbol: no struct of the boundary changed)


def test_struct_layouts_match_header(pkg, tmp_path):
    assert pkg.JOIN_SCORE_DTYPE.itemsize == 32 and C.sizeof(pkg.JoinScoreSummary) == 72
    fields = ["rb", "weight", "supported", "unsupported", "gaps", "rows_through"]
    sfields = [k for k, _ in pkg.JoinScoreSummary._fields_]
    src = tmp_path / "t.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "fseq.h"\n#include "fseq_debug.h"\nint main(void){\n'
                   '  printf("%zu %zu", sizeof(fseq_join_score_entry), sizeof(fseq_join_score_summary));\n'
                   + "".join('  printf(" %%zu", offsetof(fseq_join_score_entry, %s));\n' % f for f in fields)
                   + "".join('  printf(" %%zu", offsetof(fseq_join_score_summary, %s));\n' % f for f in sfields)
                   + '  return 0 * (fseq_join_score(0, 0, 0, 0, 0, 0) + fseq_join_score_host(0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0)\n'
                     '              + fseq_debug_join_score_path(0, 0) + fseq_debug_join_score(0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0));\n}\n')
    exe = tmp_path / "t"
    libdir = os.path.dirname(pkg.LIB_PATH)
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe),
                    "-L", libdir, "-lfseq_hip", "-Wl,-rpath," + libdir, "-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib"], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], stdout=subprocess.PIPE, text=True, check=True).stdout.split()]
    want = [32, 72] + [pkg.JOIN_SCORE_DTYPE.fields[f][1] for f in fields] + [getattr(pkg.JoinScoreSummary, f).offset for f in sfields]
    assert got == want


@pytest.mark.parametrize("case", CASES)
def test_host_form_equals_the_model_on_the_joiners_permutations(pkg, case):
    msa, res = segmented(case)
    red, X, m = res["reduced"], res["max_segment_size"], msa.shape[0]
    perms = {"greedy": pkg.greedy_match_host(m, X, red["lb"], red["rb"], res["a"], res["d"]),
             "bipartite": pkg.bipartite_match_host(m, X, red["lb"], red["rb"], res["a"], res["d"])[0],
             "random": pkg.random_join_host(m, X, red["lb"], red["rb"], res["a"], res["d"], 5)}
    for how, perm in perms.items():
        got = host_score(pkg, case, perm)
        want = jm.join_score_model(msa, red["lb"], red["rb"], perm)
        assert jm.same_score(got, want, red["rb"]) is None, (how, jm.same_score(got, want, red["rb"]))
        j = got["junctions"]
        assert np.all(j["rows_through"] <= m) and np.all(j["supported"] + j["unsupported"] + j["gaps"] == X), how
    # (the optional outputs: without the support matrix the rest is the same)
    slim = host_score(pkg, case, perms["greedy"], want_support=False)
    assert slim["support"] is None and jm.same_score(slim, jm.join_score_model(msa, red["lb"], red["rb"], perms["greedy"]), red["rb"]) is None


@pytest.mark.parametrize("case", CASES)
def test_host_form_equals_the_model_on_doctored_permutations(pkg, case):
    msa, res = segmented(case)
    red, X, m = res["reduced"], res["max_segment_size"], msa.shape[0]
    for what, perm in doctored(m, len(red), X, 77).items():
        got = host_score(pkg, case, perm)
        want = jm.join_score_model(msa, red["lb"], red["rb"], perm)
        assert jm.same_score(got, want, red["rb"]) is None, (what, jm.same_score(got, want, red["rb"]))
        j = got["junctions"]
        assert np.all(j["supported"] + j["unsupported"] + j["gaps"] == X) and np.all(j["rows_through"] <= m), what
    gapped = doctored(m, len(red), X, 77)["gaps"]
    is_gap = (gapped[:-1] >= m) | (gapped[1:] >= m)
    got = host_score(pkg, case, gapped)
    assert np.array_equal(got["junctions"]["gaps"], is_gap.sum(axis=1)) and not got["support"][is_gap].any()


@pytest.mark.parametrize("case", CASES)
def test_a_founder_that_is_one_row_never_breaks(pkg, case):
    msa, res = segmented(case)
    red, X, m = res["reduced"], res["max_segment_size"], msa.shape[0]
    rows = np.random.default_rng(3).integers(0, m, size=X).astype(np.uint32)
    got = host_score(pkg, case, np.tile(rows, (len(red), 1)))
    assert not got["junctions"]["unsupported"].any() and not got["junctions"]["gaps"].any() and not got["breaks"].any()
    assert np.all(got["support"] >= 1) and got["summary"]["max_breaks"] == 0 and got["summary"]["unsupported"] == 0


def test_every_row_goes_through_when_every_row_is_a_slot(pkg):
    case = CASES[1]
    msa, res = segmented(case)
    red, m = res["reduced"], msa.shape[0]
    # (the host form serves any slot count: here X = m, slot r holds row r in every segment)
    perm = np.tile(np.arange(m, dtype=np.uint32), (len(red), 1))
    got = pkg.join_score_host(m, m, red["lb"], red["rb"], res["a"], res["d"], perm, want_support=True)
    assert np.all(got["junctions"]["rows_through"] == m) and got["summary"]["min_rows_through"] == m
    assert jm.same_score(got, jm.join_score_model(msa, red["lb"], red["rb"], perm), red["rb"]) is None


def test_one_segment_and_refusals_of_the_host_form(pkg):
    lib = pkg.load_library()
    a = np.array([[2, 0, 1]], dtype=np.uint32)
    d = np.array([[9, 0, 4]], dtype=np.uint32)
    got = pkg.join_score_host(3, 2, [0], [9], a, d, np.array([[2, 1]], dtype=np.uint32), want_support=True)
    assert len(got["junctions"]) == 0 and got["breaks"].tolist() == [0, 0] and got["support"].shape == (0, 2)
    assert got["summary"]["junctions"] == 0 and got["summary"]["min_rows_through"] == 3 and got["summary"]["weight"] == 0
    bad = np.array([[2, 0, 3]], dtype=np.uint32)                 # (a row that is none: an index into the classes)
    with pytest.raises(pkg.FseqError) as err:
        pkg.join_score_host(3, 2, [0], [9], bad, d, np.array([[2, 1]], dtype=np.uint32))
    assert err.value.code == pkg.FSEQ_E_ARG
    p = lambda x: x.ctypes.data
    lb, rb, perm = np.zeros(1, dtype=np.uint64), np.full(1, 9, dtype=np.uint64), np.zeros((1, 2), dtype=np.uint32)
    assert lib.fseq_join_score_host(0, 2, 1, p(lb), p(rb), p(a), p(d), p(perm), None, None, None, None) == pkg.FSEQ_E_ARG
    assert lib.fseq_join_score_host(3, 0, 1, p(lb), p(rb), p(a), p(d), p(perm), None, None, None, None) == pkg.FSEQ_E_ARG
    assert lib.fseq_join_score_host(3, 2, 0, p(lb), p(rb), p(a), p(d), p(perm), None, None, None, None) == pkg.FSEQ_E_ARG
    assert lib.fseq_join_score_host(3, 2, 1, p(lb), p(rb), p(a), p(d), None, None, None, None, None) == pkg.FSEQ_E_ARG
    assert lib.fseq_join_score_host(3, 2, 1, p(lb), p(rb), p(a), p(d), p(perm), None, None, None, None) == pkg.FSEQ_OK      # (every output optional)
    assert lib.fseq_join_score(None, p(perm), None, None, None, None) == pkg.FSEQ_E_ARG
    path = C.c_int(7)
    assert lib.fseq_debug_join_score_path(None, C.byref(path)) == pkg.FSEQ_E_ARG and path.value == 7


def test_debug_entry_refuses_before_a_device_is_touched(pkg):
    """Whatever a kernel would form an index or the empty key from: FSEQ_E_ARG, on a machine without a device too (a call that got
    as far as the runtime would answer FSEQ_E_HIP or FSEQ_E_OOM there)."""
    of = np.zeros((2, 5), dtype=np.uint16)
    cl = np.zeros((1, 3), dtype=np.uint16)

    def refused(of_, cl_, cr_):
        with pytest.raises(pkg.FseqError) as err:
            pkg.debug_join_score(of_, cl_, cr_)
        return err.value.code == pkg.FSEQ_E_ARG

    top = of.copy()
    top[1, 4] = 0xFFFF
    assert refused(top, cl, cl)                                                      # a class >= 0xFFFF among the rows
    assert refused(of, np.zeros((1, 0), dtype=np.uint16), np.zeros((1, 0), dtype=np.uint16))      # X = 0
    assert refused(of, np.zeros((1, 4097), dtype=np.uint16), np.zeros((1, 4097), dtype=np.uint16))      # X = 4,097
    assert refused(np.zeros((1, 5), dtype=np.uint16), np.zeros((0, 3), dtype=np.uint16), np.zeros((0, 3), dtype=np.uint16))      # S = 1
    assert refused(np.zeros((2, 0), dtype=np.uint16), cl, cl)                        # m = 0
    assert refused(of, cl, np.zeros((1, 4), dtype=np.uint16))                        # shapes that disagree
    lib = pkg.load_library()
    p = lambda x: x.ctypes.data
    assert lib.fseq_debug_join_score(0, 5, 3, 2, None, p(cl), p(cl), None, None, None, None) == pkg.FSEQ_E_ARG
    assert lib.fseq_debug_join_score(0, 5, 3, 2, p(of), None, p(cl), None, None, None, None) == pkg.FSEQ_E_ARG
    assert lib.fseq_debug_join_score(0, 5, 3, 2, p(of), p(cl), None, None, None, None, None) == pkg.FSEQ_E_ARG
    assert lib.fseq_debug_join_score(0, 5, 3, 65537, p(of), p(cl), p(cl), None, None, None, None) == pkg.FSEQ_E_ARG
    assert lib.fseq_debug_join_score(0, 0x80000000, 3, 2, p(of), p(cl), p(cl), None, None, None, None) == pkg.FSEQ_E_ARG


def test_model_counts_a_hand_made_case():
    """The yardstick itself, on a case small enough to count by eye: three rows, two segments of two columns."""
    msa = np.frombuffer(b"AACC" b"AAGG" b"TTGG", dtype=np.uint8).reshape(3, 4)
    # slots: row 0 -> row 0 (support 1), row 0 -> row 1 (AA then GG: row 1 alone), row 2 -> row 0 (TT then CC: nobody), a gap
    perm = np.array([[0, 0, 2, 3], [0, 1, 0, 0]])
    want = jm.join_score_model(msa, [0, 2], [2, 4], perm)
    assert want["support"].tolist() == [[1, 1, 0, 0]] and want["breaks"].tolist() == [0, 0, 1, 0]
    assert {f: int(want["junctions"][f][0]) for f in jm.FIELDS} == {"supported": 2, "unsupported": 1, "gaps": 1, "rows_through": 2, "weight": 2}
    # two slots on one pair of classes: the pair's rows go through once
    twice = jm.join_score_model(msa, [0, 2], [2, 4], np.array([[1, 1], [2, 2]]))
    assert twice["support"].tolist() == [[1, 1]] and int(twice["junctions"]["rows_through"][0]) == 1 and int(twice["junctions"]["weight"][0]) == 2
    assert jm.format_join_score(want, [2, 4]) == (b"# JUNCTIONS=1\tSUPPORTED=2\tUNSUPPORTED=1\tGAPS=1\tROWS_THROUGH=2\tWEIGHT=2\tMIN_ROWS_THROUGH=2\t"
                                                  b"MIN_ROWS_THROUGH_JUNCTION=0\tMAX_BREAKS=1\nJUNCTION\tRB\tSUPPORTED\tUNSUPPORTED\tGAPS\tROWS_THROUGH\tWEIGHT\n"
                                                  b"0\t2\t2\t1\t1\t2\t2\n\nFOUNDER\tBREAKS\n0\t0\n1\t0\n2\t1\n3\t0\n")
    l, r = jm.colliding_keys(40, 127, classes=256)
    assert len(set(zip(l.tolist(), r.tolist()))) == 40 and set(jm.table_home(l << 16 | r, jm.table_log2(40)).tolist()) == {127}


def test_front_end_refuses_several_gpus_and_lists_the_option(tmp_path):
    cli = importlib.import_module("founder-sequences_amd.build").build_cli()
    (tmp_path / "list.txt").write_text("")
    r = subprocess.run([cli, "--input", str(tmp_path / "list.txt"), "--segment-length-bound", "5", "--gpus", "2", "--output-join-score", str(tmp_path / "score")],
                       capture_output=True, timeout=60)
    assert r.returncode != 0 and b"--output-join-score is not supported together with --gpus > 1" in r.stderr and not (tmp_path / "score").exists()
    assert b"--output-join-score=PATH" in subprocess.run([cli, "--help"], capture_output=True, timeout=60).stdout


def test_host_form_under_the_sanitizers(tmp_path):
    """The header is host-only: tests/join_score_sanitized.cpp includes it alone and runs constructed and random inputs on arrays of
    exactly the lengths given, as a program of its own under AddressSanitizer and UndefinedBehaviorSanitizer (nothing loaded into
    Python runs under either)."""
    here = os.path.dirname(os.path.abspath(__file__))
    exe = str(tmp_path / "join_score_sanitized")
    subprocess.run(["g++", "-std=c++17", "-g", "-O1", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", os.path.join(os.path.dirname(here), "founder-sequences_amd", "csrc"), os.path.join(here, "join_score_sanitized.cpp"), "-o", exe], check=True)
    p = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120)
    assert p.returncode == 0 and p.stdout.strip() == "ok", p.stderr[-3000:]
