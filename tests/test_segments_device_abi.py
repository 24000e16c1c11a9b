"""CPU checks of what the segments file from the device adds to the boundary (include/fseq.h: fseq_write_segments_device,
fseq_random_join_classes_host; include/fseq_debug.h: fseq_debug_segments_file, fseq_debug_random_path; the knob
FSEQ_SEGFILE_BATCH): the symbols, the unchanged ABI version, the refusals that touch no device, and the random joiner's host
tail on class tables -- what fseq_join_random runs behind its device front -- against the host joiner on the boundary states
the tables were made from.  The writer and the front themselves are tested on the GPU (tests/test_gpu_segments_device.py)."""
import ctypes as C
import importlib
import os
import subprocess

import numpy as np
import pytest

from test_join import mosaic_segmentation

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("fseq_write_segments_device", "fseq_random_join_classes_host", "fseq_debug_segments_file", "fseq_debug_random_path")
NEW_DEBUG = NEW[2:]


@pytest.fixture(scope="module")
def pkg():
    build = importlib.import_module("founder-sequences_amd.build")
    build.build()
    return importlib.import_module("founder-sequences_amd")


def test_library_exports_the_new_calls(pkg):
    lib = pkg.load_library()
    for name in NEW:
        assert hasattr(lib, name), name
        assert name in pkg.EXPORTS and (name in pkg.DEBUG_EXPORTS) == (name in NEW_DEBUG), name
    header = open(os.path.join(ROOT, "include", "fseq.h")).read()
    debug_header = open(os.path.join(ROOT, "include", "fseq_debug.h")).read()
    for name in NEW:
        assert (name + "(") in (debug_header if name in NEW_DEBUG else header), name
    for method in ("write_segments_device", "segments_file_stats", "random_path"):
        assert hasattr(pkg.SegmentationContext, method)
    assert callable(pkg.random_join_classes_host)
    assert lib.fseq_abi_version() == 5                       # (detected by symbol: no struct of the boundary changed)


def test_headers_compile_as_c(tmp_path):
    src = tmp_path / "t.c"
    src.write_text('#include "fseq_debug.h"\n'
                   'int main(void){ int path = 0; uint64_t v = 0; uint32_t w = 0;\n'
                   '  return 0 * (fseq_write_segments_device(0, FSEQ_JOIN_RANDOM, "-") + fseq_debug_random_path(0, &path)\n'
                   '            + fseq_debug_segments_file(0, &v, &v, &v, &v) + fseq_random_join_classes_host(1, 1, 0, &w, &w, &w, 0, &w)); }\n')
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)], check=True)


def test_null_arguments_fail_without_touching_a_device(pkg):
    lib = pkg.load_library()
    path, v = C.c_int(7), C.c_uint64(7)
    assert lib.fseq_write_segments_device(None, pkg.JOIN_BIPARTITE, b"/nonexistent/x") == pkg.FSEQ_E_ARG
    assert lib.fseq_debug_random_path(None, C.byref(path)) == pkg.FSEQ_E_ARG and path.value == 7
    assert lib.fseq_debug_segments_file(None, C.byref(v), None, None, None) == pkg.FSEQ_E_ARG and v.value == 7


def test_set_tuning_accepts_the_knob(pkg):
    """fseq_debug_set_tuning accepts the names of Tuning::knobs() (csrc/fseq_ctx.hpp) and no other.  A context needs a device
    (fseq_create makes its streams), so no knob can be set on one here: the name is looked for in that table, in the library's
    strings and in the README's knob table, and the call is refused without a context; test_batches of
    tests/test_gpu_segments_device.py sets the knob on a real context three ways and checks the batches it makes."""
    lib = pkg.load_library()
    assert lib.fseq_debug_set_tuning(None, b"FSEQ_SEGFILE_BATCH", b"1") == pkg.FSEQ_E_ARG
    src = open(os.path.join(ROOT, "founder-sequences_amd", "csrc", "fseq_ctx.hpp")).read()
    assert '{"FSEQ_SEGFILE_BATCH", nullptr, &Tuning::segfile_batch,' in src
    assert b"FSEQ_SEGFILE_BATCH\0" in open(pkg.LIB_PATH, "rb").read()
    assert "`FSEQ_SEGFILE_BATCH" in open(os.path.join(ROOT, "README.md")).read()


# ---- the host tail: fseq_random_join_classes_host against fseq_random_join_host

def class_tables(X, lb, a, d):
    """(count, rep, size) of every segment as k_join_classes_wide lays them out: class c of segment s starts at the c-th pBWT
    position i with lb[s] < d[s][i] (position 0 always), rep = the row there, size = the positions up to the next start."""
    S, m = a.shape
    count = np.zeros(S, dtype=np.uint32)
    rep = np.zeros((S, X), dtype=np.uint32)
    size = np.zeros((S, X), dtype=np.uint32)
    for s in range(S):
        starts = np.flatnonzero(d[s].astype(np.uint64) > np.uint64(lb[s]))
        assert len(starts) and starts[0] == 0 and len(starts) <= X
        count[s] = len(starts)
        rep[s, :len(starts)] = a[s, starts]
        size[s, :len(starts)] = np.diff(np.append(starts, m))
    return count, rep, size


def constructed_states(m, X, counts, rng, equal=False):
    """Boundary states of len(counts) segments that tile the columns, 10 columns each: random permutations, counts[s] classes
    with random borders (equal: borders m / count apart, every class equally large)."""
    S = len(counts)
    rb = np.arange(1, S + 1, dtype=np.uint64) * 10
    lb = rb - 10
    a = np.stack([rng.permutation(m).astype(np.uint32) for _ in range(S)])
    d = np.zeros((S, m), dtype=np.uint32)
    for s, k in enumerate(counts):
        if equal:
            assert m % k == 0
            starts = np.arange(k) * (m // k)
        else:
            starts = np.concatenate([[0], 1 + rng.choice(m - 1, size=k - 1, replace=False)]) if k > 1 else np.array([0])
        d[s] = rng.integers(0, int(lb[s]) + 1, size=m)             # (at most lb: inside a class)
        d[s, starts] = rng.integers(int(lb[s]) + 1, int(rb[s]) + 1, size=len(starts))
        d[s, 0] = rb[s]
    return lb, rb, a, d


SEEDS = (0, 7, 2 ** 32 - 1)


@pytest.mark.parametrize("seed", SEEDS)
def test_host_tail_on_constructed_states(pkg, seed):
    rng = np.random.default_rng(11)
    m, X = 240, 24
    # the full segment (no placeholder, no spare slot), the single class, and counts between
    counts = [X, 1, 2, X - 1, 7, X, 1, 13] + [int(k) for k in rng.integers(1, X + 1, size=8)]
    lb, rb, a, d = constructed_states(m, X, counts, rng)
    count, rep, size = class_tables(X, lb, a, d)
    assert (count == X).any() and (count == 1).any()
    want = pkg.random_join_host(m, X, lb, rb, a, d, seed)
    got = pkg.random_join_classes_host(m, X, count, rep, size, seed)
    assert np.array_equal(got, want), np.argwhere(got != want)[:5].tolist()


@pytest.mark.parametrize("seed", SEEDS)
def test_host_tail_with_equal_class_sizes(pkg, seed):
    """Every class of a segment equally large: the order the unstable sort by copy number leaves decides which class gets the
    spare slots -- the tail must run the same sort on the same vector."""
    rng = np.random.default_rng(12)
    m, X = 240, 24
    counts = [k for k in range(1, X + 1) if m % k == 0] * 2
    lb, rb, a, d = constructed_states(m, X, counts, rng, equal=True)
    count, rep, size = class_tables(X, lb, a, d)
    for s, k in enumerate(counts):
        assert (size[s, :k] == m // k).all()
    want = pkg.random_join_host(m, X, lb, rb, a, d, seed)
    got = pkg.random_join_classes_host(m, X, count, rep, size, seed)
    assert np.array_equal(got, want), np.argwhere(got != want)[:5].tolist()


@pytest.mark.parametrize("copies", [None, 4])
def test_host_tail_on_the_oracles_states_of_a_mosaic(pkg, copies):
    """The oracle's boundary states of a founder mosaic (copies: its tie-heavy form, all classes of a segment equally large)."""
    X, m = 16, 64
    msa, res = mosaic_segmentation(X, m, 900, copies)
    red = res["reduced"]
    a, d = np.ascontiguousarray(res["a"], dtype=np.uint32), np.ascontiguousarray(res["d"], dtype=np.uint32)
    count, rep, size = class_tables(X, red["lb"], a, d)
    assert np.array_equal(count, red["segment_size"])
    for seed in SEEDS:
        want = pkg.random_join_host(m, X, red["lb"], red["rb"], a, d, seed)
        got = pkg.random_join_classes_host(m, X, count, rep, size, seed)
        assert np.array_equal(got, want), (seed, np.argwhere(got != want)[:5].tolist())


def test_host_tail_refuses_bad_arguments(pkg):
    lib = pkg.load_library()
    one = np.ones(4, dtype=np.uint32)
    out = np.zeros(4, dtype=np.uint32)
    p, q = one.ctypes.data, out.ctypes.data
    f = lib.fseq_random_join_classes_host
    assert f(4, 2, 1, p, p, p, 0, q) == pkg.FSEQ_OK
    assert f(0, 2, 1, p, p, p, 0, q) == pkg.FSEQ_E_ARG            # m = 0
    assert f(4, 0, 1, p, p, p, 0, q) == pkg.FSEQ_E_ARG            # X = 0
    for k in range(4):
        args = [p, p, p, q]
        args[k] = None
        assert f(4, 2, 1, args[0], args[1], args[2], 0, args[3]) == pkg.FSEQ_E_ARG, k
    three = np.full(1, 3, dtype=np.uint32)
    assert f(4, 2, 1, three.ctypes.data, p, p, 0, q) == pkg.FSEQ_E_ARG      # a class count above X
    zero = np.zeros(1, dtype=np.uint32)
    assert f(4, 2, 1, zero.ctypes.data, p, p, 0, q) == pkg.FSEQ_E_ARG       # ... and of 0
