"""The front end's --output-restored-graph, --output-held-out-restored-graph-threads and --output-sequence-restored-graph-threads,
in child processes, against tests/block_graph_restored_model.py on the full-length rows and the segments of a run on the same
rows; every joiner, --upload-memory, and --reduce-on-upload, under which the restored graph is the same file byte for byte."""
import importlib

import numpy as np
import pytest

import block_graph_restored_model as rm
import graph_thread_model as tm
from test_gpu_input_stream import run_cli, write_list

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def pkg():
    return importlib.import_module("founder-sequences_amd")


@pytest.fixture(scope="module")
def cli():
    return importlib.import_module("founder-sequences_amd.build").build_cli()


def rows_and_strangers():
    """(full, W, queries): rm.thread_rows and 40 full-length queries: mosaics of the founders, some with exception cells, some with a
    byte outside the alphabet at a kept or at an identity column."""
    full, R, founders, kept, W = rm.thread_rows()
    S = tm.MOSAIC[2]
    q = rm.mosaic_queries(full, founders, kept, S, W, 40, 5)
    ident = np.flatnonzero(rm.kept_of(full)[0])
    for i in range(0, 40, 3):
        c = ident[(i * 11) % len(ident)]
        q[i, c] = rm.other_byte(full[0, c])
    q[1::9, kept[W + 2]] = ord("N")
    q[4::9, ident[-2]] = ord("n")
    return full, W, q


def segments_of(pkg, full, L):
    src = pkg.SegmentationContext(full.shape[0], full.shape[1], L)
    src.set_sequences(np.ascontiguousarray(full))
    ctx = src.without_identity_columns(L)
    src.close()
    ctx.run()
    red = ctx.reduced_traceback()
    ctx.close()
    return red["lb"], red["rb"]


@pytest.mark.parametrize("joining,extra", [("greedy", []), ("bipartite-matching", ["--list-memory", "1"]), ("random", ["--upload-memory", "1"]),
                                           ("bipartite-matching", ["--upload-memory", "1", "--reduce-on-upload"])])
def test_restored_graph_and_sequence_threads(pkg, cli, tmp_path, joining, extra):
    full, W, queries = rows_and_strangers()
    lst = write_list(tmp_path, full)
    (tmp_path / "q").mkdir()
    qlist = write_list(tmp_path / "q", queries)
    lb, rb = segments_of(pkg, full, W)
    want_graph = rm.expected_gfa(full, lb, rb, paths=True)
    want_table = tm.table(rm.expected_threading(full, lb, rb, queries))
    got = run_cli(cli, tmp_path, "out", ["--input", lst, "--segment-length-bound", str(W), "--segment-joining", joining, "--random-seed", "7",
                                         "--remove-identity-columns", "--graph-paths", "--match-sequences", qlist] + extra,
                  ["restored-graph", "sequence-restored-graph-threads"])
    assert want_graph.count(b"\nS\t") > 6 and got["restored-graph"] == want_graph
    assert want_table.count(b"\n") == len(queries) + 2 and got["sequence-restored-graph-threads"] == want_table


def test_restored_graph_is_the_same_file_under_reduce_on_upload(pkg, cli, tmp_path):
    full, R, kept, L = rm.label_case(65, seed=13)
    lst = write_list(tmp_path, full)
    base = ["--input", lst, "--segment-length-bound", str(L), "--segment-joining", "greedy", "--remove-identity-columns", "--graph-gap-character=", "--upload-memory", "1"]
    plain = run_cli(cli, tmp_path, "plain", base, ["restored-graph"])
    reduced = run_cli(cli, tmp_path, "reduced", base + ["--reduce-on-upload"], ["restored-graph"])
    lb, rb = segments_of(pkg, full, L)
    assert plain["restored-graph"] == reduced["restored-graph"] == rm.expected_gfa(full, lb, rb, paths=False, gap=None)


@pytest.mark.parametrize("joining,extra", [("greedy", []), ("bipartite-matching", ["--upload-memory", "1"]), ("random", [])])
def test_held_out_restored_graph_threads(pkg, cli, tmp_path, joining, extra):
    full, W, queries = rows_and_strangers()
    queries = queries[(queries != ord("N")).all(1) & (queries != ord("n")).all(1)]       # (held-out rows are the source's: their bytes are its alphabet)
    source = np.concatenate([full[:10], queries[:15], full[10:], queries[15:]])
    held = list(range(10, 25)) + list(range(len(source) - 1, len(source) - 1 - (len(queries) - 15), -1))      # a range, then single indices downwards
    assert np.array_equal(source[np.setdiff1d(np.arange(len(source)), held)], full) and len(held) == len(queries) > 20
    lst = write_list(tmp_path, source)
    lb, rb = segments_of(pkg, full, W)
    want = tm.table(rm.expected_threading(full, lb, rb, source[held]))
    spec = "10:24," + ",".join(str(i) for i in held[15:])
    got = run_cli(cli, tmp_path, "out", ["--input", lst, "--segment-length-bound", str(W), "--segment-joining", joining, "--random-seed", "3",
                                         "--remove-identity-columns", "--hold-out", spec] + extra, ["held-out-restored-graph-threads"])
    assert want.count(b"\n") == len(queries) + 2 and got["held-out-restored-graph-threads"] == want
