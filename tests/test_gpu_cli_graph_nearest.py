"""The front end's --output-held-out-graph-nearest and --output-sequence-graph-nearest with --graph-nearest-max-distance, in child
processes, against the table tests/graph_nearest_model.py makes from the raw bytes and the segments of a run on the same rows."""
import importlib

import numpy as np
import pytest

import graph_nearest_model as nm
import graph_thread_model as tm
from test_gpu_cli_graph_thread import mosaic_and_strangers, segments_of
from test_gpu_input_stream import run_cli, write_list

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def pkg():
    return importlib.import_module("founder-sequences_amd")


@pytest.fixture(scope="module")
def cli():
    return importlib.import_module("founder-sequences_amd.build").build_cli()


@pytest.mark.parametrize("joining,extra,D", [("greedy", [], 0), ("bipartite-matching", ["--list-memory", "1"], 1), ("random", ["--upload-memory", "1"], 1)])
def test_sequence_graph_nearest(pkg, cli, tmp_path, joining, extra, D):
    msa, queries, W = mosaic_and_strangers()
    lst = write_list(tmp_path, msa)
    (tmp_path / "q").mkdir()
    qlist = write_list(tmp_path / "q", queries)
    lb, rb = segments_of(pkg, msa, W)
    want = nm.table(nm.nearest_model(msa, lb, rb, queries, D), D)
    distance = ["--graph-nearest-max-distance", str(D)] if D else []         # (the default is 0)
    got = run_cli(cli, tmp_path, "out", ["--input", lst, "--segment-length-bound", str(W), "--segment-joining", joining, "--random-seed", "7",
                                         "--match-sequences", qlist] + distance + extra, ["sequence-graph-nearest"])
    assert want.count(b"\n") == len(queries) + 2 and got["sequence-graph-nearest"] == want
    assert (b"MAX_DISTANCE_ALLOWED=%d\t" % D) in want


@pytest.mark.parametrize("joining,D", [("greedy", 1), ("bipartite-matching", 0)])
def test_held_out_graph_nearest(pkg, cli, tmp_path, joining, D):
    msa, queries, W = mosaic_and_strangers()
    source = np.concatenate([msa[:10], queries[:25], msa[10:], queries[25:40]])
    held = list(range(10, 35)) + list(range(len(source) - 1, len(source) - 16, -1))      # a range, then single indices downwards
    kept = np.setdiff1d(np.arange(len(source)), held)
    assert np.array_equal(source[kept], msa)
    lst = write_list(tmp_path, source)
    lb, rb = segments_of(pkg, msa, W)
    want = nm.table(nm.nearest_model(msa, lb, rb, source[held], D), D)
    spec = "10:34," + ",".join(str(i) for i in held[25:])
    got = run_cli(cli, tmp_path, "out", ["--input", lst, "--segment-length-bound", str(W), "--segment-joining", joining, "--hold-out", spec,
                                         "--graph-nearest-max-distance=%d" % D], ["held-out-graph-nearest"])
    assert want.count(b"\n") == 40 + 2 and got["held-out-graph-nearest"] == want


def test_both_tables_of_one_run_agree_at_distance_0(pkg, cli, tmp_path):
    """--output-sequence-graph-threads beside --output-sequence-graph-nearest: the columns the two tables share are equal at D = 0."""
    msa, queries, W = mosaic_and_strangers()
    lst = write_list(tmp_path, msa)
    (tmp_path / "q").mkdir()
    qlist = write_list(tmp_path / "q", queries)
    got = run_cli(cli, tmp_path, "out", ["--input", lst, "--segment-length-bound", str(W), "--segment-joining", "greedy", "--match-sequences", qlist],
                  ["sequence-graph-threads", "sequence-graph-nearest"])
    threads = [l.split(b"\t") for l in got["sequence-graph-threads"].splitlines()[1:-1]]
    nearest = [l.split(b"\t") for l in got["sequence-graph-nearest"].splitlines()[1:-1]]
    assert len(threads) == len(nearest) == len(queries)
    # SEQUENCE_INDEX SEGMENTS MATCHED LINKED NOVEL WALKS LONGEST_WALK LONGEST_WALK_COLUMNS MATCHED_COLUMNS against the same of the wider table
    assert [t for t in threads] == [n[:3] + n[4:10] for n in nearest]
