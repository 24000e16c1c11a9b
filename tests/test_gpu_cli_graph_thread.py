"""The front end's --output-held-out-graph-threads and --output-sequence-graph-threads, in child processes, against the table
tests/graph_thread_model.py makes from the raw bytes and the segments of a run on the same rows; and the two refusals."""
import importlib
import subprocess

import numpy as np
import pytest

import graph_thread_model as tm
from test_gpu_input_stream import run_cli, write_list

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def pkg():
    return importlib.import_module("founder-sequences_amd")


@pytest.fixture(scope="module")
def cli():
    return importlib.import_module("founder-sequences_amd.build").build_cli()


def mosaic_and_strangers():
    X, m, S, W, seed = tm.MOSAIC
    msa, founders = tm.full_mosaic(X, m, S, W, seed)
    return msa, tm.case("mixed")[2], W


def segments_of(pkg, rows, L):
    ctx = pkg.SegmentationContext(rows.shape[0], rows.shape[1], L)
    ctx.set_sequences(np.ascontiguousarray(rows))
    ctx.run()
    red = ctx.reduced_traceback()
    ctx.close()
    return red["lb"], red["rb"]


@pytest.mark.parametrize("joining,extra", [("greedy", []), ("bipartite-matching", ["--list-memory", "1"]), ("random", ["--upload-memory", "1"])])
def test_sequence_graph_threads(pkg, cli, tmp_path, joining, extra):
    msa, queries, W = mosaic_and_strangers()
    lst = write_list(tmp_path, msa)
    (tmp_path / "q").mkdir()
    qlist = write_list(tmp_path / "q", queries)
    lb, rb = segments_of(pkg, msa, W)
    want = tm.table(tm.thread_model(msa, lb, rb, queries))
    got = run_cli(cli, tmp_path, "out", ["--input", lst, "--segment-length-bound", str(W), "--segment-joining", joining, "--random-seed", "7",
                                         "--match-sequences", qlist] + extra, ["sequence-graph-threads"])
    assert want.count(b"\n") == len(queries) + 2 and got["sequence-graph-threads"] == want


@pytest.mark.parametrize("joining", ["greedy", "bipartite-matching"])
def test_held_out_graph_threads(pkg, cli, tmp_path, joining):
    msa, queries, W = mosaic_and_strangers()
    source = np.concatenate([msa[:10], queries[:25], msa[10:], queries[25:40]])
    held = list(range(10, 35)) + list(range(len(source) - 1, len(source) - 16, -1))      # a range, then single indices downwards
    kept = np.setdiff1d(np.arange(len(source)), held)
    assert np.array_equal(source[kept], msa)
    lst = write_list(tmp_path, source)
    lb, rb = segments_of(pkg, msa, W)
    want = tm.table(tm.thread_model(msa, lb, rb, source[held]))
    spec = "10:34," + ",".join(str(i) for i in held[25:])
    got = run_cli(cli, tmp_path, "out", ["--input", lst, "--segment-length-bound", str(W), "--segment-joining", joining, "--hold-out", spec],
                  ["held-out-graph-threads"])
    assert want.count(b"\n") == 40 + 2 and got["held-out-graph-threads"] == want


def test_refusals(cli, tmp_path):
    (tmp_path / "list.txt").write_text("")
    base = [cli, "--input", str(tmp_path / "list.txt"), "--segment-length-bound", "5"]
    out = tmp_path / "t.txt"
    for option, with_ in (("--output-held-out-graph-threads", ["--hold-out", "0"]), ("--output-sequence-graph-threads", ["--match-sequences", str(tmp_path / "list.txt")])):
        r = subprocess.run(base + with_ + [option, str(out), "--gpus", "2"], capture_output=True, timeout=60)
        assert r.returncode != 0 and option.encode() + b" is not supported together with --gpus > 1" in r.stderr, r.stderr
        r = subprocess.run(base + with_ + [option, str(out), "--remove-identity-columns"], capture_output=True, timeout=60)
        assert r.returncode != 0 and option.encode() + b" is not supported together with --remove-identity-columns" in r.stderr, r.stderr
        assert not out.exists()
