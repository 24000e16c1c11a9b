"""The founder block graph in the source's co-ordinates from the device (fseq_write_block_graph_restored; k_graph_node_lines<true>
and k_graph_write_nodes<true>, csrc/fseq_graph.hpp).

The yardstick is tests/block_graph_restored_model.py: tests/block_graph_model.py's file of the FULL-LENGTH rows over the restored
bounds of the run's segments, byte for byte (tests/test_block_graph_restored_model.py checks it on the CPU).  The shapes sit where
the restored S kernels can go wrong: lanes along source positions in strips of 64 with two running cursors -- a strip with no kept
column, a strip of 64, a kept column on lane 0 and on lane 63, identity columns in front of the first and behind the last kept
column, row 0's byte equal to the gap byte, a label of gaps alone."""
import importlib

import numpy as np
import pytest

import block_graph_model as gm
import block_graph_restored_model as rm
from test_gpu_block_graph import first_difference, packed
from test_gpu_input_stream import run_cli, write_list

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def pkg():
    return importlib.import_module("founder-sequences_amd")


def run(ctx, pkg):
    try:
        ctx.run()
    except pkg.NoReduction:
        pass
    return ctx


def reduced_context(pkg, full, L, how="without"):
    """The context over the kept columns of `full`, run: from without_identity_columns(), from its keep_held_out form (the source
    has three more rows, held out), or from set_sequences_without_identity_columns() (the reduce-on-upload input path)."""
    m, n = full.shape
    if how == "streamed":
        src = pkg.SegmentationContext(m, n, L)
        ctx = src.set_sequences_without_identity_columns(np.ascontiguousarray(full), L, staging_bytes=1 << 16)
        src.close()
    elif how == "held":
        extra = full[[0, m // 2, m - 1]].copy()
        extra[:, ::5] = extra[:, ::5][:, ::-1]                  # (rows that are not the alignment's: they take no part in the graph)
        source = np.ascontiguousarray(np.concatenate([full[:1], extra[:1], full[1:], extra[1:]]))
        held = np.array([1, m + 1, m + 2], dtype=np.uint32)
        src = pkg.SegmentationContext(m + 3, n, L)
        src.set_sequences(source)
        sub = src.without_rows(held, L)
        src.close()
        ctx = sub.without_identity_columns(L, keep_held_out=True)
        sub.close()
    else:
        src = pkg.SegmentationContext(m, n, L)
        src.set_sequences(np.ascontiguousarray(full))
        ctx = src.without_identity_columns(L)
        src.close()
    mask, kept = rm.kept_of(full)
    assert ctx.n == len(kept) and ctx.source_n == n and ctx.m == m
    return run(ctx, pkg)


def non_s_lines(blob):
    return [x for x in blob.split(b"\n") if not x.startswith(b"S\t")]


def check_restored(pkg, ctx, full, tmp_path, gaps=(b"-",), tag="r", batches=1):
    """The restored file of ctx against the model on the full-length rows and the segments the run found, with and without paths,
    at every gap; its L and P lines against the reduced writer's on the same context; the statistics.  Returns the model's bytes
    with paths at the first gap."""
    red = ctx.reduced_traceback()
    lb, rb = red["lb"], red["rb"]
    graph, src_lb, src_rb = rm.restored_graph(full, lb, rb)
    assert graph["count"].tolist() == red["segment_size"].tolist()
    seg = ctx.segments_restored()
    assert np.array_equal(seg["lb"], src_lb) and np.array_equal(seg["rb"], src_rb)
    first = None
    for gap in gaps:
        for paths in (True, False):
            stem = "%s_%s_%d" % (tag, gap.hex() if gap else "none", paths)
            ctx.write_block_graph(str(tmp_path / (stem + ".reduced.gfa")), paths=paths, gap=gap)
            reduced = (tmp_path / (stem + ".reduced.gfa")).read_bytes()
            ctx.write_block_graph_restored(str(tmp_path / (stem + ".gfa")), paths=paths, gap=gap)
            blob, model = (tmp_path / (stem + ".gfa")).read_bytes(), gm.gfa_bytes(full, graph, paths, gap)
            assert blob == model, first_difference(blob, model)
            assert non_s_lines(blob) == non_s_lines(reduced)
            sections = gm.format_gfa(full, graph, paths=paths, gap=gap)
            st = ctx.graph_file_stats()
            for name, lines in zip(("nodes", "links", "paths"), sections):
                assert st[name]["lines"] == len(lines) and st[name]["bytes"] == sum(len(x) for x in lines), (name, st)
                if batches == 1:
                    assert st[name]["batches"] == (1 if lines else 0), (name, st)
            if paths:
                gm.check_file_spells_rows(blob, full, gap)
                first = first or blob
    return first


# ---- labels: the strips of the source positions

@pytest.mark.parametrize("W", [1, 63, 64, 65, 129])
def test_source_ranges_and_identity_runs(pkg, tmp_path, W):
    """Segments of W kept columns with the runs of label_case: identity runs of 1, 64 and 130 positions, 63 in front of the first
    kept column, two behind the last.  (Source ranges of exactly W positions: the next test.)"""
    full, R, kept, L = rm.label_case(W)
    ctx = reduced_context(pkg, full, L)
    red = ctx.reduced_traceback()
    assert ((red["rb"] - red["lb"]) == W).all() and len(red) == 6
    have = rm.reaches(full, red["lb"], red["rb"])
    listed = {"identity in front of kept[0]", "identity behind kept[n-1]", "run=1", "run=64", "run=130", "strip without a kept column", "kept column on lane 0",
              "kept column on lane 63", "row 0 is a gap in an identity column", "empty label", "S=6"} | ({"strip of 64 kept columns"} if W >= 64 else set())
    assert listed <= have, sorted(listed - have)
    blob = check_restored(pkg, ctx, full, tmp_path, gaps=(b"-", None, b"A"))
    assert b"\t*\tLN:i:0\t" in blob                             # the label all of whose bytes are gaps, identity columns included


@pytest.mark.parametrize("W", [1, 63, 64, 65, 129])
def test_source_ranges_of_exactly_w_positions(pkg, tmp_path, W):
    """Segments 1 .. 4 have no identity column: their source range is their W kept columns, 1 / 63 / 64 / 65 / 129 positions."""
    R, _ = rm.gapped(W, b"ACGT", W)
    full, kept = rm.with_runs(R, {0: b"AC-", 6 * W: b"G"})
    ctx = reduced_context(pkg, full, W)
    red = ctx.reduced_traceback()
    assert ((red["rb"] - red["lb"]) == W).all() and len(red) == 6
    assert "range=%d" % W in rm.reaches(full, red["lb"], red["rb"])
    check_restored(pkg, ctx, full, tmp_path)


@pytest.mark.parametrize("S", [1, 2])
def test_one_and_two_segments(pkg, tmp_path, S):
    R, _ = rm.mosaic(3, 9, S, 40, seed=2)
    full, kept = rm.with_runs(R, {0: b"AC-G", 17: b"T" * 70, S * 40: b"-A"})
    ctx = reduced_context(pkg, full, 20 if S == 1 else 40)
    assert ctx.result.segment_count == S
    blob = check_restored(pkg, ctx, full, tmp_path)
    assert (b"\nL\t" in blob) == (S == 2)


@pytest.mark.parametrize("alphabet,bits", [(b"ACG", 2), (b"ACGT", 4), (bytes(range(48, 88)), 8)])
def test_code_widths(pkg, tmp_path, alphabet, bits):
    """2, 4 and 8 bits a code (the gap is one of the codes, and row 0's byte in some identity columns)."""
    full, R, kept, L = rm.label_case(65, alphabet, seed=bits)
    ctx = reduced_context(pkg, full, L)
    assert ctx.alphabet()[1] == bits
    check_restored(pkg, ctx, full, tmp_path, gaps=(b"-", None))


@pytest.mark.parametrize("X", [181, 182])
def test_class_counts_around_one_strip_of_the_edge_kernel(pkg, tmp_path, X):
    R, _ = rm.mosaic(X, 2 * X + 3, 4, 30, seed=X)
    full, kept = rm.with_runs(R, {0: b"ACGT-", 45: rm.run_bytes(70, b"ACGT"), 120: b"AC-"})
    ctx = reduced_context(pkg, full, 30)
    assert (ctx.reduced_traceback()["segment_size"] == X).all() and ctx.result.segment_count == 4
    check_restored(pkg, ctx, full, tmp_path)


# ---- batches

def test_batches(pkg, tmp_path):
    """FSEQ_GRAPH_BATCH of 1, 200 and 6,000 bytes, as tests/test_gpu_block_graph.py: a border inside every section."""
    R, _ = rm.mosaic(16, 80, 48, 8, seed=16)
    full, kept = rm.with_runs(R, {0: b"AC", 100: rm.run_bytes(20, b"ACGT"), 200: b"-", 384: b"GT-"})
    ctx = reduced_context(pkg, full, 8)
    model = check_restored(pkg, ctx, full, tmp_path)
    red = ctx.reduced_traceback()
    graph = rm.restored_graph(full, red["lb"], red["rb"])[0]
    sections = gm.format_gfa(full, graph, paths=True)
    assert len(sections[1]) > 2 * 256 and max(len(x) for x in sections[2]) > 200 > 2 * max(len(x) for x in sections[0])
    for budget in (1, 200, 6000):
        ctx.set_tuning("FSEQ_GRAPH_BATCH", budget)
        path = tmp_path / ("b%d.gfa" % budget)
        ctx.write_block_graph_restored(str(path), paths=True)
        blob = path.read_bytes()
        assert blob == model, (budget, first_difference(blob, model))
        st = ctx.graph_file_stats()
        for name, lines in zip(("nodes", "links", "paths"), sections):
            expect = packed([len(x) for x in lines], budget)
            assert st[name]["batches"] == expect and expect > 1, (budget, name, st, expect)
    ctx.set_tuning("FSEQ_GRAPH_BATCH", None)
    ctx.write_block_graph_restored(str(tmp_path / "whole.gfa"), paths=True)
    assert (tmp_path / "whole.gfa").read_bytes() == model and ctx.graph_file_stats()["nodes"]["batches"] == 1


# ---- the three ways to an identity-reduced context

@pytest.mark.parametrize("how", ["without", "held", "streamed"])
def test_contexts(pkg, tmp_path, how):
    full, R, kept, L = rm.label_case(65, seed=7)
    ctx = reduced_context(pkg, full, L, how)
    check_restored(pkg, ctx, full, tmp_path, gaps=(b"-", None))


# ---- the context afterwards; refusals

def test_context_is_left_as_it_was(pkg, tmp_path):
    full, R, kept, L = rm.label_case(65, seed=9)
    ctx = reduced_context(pkg, full, L, "held")
    perm = ctx.join_greedy()
    sm = ctx.match_held_out_restored(perm)
    pieces, exc = ctx.match_pieces(), ctx.match_exceptions()
    ctx.write_block_graph(str(tmp_path / "before.gfa"), paths=True)
    graph, seg = ctx.block_graph(want_row_nodes=True), ctx.segments_restored()
    now = ctx.device_bytes()[0]
    check_restored(pkg, ctx, full, tmp_path)
    assert ctx.device_bytes()[0] == now                         # every buffer of the calls was theirs alone
    ctx.write_block_graph(str(tmp_path / "after.gfa"), paths=True)
    assert (tmp_path / "after.gfa").read_bytes() == (tmp_path / "before.gfa").read_bytes()
    again = ctx.block_graph(want_row_nodes=True)
    assert all(np.array_equal(again[k], graph[k]) for k in ("nodes", "edges", "row_nodes")) and np.array_equal(ctx.segments_restored(), seg)
    after_pieces, after_exc = ctx.match_pieces(), ctx.match_exceptions()
    assert all(np.array_equal(a, b) for a, b in zip(after_pieces, pieces)) and all(np.array_equal(a, b) for a, b in zip(after_exc, exc))
    assert np.array_equal(ctx.join_greedy(), perm)


def test_refusals(pkg, tmp_path):
    full, R, kept, L = rm.label_case(65, seed=9)
    lib = pkg.load_library()
    path = tmp_path / "g.gfa"

    def refused(ctx, code, flags=0, gap=rm.GAP, where=None, words=None):
        rc = lib.fseq_write_block_graph_restored(ctx.h, flags, gap, str(where or path).encode())
        assert rc == code and lib.fseq_last_error(ctx.h), (rc, code)
        assert words is None or words in lib.fseq_last_error(ctx.h), lib.fseq_last_error(ctx.h)
        assert not path.exists()

    plain = pkg.SegmentationContext(full.shape[0], full.shape[1], L)
    plain.set_sequences(full)
    refused(plain, pkg.FSEQ_E_ARG, words=b"not a context made by fseq_create_without_identity_columns")      # not identity-reduced, before and after a run
    run(plain, pkg)
    refused(plain, pkg.FSEQ_E_ARG, words=b"not a context made by fseq_create_without_identity_columns")
    ctx = plain.without_identity_columns(L)
    plain.close()
    refused(ctx, pkg.FSEQ_E_ARG, words=b"no result")            # before a run
    with pytest.raises(pkg.FseqError):
        ctx.graph_file_stats()
    run(ctx, pkg)
    refused(ctx, pkg.FSEQ_E_ARG, gap=256)
    refused(ctx, pkg.FSEQ_E_ARG, flags=2)
    refused(ctx, pkg.FSEQ_E_ARG, flags=pkg.GRAPH_PATHS | 4)
    refused(ctx, pkg.FSEQ_E_ARG, where=tmp_path / "no" / "such" / "dir.gfa")
    with pytest.raises(pkg.FseqError):
        ctx.graph_file_stats()                                  # (none has been written yet)
    check_restored(pkg, ctx, full, tmp_path)
    # fewer kept columns than two segments: the short path has no segments
    short = reduced_context(pkg, full, full.shape[1])
    refused(short, pkg.FSEQ_E_ARG)


# ---- the front end, in child processes

@pytest.mark.parametrize("joining", ["greedy", "bipartite-matching", "random"])
def test_front_end_restored_graph(pkg, tmp_path, joining):
    """--output-restored-graph with every joiner (the graph is the segmentation's: the same file), with and without the paths, with
    another gap character and none, under --upload-memory, and beside --output-graph, which stays reduced."""
    cli = importlib.import_module("founder-sequences_amd.build").build_cli()
    full, R, kept, L = rm.label_case(65, seed=11)
    lst = write_list(tmp_path, full)
    base = ["--input", lst, "--segment-length-bound", str(L), "--segment-joining", joining, "--random-seed", "7", "--remove-identity-columns"]
    ctx = reduced_context(pkg, full, L)
    red = ctx.reduced_traceback()
    ctx.close()
    variants = {"greedy": [("paths", ["--graph-paths"], True, b"-")],
                "random": [("plain", ["--upload-memory", "1"], False, b"-"), ("other", ["--graph-paths", "--graph-gap-character=A"], True, b"A")],
                "bipartite-matching": [("keep", ["--graph-paths", "--graph-gap-character="], True, None)]}
    for tag, extra, paths, gap in variants[joining]:
        want = rm.expected_gfa(full, red["lb"], red["rb"], paths=paths, gap=gap)
        got = run_cli(cli, tmp_path, tag, base + extra, ["restored-graph", "graph"])
        assert want.count(b"\n") > 3 and got["restored-graph"] == want, (tag, first_difference(got["restored-graph"], want))
        assert got["graph"] == gm.gfa_bytes(R, gm.block_graph_model(R, red["lb"], red["rb"]), paths=paths, gap=gap)
