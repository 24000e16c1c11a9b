"""The founder block graph from the device (fseq_block_graph, fseq_write_block_graph; csrc/fseq_graph.hpp, csrc/fseq_api_graph.hip).

The yardstick is tests/block_graph_model.py, which numbers the classes and counts the edges from the raw rows' bytes and the
run's segment borders alone (tests/test_block_graph_model.py checks it on the CPU): nodes, edges, row_nodes and the file's bytes
must equal it exactly, and the library's file, parsed back, must spell the input rows.  The shapes sit where the kernels can go
wrong: one wave a node over strips of 64 columns, 256 edges a workgroup, tiles of 64 rows x 64 segments in the paths, the 1,024
rows of a tile of k_join_classes_wide, the strips of left classes of k_join_edges_wide, and every digit border of the ids."""
import importlib
import subprocess
import threading

import numpy as np
import pytest

import block_graph_model as gm
from helpers import founder_mosaic
from test_gpu_input_stream import run_cli, write_list

pytestmark = pytest.mark.gpu

GAP = ord("-")


@pytest.fixture(scope="module")
def pkg():
    return importlib.import_module("founder-sequences_amd")


def full_mosaic(X, m, S, W, seed, alphabet=b"ACGT"):
    """[m, S W]: S blocks of W columns, every block copies all X founders (every row one of them), so that a run at segment
    length W has the blocks as its segments and X classes in each."""
    rng = np.random.default_rng(seed)
    alpha = np.frombuffer(alphabet, dtype=np.uint8)
    founders = alpha[rng.integers(0, len(alpha), size=(X, S * W))]
    msa = np.empty((m, S * W), dtype=np.uint8)
    for b in range(S):
        pick = rng.permutation(np.concatenate([np.arange(X), rng.integers(0, X, size=m - X)]))
        msa[:, b * W:(b + 1) * W] = founders[pick, b * W:(b + 1) * W]
    return msa


def gapped_blocks(W, alphabet, seed, m=41, S=6):
    """full_mosaic of four founders with planted gaps: founder 0 has none; founder 1 is all gaps in block 1 (an empty label);
    founder 2 has a gap in the first and the last column of every strip of 64 columns of every block; founder 3 a third of
    its columns."""
    rng = np.random.default_rng(seed)
    alpha = np.frombuffer(alphabet, dtype=np.uint8)
    founders = alpha[rng.integers(0, len(alpha), size=(4, S * W))]
    founders[1, W:2 * W] = GAP
    for b in range(S):
        for k in sorted({0, W - 1} | {c for c in (63, 64, 127, 128) if c < W}):
            founders[2, b * W + k] = GAP
    founders[3, rng.random(S * W) < 0.33] = GAP
    msa = np.empty((m, S * W), dtype=np.uint8)
    for b in range(S):
        pick = rng.permutation(np.concatenate([np.arange(4), rng.integers(0, 4, size=m - 4)]))
        msa[:, b * W:(b + 1) * W] = founders[pick, b * W:(b + 1) * W]
    return msa


def context(pkg, msa, L, **kw):
    m, n = msa.shape
    ctx = pkg.SegmentationContext(m, n, L)
    ctx.set_sequences(np.ascontiguousarray(msa), **kw)
    try:
        ctx.run()
    except pkg.NoReduction:                                    # (as many classes as rows somewhere: the run's result stands)
        pass
    return ctx


def first_difference(got, want):
    a, b = got.split(b"\n"), want.split(b"\n")
    i = next((i for i in range(min(len(a), len(b))) if a[i] != b[i]), min(len(a), len(b)))
    return "%d / %d lines, first difference at line %d:\n%r\n%r" % (len(a), len(b), i, a[i:i + 1], b[i:i + 1])


def check_graph(pkg, ctx, rows, tmp_path, gaps=(b"-",), tag="g"):
    """Arrays and files of ctx against the model on `rows` (the rows of the alignment the context holds) and the segments the
    run found; returns (the model's graph, the file with paths at the first gap)."""
    red = ctx.reduced_traceback()
    want = gm.block_graph_model(rows, red["lb"], red["rb"])
    assert want["count"].tolist() == red["segment_size"].tolist()
    got = ctx.block_graph(want_row_nodes=True)
    assert got["summary"]["segments"] == len(red) and got["summary"]["nodes"] == len(want["nodes"]) and got["summary"]["edges"] == len(want["edges"])
    for what in ("nodes", "edges", "row_nodes"):
        assert got[what].dtype == want[what].dtype and got[what].shape == want[what].shape, what
        assert np.array_equal(got[what], want[what]), (what, np.argwhere(got[what] != want[what])[:5].tolist())
    slim = ctx.block_graph()
    assert slim["row_nodes"] is None and np.array_equal(slim["nodes"], want["nodes"]) and np.array_equal(slim["edges"], want["edges"])
    first = None
    for gap in gaps:
        for paths in (True, False):
            path = str(tmp_path / ("%s_%s_%d.gfa" % (tag, gap.hex() if gap else "none", paths)))
            ctx.write_block_graph(path, paths=paths, gap=gap)
            blob, model = open(path, "rb").read(), gm.gfa_bytes(rows, want, paths=paths, gap=gap)
            assert blob == model, first_difference(blob, model)
            sections = gm.format_gfa(rows, want, paths=paths, gap=gap)
            st = ctx.graph_file_stats()
            for name, lines in zip(("nodes", "links", "paths"), sections):
                assert st[name]["lines"] == len(lines) and st[name]["bytes"] == sum(len(x) for x in lines), (name, st)
                assert st[name]["batches"] == (1 if lines else 0), (name, st)
            if paths:
                gm.check_file_spells_rows(blob, rows, gap)
                first = first or blob
    return want, first


# ---- segment and class counts

def test_one_segment_has_no_link(pkg, tmp_path):
    msa = founder_mosaic(3, 9, 40, brec=40, seed=2)
    ctx = context(pkg, msa, 20)
    assert ctx.result.segment_count == 1
    want, blob = check_graph(pkg, ctx, msa, tmp_path)
    assert len(want["edges"]) == 0 and b"\nL\t" not in blob and blob.count(b"\nS\t") == 3


def test_two_segments(pkg, tmp_path):
    msa = full_mosaic(3, 9, 2, 20, seed=2)
    ctx = context(pkg, msa, 20)
    assert ctx.result.segment_count == 2
    check_graph(pkg, ctx, msa, tmp_path)


@pytest.mark.parametrize("m", [2, 7])
def test_one_class_a_segment(pkg, tmp_path, m):
    msa = np.ascontiguousarray(np.broadcast_to(founder_mosaic(1, 1, 100, seed=1), (m, 100)))
    ctx = context(pkg, msa, 20)
    assert ctx.result.max_segment_size == 1
    want, _ = check_graph(pkg, ctx, msa, tmp_path)
    assert (want["nodes"]["rows"] == m).all() and (want["edges"]["rows"] == m).all()


def test_one_row(pkg, tmp_path):
    """m = 1: one class is as many as there are rows, so the run reports that nothing was reduced and leaves no merged segment
    (as the reference, which writes nothing then).  There is no segmentation to draw a graph of: both entries say so, nothing is
    written, and the context goes on to its next input."""
    msa = founder_mosaic(1, 1, 100, seed=1)
    ctx = pkg.SegmentationContext(1, 100, 20)
    ctx.set_sequences(msa)
    with pytest.raises(pkg.NoReduction):
        ctx.run()
    assert ctx.result.max_segment_size == 1 and ctx.result.segment_count == 0
    with pytest.raises(pkg.FseqError) as err:
        ctx.block_graph()
    assert err.value.code == pkg.FSEQ_E_ARG and "no segments" in str(err.value)
    with pytest.raises(pkg.FseqError) as err:
        ctx.write_block_graph(str(tmp_path / "g.gfa"), paths=True)
    assert err.value.code == pkg.FSEQ_E_ARG and not (tmp_path / "g.gfa").exists()


@pytest.mark.parametrize("m", [1023, 1024, 1025])
def test_rows_around_a_tile_of_the_class_kernel(pkg, tmp_path, m):
    msa = founder_mosaic(5, m, 300, brec=100, seed=m)
    ctx = context(pkg, msa, 20)
    assert ctx.result.segment_count >= 2
    check_graph(pkg, ctx, msa, tmp_path)


# ---- labels

@pytest.mark.parametrize("W", [1, 63, 64, 65, 129])
def test_segment_widths_and_gaps(pkg, tmp_path, W):
    """Segments of exactly W columns: one strip short of a lane, full, one lane into the next, two strips and a lane.  Gaps in
    the first and the last column of every strip, a label of gaps alone ('*'), labels without a gap, and gap=None."""
    msa = gapped_blocks(W, b"ACGT", seed=W)
    ctx = context(pkg, msa, W)
    red = ctx.reduced_traceback()
    assert ((red["rb"] - red["lb"]) == W).all() and len(red) == 6
    want, blob = check_graph(pkg, ctx, msa, tmp_path, gaps=(b"-", None, b"A"))
    parsed = gm.parse_gfa(blob)
    labels = list(parsed["labels"].values())
    assert b"" in labels and b"\t*\tLN:i:0\t" in blob                        # the label of gaps alone
    assert any(len(x) == W for x in labels)                                   # a label with no gap
    if W > 1:
        firsts = {bytes(msa[int(nd["rep_row"]), int(nd["lb"]):int(nd["rb"])]) for nd in want["nodes"]}
        assert any(x[0] == GAP and x[-1] == GAP and x.count(b"-") < W for x in firsts)      # gaps at both ends of a label that has bytes


@pytest.mark.parametrize("alphabet,bits", [(b"ACG", 2), (b"ACGT", 4), (bytes(range(48, 88)), 8)])
def test_code_widths(pkg, tmp_path, alphabet, bits):
    """2, 4 and 8 bits a code (the gap is one of the codes), m = 41: the last byte of a packed column is partial."""
    msa = gapped_blocks(65, alphabet, seed=bits)
    ctx = context(pkg, msa, 65)
    assert ctx.alphabet()[1] == bits
    check_graph(pkg, ctx, msa, tmp_path, gaps=(b"-", None))


# ---- class counts on either side of the edge kernel's strips

@pytest.mark.parametrize("X,m", [(2, 100), (64, 200), (181, 400), (182, 400), (301, 700)])
def test_unequal_class_counts(pkg, tmp_path, X, m):
    """Blocks that use subsets of the founders: junctions with unequal counts left and right.  X = 301: 108 left classes a strip
    of the edge kernel, and junctions whose left segment has more."""
    msa = founder_mosaic(X, m, 1500, seed=X)
    ctx = context(pkg, msa, 20)
    sz = ctx.reduced_traceback()["segment_size"]
    assert ctx.result.max_segment_size == X and (X == 2 or (sz[:-1] != sz[1:]).any())
    if X == 301:
        assert any(l > 32768 // 301 and r == 301 for l, r in zip(sz[:-1].tolist(), sz[1:].tolist()))
    check_graph(pkg, ctx, msa, tmp_path)


@pytest.mark.parametrize("X", [181, 182])
def test_full_junctions_around_one_strip(pkg, tmp_path, X):
    """X classes on both sides: at 181 the left classes are exactly one strip (32,768 / 181 = 181), at 182 one more than a strip."""
    msa = full_mosaic(X, 2 * X + 3, 4, 30, seed=X)
    ctx = context(pkg, msa, 30)
    assert (ctx.reduced_traceback()["segment_size"] == X).all() and ctx.result.segment_count == 4
    check_graph(pkg, ctx, msa, tmp_path)


# ---- digits

@pytest.mark.parametrize("X,S,seed", [(3, 3, 9), (5, 2, 10), (9, 11, 99), (10, 10, 100), (27, 37, 1), (25, 40, 1000)])
def test_node_counts_around_the_digit_borders(pkg, tmp_path, X, S, seed):
    """9 / 10, 99 / 100 and 999 / 1,000 nodes: the ids change their digit count inside the S lines, the L lines and a P line."""
    msa = full_mosaic(X, 2 * X + 1, S, 8, seed=seed)
    ctx = context(pkg, msa, 8)
    want, blob = check_graph(pkg, ctx, msa, tmp_path)
    assert len(want["nodes"]) == X * S
    assert (b"\nS\t%d\t" % (X * S)) in blob and (b",%d+\t*\n" % (X * S)) in blob      # the last node: its own line, and the end of a path


# ---- paths

@pytest.mark.parametrize("S", [63, 64, 65])
def test_segments_around_a_tile_of_the_paths(pkg, tmp_path, S):
    msa = full_mosaic(3, 70, S, 6, seed=S)                    # (70 rows: a second workgroup with 6 rows)
    ctx = context(pkg, msa, 6)
    assert ctx.result.segment_count == S
    check_graph(pkg, ctx, msa, tmp_path)


# ---- batches

def packed(lengths, budget):
    """Batches of whole lines of at most `budget` bytes in order, a longer line alone: their number."""
    count, used = 0, 0
    for i, n in enumerate(lengths):
        if used and used + n > budget:
            count, used = count + 1, 0
        used += n
    return count + (1 if used else 0)


def test_batches(pkg, tmp_path):
    """FSEQ_GRAPH_BATCH of 1 byte: every line is longer than the batch and leaves alone.  200 bytes: a border inside every
    section, several lines a batch in the nodes and the links, a P line above the budget alone.  6,000 bytes: the links' borders
    fall behind whole workgroups of 256 lines and inside the next one's."""
    msa = full_mosaic(16, 80, 48, 8, seed=16)
    ctx = context(pkg, msa, 8)
    want, _ = check_graph(pkg, ctx, msa, tmp_path)
    sections = gm.format_gfa(msa, want, paths=True)
    assert len(sections[1]) > 2 * 256 and max(len(x) for x in sections[2]) > 200 > 2 * max(len(x) for x in sections[0])
    model = gm.gfa_bytes(msa, want, paths=True)
    for budget in (1, 200, 6000):
        ctx.set_tuning("FSEQ_GRAPH_BATCH", budget)
        path = str(tmp_path / ("b%d.gfa" % budget))
        ctx.write_block_graph(path, paths=True)
        blob = open(path, "rb").read()
        assert blob == model, (budget, first_difference(blob, model))
        st = ctx.graph_file_stats()
        for name, lines in zip(("nodes", "links", "paths"), sections):
            expect = packed([len(x) for x in lines], budget)
            assert st[name]["batches"] == expect and expect > 1, (budget, name, st, expect)
            assert st[name]["batches"] == len(lines) or budget > 1
    ctx.set_tuning("FSEQ_GRAPH_BATCH", None)
    ctx.write_block_graph(str(tmp_path / "whole.gfa"), paths=True)
    assert open(tmp_path / "whole.gfa", "rb").read() == model and ctx.graph_file_stats()["links"]["batches"] == 1
    # (the knob is the writer's alone: the run's result stood through all of it)
    assert np.array_equal(ctx.block_graph()["nodes"], want["nodes"])


# ---- contexts that hold no rows on the host, or not the source's

def test_streamed_input(pkg, tmp_path):
    msa = founder_mosaic(16, 300, 3000, seed=4)
    ctx = context(pkg, msa, 20, staging_bytes=1 << 20)
    check_graph(pkg, ctx, msa, tmp_path)


def test_hold_out_context(pkg, tmp_path):
    msa = founder_mosaic(8, 203, 1200, seed=6)
    held = np.array([0, 7, 64, 65, 202], dtype=np.uint32)
    src = pkg.SegmentationContext(203, 1200, 20)
    src.set_sequences(msa)
    ctx = src.without_rows(held, 20)
    src.close()
    ctx.run()
    kept = np.setdiff1d(np.arange(203), held)
    check_graph(pkg, ctx, np.ascontiguousarray(msa[kept]), tmp_path)


def test_without_identity_columns(pkg, tmp_path):
    """The reduced co-ordinates and the reduced rows' bytes, as the segments file on such a context."""
    msa = founder_mosaic(8, 203, 1200, seed=6)
    msa[:, 300:650] = msa[0, 300:650]
    src = pkg.SegmentationContext(203, 1200, 20)
    src.set_sequences(msa)
    mask, _ = src.identity_columns()
    assert mask[300:650].all() and not mask.all()
    ctx = src.without_identity_columns(20)
    src.close()
    ctx.run()
    reduced = np.ascontiguousarray(msa[:, ~mask])
    assert reduced.shape == (203, ctx.n)
    want, _ = check_graph(pkg, ctx, reduced, tmp_path)
    assert int(want["nodes"]["rb"].max()) == ctx.n


# ---- the context afterwards; refusals

def test_context_is_left_as_it_was(pkg, tmp_path):
    msa = founder_mosaic(8, 203, 600, seed=21)
    ctx = context(pkg, msa, 20)
    perm = ctx.join_greedy()
    ctx.write_segments_device(pkg.JOIN_BIPARTITE, str(tmp_path / "before.txt"))
    now = ctx.device_bytes()[0]
    check_graph(pkg, ctx, msa, tmp_path)
    assert ctx.device_bytes()[0] == now                       # every buffer of the calls was theirs alone
    assert np.array_equal(ctx.join_greedy(), perm)
    ctx.write_segments_device(pkg.JOIN_BIPARTITE, str(tmp_path / "after.txt"))
    assert (tmp_path / "after.txt").read_bytes() == (tmp_path / "before.txt").read_bytes()


def test_refusals_leave_the_context_usable(pkg, tmp_path):
    msa = founder_mosaic(8, 203, 600, seed=21)
    path = tmp_path / "g.gfa"
    ctx = pkg.SegmentationContext(203, 600, 20)
    ctx.set_sequences(msa)
    lib = pkg.load_library()

    def refused(code, flags=0, gap=GAP, where=None):
        rc = lib.fseq_write_block_graph(ctx.h, flags, gap, str(where or path).encode())
        assert rc == code and lib.fseq_last_error(ctx.h), (rc, code)
        assert not path.exists()

    refused(pkg.FSEQ_E_ARG)                                     # before a run
    with pytest.raises(pkg.FseqError) as err:
        ctx.block_graph()
    assert err.value.code == pkg.FSEQ_E_ARG
    with pytest.raises(pkg.FseqError):
        ctx.graph_file_stats()
    ctx.run()
    perm = ctx.join_greedy()
    refused(pkg.FSEQ_E_ARG, gap=256)
    refused(pkg.FSEQ_E_ARG, flags=2)
    refused(pkg.FSEQ_E_ARG, flags=pkg.GRAPH_PATHS | 4)
    refused(pkg.FSEQ_E_ARG, where=tmp_path / "no" / "such" / "dir.gfa")      # a file that cannot be opened
    with pytest.raises(pkg.FseqError):
        ctx.graph_file_stats()                                  # (none has been written yet)
    check_graph(pkg, ctx, msa, tmp_path)
    assert np.array_equal(ctx.join_greedy(), perm)
    ctx.set_sequences(msa)
    refused(pkg.FSEQ_E_ARG)                                     # after a new input
    ctx.run()
    check_graph(pkg, ctx, msa, tmp_path, tag="again")
    short = context(pkg, msa[:, :30], 20)                       # n < 2L: the short path has no segments
    with pytest.raises(pkg.FseqError) as err:
        short.block_graph()
    assert err.value.code == pkg.FSEQ_E_ARG


def test_sharded_context_is_refused(pkg, tmp_path):
    msa = founder_mosaic(8, 203, 2000, seed=22)
    tw = importlib.import_module("founder-sequences_amd.dist").ThreadWorld(2)
    ctxs = [pkg.SegmentationContext(203, 2000, 20) for _ in range(2)]
    errs = []

    def rank(r):
        try:
            tw.attach(ctxs[r], r, "cuda:0")
            ctxs[r].set_sequences(msa)
            ctxs[r].run()
        except pkg.NoReduction:
            pass
        except BaseException as e:                              # a failing rank must not leave the other in a barrier for ever
            errs.append(e)
            tw.barrier.abort()

    ths = [threading.Thread(target=rank, args=(r,)) for r in range(2)]
    for t in ths:
        t.start()
    for t in ths:
        t.join()
    assert not errs, errs
    with pytest.raises(pkg.FseqError) as err:
        ctxs[0].block_graph()
    assert err.value.code == pkg.FSEQ_E_UNSUPPORTED and "sharded" in str(err.value)
    with pytest.raises(pkg.FseqError) as err:
        ctxs[0].write_block_graph(str(tmp_path / "g.gfa"), paths=True)
    assert err.value.code == pkg.FSEQ_E_UNSUPPORTED and not (tmp_path / "g.gfa").exists()


# ---- the front end, in child processes

@pytest.mark.parametrize("joining", ["greedy", "bipartite-matching", "random"])
def test_front_end_graph_file(pkg, tmp_path, joining):
    """--output-graph with every joiner (the graph is the segmentation's: the same file), with and without the paths, with another
    gap character and none, and under --remove-identity-columns in reduced co-ordinates."""
    cli = importlib.import_module("founder-sequences_amd.build").build_cli()
    msa = founder_mosaic(6, 65, 3000, brec=150, seed=31)
    msa[:, 1200:1900] = msa[0, 1200:1900]                      # a planted run of identity columns
    msa[np.random.default_rng(5).random(msa.shape) < 0.01] = GAP
    msa[:, 1200:1900] = msa[0, 1200:1900]
    lst = write_list(tmp_path, msa)
    base = ["--input", lst, "--segment-length-bound", "40", "--segment-joining", joining, "--random-seed", "7"]
    src = pkg.SegmentationContext(65, 3000, 40)
    src.set_sequences(msa)
    mask, _ = src.identity_columns()
    assert mask[1200:1900].all() and not mask.all()
    reduced = src.without_identity_columns(40)
    reduced.run()
    src.run()
    variants = {"greedy": [("paths", ["--graph-paths"], src, msa, True, b"-")],
                "random": [("plain", [], src, msa, False, b"-"), ("other", ["--graph-paths", "--graph-gap-character=A"], src, msa, True, b"A")],
                "bipartite-matching": [("keep", ["--graph-paths", "--graph-gap-character="], src, msa, True, None),
                                       ("identity", ["--remove-identity-columns", "--graph-paths"], reduced, np.ascontiguousarray(msa[:, ~mask]), True, b"-")]}
    for tag, extra, ctx, rows, paths, gap in variants[joining]:
        red = ctx.reduced_traceback()
        want = gm.gfa_bytes(rows, gm.block_graph_model(rows, red["lb"], red["rb"]), paths=paths, gap=gap)
        got = run_cli(cli, tmp_path, tag, base + extra, ["graph"])
        assert want.count(b"\n") > 3 and got["graph"] == want, (tag, first_difference(got["graph"], want))
    reduced.close()
    src.close()


def test_front_end_refuses_several_gpus(tmp_path):
    cli = importlib.import_module("founder-sequences_amd.build").build_cli()
    (tmp_path / "list.txt").write_text("")
    r = subprocess.run([cli, "--input", str(tmp_path / "list.txt"), "--segment-length-bound", "5", "--gpus", "2", "--output-graph", str(tmp_path / "g.gfa")],
                       capture_output=True, timeout=60)
    assert r.returncode != 0 and b"--output-graph is not supported together with --gpus > 1" in r.stderr and not (tmp_path / "g.gfa").exists()
