"""The nearest node of every segment for rows threaded through the founder block graph, on contexts (fseq_graph_nearest_rows,
fseq_graph_nearest_held_out; csrc/fseq_graphnearest.hpp, csrc/fseq_api_graph.hip).

The yardstick is tests/graph_nearest_model.py, numpy on the raw rows and the run's segment borders alone
(tests/test_graph_nearest_model.py checks it on the CPU): nodes, distances, ties, steps, per_row, per_segment and the summary must
equal it exactly, at max_distance 0, 1, 2 and 2^32 - 1; at 0 the nodes at distance 0, the steps and the shared statistics must also
equal fseq_graph_thread_rows on the same queries.  The kernels' own shapes are in tests/test_gpu_graph_nearest_kernel.py."""
import importlib

import numpy as np
import pytest

import graph_nearest_model as nm
import graph_thread_model as tm
from helpers import founder_mosaic
from test_gpu_block_graph import context, gapped_blocks
from test_gpu_graph_thread import bordered, strangers
from test_gpu_graph_thread import same as same_threading

pytestmark = pytest.mark.gpu

ARRAYS = ("nodes", "distances", "ties", "steps", "per_row", "per_segment")
EVERYTHING = 2 ** 32 - 1


@pytest.fixture(scope="module")
def pkg():
    return importlib.import_module("founder-sequences_amd")


@pytest.fixture(scope="module")
def mosaic(pkg):
    """The model cases' alignment on a context, shared and never given another input: (ctx, msa, founders, W)."""
    X, m, S, W, seed = tm.MOSAIC
    msa, founders = tm.full_mosaic(X, m, S, W, seed)
    ctx = context(pkg, msa, W)
    assert ctx.result.segment_count == S and ctx.result.max_segment_size == X
    msa.setflags(write=False)
    yield ctx, msa, founders, W
    ctx.close()


def same(got, want):
    for what in ARRAYS:
        assert got[what].dtype == want[what].dtype and got[what].shape == want[what].shape, (what, got[what].shape, want[what].shape)
        assert np.array_equal(got[what], want[what]), (what, np.argwhere(got[what] != want[what])[:5].tolist())
    assert {k: got["summary"][k] for k in nm.SUMMARY} == {k: want["summary"][k] for k in nm.SUMMARY}


def check(ctx, rows, queries, D=0, graph=None):
    """graph_nearest_rows of ctx (which holds `rows`) against the model on the run's segments, the full call and the one that
    leaves the arrays on the device; at D = 0 also against graph_thread_rows.  Returns (got, the model's)."""
    red = ctx.reduced_traceback()
    want = nm.nearest_model(rows, red["lb"], red["rb"], queries, D, graph=graph)
    got = ctx.graph_nearest_rows(queries, D)
    same(got, want)
    slim = ctx.graph_nearest_rows(queries, D, want_nodes=False, want_distances=False, want_ties=False, want_steps=False)
    assert all(slim[k] is None for k in ARRAYS[:4])
    assert np.array_equal(slim["per_row"], got["per_row"]) and np.array_equal(slim["per_segment"], got["per_segment"])
    assert {k: slim["summary"][k] for k in nm.SUMMARY} == {k: got["summary"][k] for k in nm.SUMMARY}
    part = ctx.graph_nearest_rows(queries, D, want_nodes=False, want_ties=False)
    assert part["nodes"] is None and part["ties"] is None and np.array_equal(part["distances"], got["distances"]) and np.array_equal(part["steps"], got["steps"])
    if D == 0:
        same_threading(nm.as_threading(got), ctx.graph_thread_rows(queries))
    return got, want


# ---- the model's cases, at every distance allowed

@pytest.mark.parametrize("D", [0, 1, 2, EVERYTHING])
@pytest.mark.parametrize("name", tm.CASES)
def test_model_cases(mosaic, name, D):
    ctx, msa, founders, W = mosaic
    rows, L, queries, listed = tm.case(name)
    assert np.array_equal(rows, msa) and L == W
    got, want = check(ctx, msa, queries, D)
    assert ("unmatched" in listed) == bool((got["distances"] > 0).any())
    if D == EVERYTHING:
        assert got["summary"]["segments_admitted"] == got["nodes"].size and (got["steps"] != nm.NONE).sum() + got["summary"]["junctions_novel"] == got["steps"].size
    # sigma = 4: the queries need the code 4, so both sides are packed at 4 bits -- a word a segment of 8 columns
    assert ctx.graph_nearest_info() == {"batches": 1, "packed_words": 6 * 5, "query_words": 6, "bits": 4}


def test_own_rows_have_distance_0_and_are_on_the_graph(mosaic):
    ctx, msa, founders, W = mosaic
    got, want = check(ctx, msa, np.ascontiguousarray(msa))
    S = ctx.result.segment_count
    assert (got["distances"] == 0).all() and (got["ties"] == 1).all() and np.array_equal(got["nodes"], ctx.block_graph(want_row_nodes=True)["row_nodes"])
    assert got["summary"]["rows_on_graph"] == len(msa) and got["summary"]["segments_exact"] == len(msa) * S and got["summary"]["mismatches"] == 0


# ---- widths of the rows and of the queries (tests/test_gpu_graph_thread.py's cases)

@pytest.mark.parametrize("alphabet,bits,query_bits", [(b"ACG", 2, 2), (b"ACGT", 2, 4), (bytes(range(65, 80)), 4, 4), (bytes(range(65, 81)), 4, 8),
                                                        (bytes(range(48, 88)), 8, 8)])
def test_code_widths(pkg, alphabet, bits, query_bits):
    S, W = 5, 65
    msa, founders = tm.full_mosaic(4, 41, S, W, seed=len(alphabet), alphabet=alphabet)
    ctx = context(pkg, msa, W)
    assert ctx.alphabet()[:2] == (len(alphabet), bits) and ctx.result.segment_count == S
    queries = np.concatenate([msa, strangers(msa, founders, S, W, ord("z"))])
    for D in (0, 1):
        got, want = check(ctx, msa, queries, D)
    per = 32 // query_bits
    assert ctx.graph_nearest_info() == {"batches": 1, "packed_words": S * 4 * -(-W // per), "query_words": S * -(-W // per), "bits": query_bits}
    assert want["distances"][S - 1, len(msa) + 30] == 1 and want["summary"]["junctions_novel"] > 0      # (the row with one byte outside the alphabet)
    ctx.close()


# ---- segment widths, with gaps as symbols

@pytest.mark.parametrize("W", [1, 63, 64, 65])
def test_gapped_blocks(pkg, W):
    msa = gapped_blocks(W, b"ACGT", seed=W)
    ctx = context(pkg, msa, W)
    red = ctx.reduced_traceback()
    assert ((red["rb"] - red["lb"]) == W).all() and len(red) == 6
    rng = np.random.default_rng(W)
    q = msa[rng.integers(0, len(msa), size=(50, 6)).repeat(W, axis=1), np.arange(6 * W)]      # mosaics of the rows by blocks
    q[40:45, rng.integers(0, 6 * W, size=5)] = ord("N")
    q[45, 0], q[46, 6 * W - 1] = ord("N"), ord("N")
    q[30:40, rng.integers(0, 6 * W, size=7)] = ord("-")                       # gaps where a row has a base, or none: a symbol like any other
    q = np.ascontiguousarray(q)
    for D in (0, 1, EVERYTHING):
        got, want = check(ctx, msa, q, D)
    assert (want["distances"] > 0).any() and (want["distances"] == 0).any()
    ctx.close()


def test_more_classes_than_the_threading_takes(pkg):
    """4,097 classes a segment: the threading refuses (its LDS table), this does not."""
    ctx, msa, founders = bordered(pkg, 4097, 4200)
    q = np.concatenate([tm.mosaic_queries(founders, 3, 16, 18, 5), msa[:2]])
    q[18, 5], q[19, 47] = ord("N"), ord("N")
    with pytest.raises(pkg.FseqError):
        ctx.graph_thread_rows(q)
    red = ctx.reduced_traceback()
    want = nm.nearest_model(msa, red["lb"], red["rb"], q, 1)
    same(ctx.graph_nearest_rows(q, 1), want)
    assert want["summary"]["segments_admitted"] == 3 * 20 and want["summary"]["segments_exact"] == 3 * 20 - 2
    ctx.close()


# ---- the held-out form

@pytest.mark.parametrize("list_memory", [0, 1 << 20])
def test_held_out_form(pkg, list_memory):
    X, m, S, W, seed = tm.MOSAIC
    msa, founders = tm.full_mosaic(X, m, S, W, seed)
    extra = np.concatenate([strangers(msa, founders, S, W, ord("N")), msa[[3, 3, 8]]])
    source = np.concatenate([msa, extra])
    order = np.random.default_rng(4).permutation(len(source))
    source = np.ascontiguousarray(source[order])
    held = np.flatnonzero(order >= m)[::-1].astype(np.uint32).copy()           # the extras' places, not ascending
    kept = np.setdiff1d(np.arange(len(source)), held)
    src = pkg.SegmentationContext(len(source), S * W, W)
    src.set_sequences(source)
    sub = src.without_rows(held, W, list_memory=list_memory)
    src.close()
    for length in (W, 2 * W):
        if length != W:
            sub.set_segment_length(length)
        sub.run()
        red = sub.reduced_traceback()
        assert len(red) == (S if length == W else 3)
        for D in (0, 1):
            want = nm.nearest_model(source[kept], red["lb"], red["rb"], source[held], D)
            got = sub.graph_nearest_held_out(D)
            same(got, want)
            same(sub.graph_nearest_rows(source[held], D), got)
            slim = sub.graph_nearest_held_out(D, want_nodes=False, want_distances=False, want_ties=False, want_steps=False)
            assert all(slim[k] is None for k in ARRAYS[:4]) and np.array_equal(slim["per_row"], want["per_row"]) and np.array_equal(slim["per_segment"], want["per_segment"])
        same_threading(nm.as_threading(sub.graph_nearest_held_out(0)), sub.graph_thread_held_out())
        assert (want["distances"] > 0).any() and want["summary"]["rows_on_graph"] >= 3
        assert sub.graph_nearest_info()["bits"] == 4                 # (N is a code of the sub-context, sigma = 5: rows and held-out rows at 4 bits)
    sub.close()


# ---- batches, a repeated call, and the context afterwards

def test_batches(mosaic):
    ctx, msa, founders, W = mosaic
    queries = tm.case("mixed")[2]
    whole = ctx.graph_nearest_rows(queries, 1)
    assert ctx.graph_nearest_info()["batches"] == 1
    try:
        for budget, batches in ((40, 3), (20, 6), (1, 6)):                  # a segment's five classes take a word each: 20 bytes
            ctx.set_tuning("FSEQ_GRAPH_NEAREST_BATCH", budget)
            assert ctx.result is not None                                # (the knob is these entries' alone: the run stands)
            same(ctx.graph_nearest_rows(queries, 1), whole)
            assert ctx.graph_nearest_info()["batches"] == batches
    finally:
        ctx.set_tuning("FSEQ_GRAPH_NEAREST_BATCH", None)
    same(ctx.graph_nearest_rows(queries, 1), whole)                      # a repeated call is equal
    assert ctx.graph_nearest_info()["batches"] == 1


def test_state_is_left_alone(mosaic, tmp_path):
    ctx, msa, founders, W = mosaic
    queries = tm.case("mixed")[2]
    perm = ctx.join_greedy()
    summary = ctx.match_rows(queries[:20], permutations=perm)
    pieces, sets = ctx.match_pieces()
    ctx.write_match(str(tmp_path / "before.txt"))
    ctx.graph_thread_rows(queries[:7])
    thread_info = ctx.graph_thread_info()
    red = ctx.reduced_traceback().copy()
    graph = ctx.block_graph(want_row_nodes=True)
    now = ctx.device_bytes()[0]
    first, _ = check(ctx, msa, queries, 1)
    same(ctx.graph_nearest_rows(queries, 1), first)
    assert ctx.device_bytes()[0] == now                        # every buffer of the calls was theirs alone
    assert ctx.graph_thread_info() == thread_info and np.array_equal(ctx.reduced_traceback(), red)
    after, after_sets = ctx.match_pieces()
    assert len(after) == summary["pieces"] and np.array_equal(after, pieces) and np.array_equal(after_sets, sets)
    ctx.write_match(str(tmp_path / "after.txt"))
    assert (tmp_path / "after.txt").read_bytes() == (tmp_path / "before.txt").read_bytes()
    again = ctx.block_graph(want_row_nodes=True)
    assert all(np.array_equal(again[k], graph[k]) for k in ("nodes", "edges", "row_nodes"))
    assert np.array_equal(ctx.join_greedy(), perm)


# ---- refusals

def test_refusals(pkg):
    msa = founder_mosaic(8, 203, 600, seed=21)
    ctx = pkg.SegmentationContext(203, 600, 20)
    ctx.set_sequences(msa)

    def refused(call, code):
        with pytest.raises(pkg.FseqError) as err:
            call()
        assert err.value.code == code and str(err.value), (err.value.code, code)

    refused(lambda: ctx.graph_nearest_rows(msa[:4]), pkg.FSEQ_E_ARG)         # before a run
    refused(ctx.graph_nearest_info, pkg.FSEQ_E_ARG)
    ctx.run()
    refused(lambda: ctx.graph_nearest_rows(msa[:0]), pkg.FSEQ_E_ARG)         # no rows
    refused(ctx.graph_nearest_held_out, pkg.FSEQ_E_ARG)                      # a plain context holds no rows out
    refused(ctx.graph_nearest_info, pkg.FSEQ_E_ARG)                          # (no call has finished)
    lib = pkg.load_library()
    assert lib.fseq_graph_nearest_rows(ctx.h, None, 3, 0, None, None, None, None, None, None, None) == pkg.FSEQ_E_ARG
    import ctypes as C
    rows = (C.c_void_p * 2)(msa.ctypes.data, None)
    assert lib.fseq_graph_nearest_rows(ctx.h, rows, 2, 0, None, None, None, None, None, None, None) == pkg.FSEQ_E_ARG and b"null query row" in lib.fseq_last_error(ctx.h)
    got = ctx.graph_nearest_rows(msa[:9])                                     # the context stays usable
    assert (got["distances"] == 0).all() and got["summary"]["rows_on_graph"] == 9
    # an identity-reduced context, and one that carries held-out rows along
    wide = msa.copy()
    wide[:, 200:320] = wide[0, 200:320]
    src = pkg.SegmentationContext(203, 600, 20)
    src.set_sequences(wide)
    reduced = src.without_identity_columns(20)
    reduced.run()
    refused(lambda: reduced.graph_nearest_rows(wide[:3, :reduced.n]), pkg.FSEQ_E_UNSUPPORTED)
    sub = src.without_rows(np.array([5, 9], dtype=np.uint32), 20)
    both = sub.without_identity_columns(20, keep_held_out=True)
    both.run()
    refused(both.graph_nearest_held_out, pkg.FSEQ_E_UNSUPPORTED)
    sub.run()
    assert sub.graph_nearest_held_out()["summary"]["rows"] == 2               # (the context it was made from serves its own)
    for c in (both, sub, reduced, src, ctx):
        c.close()
