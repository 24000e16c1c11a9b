"""Rows threaded through the founder block graph on the device (fseq_graph_thread_rows, fseq_graph_thread_held_out;
csrc/fseq_graphthread.hpp, csrc/fseq_api_graph.hip).

The yardstick is tests/graph_thread_model.py, which looks the queries' bytes up in dicts made from the raw rows and the run's
segment borders alone (tests/test_graph_thread_model.py checks it on the CPU): nodes, steps, per_row, per_segment and the summary
must equal it exactly.  The shapes sit where the kernels can go wrong: rows and queries packed at different widths, query counts
around a wave, a tile of 256 queries and a packed byte, segments of 1, 63, 64, 65 and 5,003 columns, class counts around the 256
threads that insert into the table and at its cap of 4,096, and keys of a bit or two, under which classes share keys and only the
comparison with the representative row tells them apart."""
import importlib
import threading

import numpy as np
import pytest

import fso
import graph_thread_model as tm
from helpers import founder_mosaic
from test_gpu_block_graph import context, gapped_blocks

pytestmark = pytest.mark.gpu

SUMMARY = ("rows", "segments", "segments_matched", "junctions_linked", "junctions_novel", "walks", "rows_on_graph")


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


def same(got, want, edges=None):
    """A threading of the library against the model's (or another of the library)."""
    for what in ("nodes", "steps", "per_row", "per_segment"):
        assert got[what].dtype == want[what].dtype and got[what].shape == want[what].shape, (what, got[what].shape, want[what].shape)
        assert np.array_equal(got[what], want[what]), (what, np.argwhere(got[what] != want[what])[:5].tolist())
    assert {k: got["summary"][k] for k in SUMMARY} == {k: want["summary"][k] for k in SUMMARY}
    if edges is not None:
        S, Q = got["nodes"].shape
        for p in range(S - 1):
            have = got["steps"][p] != tm.NONE
            assert (got["steps"][p][have] < len(edges)).all()
            e = edges[got["steps"][p][have]]
            assert np.array_equal(e["from"], got["nodes"][p][have]) and np.array_equal(e["to"], got["nodes"][p + 1][have]) and (e["junction"] == p).all()


def check(ctx, rows, queries):
    """graph_thread_rows of ctx (which holds `rows`) against the model on the run's segments; returns (got, the model's)."""
    red = ctx.reduced_traceback()
    want = tm.thread_model(rows, red["lb"], red["rb"], queries)
    edges = ctx.block_graph()["edges"]
    assert np.array_equal(edges, want["graph"]["edges"])
    got = ctx.graph_thread_rows(queries)
    same(got, want, edges)
    slim = ctx.graph_thread_rows(queries, want_nodes=False, want_steps=False)
    assert slim["nodes"] is None and slim["steps"] is None
    assert np.array_equal(slim["per_row"], want["per_row"]) and np.array_equal(slim["per_segment"], want["per_segment"])
    assert {k: slim["summary"][k] for k in SUMMARY} == {k: want["summary"][k] for k in SUMMARY}
    return got, want


def own_rows_are_on_the_graph(ctx, rows):
    got = ctx.graph_thread_rows(rows)
    S = ctx.result.segment_count
    assert np.array_equal(got["nodes"], ctx.block_graph(want_row_nodes=True)["row_nodes"])
    assert (got["steps"] != tm.NONE).all() and got["summary"]["rows_on_graph"] == len(rows) and got["summary"]["junctions_linked"] == len(rows) * (S - 1)
    assert (got["per_row"]["walks"] == 1).all() and (got["per_row"]["longest_walk_segments"] == S).all()
    assert (got["per_row"]["columns_matched"] == rows.shape[1]).all() and (got["per_row"]["longest_walk_columns"] == rows.shape[1]).all()
    return got


def strangers(msa, founders, S, W, outside):
    """Queries that are not rows: mosaics of the founders, a row with a byte outside the alphabet, a row with a substitution."""
    q = tm.mosaic_queries(founders, S, W, 30, 17)
    bad = msa[1].copy()
    bad[(S - 1) * W] = outside
    sub = msa[2].copy()
    sub[W - 1] = founders[0, W - 1] if founders[0, W - 1] != sub[W - 1] else founders[0, 0]
    return np.concatenate([q, [bad, sub]])


# ---- widths of the rows and of the queries

@pytest.mark.parametrize("alphabet,bits,query_bits", [(b"ACG", 2, 2), (b"ACGT", 2, 4), (bytes(range(65, 80)), 4, 4), (bytes(range(65, 81)), 4, 8),
                                                        (bytes(range(48, 88)), 8, 8)])
def test_code_widths(pkg, alphabet, bits, query_bits):
    """sigma = 3, 4, 15, 16 and 40: the queries need the code `sigma`, so at 4 and 16 they are a width above the rows.  m = 41: the
    last byte of a packed column is partial at every width."""
    S, W = 5, 65
    msa, founders = tm.full_mosaic(4, 41, S, W, seed=len(alphabet), alphabet=alphabet)
    ctx = context(pkg, msa, W)
    sigma, have_bits, table = ctx.alphabet()
    assert (sigma, have_bits, table) == (len(alphabet), bits, alphabet) and ctx.result.segment_count == S
    assert query_bits == (2 if sigma + 1 <= 4 else 4 if sigma + 1 <= 16 else 8)
    own_rows_are_on_the_graph(ctx, msa)
    got, want = check(ctx, msa, np.concatenate([msa, strangers(msa, founders, S, W, ord("z"))]))
    assert want["summary"]["junctions_novel"] > 0 and want["nodes"][S - 1, len(msa) + 30] == tm.NONE
    assert ctx.graph_thread_info()["queries_out_of_alphabet"] == 1
    ctx.close()


# ---- query counts: a wave, a tile of 256, packed bytes not filled

@pytest.mark.parametrize("Q", [1, 3, 63, 64, 65, 257])
def test_query_counts(mosaic, Q):
    ctx, msa, founders, W = mosaic
    odd = strangers(msa, founders, 6, W, ord("N"))
    # the two rows with an unmatched segment first, then rows of the alignment, then mosaics
    pool = np.concatenate([odd[-2:], msa, odd[:-2], tm.mosaic_queries(founders, 6, W, 257, 23)])[:257]
    got, want = check(ctx, msa, np.ascontiguousarray(pool[:Q]))
    if Q >= 63:
        assert want["summary"]["junctions_novel"] > 0 and (want["nodes"] == tm.NONE).any() and want["summary"]["rows_on_graph"] > 0


# ---- segment widths

@pytest.mark.parametrize("W", [1, 63, 64, 65])
def test_segment_widths(pkg, W):
    msa = gapped_blocks(W, b"ACGT", seed=W)
    ctx = context(pkg, msa, W)
    red = ctx.reduced_traceback()
    assert ((red["rb"] - red["lb"]) == W).all() and len(red) == 6
    own_rows_are_on_the_graph(ctx, msa)
    rng = np.random.default_rng(W)
    q = msa[rng.integers(0, len(msa), size=(50, 6)).repeat(W, axis=1), np.arange(6 * W)]      # mosaics of the rows by blocks
    q[40:45, rng.integers(0, 6 * W, size=5)] = ord("N")
    q[45, 0], q[46, 6 * W - 1] = ord("N"), ord("N")
    got, want = check(ctx, msa, np.ascontiguousarray(q))
    assert (want["nodes"] == tm.NONE).any() and want["summary"]["segments_matched"] > 0
    ctx.close()


def test_few_long_segments(pkg):
    """Two segments of 5,003 columns: the keys' loops and the comparisons run over thousands of columns a lane."""
    S, W = 2, 5003
    msa, founders = tm.full_mosaic(3, 20, S, W, seed=50)
    ctx = context(pkg, msa, W)
    red = ctx.reduced_traceback()
    assert len(red) == S and ((red["rb"] - red["lb"]) == W).all()
    own_rows_are_on_the_graph(ctx, msa)
    q = np.concatenate([tm.mosaic_queries(founders, S, W, 12, 51), msa[:3]])
    q[12, W - 1] = ord("N")                                    # the last column of a segment
    q[13, 2 * W - 1] = ord("A") if q[13, 2 * W - 1] != ord("A") else ord("C")      # a substituted base in the alignment's last column
    got, want = check(ctx, msa, q)
    assert want["nodes"][0, 12] == tm.NONE and want["nodes"][1, 13] == tm.NONE and want["nodes"][0, 13] != tm.NONE
    ctx.close()


# ---- the model's cases

@pytest.mark.parametrize("name", tm.CASES)
def test_model_cases(mosaic, name):
    ctx, msa, founders, W = mosaic
    rows, L, queries, listed = tm.case(name)
    assert np.array_equal(rows, msa) and L == W
    got, want = check(ctx, msa, queries)
    assert ("novel" in listed) == (got["summary"]["junctions_novel"] > 0) and ("unmatched" in listed) == bool((got["nodes"] == tm.NONE).any())
    info = ctx.graph_thread_info()
    outside = int(sum((~np.isin(queries[:, s * W:(s + 1) * W], np.frombuffer(b"ACGT", dtype=np.uint8))).any(axis=1).sum() for s in range(6)))
    assert info["queries_out_of_alphabet"] == outside and ("outside" in listed) == (outside > 0)
    assert info["key_bits"] == 64 and info["table_slots"] == 64


# ---- classes that share a key

@pytest.mark.parametrize("bits", [2, 1])
def test_key_collisions(mosaic, bits):
    """Five classes a segment and four keys (two at one bit): in every segment two classes share a key, and queries that cover every
    class meet a candidate that fails the comparison.  Nothing of the result moves."""
    ctx, msa, founders, W = mosaic
    queries = np.concatenate([msa, tm.mosaic_queries(founders, 6, W, 40, 3), tm.case("mixed")[2]])
    ctx.set_tuning("FSEQ_GRAPH_THREAD_KEY_BITS", None)
    wide = ctx.graph_thread_rows(queries)
    assert ctx.graph_thread_info()["key_bits"] == 64
    assert all(len(np.unique(wide["nodes"][s][wide["nodes"][s] != tm.NONE])) == 5 for s in range(6))      # the queries cover every class
    try:
        ctx.set_tuning("FSEQ_GRAPH_THREAD_KEY_BITS", bits)
        assert ctx.result is not None                                # (the knob is the threading's alone: the run stands)
        narrow, want = check(ctx, msa, queries)
        info = ctx.graph_thread_info()
        same(narrow, wide)
        assert info["key_bits"] == bits and info["candidates_rejected"] > 0
        assert info["candidates_verified"] - info["candidates_rejected"] == want["summary"]["segments_matched"]
    finally:
        ctx.set_tuning("FSEQ_GRAPH_THREAD_KEY_BITS", None)
    again = ctx.graph_thread_rows(queries)
    same(again, wide)
    assert ctx.graph_thread_info()["key_bits"] == 64


# ---- class counts across the workgroup's threads and at the table's cap

def bordered(pkg, X, m):
    msa, founders = tm.full_mosaic(X, m, 3, 16, seed=X)
    res = fso.segment_long(np.ascontiguousarray(msa), 16)
    assert res["status"] == 0 and res["reduced"]["segment_size"].tolist() == [X] * 3      # the oracle, on the CPU: X classes in every segment
    ctx = context(pkg, msa, 16)
    assert ctx.result.max_segment_size == X and ctx.result.segment_count == 3
    return ctx, msa, founders


@pytest.mark.parametrize("X,m", [(255, 300), (256, 300), (257, 300), (1025, 1100), (4096, 4200)])
def test_class_counts(pkg, X, m):
    ctx, msa, founders = bordered(pkg, X, m)
    own_rows_are_on_the_graph(ctx, msa)
    q = np.concatenate([tm.mosaic_queries(founders, 3, 16, 100, X), msa[:2]])
    q[100, 5], q[101, 47] = ord("N"), ord("N")
    got, want = check(ctx, msa, q)
    assert want["summary"]["junctions_novel"] > 0 and want["summary"]["segments_matched"] == 3 * 102 - 2
    info = ctx.graph_thread_info()
    assert info["table_slots"] == max(64, 1 << (2 * X - 1).bit_length()) and info["table_slots"] >= 2 * X
    ctx.close()


def test_more_than_4096_classes_are_refused(pkg):
    ctx, msa, founders = bordered(pkg, 4097, 4200)
    assert pkg.GRAPH_THREAD_MAX_CLASSES == 4096
    before = ctx.block_graph()
    with pytest.raises(pkg.FseqError) as err:
        ctx.graph_thread_rows(msa[:5])
    assert err.value.code == pkg.FSEQ_E_UNSUPPORTED and "4,096" in str(err.value)
    with pytest.raises(pkg.FseqError):
        ctx.graph_thread_info()                                      # (no call has finished)
    after = ctx.block_graph()                                        # the context stays usable
    assert np.array_equal(before["nodes"], after["nodes"]) and np.array_equal(before["edges"], after["edges"])
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
    assert sub.alphabet()[0] == 5                              # (N is a code of the sub-context: in the alphabet, in no node)
    for length in (W, 2 * W):
        if length != W:
            sub.set_segment_length(length)
        sub.run()
        red = sub.reduced_traceback()
        assert len(red) == (S if length == W else 3)
        want = tm.thread_model(source[kept], red["lb"], red["rb"], source[held])
        got = sub.graph_thread_held_out()
        same(got, want, sub.block_graph()["edges"])
        same(sub.graph_thread_rows(source[held]), got)
        slim = sub.graph_thread_held_out(want_nodes=False, want_steps=False)
        assert slim["nodes"] is None and slim["steps"] is None and np.array_equal(slim["per_row"], want["per_row"])
        assert (want["nodes"] == tm.NONE).any() and want["summary"]["rows_on_graph"] >= 3
        assert length != W or want["summary"]["junctions_novel"] > 0
    sub.close()


# ---- the context afterwards

def test_state_is_left_alone(mosaic, tmp_path):
    ctx, msa, founders, W = mosaic
    queries = tm.case("mixed")[2]
    perm = ctx.join_greedy()
    summary = ctx.match_rows(queries[:20], permutations=perm)
    pieces, sets = ctx.match_pieces()
    ctx.write_match(str(tmp_path / "before.txt"))
    graph = ctx.block_graph(want_row_nodes=True)
    now = ctx.device_bytes()[0]
    check(ctx, msa, queries)
    assert ctx.device_bytes()[0] == now                        # every buffer of the calls was theirs alone
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

    refused(lambda: ctx.graph_thread_rows(msa[:4]), pkg.FSEQ_E_ARG)          # before a run
    refused(ctx.graph_thread_info, pkg.FSEQ_E_ARG)
    ctx.run()
    refused(lambda: ctx.graph_thread_rows(msa[:0]), pkg.FSEQ_E_ARG)          # no rows
    refused(ctx.graph_thread_held_out, pkg.FSEQ_E_ARG)                       # a plain context holds no rows out
    lib = pkg.load_library()
    assert lib.fseq_graph_thread_rows(ctx.h, None, 3, None, None, None, None, None) == pkg.FSEQ_E_ARG
    import ctypes as C
    rows = (C.c_void_p * 2)(msa.ctypes.data, None)
    assert lib.fseq_graph_thread_rows(ctx.h, rows, 2, None, None, None, None, None) == pkg.FSEQ_E_ARG and b"null query row" in lib.fseq_last_error(ctx.h)
    own_rows_are_on_the_graph(ctx, msa)                                      # the context stays usable
    # an identity-reduced context, and one that carries held-out rows along
    wide = msa.copy()
    wide[:, 200:320] = wide[0, 200:320]
    src = pkg.SegmentationContext(203, 600, 20)
    src.set_sequences(wide)
    reduced = src.without_identity_columns(20)
    reduced.run()
    refused(lambda: reduced.graph_thread_rows(wide[:3, :reduced.n]), pkg.FSEQ_E_UNSUPPORTED)
    sub = src.without_rows(np.array([5, 9], dtype=np.uint32), 20)
    both = sub.without_identity_columns(20, keep_held_out=True)
    both.run()
    refused(both.graph_thread_held_out, pkg.FSEQ_E_UNSUPPORTED)
    sub.run()
    assert sub.graph_thread_held_out()["summary"]["rows"] == 2               # (the context it was made from serves its own)
    for c in (both, sub, reduced, src, ctx):
        c.close()


def test_sharded_context_is_refused(pkg):
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
        ctxs[0].graph_thread_rows(msa[:3])
    assert err.value.code == pkg.FSEQ_E_UNSUPPORTED and "sharded" in str(err.value)
