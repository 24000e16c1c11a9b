"""Full-length rows threaded through the block graph of an identity-reduced context (fseq_graph_thread_rows_restored,
fseq_graph_thread_held_out_restored; k_gt_exceptions and k_gt_rows<true>, csrc/fseq_graphthread.hpp).

The yardstick is tests/block_graph_restored_model.py: tests/graph_thread_model.py on the FULL-LENGTH rows and queries over the
restored bounds of the run's segments -- nodes, steps, per_row, per_segment and the summary, integer for integer.  Wherever the
queries' bytes are all in the source's alphabet they go through both entries: held out of a source alignment and carried along
(hold.cols and the exception cells the context was made with), and the same bytes uploaded."""
import ctypes as C
import importlib

import numpy as np
import pytest

import block_graph_restored_model as rm
import graph_thread_model as tm
import identity_model as im

pytestmark = pytest.mark.gpu

S6 = tm.MOSAIC[2]


@pytest.fixture(scope="module")
def pkg():
    return importlib.import_module("founder-sequences_amd")


def context(pkg, full, L, held_queries=None):
    """The run context over the kept columns of `full`; with held_queries, they are rows of the source held out of it and carried
    along (fseq_create_without_rows, then fseq_create_without_identity_columns_held), in the order given."""
    m, n = full.shape
    if held_queries is None:
        src = pkg.SegmentationContext(m, n, L)
        src.set_sequences(np.ascontiguousarray(full))
        ctx = src.without_identity_columns(L)
        src.close()
    else:
        q = len(held_queries)
        source = np.ascontiguousarray(np.concatenate([full[:2], held_queries, full[2:]]))
        held = np.arange(2, 2 + q, dtype=np.uint32)[::-1].copy()        # (in no ascending order: query i is source row held[i])
        source[held] = held_queries
        src = pkg.SegmentationContext(m + q, n, L)
        src.set_sequences(source)
        sub = src.without_rows(held, L)
        src.close()
        ctx = sub.without_identity_columns(L, keep_held_out=True)
        sub.close()
        assert ctx.n_held == q
    assert ctx.m == m and ctx.source_n == n and ctx.n == int((~im.identity_mask(full)).sum())
    try:
        ctx.run()
    except pkg.NoReduction:
        pass
    return ctx


def assert_equals_model(got, want, tag=""):
    for what in ("nodes", "steps", "per_row", "per_segment"):
        assert got[what].dtype == want[what].dtype and got[what].shape == want[what].shape, (tag, what)
        assert np.array_equal(got[what], want[what]), (tag, what, np.argwhere(got[what] != want[what])[:5].tolist())
    assert {k: v for k, v in got["summary"].items() if k != "ms_device"} == want["summary"], (tag, got["summary"], want["summary"])


def check_both(pkg, full, L, queries, segments=None, tuning=()):
    """queries through both entries against the model; returns (the model's threading, the context, lb, rb)."""
    ctx = context(pkg, full, L, queries)
    red = ctx.reduced_traceback()
    if segments is not None:
        assert len(red) == segments
    want = rm.expected_threading(full, red["lb"], red["rb"], queries)
    for name, value in tuning:
        ctx.set_tuning(name, value)
    assert_equals_model(ctx.graph_thread_held_out_restored(), want, "held")
    assert_equals_model(ctx.graph_thread_rows_restored(queries), want, "rows")
    slim = ctx.graph_thread_rows_restored(queries, want_nodes=False, want_steps=False)
    assert slim["nodes"] is None and slim["steps"] is None and np.array_equal(slim["per_row"], want["per_row"])
    for name, _ in tuning:
        ctx.set_tuning(name, None)
    return want, ctx, red["lb"], red["rb"]


def sprinkled(full, founders, kept, W, count, seed, alphabet=b"ACGT", S=S6):
    """count mosaics of the founders at full length: every third with an exception cell, every seventh with two, every fifth
    with a base changed at a kept column."""
    rng = np.random.default_rng(seed)
    q = rm.mosaic_queries(full, founders, kept, S, W, count, seed)
    ident = np.flatnonzero(im.identity_mask(full))
    for i in range(count):
        cells = ([ident[rng.integers(len(ident))]] if i % 3 == 0 else []) + ([ident[rng.integers(len(ident))], ident[-1]] if i % 7 == 0 else [])
        for c in cells:
            q[i, c] = rm.other_byte(full[0, c], alphabet)
        if i % 5 == 0:
            k = kept[rng.integers(len(kept))]
            q[i, k] = rm.other_byte(q[i, k], alphabet)
    return q


# ---- query counts around a tile of 256

@pytest.mark.parametrize("Q", [1, 255, 256, 257])
def test_query_counts(pkg, Q):
    full, R, founders, kept, W = rm.thread_rows()
    queries = sprinkled(full, founders, kept, W, Q, seed=Q)
    want, ctx, lb, rb = check_both(pkg, full, W, queries, segments=S6)
    if Q > 1:
        assert want["summary"]["junctions_novel"] > 0 and 0 < want["summary"]["segments_matched"] < Q * S6
        cells = rm.exception_cells(queries, full)
        assert any(len(c) == 0 for c in cells) and any(len(c) == 1 for c in cells) and any(len(c) > 1 for c in cells)


# ---- what the definitions promise

def test_own_rows_and_queries_without_exception_cells(pkg):
    full, R, founders, kept, W = rm.thread_rows()
    ctx = context(pkg, full, W)
    red = ctx.reduced_traceback()
    lb, rb = red["lb"], red["rb"]
    assert len(red) == S6
    # the alignment's own rows thread to their nodes
    got = ctx.graph_thread_rows_restored(full)
    assert_equals_model(got, rm.expected_threading(full, lb, rb, full))
    assert np.array_equal(got["nodes"], ctx.block_graph(want_row_nodes=True)["row_nodes"]) and got["summary"]["rows_on_graph"] == len(full)
    assert (got["per_row"]["columns_matched"] == full.shape[1]).all() and (got["per_row"]["longest_walk_columns"] == full.shape[1]).all()
    # no exception cell: the reduced threading of the kept columns
    reduced_queries = tm.mosaic_queries(founders, S6, W, 40, 3)
    queries = rm.expand(reduced_queries, full, kept)
    got = ctx.graph_thread_rows_restored(queries)
    assert_equals_model(got, rm.expected_threading(full, lb, rb, queries))
    want = tm.thread_model(R, lb, rb, reduced_queries)
    assert np.array_equal(got["nodes"], want["nodes"]) and np.array_equal(got["steps"], want["steps"]) and np.array_equal(got["per_segment"], want["per_segment"])


def test_single_cells(pkg):
    """One exception cell at source column 0 (= src_lb of segment 0), at n_src - 1, at src_rb_s - 1; and, src_lb_s of s > 0 being a
    kept column by definition, a base changed there: exactly that segment is unmatched and both junctions beside it lose their step."""
    full, R, founders, kept, W = rm.thread_rows()
    lb, rb = rm.blocks(S6, W)
    _, src_lb, src_rb = rm.restored_graph(full, lb, rb)
    row = 5
    places = [(0, 0), (S6 - 1, full.shape[1] - 1), (2, int(src_rb[2]) - 1), (3, int(src_rb[3]) - 1), (4, int(src_rb[4]) - 1)]
    queries = [full[row].copy()] + [rm.plant(full[row], full, cell) for _, cell in places]
    changed = tm.substituted(R, W, row, 3 * W)                  # (kept column 3 W is segment 3's src_lb)
    q = full[row].copy()
    q[kept] = changed
    assert q[int(src_lb[3])] != full[row, int(src_lb[3])] and int((q != full[row]).sum()) == 1
    queries.append(q)
    places.append((3, int(src_lb[3])))
    queries = np.stack(queries)
    want, ctx, got_lb, got_rb = check_both(pkg, full, W, queries, segments=S6)
    assert np.array_equal(got_lb, lb) and np.array_equal(got_rb, rb)
    assert (want["nodes"][:, 0] != tm.NONE).all() and (want["steps"][:, 0] != tm.NONE).all()
    for i, (s, cell) in enumerate(places, start=1):
        assert [x for x in range(S6) if want["nodes"][x, i] != want["nodes"][x, 0]] == [s] and want["nodes"][s, i] == tm.NONE, (s, cell)
        lost = [p for p in range(S6 - 1) if want["steps"][p, i] != want["steps"][p, 0]]
        assert lost == [p for p in (s - 1, s) if 0 <= p < S6 - 1] and all(want["steps"][p, i] == tm.NONE for p in lost), (s, cell)


def test_a_cell_in_every_segment_and_bytes_outside_the_alphabet(pkg):
    full, R, founders, kept, W = rm.thread_rows()
    ctx = context(pkg, full, W)
    red = ctx.reduced_traceback()
    lb, rb = red["lb"], red["rb"]
    _, src_lb, src_rb = rm.restored_graph(full, lb, rb)
    every = full[7].copy()
    for s in range(len(lb)):
        every = rm.plant(every, full, int(src_rb[s]) - 1)
    outside_identity = rm.plant(full[7], full, int(src_rb[1]) - 1, byte=ord("N"))
    outside_kept = full[7].copy()
    outside_kept[int(kept[3 * W + 2])] = ord("N")
    queries = np.stack([every, outside_identity, outside_kept, full[7]])
    got = ctx.graph_thread_rows_restored(queries)
    assert_equals_model(got, rm.expected_threading(full, lb, rb, queries))
    assert (got["nodes"][:, 0] == tm.NONE).all() and got["per_row"]["walks"][0] == 0
    assert got["nodes"][1, 1] == tm.NONE and (np.delete(got["nodes"][:, 1], 1) != tm.NONE).all()
    assert got["nodes"][3, 2] == tm.NONE and (np.delete(got["nodes"][:, 2], 3) != tm.NONE).all()
    assert ctx.graph_thread_info()["queries_out_of_alphabet"] == 1      # (the kept column's: an identity column is no cell of the kernels' queries)


# ---- few segments, code widths

@pytest.mark.parametrize("S", [1, 2])
def test_one_and_two_segments(pkg, S):
    R, founders = rm.mosaic(3, 9, S, 40, seed=2)
    full, kept = rm.with_runs(R, {0: b"AC-G", 17: b"T" * 70, S * 40: b"-A"})
    queries = sprinkled(full, founders, kept, 40, 12, seed=S, S=S)
    check_both(pkg, full, 20 if S == 1 else 40, queries, segments=S)


@pytest.mark.parametrize("alphabet,bits", [(b"ACG", 2), (b"ACGT", 4), (bytes(range(48, 88)), 8)])
def test_code_widths(pkg, alphabet, bits):
    """2, 4 and 8 bits a code of the alignment (the gap byte of the runs is one of the codes); the uploaded queries are packed at
    4, 4 and 8."""
    full, R, founders, kept, W = rm.thread_rows(alphabet)
    queries = sprinkled(full, founders, kept, W, 30, seed=bits, alphabet=alphabet)
    want, ctx, lb, rb = check_both(pkg, full, W, queries, segments=S6)
    assert ctx.alphabet()[1] == bits and 0 < want["summary"]["segments_matched"] < 30 * S6


# ---- the upload in chunks; keys that collide

def test_upload_in_chunks_of_64_columns(pkg):
    """FSEQ_MATCH_STAGE_BYTES = 64: the queries go up 64 source columns at a time; exception cells at 63 and 64, on both sides of a
    chunk's border, at 128 and in the last, partial chunk."""
    full, R, founders, kept, W = rm.thread_rows()
    mask = im.identity_mask(full)
    assert mask[63] and mask[64] and mask[128] and 128 < full.shape[1] - 1 < 192
    queries = np.stack([rm.plant(full[3], full, 63), rm.plant(full[4], full, 64), rm.plant(rm.plant(full[6], full, 63), full, 64),
                        rm.plant(full[8], full, 128), rm.plant(full[9], full, full.shape[1] - 1), full[10]])
    want, ctx, lb, rb = check_both(pkg, full, W, queries, segments=S6, tuning=[("FSEQ_MATCH_STAGE_BYTES", "64")])
    assert [int((want["nodes"][:, i] == tm.NONE).sum()) for i in range(6)] == [1, 1, 1, 1, 1, 0]


def test_one_bit_keys(pkg):
    full, R, founders, kept, W = rm.thread_rows()
    queries = sprinkled(full, founders, kept, W, 60, seed=60)
    want, ctx, lb, rb = check_both(pkg, full, W, queries, segments=S6, tuning=[("FSEQ_GRAPH_THREAD_KEY_BITS", 1)])
    ctx.set_tuning("FSEQ_GRAPH_THREAD_KEY_BITS", 1)
    ctx.graph_thread_held_out_restored()
    info = ctx.graph_thread_info()
    assert info["key_bits"] == 1 and info["candidates_rejected"] > 0


# ---- the context afterwards; refusals

def test_the_last_match_stays(pkg):
    full, R, founders, kept, W = rm.thread_rows()
    held = sprinkled(full, founders, kept, W, 9, seed=9)
    ctx = context(pkg, full, W, held)
    red = ctx.reduced_traceback()
    perm = ctx.join_greedy()
    others = sprinkled(full, founders, kept, W, 14, seed=14)
    for match in (lambda: ctx.match_rows_restored(others, perm), lambda: ctx.match_held_out_restored(perm)):
        summary = match()
        pieces, exc = ctx.match_pieces(), ctx.match_exceptions()
        now = ctx.device_bytes()[0]
        third = sprinkled(full, founders, kept, W, 5, seed=5)
        assert_equals_model(ctx.graph_thread_rows_restored(third), rm.expected_threading(full, red["lb"], red["rb"], third))
        assert_equals_model(ctx.graph_thread_held_out_restored(), rm.expected_threading(full, red["lb"], red["rb"], held))
        assert ctx.device_bytes()[0] == now                     # every buffer of the calls was theirs alone
        after_pieces, after_exc = ctx.match_pieces(), ctx.match_exceptions()
        assert all(np.array_equal(a, b) for a, b in zip(after_pieces, pieces)) and all(np.array_equal(a, b) for a, b in zip(after_exc, exc))
    assert np.array_equal(ctx.join_greedy(), perm) and np.array_equal(ctx.reduced_traceback(), red)


def test_refusals(pkg):
    full, R, founders, kept, W = rm.thread_rows()
    lib = pkg.load_library()
    queries = np.ascontiguousarray(full[:3])
    rows = (C.c_void_p * 3)(*[queries.ctypes.data + r * queries.strides[0] for r in range(3)])
    per_row = np.full(3, 7, dtype=np.uint8).repeat(40).view(pkg.GRAPH_THREAD_ROW_DTYPE)

    def refused(ctx, code, held=False, words=None, rows_=rows, n=3):
        before = per_row.copy()
        rc = (lib.fseq_graph_thread_held_out_restored(ctx.h, None, None, per_row.ctypes.data, None, None) if held
              else lib.fseq_graph_thread_rows_restored(ctx.h, rows_, n, None, None, per_row.ctypes.data, None, None))
        assert rc == code and lib.fseq_last_error(ctx.h), (rc, code)
        assert words is None or words in lib.fseq_last_error(ctx.h), lib.fseq_last_error(ctx.h)
        assert np.array_equal(per_row, before)                  # nothing written

    plain = pkg.SegmentationContext(full.shape[0], full.shape[1], W)
    plain.set_sequences(full)
    plain.run()
    for held in (False, True):                                  # not identity-reduced
        refused(plain, pkg.FSEQ_E_ARG, held, b"not a context made by fseq_create_without_identity_columns")
    ctx = plain.without_identity_columns(W)
    plain.close()
    refused(ctx, pkg.FSEQ_E_ARG, words=b"no result")            # before a run
    ctx.run()
    refused(ctx, pkg.FSEQ_E_ARG, held=True, words=b"not a context made by fseq_create_without_identity_columns_held")       # no carried held-out rows
    refused(ctx, pkg.FSEQ_E_ARG, rows_=None, words=b"no query rows")
    refused(ctx, pkg.FSEQ_E_ARG, n=0, words=b"no query rows")
    refused(ctx, pkg.FSEQ_E_ARG, rows_=(C.c_void_p * 3)(queries.ctypes.data, None, queries.ctypes.data), words=b"null query row")
    with pytest.raises(pkg.FseqError):
        ctx.graph_thread_info()                                 # (none has finished)
    # the reduced twins refuse such a context as they did, word for word
    with pytest.raises(pkg.FseqError) as err:
        ctx.graph_thread_rows(np.ascontiguousarray(full[:3, kept]))
    assert err.value.code == pkg.FSEQ_E_UNSUPPORTED and "queries in source co-ordinates, with their exception cells, are not served" in str(err.value)
    with pytest.raises(ValueError):
        ctx.graph_thread_rows_restored(np.ascontiguousarray(full[:3, kept]))      # (rows of the reduced length)
    got = ctx.graph_thread_rows_restored(queries)
    assert got["summary"]["rows_on_graph"] == 3
    short = context(pkg, full, full.shape[1])                   # fewer kept columns than two segments: the short path has no segments
    refused(short, pkg.FSEQ_E_ARG)
