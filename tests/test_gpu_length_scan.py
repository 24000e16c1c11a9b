"""fseq_scan_segment_lengths on the card: the maximum segment size at many segment lengths from one resident alignment.  Expected
values come from the CPU oracle (fso.segment_long at every long-path length, fso.segment_short for n < 2L); what the summary and
the entries must say about built and folded lists comes from the model (tests/proto_length_scan.py, CASES)."""
import functools
import importlib

import numpy as np
import pytest

import fso
import proto_length_scan as P

pytestmark = pytest.mark.gpu

E_ARG, E_UNSUPPORTED = 1, 5


@pytest.fixture(scope="module")
def pkg():
    return importlib.import_module("founder-sequences_amd")


def oracle_sizes(msa, lengths):
    n = msa.shape[1]
    short = len(fso.segment_short(msa)[0])
    return {int(L): (int(fso.segment_long(msa, int(L), threads=4)["max_segment_size"]) if n >= 2 * int(L) else short) for L in set(lengths)}


@functools.lru_cache(maxsize=None)
def case(name):
    msa = P.case_msa(name)
    return msa, oracle_sizes(msa, P.CASES[name]["lengths"])


def make_ctx(pkg, msa, L, knobs=(), **kw):
    ctx = pkg.SegmentationContext(msa.shape[0], msa.shape[1], L, **kw)
    for k, v in dict(knobs).items():
        ctx.set_tuning(k, v)
    ctx.set_sequences(msa)
    return ctx


def check_entries(entries, lengths, want, n):
    assert [int(x) for x in entries["segment_length"]] == [int(x) for x in lengths]
    for e in entries:
        L = int(e["segment_length"])
        assert int(e["max_segment_size"]) == want[L], (L, int(e["max_segment_size"]), want[L])
        assert int(e["short_path"]) == (1 if n < 2 * L else 0)
        assert (int(e["lists"]) == pkg_none()) == (n < 2 * L)


def pkg_none():
    return 2        # FSEQ_SCAN_LISTS_NONE


def refused(pkg, call, code=E_ARG):
    with pytest.raises(pkg.FseqError) as e:
        call()
    assert e.value.code == code


def test_lds_resident_rows_shuffled_with_repeats(pkg):
    c = P.CASES["lds_resident"]
    msa, want = case("lds_resident")
    n = msa.shape[1]
    rng = np.random.default_rng(0)
    lengths = list(c["lengths"]) + [7, 200, 4000, 5]
    rng.shuffle(lengths)
    ctx = make_ctx(pkg, msa, 20, list_cap=c["list_cap"])
    entries, sm = ctx.scan_segment_lengths(lengths)
    check_entries(entries, lengths, want, n)
    long_lengths = sorted({L for L in lengths if n >= 2 * L})
    # X >= m: every list is complete, so the lists are built once and folded to every further length
    assert sm["lists_built"] == 1 and sm["lists_folded"] == len(long_lengths) - 1 and sm["retries"] == 0
    assert sm["short_entries"] == sum(1 for L in lengths if n < 2 * L)
    for e in entries:
        L = int(e["segment_length"])
        if n >= 2 * L:
            assert int(e["lists"]) == (pkg.SCAN_LISTS_BUILT if L == long_lengths[0] else pkg.SCAN_LISTS_FOLDED), L
            assert int(e["list_cap"]) == msa.shape[0]
    # the DP in the form a run at that length chooses: speculative sweeps at the small lengths, the serial kernel at L = 200
    by_L = {int(e["segment_length"]): e for e in entries}
    assert all(int(by_L[L]["dp_chunks"]) > 0 for L in (5, 6, 7, 10, 20)) and int(by_L[200]["dp_chunks"]) == 0
    assert sm["ms_phase_a"] > 0 and sm["ms_total"] > 0
    ctx.close()


def test_folded_lists_in_place(pkg):
    """After a scan of [L1, L2] the context holds the lists of a scan of [L1] folded by the model."""
    msa, _ = case("lds_resident")
    m, n = msa.shape
    L1, L2 = 7, 56
    a = make_ctx(pkg, msa, 20, list_cap=63)
    b = make_ctx(pkg, msa, 20, list_cap=63)
    a.scan_segment_lengths([L1])
    eb, _ = b.scan_segment_lengths([L1, L2])
    assert int(eb[1]["lists"]) == pkg.SCAN_LISTS_FOLDED
    moved = 0
    for k in sorted({k for k in range(n) if k % 97 == 0 or k in (L2 - 2, L2 - 1, L2, n - 1)}):
        v, c, cnt0, complete = a.debug_column_list(k)
        ent = np.stack([v, c], axis=1).astype(np.uint32)
        hdr = np.array([len(v), cnt0, int(complete), int(c.sum())], dtype=np.uint32)
        want_ent, want_hdr = P.relump(ent, hdr, k, L2)
        gv, gc, gcnt0, gcomplete = b.debug_column_list(k)
        assert len(gv) == int(want_hdr[0]) and np.array_equal(gv, want_ent[:len(gv), 0]) and np.array_equal(gc, want_ent[:len(gv), 1]), k
        assert (gcnt0, gcomplete) == (cnt0, complete)
        moved += len(v) - len(gv)
    assert moved > 0
    a.close()
    b.close()


def test_overflow_builds_again_where_the_folded_lists_do_not_prove(pkg):
    c = P.CASES["overflow"]
    msa, want = case("overflow")
    ctx = make_ctx(pkg, msa, 20, list_cap=c["list_cap"])
    entries, sm = ctx.scan_segment_lengths(c["lengths"])
    check_entries(entries, c["lengths"], want, msa.shape[1])
    assert any(int(e["lists"]) == pkg.SCAN_LISTS_BUILT for e in entries[1:])
    # every retry doubles the capacity and adds one; the capacity never falls along the scan
    caps = [int(e["list_cap"]) for e in entries]
    assert caps == sorted(caps)
    X = c["list_cap"]
    for _ in range(sm["retries"]):
        X = min(msa.shape[0], 2 * X + 1)
    assert caps[-1] == X and sm["retries"] > 0
    assert sm["lists_built"] + sm["lists_folded"] == len(entries)
    ctx.close()


@pytest.mark.parametrize("name", ["bits4", "bits8"])
def test_wider_symbols(pkg, name):
    c = P.CASES[name]
    msa, want = case(name)
    ctx = make_ctx(pkg, msa, 20, list_cap=c["list_cap"])
    entries, sm = ctx.scan_segment_lengths(c["lengths"])
    check_entries(entries, c["lengths"], want, msa.shape[1])
    assert sm["lists_built"] == 1                                 # (X >= m: complete lists)
    ctx.close()


STREAMED_LENGTHS = [20, 64, 200, 700]


@functools.lru_cache(maxsize=None)
def streamed_case():
    msa = P.mosaic(8, 11265, 4000, seed=31, mu=0.0005)
    return msa, oracle_sizes(msa, STREAMED_LENGTHS)


@pytest.mark.parametrize("knob", ["FSEQ_REDUCED_ALWAYS", "FSEQ_NO_REDUCED"])
def test_streamed_rows(pkg, knob):
    msa, want = streamed_case()
    ctx = make_ctx(pkg, msa, 64, knobs={knob: "1"})
    try:
        ctx.run()
    except pkg.NoReduction:
        pass
    assert (ctx.timings()["reduced_blocks"] > 0) == (knob == "FSEQ_REDUCED_ALWAYS")
    entries, sm = ctx.scan_segment_lengths(STREAMED_LENGTHS)
    check_entries(entries, STREAMED_LENGTHS, want, msa.shape[1])
    assert sm["lists_built"] >= 1 and sm["lists_built"] + sm["lists_folded"] == len(STREAMED_LENGTHS)
    ctx.close()


def test_forced_rebuild_and_list_budget_build_every_entry(pkg):
    c = P.CASES["lds_resident"]
    msa, want = case("lds_resident")
    m, n = msa.shape
    lengths = [5, 20, 56, 97, 200, 1500, 1501]
    nlong = sum(1 for L in lengths if n >= 2 * L)
    ctx = make_ctx(pkg, msa, 20, knobs={"FSEQ_SCAN_REBUILD": "1"}, list_cap=c["list_cap"])
    entries, sm = ctx.scan_segment_lengths(lengths)
    check_entries(entries, lengths, want, n)
    assert sm["lists_built"] == nlong and sm["lists_folded"] == 0
    ctx.close()
    # a budget of a third of the lists: every attempt runs in windows, no whole list set exists to fold (lengths whose halo,
    # up to L columns in front of the last window, leaves room for a window)
    lengths = [5, 20, 56, 97, 200]
    full = n * ((m + 3) & ~1) * 8
    ctx = make_ctx(pkg, msa, 20, list_cap=c["list_cap"], list_memory=full // 3)
    entries, sm = ctx.scan_segment_lengths(lengths)
    check_entries(entries, lengths, want, n)
    assert sm["lists_built"] == len(lengths) and sm["lists_folded"] == 0
    ctx.close()


def outcome(ctx):
    res = ctx.run()
    red = ctx.reduced_traceback()
    return (res.max_segment_size, res.short_path, ctx.traceback().tobytes(), red.tobytes(),
            [tuple(x.tobytes() for x in ctx.boundary_state(i)) for i in range(len(red))])


def test_context_state_around_a_scan(pkg):
    msa, want = case("lds_resident")
    ctx = make_ctx(pkg, msa, 20)
    before = outcome(ctx)
    assert before[0] == want[20]
    ctx.scan_segment_lengths([10, 97, 4000])
    assert ctx.segment_length == 20
    out = np.zeros(4, dtype=pkg.SEGMENT_DTYPE)
    assert ctx.L.fseq_get_segments(ctx.h, out.ctypes.data) == E_ARG
    assert ctx.L.fseq_get_traceback(ctx.h, out.ctypes.data) == E_ARG
    assert ctx.L.fseq_boundary_state(ctx.h, 0, None, None) == E_ARG
    v, c, _, _ = ctx.debug_column_list(500)                       # the lists of the last long-path entry are held
    assert v[0] == 501 and c.sum() <= msa.shape[0]
    assert outcome(ctx) == before
    # refusals: nothing is written to the entries
    entries = np.zeros(2, dtype=pkg.LENGTH_SCAN_DTYPE)
    entries["segment_length"] = [10, 0]
    entries["max_segment_size"] = 77
    sm = pkg.LengthScanSummary()
    import ctypes as C
    assert ctx.L.fseq_scan_segment_lengths(ctx.h, entries.ctypes.data, 2, C.byref(sm)) == E_ARG
    assert ctx.L.fseq_scan_segment_lengths(ctx.h, None, 2, C.byref(sm)) == E_ARG
    assert ctx.L.fseq_scan_segment_lengths(ctx.h, entries.ctypes.data, 0, C.byref(sm)) == E_ARG
    assert list(entries["max_segment_size"]) == [77, 77]
    assert outcome(ctx) == before
    ctx.close()
    empty = pkg.SegmentationContext(60, 3000, 20)
    refused(pkg, lambda: empty.scan_segment_lengths([10]))       # no input
    empty.close()


def test_sharded_context_is_refused(pkg):
    import torch
    a = pkg.SegmentationContext(300, 5000, 10)
    words = int(a.L.fseq_shard_xbuf_words(a.h, 2))
    xbuf = torch.zeros(words + 64, dtype=torch.int32, device="cuda:0")
    a.set_shard(0, 2, xbuf.data_ptr(), xbuf.numel(), lambda off, cnt, op: 0)
    refused(pkg, lambda: a.scan_segment_lengths([10, 20]), E_UNSUPPORTED)
    refused(pkg, lambda: a.set_segment_length(20), E_UNSUPPORTED)
    a.close()
