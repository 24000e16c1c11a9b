"""The chunked input that drops the identity columns on the way (fseq_input_scan_identity .. fseq_input_end_kept,
fseq_set_rows_streamed_without_identity_columns; csrc/fseq_input_reduced.hpp) against the existing chain on the same bytes:
set_sequences(msa, staging_bytes=...) then without_identity_columns(L).  Integer work: every comparison is exact, the packed
bytes with their padding included.  Shapes sit at the edges of the kernels' tiles (a lane's rows, 64 packed bytes at each code
width, 16 rows a step and several row slabs of the scan, 16-column pieces, 128 kept columns a tile), not at the workload's."""
import ctypes as C
import importlib
import os
import subprocess

import numpy as np
import pytest

import identity_model as im
import input_model as model
import input_reduced_model as rmodel

pytestmark = pytest.mark.gpu

ROWS = [1, 2, 3, 15, 16, 17, 63, 64, 65, 255, 256, 257, 1025]
ALPHABETS = [2, 4, 5, 16, 17, 256]
WIDTHS = [1, 15, 16, 17, 64, 65, 100, 129]
N, L = 300, 20
E_ARG, E_UNSUPPORTED = 1, 5
JOIN_BIPARTITE = 1                                            # include/fseq.h, FSEQ_JOIN_BIPARTITE
staging_for = rmodel.staging_for


@pytest.fixture(scope="module")
def pkg():
    return importlib.import_module("founder-sequences_amd")


@pytest.fixture(scope="module")
def build():
    return importlib.import_module("founder-sequences_amd.build")


def outcome(pkg, ctx):
    """everything a run on the context's input gives, as comparable values"""
    try:
        res = ctx.run()
    except pkg.NoReduction:
        return ("no reduction",)
    if res.short_path:
        first, runs = ctx.short_path_runs()
        return ("short", res.max_segment_size, first.tolist(), runs.tolist())
    states = [tuple(x.tobytes() for x in ctx.boundary_state(i)) for i in range(res.segment_count)]
    return ("long", res.max_segment_size, ctx.traceback().tobytes(), ctx.reduced_traceback().tobytes(), states, ctx.join_greedy().tobytes())


def resident(ctx):
    """what the context holds of its input and of its source, as comparable values"""
    packed, bits = ctx.packed_columns()
    return {"n": ctx.n, "source_n": ctx.source_n, "bits": bits, "packed": packed.tobytes(), "ld": packed.shape[1], "alphabet": ctx.alphabet(),
            "mask": ctx.identity_mask().tobytes(), "kept": ctx.kept_columns().tobytes(), "rows": ctx.get_sequences().tobytes(),
            "summary": {k: v for k, v in ctx.identity_summary.items() if k != "ms_device"}}


def refused(pkg, call, code=E_ARG):
    with pytest.raises(pkg.FseqError) as ei:
        call()
    assert ei.value.code == code, ei.value
    return str(ei.value)


_rows = {}


def case_rows(m, size):
    """the rows of a case of the table: made once, shared, not changed"""
    if (m, size) not in _rows:
        _rows[(m, size)] = rmodel.planted(7 * m + size, m, N, model.alphabet_bytes(size, m), 0.5)
        _rows[(m, size)].setflags(write=False)
    return _rows[(m, size)]


_reference = {}


def reference(pkg, msa, key, width=64):
    """what the existing chain gives on the rows of a case: computed once, shared, not changed"""
    if key not in _reference:
        msa.setflags(write=False)
        ctx = rmodel.chain(pkg, msa, L, width)
        _reference[key] = (resident(ctx), outcome(pkg, ctx))
        ctx.close()
    return _reference[key]


def check_against_chain(pkg, msa, key, width, alphabet=None, skip=True):
    want_resident, want_outcome = reference(pkg, msa, key)
    m, n = msa.shape
    src = pkg.SegmentationContext(m, n, L)
    new = rmodel.feed(src, msa, width, L, alphabet, skip)
    mask = im.identity_mask(msa)
    assert np.array_equal(new.identity_mask(), mask) and np.array_equal(new.kept_columns(), np.nonzero(~mask)[0])
    assert resident(new) == want_resident                      # (the packed bytes with their padding, the mask, the kept list, sigma, the bits)
    assert src.device_bytes()[0] == 0 and src.input_chunk_columns() == 0      # src is left without an input and without a buffer
    src.close()                                               # (the new context stands alone)
    assert outcome(pkg, new) == want_outcome
    skipped = new.skipped_chunks
    new.close()
    return skipped


# ---- 1. parity over the shape table
CASES = [(m, size, WIDTHS[(i + j) % len(WIDTHS)]) for i, m in enumerate(ROWS) for j, size in enumerate(ALPHABETS)]


def test_the_cases_cover_what_they_claim():
    assert {c[0] for c in CASES} == set(ROWS) and {c[1] for c in CASES} == set(ALPHABETS) and {c[2] for c in CASES} == set(WIDTHS)
    assert 1 in WIDTHS and any(N % w not in (0, 1) for w in WIDTHS)     # ragged last chunks
    for size in ALPHABETS:
        assert max(model.alphabet_bytes(size, 3)) > 127
    # one lane's rows, a tile of 64 packed bytes at each width (256 / 128 / 64 rows) on both sides, and more than one row slab of the scan (16 rows a step)
    for edge in (64, 256):
        assert {edge - 1, edge, edge + 1} <= set(ROWS)
    assert max(ROWS) > 1024 and {15, 16, 17} <= set(ROWS)
    for m, size, _ in CASES:
        msa = case_rows(m, size)
        # every code width is reached: 2, 4 and 8 bits (a few hundred cells need not hold all of 256 values)
        assert model.code_table(msa)[2] == (2 if size <= 4 else 4 if size <= 16 else 8) and (len(np.unique(msa)) == size or size == 256), (m, size)
        mask = im.identity_mask(msa)
        assert m == 1 or (mask.any() and not mask.all())


@pytest.mark.parametrize("m,size,width", CASES, ids=["m%d-s%d-w%d" % c for c in CASES])
def test_parity(pkg, m, size, width):
    msa = case_rows(m, size)
    if m == 1:
        # one row: every column is an identity column, on both ways
        src = pkg.SegmentationContext(m, N, L)
        src.set_sequences(msa, staging_bytes=staging_for(m, width))
        want = refused(pkg, lambda: src.without_identity_columns(L))
        got = refused(pkg, lambda: rmodel.feed(src, msa, width, L))
        assert got == want and "every column is an identity column" in got
        src.close()
        return
    check_against_chain(pkg, msa, (m, size), width)
    assert m < 15 or reference(pkg, msa, (m, size))[1][0] == "long"      # (the outcome compared is that of a segmentation, not a refusal)


# ---- 2. identity patterns
def pattern_rows(m, n, kept_columns, seed=3, differ_rows=None, alphabet=b"ACT\xe7"):
    ident = np.ones(n, dtype=bool)
    ident[list(kept_columns)] = False
    return rmodel.planted(seed, m, n, alphabet, ident, differ_rows)


def test_no_identity_column(pkg):
    msa = rmodel.planted(5, 65, N, b"ACT\xe7", np.zeros(N, dtype=bool))
    assert check_against_chain(pkg, msa, "none", 64) == 0


def test_every_column_but_one(pkg):
    msa = pattern_rows(65, N, [137])
    assert check_against_chain(pkg, msa, "but-one", 64) == 4       # the other four chunks go without rows


def test_every_column_an_identity_column(pkg):
    m = 17
    msa = pattern_rows(m, N, [])
    other, _ = case_rows(m, 4), None
    src = pkg.SegmentationContext(m, N, L)
    src.input_begin(staging_bytes=staging_for(m, 64))
    begun = src.device_bytes()[0]
    assert staging_for(m, 64) <= begun <= staging_for(m, 64) + 320      # the staging and the input's two tables
    for c0 in range(0, N, 64):
        src.input_scan_identity(c0, msa[:, c0:c0 + 64])
    assert src.device_bytes()[0] > begun
    message = refused(pkg, lambda: src.input_reduce(L))
    assert "every column is an identity column" in message
    assert src.device_bytes()[0] == begun                      # nothing of the reduction is left allocated
    refused(pkg, lambda: src.input_columns_kept(0, 64))
    refused(pkg, lambda: src.input_end_kept())
    # ... and src takes a new input afterwards
    new = rmodel.feed(src, other, 64, L)
    assert resident(new) == reference(pkg, other, (m, 4))[0]
    new.close()
    src.close()


def test_identity_columns_at_the_ends_of_a_chunk_and_kept_columns_across_a_border(pkg):
    """chunks of 64: column 64 (first of a chunk) and 127 (last of one) are identity columns, 63 | 64' = 128 | 129 are kept on
    both sides of a border, the chunk [192, 256) holds no kept column and [256, 300) only kept ones"""
    kept = [3, 63, 65, 100, 126, 128, 129, 191] + list(range(256, N))
    msa = pattern_rows(33, N, kept)
    mask = im.identity_mask(msa)
    assert mask[64] and mask[127] and not mask[63] and not mask[128] and not mask[191] and mask[192:256].all() and not mask[256:].any()
    assert check_against_chain(pkg, msa, "ends", 64) == 1
    # the same without skipping: a chunk without a kept column may come with its rows as well
    assert check_against_chain(pkg, msa, "ends", 64, skip=False) == 0


def test_null_rows_only_for_a_chunk_without_a_kept_column(pkg):
    m = 33
    msa = pattern_rows(m, N, [3, 63, 65] + list(range(256, N)))
    src = pkg.SegmentationContext(m, N, L)
    src.input_begin(staging_bytes=staging_for(m, 64))
    for c0 in range(0, N, 64):
        src.input_scan_identity(c0, msa[:, c0:c0 + 64])
    src.input_reduce(L)
    assert [src.input_kept_columns(c0, min(64, N - c0)) for c0 in range(0, N, 64)] == [2, 1, 0, 0, 44]
    assert src.input_kept_columns(0, N) == 47 and src.input_kept_columns(4, 59) == 0
    refused(pkg, lambda: src.input_columns_kept(0, 64))        # this chunk holds kept columns: it needs its rows
    src.input_columns_kept(0, msa[:, 0:64])
    src.input_columns_kept(64, msa[:, 64:128])
    before = src.device_bytes()
    src.input_columns_kept(128, 64)
    src.input_columns_kept(192, 64)
    assert src.device_bytes() == before
    src.input_columns_kept(256, msa[:, 256:])
    new = src.input_end_kept()
    assert resident(new) == reference(pkg, msa, "null-rows")[0]
    new.close()
    src.close()


@pytest.mark.parametrize("m", [2, 17, 257, 1025])
def test_a_column_that_differs_in_one_row_only(pkg, m):
    """row 1 alone, and row m - 1 alone (the last row of the last slab of the scan), in the first, a middle and the last column"""
    rows = {0: 1, 1: m - 1, 150: 1, 151: m - 1, N - 2: m - 1, N - 1: 1, 77: 0}
    msa = pattern_rows(m, N, list(rows) + list(range(200, 260)), differ_rows=rows)
    for k, r in rows.items():
        differs = np.nonzero(msa[:, k] != (msa[0, k] if r else msa[1, k]))[0].tolist()
        assert differs == [r] or (m == 2 and r == m - 1 == 1 and differs == [1]), (k, r, differs)
    check_against_chain(pkg, msa, ("needle", m), 100)


def test_stale_bytes_behind_a_narrow_chunk(pkg):
    """a wide chunk, then narrow ones: the staged rows of the half hold the wide chunk's differing bytes behind the narrow chunk's
    last column, in both passes.  Chunks: 129 columns that all differ, then 33, 3 and 1 columns that are identity columns but one"""
    m = 65
    kept = list(range(0, 129)) + [140, 163, 165]
    msa = pattern_rows(m, 166, kept)
    widths = [129, 33, 3, 1]
    want = reference(pkg, msa, "stale")
    src = pkg.SegmentationContext(m, 166, L)
    src.input_begin(staging_bytes=staging_for(m, 129))
    at = 0
    for w in widths + widths:
        c0 = at % 166
        if at < 166:
            src.input_scan_identity(c0, msa[:, c0:c0 + w])
        else:
            src.input_columns_kept(c0, msa[:, c0:c0 + w])
        at += w
        if at == 166:
            src.input_reduce(L)
    new = src.input_end_kept()
    assert resident(new) == want[0] and outcome(pkg, new) == want[1]
    new.close()
    src.close()


def test_kept_list_across_two_tiles_of_its_scan(pkg):
    m, n = 3, 4097
    msa = rmodel.planted(9, m, n, b"ACG\xf4", 0.6)
    mask = im.identity_mask(msa)
    assert not mask[:2048].all() and not mask[2048:4096].all()
    msa = np.array(msa)
    msa[:, 4096] = [65, 67, 65]                                # the one column of the third tile is kept
    check_against_chain(pkg, msa, "tiles", 1000)


# ---- 3. the alphabet is the whole source's
def test_a_byte_that_occurs_only_in_identity_columns_takes_a_code(pkg):
    m = 65
    msa = np.array(rmodel.planted(21, m, N, b"ACGT", 0.5))
    mask = im.identity_mask(msa)
    msa[:, np.nonzero(mask)[0][::5]] = ord("N")
    assert set(np.unique(msa[:, ~mask]).tolist()) == set(b"ACGT") and set(np.unique(msa).tolist()) == set(b"ACGNT")
    want = reference(pkg, msa, "fifth")
    assert want[0]["bits"] == 4 and want[0]["alphabet"] == (5, 4, b"ACGNT")
    check_against_chain(pkg, msa, "fifth", 64)


def test_supplied_alphabet(pkg):
    m = 33
    msa = np.array(rmodel.planted(22, m, N, b"ACGT", 0.5))
    mask = im.identity_mask(msa)
    # listed in any order, with a byte that never occurs: it keeps its code, as in the existing chain from the same alphabet
    src = pkg.SegmentationContext(m, N, L)
    src.input_begin(alphabet=b"TN-GCA", staging_bytes=staging_for(m, 64))
    for c0 in range(0, N, 64):
        src.input_columns(c0, msa[:, c0:c0 + 64])
    src.input_end()
    want = src.without_identity_columns(L)
    src.close()
    src = pkg.SegmentationContext(m, N, L)
    new = rmodel.feed(src, msa, 64, L, alphabet=b"TN-GCA")
    assert resident(new) == resident(want) and new.alphabet() == (6, 4, b"-ACGNT")
    assert outcome(pkg, new) == outcome(pkg, want)
    new.close()
    want.close()
    # the existing chain's message for a byte outside the alphabet
    stray = 0xE9
    bad = np.array(msa)
    bad[m - 1, N - 1] = stray
    src.input_begin(alphabet=b"ACGT", staging_bytes=staging_for(m, 64))
    for c0 in range(0, N, 64):
        src.input_columns(c0, bad[:, c0:c0 + 64])
    message = refused(pkg, lambda: src.input_end())
    assert "0x%02X" % stray in message
    # ... in an identity column: refused by the reduce, the input is over
    bad = np.array(msa)
    bad[:, np.nonzero(mask)[0][7]] = stray
    assert im.identity_mask(bad).sum() == mask.sum()
    src.input_begin(alphabet=b"ACGT", staging_bytes=staging_for(m, 64))
    for c0 in range(0, N, 64):
        src.input_scan_identity(c0, bad[:, c0:c0 + 64])
    assert refused(pkg, lambda: src.input_reduce(L)) == message
    assert src.device_bytes()[0] == 0 and src.input_chunk_columns() == 0
    refused(pkg, lambda: src.input_columns_kept(0, bad[:, 0:64]))
    # ... in a kept column (one cell of it: the column stays a kept one): the same refusal
    bad = np.array(msa)
    bad[m - 1, np.nonzero(~mask)[0][11]] = stray
    src.input_begin(alphabet=b"ACGT", staging_bytes=staging_for(m, 64))
    for c0 in range(0, N, 64):
        src.input_scan_identity(c0, bad[:, c0:c0 + 64])
    assert refused(pkg, lambda: src.input_reduce(L)) == message
    assert src.device_bytes()[0] == 0
    # the second pass has its own check, for rows that changed between the passes: reported at the end, nothing is handed out
    src.input_begin(alphabet=b"ACGT", staging_bytes=staging_for(m, 64))
    for c0 in range(0, N, 64):
        src.input_scan_identity(c0, msa[:, c0:c0 + 64])
    src.input_reduce(L)
    for c0 in range(0, N, 64):
        src.input_columns_kept(c0, bad[:, c0:c0 + 64])
    assert refused(pkg, lambda: src.input_end_kept()) == message
    assert src.device_bytes()[0] == 0
    # src still works
    new = rmodel.feed(src, msa, 64, L, alphabet=b"ACGT")
    assert resident(new) == reference(pkg, msa, "supplied")[0]
    new.close()
    src.close()


# ---- 4. downstream on the new context
def test_downstream_outputs_are_the_chain_s(pkg, tmp_path):
    m, n, Ld = 40, 3000, 25
    msa = im.mosaic_with_identity(13, m, n, 250)             # (founder blocks of 250 source columns)
    rng = np.random.default_rng(4)
    queries = np.array(msa[rng.choice(m, size=5, replace=False)])
    mask = im.identity_mask(msa)
    for q in range(5):                                         # exception cells: a query differs from row 0 in identity columns
        queries[q, np.nonzero(mask)[0][rng.choice(int(mask.sum()), size=3 + q, replace=False)]] = ord("T") if q % 2 else ord("G")
    src = pkg.SegmentationContext(m, n, Ld)
    src.set_sequences(msa, staging_bytes=staging_for(m, 1024))
    a = src.without_identity_columns(Ld)
    src.close()
    src = pkg.SegmentationContext(m, n, Ld)
    b = src.set_sequences_without_identity_columns(msa, Ld, staging_bytes=staging_for(m, 1024))
    src.close()
    assert resident(a) == resident(b)
    files = {}
    for tag, ctx in (("a", a), ("b", b)):
        out = {}
        res = ctx.run()
        assert not res.short_path
        perm = ctx.join_bipartite()
        out["perm"] = perm.tobytes()
        names = ["founders", "identity", "segments-bip", "match-founders", "match-rows"]
        paths = {k: str(tmp_path / (tag + "-" + k)) for k in names}
        ctx.write_founders_restored(perm, paths["founders"])
        ctx.write_identity_columns(paths["identity"])
        out["segments_restored"] = ctx.segments_restored().tobytes()
        ctx.write_segments_restored(JOIN_BIPARTITE, paths["segments-bip"])
        out["match-founders-summary"] = {k: v for k, v in ctx.match_founders_restored(perm).items() if not k.startswith("ms")}
        ctx.write_match(paths["match-founders"])
        out["match-rows-summary"] = {k: v for k, v in ctx.match_rows_restored(queries, perm).items() if not k.startswith("ms")}
        ctx.write_match(paths["match-rows"])
        off, cols = ctx.match_exceptions()
        out["exceptions"] = (off.tobytes(), cols.tobytes())
        assert len(cols) >= 5
        for k in names:
            if os.path.exists(paths[k]):
                out[k] = open(paths[k], "rb").read()
        # another segment length on the same context, then a run
        ctx.set_segment_length(40)
        out["L40"] = outcome(pkg, ctx)
        files[tag] = out
    assert files["a"].keys() == files["b"].keys() and {"founders", "identity", "segments-bip", "match-founders", "match-rows"} <= files["a"].keys()
    for k in files["a"]:
        assert files["a"][k] == files["b"][k], k
    assert files["a"]["identity"] == im.mask_text(mask)
    a.close()
    b.close()


# ---- 5. call order and refusals
def test_call_order_refusals(pkg):
    m, width = 17, 64
    msa = case_rows(m, 4)
    want = reference(pkg, msa, (m, 4))
    src = pkg.SegmentationContext(m, N, L)
    chunk = lambda c0, w=width: msa[:, c0:c0 + w]
    # without a begin
    refused(pkg, lambda: src.input_scan_identity(0, chunk(0)))
    refused(pkg, lambda: src.input_reduce(L))
    refused(pkg, lambda: src.input_kept_columns(0, 64))
    refused(pkg, lambda: src.input_columns_kept(0, chunk(0)))
    refused(pkg, lambda: src.input_end_kept())
    src.input_begin(staging_bytes=staging_for(m, width))
    assert "fseq_input_reduce" in refused(pkg, lambda: src.input_reduce(L))               # before any scan
    assert "fseq_input_columns_kept" in refused(pkg, lambda: src.input_columns_kept(0, chunk(0)))
    assert "fseq_input_end_kept" in refused(pkg, lambda: src.input_end_kept())
    refused(pkg, lambda: src.input_scan_identity(64, chunk(64)))                          # out of order
    refused(pkg, lambda: src.input_scan_identity(0, chunk(0, 65)))                        # wider than a chunk
    src.input_scan_identity(0, chunk(0))
    assert "fseq_input_scan" in refused(pkg, lambda: src.input_scan(64, chunk(64)))       # the two scan entries do not mix
    refused(pkg, lambda: src.input_scan_identity(0, chunk(0)))                            # again
    refused(pkg, lambda: src.input_scan_identity(128, chunk(128)))                        # gapped
    message = refused(pkg, lambda: src.input_reduce(L))                                   # the scan is incomplete
    assert "fseq_input_reduce" in message and "64 of 300" in message
    refused(pkg, lambda: src.input_columns(0, chunk(0)))
    for c0 in range(64, N, width):
        src.input_scan_identity(c0, chunk(c0))
    refused(pkg, lambda: src.input_kept_columns(0, 64))                                   # before the reduce
    assert "fseq_input_reduce" in refused(pkg, lambda: src.input_columns_kept(0, chunk(0)))
    p = pkg.Params(0, 5, L, 0, 0, 0, 0)
    sm = pkg.IdentitySummary()
    assert src.L.fseq_input_reduce(src.h, C.byref(p), C.byref(sm)) == E_ARG               # params->n must be 0
    p = pkg.Params(m + 1, 0, L, 0, 0, 0, 0)
    assert src.L.fseq_input_reduce(src.h, C.byref(p), C.byref(sm)) == E_ARG               # params->m is 0 or the source's
    src.input_reduce(L)
    refused(pkg, lambda: src.input_reduce(L))                                             # twice
    refused(pkg, lambda: src.input_scan_identity(0, chunk(0)))
    assert "fseq_input_columns_kept" in refused(pkg, lambda: src.input_columns(0, chunk(0)))
    assert "fseq_input_end_kept" in refused(pkg, lambda: src.input_end())
    refused(pkg, lambda: src.run())
    refused(pkg, lambda: src.input_columns_kept(64, chunk(64)))                           # out of order
    src.input_columns_kept(0, chunk(0))
    message = refused(pkg, lambda: src.input_end_kept())                                  # before the columns are complete
    assert "fseq_input_end_kept" in message and "64 of 300" in message
    for c0 in range(64, N, width):
        src.input_columns_kept(c0, chunk(c0))
    refused(pkg, lambda: src.input_columns_kept(N - 1, chunk(N - 1)))
    new = src.input_end_kept()
    refused(pkg, lambda: src.input_end_kept())
    refused(pkg, lambda: src.run())                                                       # src is left without an input
    # every refusal left the passes where they were
    assert resident(new) == want[0] and outcome(pkg, new) == want[1]
    # the result is an identity-made context: no rows held out of it, no other input
    assert "fseq_create_without_identity_columns" in refused(pkg, lambda: new.without_rows([1], L), E_UNSUPPORTED)
    refused(pkg, lambda: new.input_begin())
    refused(pkg, lambda: new.set_sequences(np.zeros((new.m, new.n), dtype=np.uint8)))
    assert resident(new) == want[0]
    new.close()
    # after the ordinary scan the identity scan is refused
    src.input_begin(staging_bytes=staging_for(m, width))
    src.input_scan(0, chunk(0))
    assert "fseq_input_scan_identity" in refused(pkg, lambda: src.input_scan_identity(64, chunk(64)))
    refused(pkg, lambda: src.input_reduce(L))
    src.close()


def test_a_new_begin_in_the_middle_of_the_second_pass(pkg):
    m = 65
    msa = case_rows(m, 5)
    want = reference(pkg, msa, (m, 5))
    src = pkg.SegmentationContext(m, N, L)
    for again in range(2):
        src.input_begin(staging_bytes=staging_for(m, 64))
        for c0 in range(0, N, 64):
            src.input_scan_identity(c0, msa[:, c0:c0 + 64])
        src.input_reduce(L)
        src.input_columns_kept(0, msa[:, 0:64])
        src.input_columns_kept(64, msa[:, 64:128])
        assert src.device_bytes()[0] <= staging_for(m, 64) + 320      # the half-built context's buffers are its own ...
    src.set_sequences(msa)                                     # (... and another input on src destroys it, too)
    assert np.array_equal(src.get_sequences(), msa) and isinstance(outcome(pkg, src), tuple)
    new = rmodel.feed(src, msa, 64, L)
    assert resident(new) == want[0] and outcome(pkg, new) == want[1]
    new.close()
    src.close()                                                # (destroying src with nothing half-built)
    src = pkg.SegmentationContext(m, N, L)
    src.input_begin(staging_bytes=staging_for(m, 64))
    for c0 in range(0, N, 64):
        src.input_scan_identity(c0, msa[:, c0:c0 + 64])
    src.input_reduce(L)
    src.close()                                                # ... and with a half-built context, which goes with it


def test_sharded_source_is_unsupported(pkg):
    import torch
    m, n = 300, 5000
    rows = np.zeros((m, 64), dtype=np.uint8)
    b = pkg.SegmentationContext(m, n, 10)
    words = int(b.L.fseq_shard_xbuf_words(b.h, 2))
    xbuf = torch.zeros(words + 64, dtype=torch.int32, device="cuda:0")
    b.input_begin(staging_bytes=staging_for(m, 64))
    b.set_shard(0, 2, xbuf.data_ptr(), xbuf.numel(), lambda off, cnt, op: 0)      # (no input yet: the shard is accepted)
    refused(pkg, lambda: b.input_scan_identity(0, rows), E_UNSUPPORTED)
    refused(pkg, lambda: b.input_reduce(10), E_UNSUPPORTED)
    refused(pkg, lambda: b.input_kept_columns(0, 64), E_UNSUPPORTED)
    refused(pkg, lambda: b.input_columns_kept(0, rows), E_UNSUPPORTED)
    refused(pkg, lambda: b.input_end_kept(), E_UNSUPPORTED)
    refused(pkg, lambda: b.set_sequences_without_identity_columns(np.zeros((m, n), dtype=np.uint8), 10, staging_bytes=1 << 20), E_UNSUPPORTED)
    b.close()


# ---- 6. rows that are not one matrix
def test_rows_that_are_not_one_matrix(pkg):
    """separately allocated rows (no constant step between them) go up row by row, through the one-call entry"""
    m = 65
    msa = case_rows(m, 5)
    want = reference(pkg, msa, (m, 5))
    rows = [np.array(msa[r]) for r in range(m)]
    rows[3], rows[40] = np.array(msa[3]), np.array(msa[40])   # (out of allocation order)
    for staging in (staging_for(m, 64), staging_for(m, 48), staging_for(m, 320)):
        src = pkg.SegmentationContext(m, N, L)
        new = src.set_sequences_without_identity_columns(rows, L, staging_bytes=staging)
        assert src.device_bytes()[0] == 0
        src.close()
        assert resident(new) == want[0] and outcome(pkg, new) == want[1]
        new.close()
    # ... and a matrix, with every column an identity column: nothing is handed out, src is left without an input
    src = pkg.SegmentationContext(m, N, L)
    same = np.repeat(msa[0:1], m, axis=0)
    assert "every column is an identity column" in refused(pkg, lambda: src.set_sequences_without_identity_columns(same, L, staging_bytes=staging_for(m, 64)))
    assert src.device_bytes()[0] == 0
    src.close()


# ---- 7. memory
def test_device_memory_never_holds_the_source_s_packed_form(pkg):
    """Accounting through device_bytes(), a condition and not a measurement.  b = 6 bytes per source column is what include/fseq.h
    documents for n >= 1,024: the mask and the reference row count in both peaks (src hands them over: 4), the accumulators of a
    chunk (at most 1) and the constants (tables, the tile counts of the kept list's scan)."""
    m, n, width, b = 257, 4096, 64, 6
    ident = np.ones(n, dtype=bool)
    ident[np.random.default_rng(8).choice(n, size=410, replace=False)] = False
    msa = rmodel.planted(8, m, n, b"ACGT", ident)
    ld, kept, staging = 80, 410, staging_for(m, width)
    src = pkg.SegmentationContext(m, n, L)
    assert src.device_bytes() == (0, 0)
    src.input_begin(staging_bytes=staging)
    for c0 in range(0, n, width):
        src.input_scan_identity(c0, msa[:, c0:c0 + width])
    src.input_reduce(L)
    for c0 in range(0, n, width):
        if src.input_kept_columns(c0, width):
            src.input_columns_kept(c0, msa[:, c0:c0 + width])
        else:
            src.input_columns_kept(c0, width)
    new = src.input_end_kept()
    peak_src, peak_new = src.device_bytes()[1], new.device_bytes()[1]
    bound = staging + ld * kept + 16 + 4 * kept + b * n
    print("peaks: src %d + new %d = %d bytes; bound %d; the packed source alone %d" % (peak_src, peak_new, peak_src + peak_new, bound, ld * n))
    assert new.packed_columns()[0].shape == (kept, ld)
    assert peak_src + peak_new <= bound
    assert bound < ld * n == 327680
    assert src.device_bytes()[0] == 0 and new.device_bytes()[0] == ld * kept + 16 + 4 * kept + 2 * n
    src.close()
    # the existing path allocates that much for the same input
    old = pkg.SegmentationContext(m, n, L)
    old.set_sequences(msa, staging_bytes=staging)
    assert old.device_bytes()[1] >= ld * n
    chain = old.without_identity_columns(L)
    assert resident(chain) == resident(new)
    for c in (old, chain, new):
        c.close()


# ---- 8. the front end
def write_list(tmp_path, msa):
    src = tmp_path / "in"
    src.mkdir()
    names = []
    for i, row in enumerate(msa):
        (src / ("s%02d" % i)).write_bytes(row.tobytes())
        names.append(str(src / ("s%02d" % i)))
    (tmp_path / "list.txt").write_text("\n".join(names) + "\n")
    return str(tmp_path / "list.txt"), names


def run_cli(cli, tmp_path, tag, args, outputs):
    out = tmp_path / tag
    out.mkdir()
    cmd = [cli] + args + ["--output-founders", str(out / "founders")]
    for name in outputs:
        cmd += ["--output-" + name, str(out / name)]
    r = subprocess.run(cmd, capture_output=True, timeout=300)
    assert r.returncode == 0, r.stderr.decode()
    return {name: (out / name).read_bytes() for name in ["founders"] + [o for o in outputs]}, r.stderr


@pytest.fixture(scope="module")
def front_end_input(tmp_path_factory):
    m, n = 20, 100000                                          # 1 MiB of upload memory: chunks of 26,176 columns, 4 of them
    msa = np.array(im.mosaic_with_identity(11, m, n, 250))
    msa[:, 30000:85000] = msa[0, 30000:85000]                # the chunk [52352, 78528) holds no kept column: the second pass does not read it
    queries = np.array(msa[[3, 7]])
    queries[0, 60000] = ord("T") if msa[0, 60000] != ord("T") else ord("G")
    tmp = tmp_path_factory.mktemp("reduced")
    lst, names = write_list(tmp, msa)
    q = tmp / "queries"
    q.mkdir()
    for i, row in enumerate(queries):
        (q / ("q%d" % i)).write_bytes(row.tobytes())
    (tmp / "queries.txt").write_text("\n".join(str(q / ("q%d" % i)) for i in range(2)) + "\n")
    return tmp, lst, names, msa, str(tmp / "queries.txt")


@pytest.mark.parametrize("joining", ["greedy", "bipartite-matching", "random"])
def test_front_end_writes_the_same_files(build, front_end_input, joining):
    cli = build.build_cli()
    tmp, lst, _, msa, queries = front_end_input
    base = ["--input", lst, "--segment-length-bound", "20", "--segment-joining", joining, "--random-seed", "7", "--remove-identity-columns", "--upload-memory=1",
            "--match-sequences", queries]
    outputs = ["identity-columns", "restored-segments", "restored-matches", "sequence-restored-matches"]
    want, _ = run_cli(cli, tmp, joining + "-resident", base, outputs)
    got, err = run_cli(cli, tmp, joining + "-reduced", base + ["--reduce-on-upload"], outputs)
    mask = im.identity_mask(msa)
    assert ("Removed %d of %d columns in which all sequences agree." % (mask.sum(), msa.shape[1])).encode() in err
    assert want["identity-columns"] == im.mask_text(mask) and len(want["founders"]) > msa.shape[1]
    for name in want:
        assert got[name] == want[name], name


def test_front_end_against_the_chain_of_tools(build, front_end_input, tmp_path):
    """founder_sequences --remove-identity-columns --upload-memory --reduce-on-upload against remove_identity_columns ->
    founder_sequences -> insert_identity_columns -r <row 0's file> with the project's own host tools"""
    cli = build.build_cli()
    tools = dict(zip(build.AUX_TOOLS, build.build_aux()))
    _, lst, names, msa, _ = front_end_input
    common = ["--segment-length-bound", "20", "--segment-joining", "greedy"]
    r = subprocess.run([cli, "--input", lst, "--remove-identity-columns", "--upload-memory=1", "--reduce-on-upload", "--output-identity-columns=" + str(tmp_path / "M"),
                        "--output-founders=" + str(tmp_path / "F"), "--output-segments=" + str(tmp_path / "E")] + common, capture_output=True, timeout=300)
    assert r.returncode == 0, r.stderr
    red = tmp_path / "reduced"
    red.mkdir()
    r = subprocess.run([tools["remove_identity_columns"], "--input", lst], capture_output=True, cwd=str(red), timeout=300)
    assert r.returncode == 0, r.stderr
    (tmp_path / "M2").write_bytes(r.stdout)
    (tmp_path / "list2.txt").write_text("\n".join(str(red / os.path.basename(p)) for p in names) + "\n")
    r = subprocess.run([cli, "--input", str(tmp_path / "list2.txt"), "--output-founders=" + str(tmp_path / "F2"), "--output-segments=" + str(tmp_path / "E2")] + common,
                       capture_output=True, timeout=300)
    assert r.returncode == 0, r.stderr
    back = tmp_path / "back"
    back.mkdir()
    r = subprocess.run([tools["insert_identity_columns"], "--input", str(tmp_path / "F2"), "--reference", names[0], "--identity-columns", str(tmp_path / "M2")],
                       capture_output=True, cwd=str(back), timeout=300)
    assert r.returncode == 0, r.stderr
    K = len(os.listdir(str(back)))
    chain = b"".join((back / str(i + 1)).read_bytes() + b"\n" for i in range(K))
    assert (tmp_path / "M").read_bytes() == (tmp_path / "M2").read_bytes() == im.mask_text(im.identity_mask(msa))
    assert (tmp_path / "F").read_bytes() == chain and K >= 2
    assert (tmp_path / "E").read_bytes() == (tmp_path / "E2").read_bytes()


def test_front_end_every_column_an_identity_column(build, tmp_path):
    cli = build.build_cli()
    lst, _ = write_list(tmp_path, np.repeat(np.frombuffer(b"ACGTACGTAC" * 10, dtype=np.uint8)[None, :], 3, axis=0))
    r = subprocess.run([cli, "--input", lst, "--segment-length-bound", "2", "--remove-identity-columns", "--upload-memory=1", "--reduce-on-upload",
                        "--output-founders=" + str(tmp_path / "F")], capture_output=True, timeout=120)
    assert r.returncode != 0 and b"every column is an identity column" in r.stderr
