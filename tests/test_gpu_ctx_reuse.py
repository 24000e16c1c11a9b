"""One context, many inputs and modes: a SegmentationContext that is given another alignment (through any of the input
setters), or another setting, and run again must compute what a fresh context computes -- bit for bit against the CPU
oracle: the DP arrays, the traceback, the merged segments and every boundary (a, d) -- and must not hand out what it held
for the alignment before.

What a new input has to reset is whatever the library decides only where it allocates a buffer (the form, packing and
spacing of the stride states, the rebase of the streamed workspace, everything sized by the block count, the plan of the
representatives): fseq::take_new_input (csrc/fseq_api.hip) drops the work buffers, the result and the last match.  Every
sequence here uses inputs of different alphabets (2-, 4- and 8-bit columns; one and several digit passes; staged and
unstaged streamed columns) with distinct seeds, and asserts that consecutive inputs have different merged segments in the
oracle, so no step passes on what the step before left behind."""
import importlib

import numpy as np
import pytest

import fso
from test_gpu_parity import check_long

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def pkg():
    return importlib.import_module("founder-sequences_amd")


def mosaic(sigma, m, n, seed, spread=True):
    """test_gpu_parity.test_wide_and_odd_alphabets' input: a mosaic of five founders plus noise over `sigma` symbols, the
    bytes spread over the byte range (spread=False: the dense codes 0 .. sigma - 1 themselves).  The noise falls with the row
    count (about six changed cells per column at most), so that the segments of the tall shapes stay small."""
    rng = np.random.default_rng(seed)
    brec = max(25, n // 10)
    founders = rng.integers(0, sigma, size=(5, n))
    pick = rng.integers(0, 5, size=(m, (n + brec - 1) // brec))
    msa = np.empty((m, n), dtype=np.uint8)
    for b in range(pick.shape[1]):
        msa[:, b * brec:(b + 1) * brec] = founders[pick[:, b], b * brec:(b + 1) * brec]
    noise = rng.random((m, n)) < min(2e-3, 6.0 / m)
    msa[noise] = rng.integers(0, sigma, size=int(noise.sum()))
    if spread and sigma < 256:
        msa = (msa.astype(np.uint16) * (255 // sigma)).astype(np.uint8)
    return msa


SYNTH = (22, 8, 200, 2e-3, 0)            # seed, founders, block, mutation rate, kind: test_gpu_parity's case of 300 rows


def give(pkg, ctx, step, seed):
    """Hands the context the input of one step; returns the alignment as the oracle is to see it.
    step: (setter, sigma) with setter one of matrix, rows, chunked, device, packed, synthetic."""
    import torch
    how, sigma = step
    m, n = ctx.m, ctx.n
    if how == "synthetic":
        s, K, brec, mu, kind = SYNTH
        ctx.generate_synthetic(s + seed, K, brec, mu, kind)
        return fso.synth_msa(fso.synth_spec(s + seed, K, brec, mu, kind), m, n)
    if how in ("device", "packed"):
        codes = mosaic(sigma, m, n, seed, spread=False)
        bits = 8 if how == "device" else 2 if sigma <= 4 else 4
        cols, ld = pkg.pack_columns(codes, bits)
        dev = torch.from_numpy(cols).to("cuda")
        if how == "device":
            ctx.set_device_columns(dev.data_ptr(), ld, sigma, keepalive=dev)
        else:
            ctx.set_device_columns_packed(dev.data_ptr(), ld, sigma, bits, keepalive=dev)
        return codes
    msa = mosaic(sigma, m, n, seed)
    if how == "matrix":
        ctx.set_sequences(msa)
    elif how == "rows":
        ctx._check(ctx.L.fseq_set_rows(ctx.h, ctx._row_pointers(msa)))
    elif how == "chunked":
        ctx.set_sequences(msa, staging_bytes=max(1 << 16, 64 * m))
    else:
        raise ValueError(how)
    return msa


def fresh_run(pkg, msa, L, knobs=(), **kw):
    ctx = pkg.SegmentationContext(msa.shape[0], msa.shape[1], L, **kw)
    for k in knobs:
        ctx.set_tuning(k)
    ctx.set_sequences(msa)
    ctx.run()
    return ctx


def run_and_compare(pkg, ctx, msa, L, before, knobs=(), join=True, **kw):
    """Runs the context on the input it was just given: the oracle bit for bit, the greedy joiner's permutations equal to a
    fresh context's.  before: the oracle's merged segments of the step in front (they must differ).  Returns this step's."""
    ref = fso.segment_long(msa, L, keep_dp=True, threads=4)
    assert ref["status"] == 0 and len(ref["reduced"]) >= 2
    red = ref["reduced"]
    if before is not None:
        assert len(before) != len(red) or any(not np.array_equal(before[f], red[f]) for f in ("lb", "rb", "segment_size")), "consecutive steps must differ"
    ctx.run()
    check_long(ctx, ref, msa.shape[1], L)
    if join:
        fresh = fresh_run(pkg, msa, L, knobs, **kw)
        assert np.array_equal(ctx.join_greedy(), fresh.join_greedy())
        fresh.close()
    return red


def run_sequence(pkg, m, n, L, steps, knobs=(), **kw):
    ctx = pkg.SegmentationContext(m, n, L, **kw)
    for k in knobs:
        ctx.set_tuning(k)
    before = None
    for i, step in enumerate(steps):
        msa = give(pkg, ctx, step, 7919 * (i + 1) + m)
        before = run_and_compare(pkg, ctx, msa, L, before, knobs, **kw)
    ctx.close()


# ---- input transitions

def test_lds_resident_context_takes_every_kind_of_input(pkg):
    """32-bit LDS state.  2-, 4- and 8-bit columns and back, one, two and three digit passes, every input setter: the geometry
    (the block length is the library's choice here: it is refitted to the kernel's occupancy, which follows the alphabet)
    and every buffer sized by it change from step to step."""
    steps = [("matrix", 4), ("matrix", 16), ("matrix", 40), ("matrix", 2), ("device", 7), ("packed", 4), ("synthetic", 4),
             ("chunked", 16), ("rows", 4)]
    run_sequence(pkg, 300, 2000, 25, steps)


def test_16_bit_lds_state_across_alphabets(pkg):
    """m = 9,000 (16-bit LDS state): the stride states are 16 columns apart for one digit pass a column and 8 for two."""
    run_sequence(pkg, 9000, 1200, 40, [("matrix", 4), ("matrix", 16), ("matrix", 4)], block_len=128)


@pytest.mark.parametrize("knobs", [(), ("FSEQ_NO_REDUCED",)], ids=["representatives", "all_rows"])
def test_streamed_context_across_alphabets(pkg, knobs):
    """m = 12,000: streamed rows, every column width staged.  On all rows (FSEQ_NO_REDUCED) phase C drops stride states in id form
    and pass 2 replays them; by default the blocks run on their representatives, whose buffers follow the packing too."""
    run_sequence(pkg, 12000, 500, 20, [("matrix", 4), ("matrix", 16), ("matrix", 200), ("matrix", 4)], knobs, block_len=64)


# m = 130,000: the smallest round row count whose 8-bit column (130,000 bytes + 32 KiB of tile staging + the kernel's scratch) is
# beyond the 160 KiB of LDS (from 125,137 rows on) while its 4- and 2-bit columns are staged: the streamed phase C has its
# second form, and stride states in id form, for up to 16 symbols only
UNSTAGED_M = 130000


@pytest.mark.parametrize("knobs", [(), ("FSEQ_NO_REDUCED",)], ids=["representatives", "all_rows"])
@pytest.mark.parametrize("order", [(4, 40), (40, 4), (4, 16, 40, 4)], ids=lambda o: "-".join(map(str, o)))
def test_streamed_context_between_staged_and_unstaged_columns(pkg, order, knobs):
    """From an alphabet whose column is staged to one whose column is not, and back: the second form of phase C, the id form of
    the stride states, their packing and the block start states in id form come and go with the input."""
    run_sequence(pkg, UNSTAGED_M, 160, 10, [("matrix", s) for s in order], knobs)


@pytest.mark.parametrize("m", [500, 12000])
def test_short_path_context_takes_another_input(pkg, m):
    """n < 2L: one sweep; the runs of equal rows against fresh contexts' (LDS-resident and streamed rows)."""
    n, L = 60, 40
    ctx = pkg.SegmentationContext(m, n, L)
    seen = []
    for i, sigma in enumerate((4, 40, 4)):
        rng = np.random.default_rng(100 * i + m)
        msa = (rng.integers(0, sigma, size=(9 + 4 * i, n))[rng.integers(0, 9 + 4 * i, size=m)] * (255 // sigma)).astype(np.uint8)
        ctx.set_sequences(msa)
        ctx.run()
        fresh = fresh_run(pkg, msa, L)
        assert ctx.result.short_path == 1 and ctx.result.max_segment_size == fresh.result.max_segment_size == len({bytes(r) for r in msa})
        for x, y in zip(ctx.short_path_runs(), fresh.short_path_runs()):
            assert np.array_equal(x, y)
        seen.append(ctx.result.max_segment_size)
        fresh.close()
    assert len(set(seen)) == 3
    ctx.close()


# ---- mode transitions

def test_list_budget_set_and_cleared_between_runs_and_inputs(pkg):
    """test_gpu_list_window's first shape: every list held, then windows, then every list held again on one context; then
    another input while the budget is set."""
    m, n, L, K, brec, mu, seed, kind, B = 300, 5000, 10, 8, 200, 2e-3, 28, 0, 16
    msa = fso.synth_msa(fso.synth_spec(seed, K, brec, mu, kind), m, n)
    ref = fso.segment_long(msa, L, keep_dp=True, threads=4)
    ctx = pkg.SegmentationContext(m, n, L, block_len=B)
    ctx.set_sequences(msa)
    ctx.run()
    check_long(ctx, ref, n, L)
    lw = ctx.list_windows()
    assert lw["windows"] == 1
    budget = lw["bytes_held"] // 5
    ctx.set_list_memory(budget)
    ctx.run()
    w = ctx.list_windows()
    assert w["windows"] >= 3 and 0 < w["bytes_held"] <= budget, w
    check_long(ctx, ref, n, L)
    ctx.set_list_memory(0)
    ctx.run()
    assert ctx.list_windows()["windows"] == 1
    check_long(ctx, ref, n, L)
    ctx.set_list_memory(budget)
    other = mosaic(16, m, n, 5)
    ctx.set_sequences(other)
    red = run_and_compare(pkg, ctx, other, L, ref["reduced"], block_len=B)
    assert len(red) and ctx.list_windows()["windows"] >= 3
    ctx.close()


def test_knobs_change_on_a_live_streamed_context(pkg):
    """set_tuning between runs of one input: the form of the stride states (ids, divergences), the form of phase C and whether the
    blocks run on their representatives change under buffers of the run before."""
    m, n, L, B = 12000, 500, 20, 64
    msa = fso.synth_msa(fso.synth_spec(41, 12, 120, 3e-4, 0), m, n)
    ref = fso.segment_long(msa, L, keep_dp=True, threads=4)
    ctx = pkg.SegmentationContext(m, n, L, block_len=B)
    ctx.set_sequences(msa)
    ctx.run()
    check_long(ctx, ref, n, L)
    for knobs in (("FSEQ_SS_ABSOLUTE",), ("FSEQ_STREAM_PLAIN_SCAN",), ("FSEQ_NO_REDUCED",), ("FSEQ_NO_REDUCED", "FSEQ_SS_ABSOLUTE"), ("FSEQ_REDUCED_ALWAYS",), ()):
        for k in knobs:
            ctx.set_tuning(k)
        with pytest.raises(pkg.FseqError):                  # (a knob drops the result as a new input does)
            ctx.boundary_state(0)
        ctx.run()
        check_long(ctx, ref, n, L)
        for k in knobs:
            ctx.set_tuning(k, None)
    ctx.close()


@pytest.mark.parametrize("knobs", [("FSEQ_SS_UNPACKED",), ("FSEQ_SS_UNPACKED", "FSEQ_STREAM_PLAIN_SCAN")], ids=["second_form", "first_form"])
@pytest.mark.parametrize("all_rows", [False, True], ids=["representatives", "all_rows"])
@pytest.mark.parametrize("m,n,L,K,brec,mu,seed,B", [(12000, 500, 20, 12, 120, 3e-4, 41, 64), (70000, 200, 12, 20, 64, 1e-4, 43, 40)])
def test_unpacked_stride_states(pkg, m, n, L, K, brec, mu, seed, B, all_rows, knobs):
    """FSEQ_SS_UNPACKED: the streamed stride states as two words per row (and no id form), written by the second form of phase C
    and -- with FSEQ_STREAM_PLAIN_SCAN -- by the first, read by pass 2 on the first form's tile step.  The stride states are
    phase C's on all rows (FSEQ_NO_REDUCED); the default run takes the representatives and must not mind the knob."""
    knobs = knobs + (("FSEQ_NO_REDUCED",) if all_rows else ())
    msa = fso.synth_msa(fso.synth_spec(seed, K, brec, mu, 0), m, n)
    ref = fso.segment_long(msa, L, keep_dp=True, threads=4)
    ctx = fresh_run(pkg, msa, L, knobs, block_len=B)
    check_long(ctx, ref, n, L)
    ctx.close()


# ---- what a context holds for the input before

SETTERS = [("matrix", 16), ("rows", 4), ("chunked", 16), ("device", 7), ("packed", 4), ("synthetic", 4)]


def refused(pkg, call, *words):
    with pytest.raises(pkg.FseqError) as ei:
        call()
    assert ei.value.code == pkg.FSEQ_E_ARG
    assert all(w in str(ei.value) for w in words), str(ei.value)


@pytest.mark.parametrize("step", SETTERS, ids=[s[0] for s in SETTERS])
def test_new_input_drops_the_result_and_the_match(pkg, tmp_path, step):
    m, n, L = 300, 2000, 25
    first = mosaic(4, m, n, 1)
    ctx = pkg.SegmentationContext(m, n, L)
    ctx.set_sequences(first)
    ctx.run()
    perm = ctx.join_greedy()
    out = str(tmp_path / "founders.txt")
    ctx.write_founders_device(perm, out)
    founders = np.array([np.frombuffer(line, dtype=np.uint8) for line in open(out, "rb").read().split(b"\n")[:-1]])
    assert founders.shape == (ctx.result.max_segment_size, n)
    assert ctx.match_founders(founders=founders, min_segment_length=L)["pieces"] >= m
    pieces, _ = ctx.match_pieces()
    assert len(pieces) >= m
    msa = give(pkg, ctx, step, 2)
    # the result of the alignment before is gone, and fseq_last_error says so
    no_result = ("no result", "fseq_run_segmentation")
    refused(pkg, ctx.traceback, *no_result)
    refused(pkg, ctx.reduced_traceback, *no_result)
    refused(pkg, lambda: ctx.boundary_state(0), *no_result)
    refused(pkg, ctx.join_greedy, *no_result)
    refused(pkg, ctx.join_bipartite, *no_result)
    refused(pkg, ctx.join_random, *no_result)
    refused(pkg, lambda: ctx.write_founders_device(perm, str(tmp_path / "stale.txt")), *no_result)
    refused(pkg, lambda: ctx.match_founders(permutations=perm), "finished long-path run")
    # ... and so is the match
    refused(pkg, ctx.match_pieces, "no match")
    refused(pkg, lambda: ctx.write_match(str(tmp_path / "match.txt")), "no match")
    # the context serves the new alignment
    run_and_compare(pkg, ctx, msa, L, None)
    ctx.close()


def test_context_without_identity_columns_refuses_another_input(pkg, tmp_path):
    """Its identity relation (mask, kept columns, row 0 of its source) belongs to the columns it was made from: every input
    setter refuses, nothing it holds changes, and the restored outputs stay those of its own alignment."""
    m, n, L = 300, 2400, 25
    msa = mosaic(16, m, n, 3)
    msa[:, ::6] = msa[0, ::6]                                    # every sixth column an identity column
    src = pkg.SegmentationContext(m, n, L)
    src.set_sequences(msa)
    red = src.without_identity_columns(L)
    src.close()
    assert red.n == n - n // 6
    red.run()
    perm = red.join_greedy()
    a, b = str(tmp_path / "a.txt"), str(tmp_path / "b.txt")
    red.write_founders_restored(perm, a)
    summary = red.match_founders_restored(perm, L)
    for step in SETTERS:
        refused(pkg, lambda: give(pkg, red, step, 4), "takes no other input")
    assert np.array_equal(red.get_sequences(), msa[:, np.arange(n) % 6 != 0])
    assert np.array_equal(red.join_greedy(), perm)
    red.write_founders_restored(perm, b)
    assert open(a, "rb").read() == open(b, "rb").read()
    again = red.match_founders_restored(perm, L)
    assert {k: v for k, v in again.items() if k != "ms_device"} == {k: v for k, v in summary.items() if k != "ms_device"}
    red.close()


@pytest.mark.parametrize("m,n,L,kw", [(300, 2000, 25, {}), (12000, 500, 20, {"block_len": 64})])
def test_cycling_inputs_does_not_grow_the_context(pkg, m, n, L, kw):
    """Two inputs of different widths, three times round: what the context holds after the third round is what it held after
    the second (device_bytes: the context's own accounting, which fseq_destroy checks against its allocations)."""
    inputs = [mosaic(4, m, n, 11), mosaic(40, m, n, 12)]
    refs = [fso.segment_long(x, L, keep_dp=True, threads=4) for x in inputs]
    ctx = pkg.SegmentationContext(m, n, L, **kw)
    held = []
    for cycle in range(3):
        for msa, ref in zip(inputs, refs):
            ctx.set_sequences(msa)
            ctx.run()
            ctx.join_greedy()
            if cycle == 2:
                check_long(ctx, ref, n, L)
        held.append(ctx.device_bytes()[0])
    assert held[2] == held[1], held
    ctx.close()
