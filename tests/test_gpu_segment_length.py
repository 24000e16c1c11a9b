"""The segmentation path along the segment-length bound L, bit for bit against the CPU oracle (tests/segment_length_cases.py
holds the inputs, tests/test_segment_length_cases.py what the oracle makes of them).

L is not a passive parameter.  What each group of cases reaches:
  * every L in 1..130, at ~14 L columns and at n = 2 L + j: the three forms of the DP schedule (rounds of L cells below 56,
    of 56 cells up to 95, the pipelined rounds of 48 cells with their drain round from 96 on) with both sides of 55 | 56 and
    95 | 96, every number of compute waves that hold cells (L = 14 | 15, 28 | 29, 42 | 43), and every tail of the schedule:
    last rounds of 1, 2, RL - 1 and RL cells;
  * L around 512, 2,048, 4,096, 8,192, 12,288, 16,384 and 65,536 at 6 L columns: the serial DP kernel whose cells read
    entries <= end - 2 L -- from L > 4,096 on none of them is in the LDS ring of 4,096 entries and every level of the sparse
    table comes from memory --, traceback windows of 8,192 entries in which a hop covers from a 16th of the window to more
    than the whole window, block borders of which L spans 5 to 655 (blocks of 100 columns), blocks in front of column L --
    each on the blocks' representative rows (forced: with 48 rows the library's own plan declines them, see run()) and on all
    rows;
  * the same L at 30 L columns on the library's own speculative plan (chunks of 8 L entries, tail windows of 4 L), and
    L = 16,385 / 65,537 on chunks of a third of the rounds;
  * L in the thousands on 2,504, 10,000 (sigma = 16) and 12,000 rows, on the representatives and on all rows;
  * list windows narrower than L;
  * sharded runs whose ranks hold fewer than two segment lengths of columns, and shapes whose leading ranks lie in front
    of column L.

Every run is held to the oracle as test_gpu_parity.check_long does (check_dp = True): the DP array where cells write it,
the traceback, the merged segments and every boundary state."""
import importlib
import re

import pytest

import fso
import segment_length_cases as slc
from test_gpu_list_window import same_results
from test_gpu_parity import check_long, run_gpu
from test_gpu_shard import check_against_oracle, run_world

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def pkg():
    return importlib.import_module("founder-sequences_amd")


_refs = {}


def oracle(case):
    """(alignment, oracle result with its DP array) of a case: computed once, shared by every form, never written to."""
    if case not in _refs:
        msa = slc.make(case)
        _refs[case] = (msa, fso.segment_long(msa, case[2], keep_dp=True, threads=8))
    return _refs[case]


def run(pkg, msa, L, block_len=0, rows=None, tuning=(), **kw):
    """rows: None -- the library's own choice between a block's representative rows and all rows; "representatives" --
    FSEQ_REDUCED_ALWAYS on the context: the reduced phase C and pass 2 wherever a block has fewer representatives than rows
    (by itself the library takes them only where they are below a fifth of the rows over all blocks, red_plan: not at 48
    rows of five founders, and not where L is a fifth of the columns); "all" -- FSEQ_NO_REDUCED."""
    m, n = msa.shape
    ctx = pkg.SegmentationContext(m, n, L, block_len=block_len, **kw)
    if rows is not None:
        ctx.set_tuning({"representatives": "FSEQ_REDUCED_ALWAYS", "all": "FSEQ_NO_REDUCED"}[rows], "1")
    for name, value in tuning:
        ctx.set_tuning(name, value)
    ctx.set_sequences(msa)
    try:
        ctx.run()
    except pkg.NoReduction:
        pass
    return ctx


def check(ctx, ref, n, L):
    # (a short traceback must not pass by both sides being compared over a truncated length)
    assert len(ctx.traceback()) == len(ref["traceback"]) == ctx.result.dp_segment_count
    assert ctx.result.segment_count == len(ref["reduced"])
    check_long(ctx, ref, n, L, check_dp=True)


def check_rows(ctx, rows, m):
    """The run was on the rows it was asked to be on."""
    t = ctx.timings()
    if rows == "representatives":
        assert t["reduced_blocks"] > 0 and 0 < t["reduced_rows_mean"] < m, t
    else:
        assert t["reduced_blocks"] == 0, t
    return t


@pytest.mark.parametrize("L0", range(1, 131, 10))
def test_every_small_segment_length(pkg, L0):
    """Ten consecutive L, each at ~14 L columns and at n = 2 L + j, on the library's own blocks; L mod 10 == 6 (56 and 96
    among them) also on blocks of 33 columns."""
    for L in range(L0, L0 + 10):
        for case in (slc.small_long(L), slc.small_short(L)):
            msa, ref = oracle(case)
            n = msa.shape[1]
            for B in (0, 33) if L % 10 == 6 else (0,):
                check(run(pkg, msa, L, block_len=B), ref, n, L)


@pytest.mark.parametrize("L", slc.LARGE_L)
def test_large_segment_lengths(pkg, L):
    """6 L columns: the serial DP kernel (dp_chunks == 0), on the library's own blocks and on blocks of 100 columns (L spans 5
    to 655 of them), each on the blocks' representatives (reduced_blocks > 0) and on all rows of every block."""
    msa, ref = oracle(slc.large(L))
    m, n = msa.shape
    for B in (0, 100):
        for rows in ("representatives", "all"):
            ctx = run(pkg, msa, L, block_len=B, rows=rows)
            t = check_rows(ctx, rows, m)
            print("L = %d, blocks of %d columns, %s: %d of %d blocks reduced, %d rows on average" % (L, t["block_len"], rows, t["reduced_blocks"], t["n_blocks"], t["reduced_rows_mean"]))
            assert t["dp_chunks"] == 0, t
            if B:
                assert t["block_len"] == B and t["n_blocks"] == (n + B - 1) // B, t
            check(ctx, ref, n, L)


SPECULATIVE = [("own_plan", L) for L in slc.SPECULATIVE_L] + [("forced_rounds", L) for L in slc.FORCED_SPECULATIVE_L]


@pytest.mark.parametrize("plan,L", SPECULATIVE)
def test_large_segment_lengths_on_the_speculative_dp(pkg, monkeypatch, plan, L):
    """30 L columns on the library's own plan (at least three chunks of 8 L entries); 6 L columns at L = 16,385 and 65,537
    with chunks of a third of the regular rounds.  The lists start out poisoned."""
    monkeypatch.setenv("FSEQ_POISON_LISTS", "1")
    if plan == "own_plan":
        case, tuning, least = slc.speculative(L), (), 3
    else:
        case = slc.large(L)
        tuning, least = (("FSEQ_DP_SPEC_ROUNDS", str(slc.forced_spec_rounds(L, case[1]))),), 2
    msa, ref = oracle(case)
    n = msa.shape[1]
    ctx = run(pkg, msa, L, tuning=tuning)
    t = ctx.timings()
    assert t["dp_chunks"] >= least, t
    check(ctx, ref, n, L)


@pytest.mark.parametrize("name", list(slc.ROW_CASES))
def test_large_segment_length_on_larger_row_counts(pkg, name):
    """L in the thousands on 2,504 rows, on 10,000 rows of sigma = 16 (4 bits per stored symbol) and on 12,000 rows: on the
    blocks' representatives (forced as in test_large_segment_lengths: a fifth of the blocks start in front of column L, where
    every row that differs anywhere before is a representative, and the library's own plan declines) and on all rows.  (The
    alignment and the oracle's result are this test's own: nothing of ~200 MB stays behind.)"""
    case = slc.ROW_CASES[name]
    m, n, L = case[:3]
    msa = slc.make(case)
    ref = fso.segment_long(msa, L, keep_dp=True, threads=8)
    for rows in ("representatives", "all"):
        ctx = run(pkg, msa, L, rows=rows)
        t = check_rows(ctx, rows, m)
        bits = ctx.packed_columns(0, 1)[1]
        print("%s, %s: %d of %d blocks of %d columns reduced, %d rows on average, %d bits per symbol" % (name, rows, t["reduced_blocks"], t["n_blocks"], t["block_len"], t["reduced_rows_mean"], bits))
        assert bits == slc.ROW_CASE_BITS[name]
        check(ctx, ref, n, L)


def budget_of(per_column, columns):
    return per_column * columns + 2048                   # (2,048 bytes of padding behind the last list)


def test_windowed_lists_with_a_large_segment_length(pkg):
    """L = 4,097 with a list budget that leaves a window fewer than L columns: no window holds the lists of one segment.

    The drain round and the final cell run with the last window and read the lists from column n - L on, so the last window
    needs a halo that reaches back there: window and halo together are never fewer than L columns, and a budget below L
    columns of lists holds no window (asserted: FSEQ_E_OOM).  A budget of L + L / 10 columns settles on windows of ~2,800
    columns with a halo of ~1,700; at L + 100 columns the only shapes that fit have a short halo because the last window
    starts just behind column n - L (the planner used to refuse that budget: it raised the halo without trying other
    widths)."""
    L = 4097
    msa, ref = oracle(slc.large(L))
    m, n = msa.shape
    full = run_gpu(pkg, msa, L)
    lw = full.list_windows()
    assert lw["windows"] == 1 and lw["merge_windows"] == 0 and lw["columns_per_window"] == n
    per_column = lw["bytes_held"] // n
    for columns in (L + L // 10, L + 100):
        budget = budget_of(per_column, columns)
        ctx = run(pkg, msa, L, list_memory=budget)
        w = ctx.list_windows()
        print("budget of %d columns: %s" % (columns, w))
        assert w["columns_per_window"] < L and w["windows"] >= 3 and 0 < w["bytes_held"] <= budget, w
        assert w["merge_windows"] >= 1, w
        check(ctx, ref, n, L)
        same_results(ctx, full)


def test_every_list_budget_that_holds_a_window_runs(pkg):
    """The window planner over budgets of L - 100 .. L + 420 columns of lists at L = 4,097 (n = 24,621, blocks of 25 columns),
    every 13th: a budget is either refused with the least budget that holds a window in the message -- the same figure
    whatever the budget, and a budget of exactly that many bytes runs, one byte less does not -- or it runs, in three or
    more windows, with the oracle's result.  (The halo of the last window is its start minus n - L, no monotonic function
    of the window width: the planner used to refuse every budget of L + 54 .. L + 150 columns, L + 54 being the least.)"""
    L = 4097
    msa, ref = oracle(slc.large(L))
    m, n = msa.shape
    full = run_gpu(pkg, msa, L)
    per_column = full.list_windows()["bytes_held"] // n
    ctx = pkg.SegmentationContext(m, n, L)
    ctx.set_sequences(msa)
    least, ran = set(), []
    for columns in range(L - 100, L + 420, 13):
        budget = budget_of(per_column, columns)
        ctx.set_list_memory(budget)
        try:
            ctx.run()
        except pkg.FseqError as e:
            assert e.code == pkg.FSEQ_E_OOM and "list memory budget of %d bytes holds no window" % budget in str(e), (columns, e)
            needs = int(re.search(r"needs (\d+) bytes", str(e)).group(1))
            assert needs > budget, (columns, e)
            least.add(needs)
            assert not ran, (columns, ran)                # (a wider budget holds whatever a narrower one does)
            continue
        w = ctx.list_windows()
        assert w["windows"] >= 3 and w["columns_per_window"] < columns and 0 < w["bytes_held"] <= budget, (columns, w)
        check(ctx, ref, n, L)
        ran.append(columns)
    print("refused below %s bytes (%d bytes per column); ran at %s columns" % (sorted(least), per_column, ran))
    assert len(least) == 1 and len(ran) >= 25, (least, ran)
    needs = least.pop()
    assert budget_of(per_column, L) < needs < budget_of(per_column, ran[0])
    ctx.set_list_memory(needs)
    ctx.run()
    w = ctx.list_windows()
    assert w["windows"] >= 3 and w["bytes_held"] == needs, w
    check(ctx, ref, n, L)
    ctx.set_list_memory(needs - 1)
    with pytest.raises(pkg.FseqError) as e:
        ctx.run()
    assert e.value.code == pkg.FSEQ_E_OOM and "needs %d bytes" % needs in str(e.value)


# (case, world, runs): what a sharded run does.  A regular round of the DP belongs to the rank that holds its first column
# L + r RL - 1 -- these columns lie in [L - 1, n - L) --, and the library takes a world only if every rank that holds blocks
# owns a round (fseq_set_shard).  Blocks are of 48 columns here (the halo, RL), a rank holds q 4^k of them.
#   * 6 L columns: two and three ranks run (their shares are 1.6 to 3.7 L columns).  The fourth of four ranks holds the
#     columns from 2,880 (L = 513: n - L = 2,605) and from 20,736 (L = 4,097: n - L = 20,524): behind every round.
#   * 2 L + 3 RL columns have four regular rounds.  L = 100: two ranks of 192 and 152 columns own two rounds each; of three
#     ranks of 144 columns the third lies behind the last round; of four ranks of 96 the first lies in front of column L - 1.
#     L = 1,000: the four rounds start in columns 999 .. 1,143 -- all in the first of two ranks (1,152 columns), none in the
#     first of three or four (768, 576 columns).
REFUSAL = "too few columns per rank for this segment length: use fewer ranks"
SHARDED = [(slc.large(L), world, world < 4) for L in slc.SHARD_L_LONG for world in (2, 3, 4)] + \
          [(slc.shard_short(L), world, (L, world) == (100, 2)) for L in slc.SHARD_L_SHORT for world in (2, 3, 4)]


@pytest.mark.parametrize("case,world,runs", SHARDED, ids=["L%d_n%d_world%d" % (c[2], c[1], w) for c, w, _ in SHARDED])
def test_sharded_runs_with_ranks_shorter_than_a_segment(pkg, case, world, runs):
    """Ranks of fewer than two segment lengths of columns: every rank's DP entries, traceback and merged segments and the
    owners' boundary states against the oracle.  A world whose leading or trailing ranks would own no DP round is refused,
    with the same code and message on every rank, before any exchange."""
    m, n, L = case[:3]
    msa = slc.make(case)
    if runs:
        ctxs = run_world(pkg, world, lambda c: c.set_sequences(msa), m, n, L)
        check_against_oracle(pkg, ctxs, msa, L)
        cols = [c.shard_columns() for c in ctxs]
        assert cols[0][0] == 0 and cols[-1][1] == n
        assert 2 * min(hi - lo for lo, hi in cols) < 5 * L                         # (tests/test_gpu_shard.py: 12.5 L and more)
        assert len({c._transport.calls for c in ctxs}) == 1                        # every rank made the same exchanges
        return
    with pytest.raises(pkg.FseqError) as e:
        run_world(pkg, world, lambda c: c.set_sequences(msa), m, n, L)
    assert e.value.code == pkg.FSEQ_E_UNSUPPORTED and REFUSAL in str(e.value)
    fdist = importlib.import_module("founder-sequences_amd.dist")
    tw = fdist.ThreadWorld(world)
    for r in range(world):
        ctx = pkg.SegmentationContext(m, n, L)
        with pytest.raises(pkg.FseqError) as e:
            tw.attach(ctx, r, "cuda:0")
        assert e.value.code == pkg.FSEQ_E_UNSUPPORTED and REFUSAL in str(e.value), r
        ctx.close()
