"""The segmentation path on the structured families of tests/structured_inputs.py, bit for bit against the CPU oracle.

Every exact-parity test elsewhere draws its rows from mosaics of a few founders plus noise.  These inputs are built so that
the ORACLE'S OWN RESULT has another shape (see the table in structured_inputs.py and the CPU property checks of
test_structured_inputs.py): thousands of distinct divergence values in a block, identity stretches of thousands of columns
in front and behind, a traceback of one segment per column over three traceback windows, merges that remove half of a
thousand boundaries, recombination on block borders, keys that repeat with a period.  They reach the kernels through the
public path only.

Every family runs
  (a) on its own plan (the library's block length; border_recombination: blocks of 50 columns),
  (b) with blocks of 33 and of 100 columns,
  (c) each of them again on all rows of every block (FSEQ_NO_REDUCED, set on the context before the input),
and every run is held to the oracle as test_gpu_parity.check_long does: the DP array where cells write it, the traceback,
the merged segments and EVERY boundary state (the 20,000 of every_column_a_segment take ~2 s: all of them are read)."""
import importlib
import re

import numpy as np
import pytest

import fso
import structured_inputs as si
from test_gpu_parity import check_depth_against_oracle, check_long

pytestmark = pytest.mark.gpu

SLIM = (512, 15)                     # threads x rows of the slim configuration (csrc/fseq_kernels.hpp)
SLIM_FIRST_ROWS = 4801               # it takes the blocks of 4,801 .. 6,720 representatives (csrc/fseq_reduced.hip)
PLAN_LINE = re.compile(r"configuration of (\d+) rows: (\d+) blocks, (\d+) representatives on average \((\d+) threads x (\d+) rows, (\d+) distinct values")
ATTEMPT_LINE = re.compile(r"reduced phase C: (\d+) of (\d+) blocks on their representatives \(mean (\d+) of (\d+) rows, most (\d+)\), (\d+) on all rows")
REFUSAL = "more distinct start values than the slim configuration"


@pytest.fixture(scope="module")
def pkg():
    return importlib.import_module("founder-sequences_amd")


_refs = {}


def oracle(name):
    """(alignment, oracle result with its DP array) of a family: computed once, shared by every form, never written to."""
    if name not in _refs:
        gen, L, _, want = si.FAMILIES[name]
        msa = gen()
        ref = fso.segment_long(msa, L, keep_dp=True, threads=8)
        assert (ref["status"], ref["max_segment_size"], len(ref["traceback"]), len(ref["reduced"])) == want
        msa.setflags(write=False)
        _refs[name] = (msa, ref)
    return _refs[name]


def run(pkg, msa, L, block_len, full, debug=False):
    m, n = msa.shape
    ctx = pkg.SegmentationContext(m, n, L, block_len=block_len)
    if full:
        ctx.set_tuning("FSEQ_NO_REDUCED", "1")
    if debug:
        ctx.set_tuning("FSEQ_DEBUG", "1")
    ctx.set_sequences(msa)
    try:
        ctx.run()
    except pkg.NoReduction:
        pass
    return ctx


def block_len_of(name, form):
    return si.FAMILIES[name][2] if form == "own" else int(form)


@pytest.mark.parametrize("full", [False, True], ids=["representatives", "all_rows"])
@pytest.mark.parametrize("form", ["own", "33", "100"])
@pytest.mark.parametrize("name", list(si.FAMILIES))
def test_family_matches_oracle(pkg, name, form, full):
    _, L, _, _ = si.FAMILIES[name]
    msa, ref = oracle(name)
    n = msa.shape[1]
    ctx = run(pkg, msa, L, block_len_of(name, form), full)
    if full:
        assert ctx.timings()["reduced_blocks"] == 0
    # (a short traceback must not pass by both sides being compared over a truncated length)
    assert len(ctx.traceback()) == len(ref["traceback"]) == ctx.result.dp_segment_count
    assert ctx.result.segment_count == len(ref["reduced"])
    if name in ("every_column_a_segment", "every_other_column"):
        assert len(ctx.traceback()) == n // L
    check_long(ctx, ref, n, L, check_dp=True)


def plans_of(err):
    """The library's report of a run with FSEQ_DEBUG: per attempt of the reduced phase C (blocks reduced, blocks in all, most
    representatives of a block, blocks on all rows) and the configurations in use as (rows, blocks, mean, threads, rows per thread,
    distinct values)."""
    attempts = []
    for line in err.splitlines():
        mm = ATTEMPT_LINE.search(line)
        if mm:
            g = [int(x) for x in mm.groups()]
            attempts.append(dict(reduced=g[0], blocks=g[1], most=g[4], on_all_rows=g[5], configs=[]))
        mm = PLAN_LINE.search(line)
        if mm and attempts:
            attempts[-1]["configs"].append(tuple(int(x) for x in mm.groups()))
    return attempts


@pytest.mark.parametrize("form", ["own", "100"])
@pytest.mark.parametrize("name", ["staircase", "staircase_wide"])
def test_staircase_runs_on_its_representatives_below_the_slim_configuration(pkg, capfd, name, form):
    """Where the staircases run, from the library's own report (FSEQ_DEBUG on the context, its stderr captured).

    A staircase block starts with thousands of distinct divergence values (more than the slim configuration's 4,096 and
    more than the 2,048 of the search window for vmin: test_structured_inputs.py), but vmin >= thr0 - 2,048 leaves it a few
    hundred representatives -- the rows that mutate inside the block start it with divergence 0 --, far below the 4,801 from
    which on the plan takes the slim configuration.  So the library reduces the blocks, on small configurations, and the
    slim configuration's refusal (RED_WIDE) is NOT reached by this family at any m or block length; the report must say
    exactly that: blocks on their representatives, none of them on 512 x 15, no refusal, no block of 4,801 representatives.
    With blocks of 100 columns more than 4,096 mutation columns lie behind the start of the last blocks."""
    _, L, _, _ = si.FAMILIES[name]
    msa, ref = oracle(name)
    m, n = msa.shape
    capfd.readouterr()
    ctx = run(pkg, msa, L, block_len_of(name, form), False, debug=True)
    err = capfd.readouterr().err
    attempts = plans_of(err)
    t = ctx.timings()
    print("%s, block length %s: %d blocks of %d columns, %s" % (name, form, t["n_blocks"], t["block_len"], attempts))
    assert attempts, err[-3000:]
    last = attempts[-1]
    assert last["blocks"] == t["n_blocks"] and last["reduced"] == t["reduced_blocks"] > 0, (last, t)
    assert 2 * last["reduced"] > last["blocks"], last
    assert last["configs"] and sum(c[1] for c in last["configs"]) == last["reduced"], last
    for a in attempts:
        assert a["most"] < SLIM_FIRST_ROWS, a
        assert all((c[3], c[4]) != SLIM and c[0] < SLIM_FIRST_ROWS for c in a["configs"]), a
    assert REFUSAL not in err
    if form == "100":
        c0, step = (200, 1) if name == "staircase" else (100, 3)
        behind = min(m, ((t["n_blocks"] - 1) * 100 - c0 + step - 1) // step)          # mutation columns in front of the last block
        assert t["block_len"] == 100 and behind > min(4096, m - 1), (t, behind)
    check_long(ctx, ref, n, L, check_dp=True)
    # ... and the run on all rows says so
    ctx = run(pkg, msa, L, block_len_of(name, form), True, debug=True)
    err = capfd.readouterr().err
    assert not plans_of(err) and ctx.timings()["reduced_blocks"] == 0
    check_long(ctx, ref, n, L, check_dp=False)


# the columns whose blocks are replayed: (family, columns of interest)
LIST_BLOCKS = {
    "staircase": (2700, 5250),           # in the middle of the stairs; behind the last mutation (all 5,000 values distinct)
    "trail_identity": (1500, 11000),     # in the mosaic; 8,000 columns into the identity tail
    "sweep": (350, 2990),                # the first round over the rows; the last block
}


@pytest.mark.parametrize("full", [False, True], ids=["representatives", "all_rows"])
@pytest.mark.parametrize("form", ["own", "100"])
@pytest.mark.parametrize("name", list(LIST_BLOCKS))
def test_lists_of_the_unusual_families_match_the_oracle_counts(pkg, name, form, full):
    """The families whose per-column lists differ in kind from a mosaic's (every value distinct; every value thousands of
    columns behind; one row moving per column): two blocks are replayed by the oracle's pBWT from the device's boundary
    state (test_gpu_parity.check_depth_against_oracle) -- the lists of about twenty columns per block, the block's first
    and its last eight among them, against Pbwt.counts(), sampled DP cells, the merged boundaries inside, the end state."""
    _, L, _, _ = si.FAMILIES[name]
    msa, ref = oracle(name)
    m, n = msa.shape
    ctx = run(pkg, msa, L, block_len_of(name, form), full)
    B = ctx.timings()["block_len"]
    blocks = sorted({c // B for c in LIST_BLOCKS[name]})
    checked = check_depth_against_oracle(pkg, ctx, m, n, L, blocks, list_every=max(1, B // 12), cells_per_block=20, seed=7)
    assert checked["blocks"] == len(blocks) and checked["lists"] >= 8 * len(blocks) and checked["cells"] > 0, checked
