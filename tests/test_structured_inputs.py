"""The structured families of tests/structured_inputs.py still have the properties they are there for (CPU, oracle only).

A family that has lost its property tests nothing on the device: every generator is held to the oracle figures recorded
in FAMILIES (status, maximum segment size, traceback and merged lengths) and to the structure its row of the table names."""
import numpy as np
import pytest

import fso
import structured_inputs as si

RED_W = 2048            # values below a block's first threshold the search for vmin looks at (csrc/fseq_reduced.hpp)
SLIM_VALUES = 4096      # distinct start values the slim configuration holds (csrc/fseq_kernels.hpp)
SLIM_FIRST_ROWS = 4801  # the slim configuration takes blocks of 4,801 .. 6,720 representatives (csrc/fseq_reduced.hip)

_refs = {}


def distinct_rows(msa):
    return len(np.unique(np.ascontiguousarray(msa).view(np.dtype((np.void, msa.shape[1])))))


def oracle(name):
    """(alignment, oracle result) of a family, computed once."""
    if name not in _refs:
        gen, L, _, _ = si.FAMILIES[name]
        msa = gen()
        _refs[name] = (msa, fso.segment_long(msa, L, threads=8))
    return _refs[name]


@pytest.mark.parametrize("name", list(si.FAMILIES))
def test_family_gives_the_recorded_oracle_figures(name):
    gen, L, _, want = si.FAMILIES[name]
    msa, ref = oracle(name)
    assert msa.dtype == np.uint8 and msa.ndim == 2 and msa.flags["C_CONTIGUOUS"]
    assert np.array_equal(msa, gen()), "deterministic"
    got = (ref["status"], ref["max_segment_size"], len(ref["traceback"]), len(ref["reduced"]))
    assert got == want
    tb = ref["traceback"]
    assert tb["lb"][0] == 0 and tb["rb"][-1] == msa.shape[1] and np.array_equal(tb["lb"][1:], tb["rb"][:-1])


def _block_states(msa, B):
    """(k0, d at k0) for every block start k0 = 0, B, 2B, ... and for n."""
    n = msa.shape[1]
    p = fso.Pbwt(msa, with_counts=False, debug=False)
    out = []
    for k in range(n + 1):
        if k % B == 0 or k == n:
            out.append((k, p.d))
        if k < n:
            p.step()
    return out


@pytest.mark.parametrize("name,B", [("staircase", 100), ("staircase_wide", 100)])
def test_staircase_blocks_hold_thousands_of_distinct_values(name, B):
    """Some block of B = 100 columns starts with more distinct divergence values >= 1 than the slim configuration's table
    holds (4,096) -- staircase only: staircase_wide has 3,000 rows -- and with more than RED_W = 2,048 distinct values
    below its first threshold thr0 = k0 + 2 - L: the histogram of the search for vmin does not reach them all.

    What phase C makes of it: a block's representatives are the rows with d1 >= vmin in the state BEHIND the block, and
    vmin >= thr0 - RED_W whatever the list capacity, so a block has at most #{ d1 >= max(1, thr0 - RED_W) } of them.  Here
    that is fewer than the 4,801 from which on the plan takes the slim configuration: no shape of this family at L <= 100
    reaches the slim configuration's refusal (distinct values among representatives <= representatives), and growing m or
    the block length does not change that -- rows that mutate inside or behind the block start it with divergence 0."""
    gen, L, _, _ = si.FAMILIES[name]
    msa, _ = oracle(name)
    m, n = msa.shape
    states = _block_states(msa, B)
    most_values = most_below = most_reps = 0
    for (k0, d0), (_, d1) in zip(states[:-1], states[1:]):
        thr0 = max(0, k0 + 2 - L)
        vals = np.unique(d0[d0 >= 1])
        below = int((vals < thr0).sum())
        if len(vals) > most_values:
            most_values, most_below = len(vals), below
        most_reps = max(most_reps, int((d1 >= max(1, thr0 - RED_W)).sum()))
    if name == "staircase":
        assert most_values > SLIM_VALUES and most_below > RED_W, (most_values, most_below)
    else:
        assert most_values > RED_W and most_below > RED_W, (most_values, most_below)
    assert 0 < most_reps < SLIM_FIRST_ROWS, most_reps
    # every row is its own class behind the last mutation
    assert distinct_rows(msa) == m


def test_trail_identity_values_lie_below_the_vmin_window():
    """At column k = 11,000 every divergence value is below k + 2 - L - RED_W: the histogram of the search for vmin is empty."""
    gen, L, _, _ = si.FAMILIES["trail_identity"]
    msa, _ = oracle("trail_identity")
    k = 11000
    p = fso.Pbwt(msa, with_counts=False, debug=False)
    while p.idx < k:
        p.step()
    d = p.d
    assert d[0] == k                                    # (the first position holds the column itself, by the pBWT's convention)
    d = d[1:]
    assert d.max() < k + 2 - L - RED_W, d.max()
    assert len(np.unique(d)) > 10                       # (and they are values, not one zero)


def test_lead_identity_first_boundary_lies_behind_the_first_traceback_window():
    _, ref = oracle("lead_identity")
    assert ref["traceback"]["rb"][0] > 8192
    assert ref["reduced"]["rb"][0] > 8192


def test_counter_has_1024_distinct_rows_in_four_copies():
    msa, _ = oracle("counter")
    rows, copies = np.unique(msa, axis=0, return_counts=True)
    assert len(rows) == 1024 and (copies == 4).all()
    # the order is reshuffled in every column: both symbols in every column, half of the rows each
    assert ((msa == ord("A")).sum(axis=0) == msa.shape[0] // 2).all()
    assert distinct_rows(oracle("counter_all_distinct")[0]) == 4096


def test_sweep_moves_one_row_per_column():
    msa, _ = oracle("sweep")
    m, n = msa.shape
    for k in range(n):
        syms, cnt = np.unique(msa[:, k], return_counts=True)
        assert sorted(cnt.tolist()) == [1, m - 1], k


def test_every_column_families_cut_at_every_lth_column():
    for name in ("every_column_a_segment", "every_other_column"):
        gen, L, _, _ = si.FAMILIES[name]
        msa, ref = oracle(name)
        n = msa.shape[1]
        assert len(ref["traceback"]) == n // L == len(ref["reduced"])
        assert np.array_equal(ref["traceback"]["rb"], np.arange(L, n + 1, L))
    assert 20000 > 2 * 8192 and 17000 > 2 * 8192           # three traceback windows of 8,192 DP entries each


def test_border_recombination_merges_on_block_borders():
    msa, ref = oracle("border_recombination")
    rb = ref["reduced"]["rb"]
    assert int((rb % si.BORDER_B == 0).sum()) >= 10
    # ... and the cut set has cuts on, one before and one behind borders
    cuts = np.array(si.border_cuts(msa.shape[1]))
    for phase in (0, 1, si.BORDER_B - 1):
        assert int((cuts % si.BORDER_B == phase).sum()) >= 10, phase


def test_periodic_rows_repeat_with_period_37():
    msa, _ = oracle("periodic")
    assert np.array_equal(msa[:-si.PERIOD], msa[si.PERIOD:])
    assert distinct_rows(msa) == si.PERIOD
    assert np.array_equal(msa[:, :-si.PERIOD], msa[:, si.PERIOD:])


def test_halving_merges_remove_half_of_the_boundaries():
    for name in ("halving_merge", "halving_merge_l1"):
        _, ref = oracle(name)
        assert len(ref["reduced"]) * 2 <= len(ref["traceback"]) + 1


def test_long_merge_removes_a_third_of_a_thousand_segments():
    _, ref = oracle("long_merge")
    tb, red = ref["traceback"], ref["reduced"]
    assert len(tb) >= 1000 and 3 * len(red) <= 2 * len(tb), (len(tb), len(red))
    joined = np.bincount(np.diff(np.searchsorted(tb["rb"], red["rb"])))
    assert joined[2] > 100 and joined[3] > 100, joined     # runs of two and of three traceback segments in one merged segment
