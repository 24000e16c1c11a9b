"""The cases of tests/segment_length_cases.py still have the properties they are there for (CPU, oracle only).

A case without a reduction, or whose optimum is one segment, runs no traceback to speak of, no merge and no pass 2 on the
device: every long-width, large, speculative and large-row case must have status 0, max_segment_size < m, at least three
traceback entries and at least two merged segments; at least half of the small-L cases must have merges (fewer merged
segments than traceback entries).  The short widths n = 2 L + j are exempt: they are there for the tail of the DP schedule.
A case that fails a condition is a defect of the table."""
import importlib

import numpy as np
import pytest

import fso
import segment_length_cases as slc

_refs = {}


def oracle(name, case):
    if name not in _refs:
        _refs[name] = fso.segment_long(slc.make(case), case[2], threads=8)
    return _refs[name]


def _holds(name, case):
    m, n, L = case[:3]
    ref = oracle(name, case)
    got = (ref["status"], ref["max_segment_size"], len(ref["traceback"]), len(ref["reduced"]))
    assert ref["status"] == 0, (name, got)
    assert ref["max_segment_size"] < m, (name, got)
    assert len(ref["traceback"]) >= 3, (name, got)
    assert len(ref["reduced"]) >= 2, (name, got)
    tb = ref["traceback"]
    assert tb["lb"][0] == 0 and tb["rb"][-1] == n and np.array_equal(tb["lb"][1:], tb["rb"][:-1])
    assert (tb["rb"] - tb["lb"]).min() >= L


def _chunks_of_the_least_length(case):
    """Chunks of the speculative DP when a chunk has its least length, max(400, 8 L) entries in whole rounds (with one chunk
    per CU of a device the chunks are longer only on far wider inputs)."""
    m, n, L = case[:3]
    RL = slc.round_length(L)
    nreg = (n - 2 * L) // RL + 1
    rounds_per_chunk = -(-max(400, 8 * L) // RL)
    return -(-nreg // rounds_per_chunk)


@pytest.mark.parametrize("L0", range(1, 131, 10))
def test_small_segment_lengths_reduce_to_several_segments(L0):
    for L in range(L0, L0 + 10):
        _holds("small_long_%d" % L, slc.small_long(L))


def test_every_small_segment_length_is_in_the_table_once():
    assert slc.SMALL_L == tuple(range(1, 131))
    for L in slc.SMALL_L:
        m, n, LL = slc.small_short(L)[:3]
        RL = slc.round_length(L)
        assert LL == L and 2 * L <= n <= 2 * L + 2 * RL - 1
    # every tail of the schedule at both sides of the schedule's edges
    for lo, hi in ((1, 55), (56, 95), (96, 130)):
        assert {L % 6 for L in range(lo, hi + 1)} == set(range(6))


def test_at_least_half_of_the_small_segment_lengths_have_merges():
    merged = 0
    for L in slc.SMALL_L:
        ref = oracle("small_long_%d" % L, slc.small_long(L))
        merged += len(ref["reduced"]) < len(ref["traceback"])
    assert 2 * merged >= len(slc.SMALL_L), merged


@pytest.mark.parametrize("L", slc.LARGE_L)
def test_large_segment_lengths_reduce_to_several_segments(L):
    case = slc.large(L)
    _holds("large_%d" % L, case)
    assert _chunks_of_the_least_length(case) < 3             # the serial DP kernel (spec_plan, csrc/fseq_path_dp.hip)


@pytest.mark.parametrize("L", slc.SPECULATIVE_L)
def test_speculative_widths_reduce_to_many_segments(L):
    case = slc.speculative(L)
    _holds("speculative_%d" % L, case)
    assert len(oracle("speculative_%d" % L, case)["traceback"]) >= 10
    assert _chunks_of_the_least_length(case) >= 3


@pytest.mark.parametrize("name", list(slc.ROW_CASES))
def test_large_row_cases_reduce_to_several_segments(name):
    _holds(name, slc.ROW_CASES[name])


def test_round_length_is_the_schedules():
    """The table's tails and the forced chunk lengths rest on the cells per round: a change of dp_schedule makes them stale."""
    pkg = importlib.import_module("founder-sequences_amd")
    for L in list(slc.SMALL_L) + list(slc.LARGE_L):
        n = slc.large(L)[1]
        rounds, RL, _, pipelined = pkg.dp_schedule(L, n, n)
        assert RL == slc.round_length(L), L
        assert pipelined == (L >= slc.DP_PIPE_MIN_L), L
        assert rounds == (n - 2 * L) // RL + 1 + (2 if pipelined else 1), L
