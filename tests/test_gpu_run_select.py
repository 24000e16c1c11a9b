"""The run steps of pass 2 (k_chain_snap_grouped through pkg.pass2_step, with and without phase B's handed-over keys) and of phase B
(k_chain_wg through pkg.chain_launch_wg) where the runs' bitmap select, pass 2's pass over the run heads and its 16-byte sweeps over
the ranks can go wrong (csrc/fseq_chainsort.hpp), against the numpy model of tests/chain_step_cases.py: every output word and the
kernels' counters, integers, no tolerance.  The cases are tests/run_select_cases.py's; tests/test_proto_run_select.py checks on the
CPU that each asks for what it is listed for."""
import importlib

import numpy as np
import pytest

import chain_step_cases as cs
import chain_wg_cases as cw
import run_select_cases as rs

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def pkg():
    return importlib.import_module("founder-sequences_amd")


def same(got, want):
    return got.shape == np.shape(want) and np.array_equal(got, want)


@pytest.mark.parametrize("case", rs.PASS2_CASES, ids=[c["id"] for c in rs.PASS2_CASES])
def test_pass2_run_steps_equal_the_model(pkg, case):
    B = rs.build_pass2(case)
    nb = len(case["blocks"])
    want_a, want_d, want_stats = cs.pass2_model(B["a0"], B["d0"], B["rank"], B["task_blk"], B["cls"], B["headd"], B["ncls"], case["run_cap"])
    # the path, from the model's counters: the cases say which
    assert (want_stats[0], want_stats[1]) == ((nb, 0) if case["path"] == "runs" else (0, nb))
    handed = int(B["hand_flag"].sum())
    for workgroups in (1, 2):
        if handed:
            # (the ranks of a block handed over are zeroed: its keys can only come from hand_keys)
            got_a, got_d, stats, hand = pkg.pass2_step(B["a0"], B["d0"], B["rank_given"], B["task_blk"], B["cls"], B["headd"], B["ncls"],
                                                       run_cap=case["run_cap"], workgroups=workgroups, hand_keys=B["hand_keys"], hand_flag=B["hand_flag"])
            assert (int(hand[0]), int(hand[1])) == (handed, nb - handed)
        else:
            got_a, got_d, stats = pkg.pass2_step(B["a0"], B["d0"], B["rank"], B["task_blk"], B["cls"], B["headd"], B["ncls"],
                                                 run_cap=case["run_cap"], workgroups=workgroups)
        assert same(got_a, want_a), "a"
        assert same(got_d, want_d), "d"
        assert same(stats, want_stats), (list(stats), list(want_stats))
        if case["runs"] is not None:
            assert stats[3] == case["runs"]


def test_pass2_without_the_hand_over_equals_the_model(pkg):
    """The edge layout gathered in both blocks, through the entry without hand_keys."""
    case = dict(rs.PASS2_CASES[0], blocks=("gathered", "gathered"))
    B = rs.build_pass2(case)
    want_a, want_d, want_stats = cs.pass2_model(B["a0"], B["d0"], B["rank"], B["task_blk"], B["cls"], B["headd"], B["ncls"], case["run_cap"])
    got_a, got_d, stats = pkg.pass2_step(B["a0"], B["d0"], B["rank"], B["task_blk"], B["cls"], B["headd"], B["ncls"], run_cap=case["run_cap"], workgroups=2)
    assert same(got_a, want_a) and same(got_d, want_d) and same(stats, want_stats) and stats[0] == 2


@pytest.mark.parametrize("case", rs.CW_CASES, ids=[c["id"] for c in rs.CW_CASES])
def test_chain_wg_on_both_sides_of_the_bitmap(pkg, case):
    B = cw.build_wg(case)
    sa, sd = cw.launch_args(case, B)
    want = cs.chain(B["rank"], B["keyd"], B["nkeys"], case["G"], cs.COLS, case["first"], case["chains"], sa, sd, states=True, keys=False)
    _, want_stats = cw.walk(B["rank"], B["keyd"], B["nkeys"], case["G"], cs.COLS, case["first"], case["chains"], sa, sd, False, case["run_cap"])
    got = pkg.chain_launch_wg(B["rank"], B["keyd"], B["nkeys"], case["G"], cs.COLS, first_chain=case["first"], chains=case["chains"], start_a=sa, start_d=sd,
                              states=True, keys=False, run_cap=case["run_cap"], workgroups=1)
    stats = got.pop("stats")
    for name in sorted(want):
        assert same(got[name], want[name]), name
    assert same(stats, want_stats) and stats[0] == 1, list(stats)
    if case["runs"] is not None:
        assert stats[3] == case["runs"][0]
