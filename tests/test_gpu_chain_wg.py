"""Phase B's chain-per-workgroup kernel (k_chain_wg, csrc/fseq_chainsort.hpp) through fseq_debug_chain_launch_wg against the numpy
model of tests/chain_step_cases.py: every output word, integers, no tolerance, and the form every step took from the kernel's own
counters.  The cases of tests/chain_wg_cases.py (tests/test_chain_wg_cases.py checks on the CPU that each has the property it is
listed for), and every case of the spread kernels' table, chain_step_cases.CHAIN_CASES, forced through this kernel."""
import importlib

import numpy as np
import pytest

import chain_step_cases as cs
import chain_wg_cases as cw

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def pkg():
    return importlib.import_module("founder-sequences_amd")


def same(got, want):
    return got.shape == np.shape(want) and np.array_equal(got, want)


def check(pkg, B, G, first, chains, start_a, start_d, states, keys, run_cap, workgroups):
    want = cs.chain(B["rank"], B["keyd"], B["nkeys"], G, cs.COLS, first, chains, start_a, start_d, states=states, keys=keys)
    steps, want_stats = cw.walk(B["rank"], B["keyd"], B["nkeys"], G, cs.COLS, first, chains, start_a, start_d, keys, run_cap)
    got = pkg.chain_launch_wg(B["rank"], B["keyd"], B["nkeys"], G, cs.COLS, first_chain=first, chains=chains, start_a=start_a, start_d=start_d,
                              states=states, keys=keys, run_cap=run_cap, workgroups=workgroups)
    stats = got.pop("stats")
    assert sorted(got) == sorted(want)
    for name in sorted(want):
        assert same(got[name], want[name]), name
    assert same(stats, want_stats), (list(stats), list(want_stats))
    return steps, stats


@pytest.mark.parametrize("case", cw.WG_CASES, ids=[c["id"] for c in cw.WG_CASES])
def test_chain_wg_equals_the_model(pkg, case):
    B = cw.build_wg(case)
    start_a, start_d = cw.launch_args(case, B)
    steps, stats = check(pkg, B, case["G"], case["first"], case["chains"], start_a, start_d, case["states"], case["keys"], case["run_cap"],
                         case["workgroups"])
    flat = [s for chain in steps for s in chain]
    # the forms the table names, from the kernel's own counters
    assert [s[1] for s in flat] == list(case["paths"])
    assert tuple(int(x) for x in stats[:3]) == tuple(case["paths"].count(p) for p in ("runs", "sort", "ident"))
    if case["runs"] is not None and "runs" in case["paths"]:
        assert stats[3] == max(case["runs"])


@pytest.mark.parametrize("case", cs.CHAIN_CASES, ids=[c["id"] for c in cs.CHAIN_CASES])
def test_the_spread_kernels_cases_through_chain_wg(pkg, case):
    B = cs.build_chain(case)
    G, first, chains = case["G"], case["first"], case["chains"]
    start_a = start_d = None
    if case["own_start"]:
        seq_a, seq_d = cs.sequential_states(B["a"], B["d"], B["rank"], B["keyd"])
        start_a = [seq_a[(first + c) * G] for c in range(chains)]
        start_d = [seq_d[(first + c) * G] for c in range(chains)]
    check(pkg, B, G, first, chains, start_a, start_d, case["states"], case["keys"], cw.CW_RUN_CAP, min(chains, 3))


def test_refusals(pkg):
    B = cw.build_wg(cw.WG_CASES[0])
    sa, sd = cw.launch_args(cw.WG_CASES[0], B)
    for kw in (dict(run_cap=cw.CW_RUN_CAP + 1), dict(workgroups=0), dict(workgroups=1025)):
        with pytest.raises(pkg.FseqError):
            pkg.chain_launch_wg(B["rank"], B["keyd"], B["nkeys"], 1, cs.COLS, start_a=sa, start_d=sd, **kw)
