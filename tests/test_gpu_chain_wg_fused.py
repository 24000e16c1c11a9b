"""Phase B's chain-per-workgroup kernel (k_chain_wg, csrc/fseq_chainsort.hpp): runs against the chunks of its waves, and the keys it
hands to pass 2.  The table of tests/chain_wg_fused_cases.py (tests/test_chain_wg_fused_cases.py proves on the CPU what each case is
listed for) against the numpy model of tests/chain_step_cases.py, every output word and the kernel's counters; that table and
tests/chain_wg_cases.py's through fseq_debug_chain_launch_wg_keys: for every block the launch steps through, either the flag is
clear or the 16-bit array holds rank[b] in the order in front of b.  Integers, no tolerance."""
import importlib

import numpy as np
import pytest

import chain_step_cases as cs
import chain_wg_cases as cw
import chain_wg_fused_cases as cf

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def pkg():
    return importlib.import_module("founder-sequences_amd")


def same(got, want):
    return got.shape == np.shape(want) and np.array_equal(got, want)


def launch(pkg, B, case, entry):
    """One launch of the case through `entry`, held to the model: (steps, model's outputs, hand-over keys, flags)."""
    sa, sd = cw.launch_args(case, B)
    G, first, chains = case["G"], case["first"], case["chains"]
    want = cs.chain(B["rank"], B["keyd"], B["nkeys"], G, cs.COLS, first, chains, sa, sd, states=case["states"], keys=case["keys"])
    steps, want_stats = cw.walk(B["rank"], B["keyd"], B["nkeys"], G, cs.COLS, first, chains, sa, sd, case["keys"], case["run_cap"])
    got = entry(B["rank"], B["keyd"], B["nkeys"], G, cs.COLS, first_chain=first, chains=chains, start_a=sa, start_d=sd, states=case["states"],
                keys=case["keys"], run_cap=case["run_cap"], workgroups=case["workgroups"])
    stats = got.pop("stats")
    hk, hf = got.pop("hand_keys", None), got.pop("hand_flag", None)
    assert sorted(got) == sorted(want)
    for name in sorted(want):
        assert same(got[name], want[name]), name
    assert same(stats, want_stats), (list(stats), list(want_stats))
    assert [s[1] for ch in steps for s in ch] == list(case["paths"])
    return steps, want, hk, hf


def check_hand_over(pkg, B, case, steps, want, hk, hf):
    """The rule of the hand-over on one launch: an expansion's run or sort step through b whose keys fit 16 bits hands rank[b] over in
    the order in front of b (the model's state there) and sets the flag; every other block keeps its pattern and a clear flag."""
    nb, m = B["rank"].shape
    assert hk.shape == (nb, m) and hk.dtype == np.uint16 and hf.shape == (nb,)
    expansion = case["states"] and not case["keys"]
    handed = set()
    for ch in steps:
        for b, path, _ in ch:
            if expansion and path != "ident" and B["nkeys"][b] <= 65536:
                handed.add(b)
    for b in range(nb):
        if hf[b]:
            front = want["state_a"][b]
            assert b in handed and np.all(front != cs.NOT_WRITTEN)
            assert np.array_equal(hk[b], B["rank"][b][front].astype(np.uint16)), b
        else:
            assert np.all(hk[b] == pkg.HAND_FILL), b
    # (the library's own rule sets every flag it may: the steps above)
    assert set(np.flatnonzero(hf).tolist()) == handed
    return handed


@pytest.mark.parametrize("case", cf.FUSED_CASES, ids=[c["id"] for c in cf.FUSED_CASES])
def test_the_fused_table_equals_the_model(pkg, case):
    B = cf.build_fused(case)
    steps, want, hk, hf = launch(pkg, B, case, pkg.chain_launch_wg_keys)
    assert check_hand_over(pkg, B, case, steps, want, hk, hf) == {0}
    # the same launch without a hand-over array
    if case["m"] >= cs.M_MIN:
        launch(pkg, B, case, pkg.chain_launch_wg)


@pytest.mark.parametrize("case", cw.WG_CASES, ids=[c["id"] for c in cw.WG_CASES])
def test_the_hand_over_on_the_kernels_own_table(pkg, case):
    B = cw.build_wg(case)
    steps, want, hk, hf = launch(pkg, B, case, pkg.chain_launch_wg_keys)
    handed = check_hand_over(pkg, B, case, steps, want, hk, hf)
    if case["keys"]:
        # a composition (and a launch that wants both): every flag clear, the array untouched
        assert not handed and not hf.any() and np.all(hk == pkg.HAND_FILL)


def test_keys_beyond_16_bits_are_not_handed_over(pkg):
    """70,000 rows, every position a key of its own: more keys than 16 bits hold (and than share a word with a position: the step sorts
    its rows).  The flag stays clear, the array untouched, the states are the model's."""
    case = dict(name="wide-keys", m=70000, blocks=(("perm",),), G=1, first=0, chains=1, own_start=True, states=True, keys=False, run_cap=cw.CW_RUN_CAP,
                workgroups=1, paths=("sort",), runs=None, start="random", seed=9700)
    B = cw.build_wg(case)
    assert B["nkeys"][0] == 70000 > 65536
    steps, want, hk, hf = launch(pkg, B, case, pkg.chain_launch_wg_keys)
    assert not hf.any() and np.all(hk == pkg.HAND_FILL)
    assert check_hand_over(pkg, B, case, steps, want, hk, hf) == set()


def test_refusals(pkg):
    B = cf.build_fused(cf.FUSED_CASES[0])
    sa, sd = cw.launch_args(cf.FUSED_CASES[0], B)
    for kw in (dict(run_cap=cw.CW_RUN_CAP + 1), dict(workgroups=0)):
        with pytest.raises(pkg.FseqError):
            pkg.chain_launch_wg_keys(B["rank"], B["keyd"], B["nkeys"], 1, cs.COLS, start_a=sa, start_d=sd, **kw)
    # 64 rows: below what the entry takes
    with pytest.raises(pkg.FseqError):
        pkg.chain_launch_wg_keys(np.zeros((1, 64)), np.zeros((1, 64)), [1], 1, cs.COLS)
