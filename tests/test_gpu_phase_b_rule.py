"""Whole runs on streamed rows with phase B as a run by itself chooses it: FSEQ_CHAIN_WG and FSEQ_CHAIN_FAN unset, on block counts
at which the rule fires (level 0 has at least a chain per CU) -- what a BASELINE C4 benchmark runs and no forced-knob test does.  Level 0
is composed and expanded by k_chain_wg, the levels above go through the spread kernels k_cm_* on the same workspace, and the hand-over
of level 0's keys to pass 2 is armed by the rule.  Two shapes, derived from the device's CU count through the plan's host entry
(fseq_debug_chain_plan); on 256 CUs, at 11,300 rows in blocks of 12 columns:
  one turn   1,280 blocks: fan 5 where round 5's model gives 3, 256 chains, levels 1,280 / 256 / 52 / 11 / 3
  two turns  1,100 blocks: fan 3, 367 chains on 256 workgroups -- a workgroup walks a second chain over one workspace
Everything is read from fseq_debug_phase_b, nothing from the library's notes."""
import importlib

import numpy as np
import pytest

import fso
from helpers import founder_mosaic
from test_gpu_parity import check_long

pytestmark = pytest.mark.gpu

M, L, B = 11300, 10, 12
MAX_COLUMNS = 30000
SEED = {"one_turn": 1501, "two_turns": 1502}


@pytest.fixture(scope="module")
def pkg():
    return importlib.import_module("founder-sequences_amd")


def rule_plan(pkg, nblocks, cus):
    """The plan of nblocks blocks if the rule sends exactly level 0 to k_chain_wg, else None."""
    p = pkg.chain_plan_host(M, nblocks, cus)
    on_wg = [l for l in p["launches"] if l[5]]
    if p["turns"] and [l[:2] for l in on_wg] == [(0, pkg.CHAIN_COMPOSE), (0, pkg.CHAIN_EXPAND)]:
        return p
    return None


@pytest.fixture(scope="module")
def shapes(pkg):
    """name -> (nblocks, plan): the smallest runs at which the rule fires on this device -- the issue's block counts scaled to its CUs
    first (5 and 1,100 / 256 blocks a CU), then every count whose columns stay below MAX_COLUMNS."""
    import torch
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    most = MAX_COLUMNS // B - 1
    want = {"one_turn": lambda p: p["turns"] == 1 and p["fan"] > p["fan_round5"], "two_turns": lambda p: p["turns"] == 2}
    first = {"one_turn": 5 * cus, "two_turns": 1100 * cus // 256}
    out = {}
    for name, ok in want.items():
        for nblocks in [first[name]] + list(range(cus, most + 1)):
            p = rule_plan(pkg, nblocks, cus) if nblocks <= most else None
            if p and ok(p):
                out[name] = (nblocks, p)
                break
    return cus, out


class Runs:
    """The inputs, the oracle's results and the contexts of this module, made once."""

    def __init__(self):
        self.inputs, self.ctxs = {}, {}

    def input(self, nblocks, seed):
        if (nblocks, seed) not in self.inputs:
            msa = founder_mosaic(12, M, nblocks * B, brec=100, seed=seed)
            self.inputs[nblocks, seed] = (msa, fso.segment_long(msa, L, keep_dp=False, threads=4))
        return self.inputs[nblocks, seed]

    def ctx(self, pkg, nblocks, seed, **knobs):
        key = (nblocks, seed, tuple(sorted(knobs.items())))
        if key not in self.ctxs:
            ctx = pkg.SegmentationContext(M, nblocks * B, L, block_len=B)
            ctx.set_tuning("FSEQ_DEBUG", 1)                   # (k_chain_wg keeps its counters)
            for name, value in knobs.items():
                ctx.set_tuning(name, value)
            ctx.set_sequences(self.input(nblocks, seed)[0])
            run(pkg, ctx)
            self.ctxs[key] = ctx
        return self.ctxs[key]


@pytest.fixture(scope="module")
def runs():
    return Runs()


def run(pkg, ctx):
    try:
        ctx.run()
    except pkg.NoReduction:
        pass


def shape(shapes, name):
    cus, found = shapes
    if name not in found:
        pytest.skip("%d CUs: no run of %d rows in blocks of %d columns below %d columns fires the rule for the %s shape" % (cus, M, B, MAX_COLUMNS, name))
    return (cus,) + found[name]


def states(ctx):
    return [ctx.boundary_state(i) for i in range(len(ctx.reduced_traceback()))]


def same_states(x, y):
    sx, sy = states(x), states(y)
    assert len(sx) == len(sy)
    for (a, d), (a2, d2) in zip(sx, sy):
        assert np.array_equal(a, a2) and np.array_equal(d, d2)


def check_report(pkg, ctx, cus, nblocks, plan):
    """fseq_debug_phase_b against the plan: exactly level 0's two launches on k_chain_wg, and the kernel's steps accounted for."""
    info = ctx.phase_b()
    chains, fan = plan["level_items"][1], plan["fan"]
    assert (info["cus"], info["nblocks"], info["fan"]) == (cus, nblocks, fan)
    assert ctx.timings()["n_blocks"] == nblocks and ctx.timings()["block_len"] == B
    assert info["fit"] >= 1 and info["resident"] >= 1
    want = pkg.chain_plan_host(M, nblocks, cus, fit=info["fit"], resident=info["resident"])["launches"]
    assert info["launches"] == want
    on_wg = [l for l in info["launches"] if l[5]]
    assert [l[:4] for l in on_wg] == [(0, pkg.CHAIN_COMPOSE, chains, fan), (0, pkg.CHAIN_EXPAND, chains, fan)]
    assert all(1 <= l[5] <= min(chains, cus * info["resident"]) for l in on_wg)
    assert len(info["launches"]) == 2 * (len(plan["level_items"]) - 1) + 1
    # up: every block once, the first of every chain from the identity; down: all but the last block of every chain, and the last of all
    s = info["cw_stats"]
    assert info["stats_kept"] and s is not None
    assert s["from_identity"] == chains
    assert s["by_runs"] + s["by_sort"] + s["from_identity"] == nblocks + (nblocks - chains + 1)
    assert s["by_runs"] > 0
    return info


@pytest.mark.parametrize("name", ["one_turn", "two_turns"])
def test_run_under_the_rule_equals_the_oracle_and_the_spread_kernels(pkg, shapes, runs, name):
    cus, nblocks, plan = shape(shapes, name)
    chains = plan["level_items"][1]
    assert chains >= cus and all(c < cus for c in plan["level_items"][2:])        # the precondition: level 0 alone reaches the rule
    if name == "two_turns":
        assert cus < chains <= 2 * cus
    else:
        assert chains == cus and plan["fan"] > plan["fan_round5"]
    msa, ref = runs.input(nblocks, SEED[name])
    n = nblocks * B
    ctx = runs.ctx(pkg, nblocks, SEED[name])
    check_long(ctx, ref, n, L, check_dp=False)
    check_report(pkg, ctx, cus, nblocks, plan)
    # block states against the oracle's sweep: about every 50th block, and behind the last
    p = fso.Pbwt(msa, debug=False)
    for b in sorted(set(range(0, nblocks, 50)) | {chains // 2 * plan["fan"] + 1, nblocks - 1, nblocks}):
        while p.idx < min(n, b * B):
            p.step()
        a, d = ctx.debug_block_state(b)
        assert np.array_equal(a, p.a) and np.array_equal(d, p.d), b
    # the same run on the spread kernels alone (round 5's fan): identical
    spread = runs.ctx(pkg, nblocks, SEED[name], FSEQ_CHAIN_WG=2)
    info = spread.phase_b()
    assert info["fan"] == plan["fan_round5"] and all(l[5] == 0 for l in info["launches"]) and not info["stats_kept"] and not info["hand_armed"]
    check_long(spread, ref, n, L, check_dp=False)
    for f in ("lb", "rb", "segment_max_size", "segment_size"):
        assert np.array_equal(ctx.traceback()[f], spread.traceback()[f]), f
    same_states(ctx, spread)


@pytest.mark.parametrize("name", ["one_turn", "two_turns"])
def test_the_rule_arms_the_hand_over(pkg, shapes, runs, name):
    cus, nblocks, plan = shape(shapes, name)
    chains = plan["level_items"][1]
    msa, ref = runs.input(nblocks, SEED[name])
    ctx = runs.ctx(pkg, nblocks, SEED[name])
    info = ctx.phase_b()
    assert info["hand_armed"]
    # the expansion of level 0 steps through all but the last block of its chains, and the last of all
    assert 1 <= info["p2_groups_took_keys"] <= nblocks - chains + 1
    assert info["p2_groups"] > 0 and info["p2_groups_took_keys"] + info["p2_groups_gathered"] == info["p2_groups"]
    gathered = runs.ctx(pkg, nblocks, SEED[name], FSEQ_P2_KEYS=2)
    info2 = gathered.phase_b()
    assert not info2["hand_armed"] and info2["p2_groups_took_keys"] == 0 and info2["p2_groups_gathered"] == info2["p2_groups"] == info["p2_groups"]
    assert [l[:5] for l in info2["launches"]] == [l[:5] for l in info["launches"]]          # (the same phase B)
    check_long(gathered, ref, nblocks * B, L, check_dp=False)
    same_states(ctx, gathered)


def test_a_second_input_and_the_rule_switched_off_on_one_context(pkg, shapes, runs):
    """The context of the two-turn run takes another input -- armed again, and a flag left over from the first input would be a wrong
    state --, then FSEQ_CHAIN_WG=2: the rule cannot fire, so nothing may be taken from the keys the runs before handed over."""
    cus, nblocks, plan = shape(shapes, "two_turns")
    n = nblocks * B
    msa, ref = runs.input(nblocks, SEED["two_turns"])
    ctx = runs.ctx(pkg, nblocks, SEED["two_turns"])
    assert ctx.phase_b()["hand_armed"]
    msa_b, ref_b = runs.input(nblocks, SEED["two_turns"] + 100)
    assert not np.array_equal(ref_b["reduced"]["rb"], ref["reduced"]["rb"])
    try:
        ctx.set_sequences(msa_b)
        run(pkg, ctx)
        check_long(ctx, ref_b, n, L, check_dp=False)
        info = check_report(pkg, ctx, cus, nblocks, plan)
        assert info["hand_armed"] and info["p2_groups_took_keys"] >= 1
        assert info["p2_groups_took_keys"] + info["p2_groups_gathered"] == info["p2_groups"]
        ctx.set_tuning("FSEQ_CHAIN_WG", 2)
        run(pkg, ctx)
        check_long(ctx, ref_b, n, L, check_dp=False)
        info = ctx.phase_b()
        assert not info["hand_armed"] and all(l[5] == 0 for l in info["launches"])
        assert info["p2_groups"] > 0 and info["p2_groups_took_keys"] == 0 and info["p2_groups_gathered"] == info["p2_groups"]
    finally:
        runs.ctxs.clear()            # (this context no longer holds what its key says)
