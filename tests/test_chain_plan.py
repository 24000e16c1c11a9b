"""CPU checks of the plan of phase B (csrc/fseq_chainplan.hpp through fseq_debug_chain_plan and fseq_debug_chain_plan_sharded; no
device): the fans DESIGN.md records for BASELINE C4 and its cuts, the properties of the fan, the levels and the launches over a sweep
of block counts, a sharded rank's (k, q) and block range, and the rule that sends a launch to the chain-per-workgroup kernel."""
import ctypes as C
import importlib

import pytest

NEW_DEBUG = ["fseq_debug_chain_plan", "fseq_debug_chain_plan_sharded", "fseq_debug_phase_b"]
LDS_ROWS = 11264                # the most rows of the LDS-resident kernels
ROWS = (11265, 100000, 540000)
CUS = (64, 256, 304)


@pytest.fixture(scope="module")
def pkg():
    build = importlib.import_module("founder-sequences_amd.build")
    build.build()
    return importlib.import_module("founder-sequences_amd")


def ceil_div(a, b):
    return (a + b - 1) // b


def level0(plan):
    """(chains, workgroups) of the two launches on the alignment's own blocks: the composition and the expansion."""
    return [(l[2], l[5]) for l in plan["launches"] if l[0] == 0 and l[1] != 1]


def test_symbols_and_layouts(pkg):
    lib = pkg.load_library()
    for name in NEW_DEBUG:
        assert hasattr(lib, name) and name in pkg.EXPORTS and name in pkg.DEBUG_EXPORTS, name
    assert C.sizeof(pkg.ChainLaunchInfo) == 24
    assert C.sizeof(pkg.ChainPlan) == 4 * 12 + 4 * pkg.CHAIN_LEVELS_MAX + 24 * pkg.CHAIN_LAUNCHES_MAX
    assert C.sizeof(pkg.PhaseBInfo) == 32 + 8 + 16 + 4 * 23 + 4 + 24 * pkg.CHAIN_LAUNCHES_MAX
    assert pkg.PhaseBInfo.fit.offset == 32 and pkg.PhaseBInfo.cw_stats.offset == 56 and pkg.PhaseBInfo.launches.offset == 152
    assert pkg.CW_STATS == 23
    info = pkg.PhaseBInfo()
    assert lib.fseq_debug_phase_b(None, C.byref(info)) == pkg.FSEQ_E_ARG


def test_refusals(pkg):
    lib = pkg.load_library()
    p = pkg.ChainPlan()
    ok = (100000, 1, 6143, 256, 0, 0, 1000, 1)
    assert lib.fseq_debug_chain_plan(*ok, C.byref(p)) == 0
    assert lib.fseq_debug_chain_plan(*ok, None) == pkg.FSEQ_E_ARG
    for i, bad in ((0, 0), (2, 0), (4, 3), (4, -1), (5, 1)):
        args = list(ok)
        args[i] = bad
        assert lib.fseq_debug_chain_plan(*args, C.byref(p)) == pkg.FSEQ_E_ARG, (i, bad)
    oks = (6143, 2, 1, 0, 1, 256, 0, 1000, 1)
    assert lib.fseq_debug_chain_plan_sharded(*oks, C.byref(p)) == 0
    assert lib.fseq_debug_chain_plan_sharded(*oks, None) == pkg.FSEQ_E_ARG
    for i, bad in ((0, 0), (1, 0), (1, 4097), (2, 2), (3, 1), (6, 3)):
        args = list(oks)
        args[i] = bad
        assert lib.fseq_debug_chain_plan_sharded(*args, C.byref(p)) == pkg.FSEQ_E_ARG, (i, bad)


# ---- the recorded choices ("[r14] ... The fan" and the measurements of section 4), on 256 CUs

def test_c4_takes_fan_24_in_one_turn(pkg):
    p = pkg.chain_plan_host(100000, 6143, 256)
    assert (p["fan"], p["fan_round5"], p["turns"]) == (24, 11, 1)
    assert p["level_items"] == [6143, 256, 11]
    assert level0(p) == [(256, 256), (256, 256)]
    # everything above level 0 on the spread kernels
    assert all(l[5] == 0 for l in p["launches"] if l[0] > 0)
    assert [l[:4] for l in p["launches"]] == [(0, 0, 256, 24), (1, 0, 11, 24), (2, 1, 1, 11), (1, 2, 11, 24), (0, 2, 256, 24)]


@pytest.mark.parametrize("knob", [1, 2])
def test_c4_under_a_forced_kernel_keeps_round_5s_fan(pkg, knob):
    p = pkg.chain_plan_host(100000, 6143, 256, chain_wg=knob)
    assert (p["fan"], p["fan_round5"], p["turns"]) == (11, 11, 0)
    assert p["level_items"] == [6143, 559, 51, 5]
    assert [c for c, _ in level0(p)] == [559, 559]
    # 1: every launch on k_chain_wg, at most a workgroup a CU; 2: none
    assert [l[5] for l in p["launches"]] == ([min(l[2], 256) for l in p["launches"]] if knob == 1 else [0] * 7)


def test_c4slice_keeps_fan_5_and_the_spread_kernels(pkg):
    p = pkg.chain_plan_host(100000, 512, 256)
    assert (p["fan"], p["fan_round5"], p["turns"]) == (5, 5, 0)
    assert p["level_items"] == [512, 103, 21, 5]
    assert all(l[5] == 0 for l in p["launches"])


def test_c4_cut_to_2048_blocks_moves_from_fan_7_to_8(pkg):
    p = pkg.chain_plan_host(100000, 2048, 256)
    assert (p["fan"], p["fan_round5"], p["turns"]) == (8, 7, 1)
    assert level0(p) == [(256, 256), (256, 256)]
    for knob in (1, 2):
        assert pkg.chain_plan_host(100000, 2048, 256, chain_wg=knob)["fan"] == 7
    assert pkg.chain_plan_host(100000, 2048, 0)["fan"] == 7


def test_a_forced_fan_stands(pkg):
    for fan in (2, 4, 64, 200):
        p = pkg.chain_plan_host(100000, 6143, 256, chain_fan=fan)
        assert (p["fan"], p["fan_round5"], p["turns"]) == (fan, 11, 0)
        assert p["level_items"][1] == ceil_div(6143, fan)


# ---- properties over a sweep

def round5_fan(m, nblocks):
    """Round 5's cost model, restated: the steps of every level up and down and of the top chain, 3.5 us a step at 100,000 rows, and
    50 us a round of launches."""
    best, best_g = None, None
    for g in range(2, min(64, nblocks - 1) + 1):
        steps = rounds = 0.0
        cnt = nblocks
        while cnt > g:
            steps += cnt * (2.0 * g - 1.0) / g
            rounds += 2.0 * g - 1.0
            cnt = ceil_div(cnt, g)
        cost = (steps + cnt) * 3.5e-3 * (m / 1e5) + (rounds + cnt) * 0.05
        if best is None or cost < best:
            best, best_g = cost, g
    return best_g


def depth_fan(nblocks):
    """The model of LDS-resident rows, restated: 2 levels - 1 launches of 2 g + 1 half-steps each."""
    best, best_g = None, nblocks
    for g in range(2, min(64, max(3, nblocks) - 1) + 1):
        lv, cap = 1, g
        while cap < nblocks:
            cap *= g
            lv += 1
        cost = (2 * lv - 1) * (2 * g + 1)
        if best is None or cost < best:
            best, best_g = cost, g
    return nblocks if nblocks <= 8 else best_g


def raw_plan(pkg, lib, p, m, streamed, nblocks, cus, knob):
    assert lib.fseq_debug_chain_plan(m, int(streamed), nblocks, cus, knob, 0, pkg.CHAIN_FIT_ANY, 1, C.byref(p)) == 0
    return p.fan, p.fan_round5, p.turns, p.level_items[:p.n_levels]


@pytest.mark.parametrize("m", ROWS)
def test_fan_and_levels_over_a_sweep(pkg, m):
    lib = pkg.load_library()
    p = pkg.ChainPlan()
    moved = 0
    for nblocks in range(1, 10001):
        none = raw_plan(pkg, lib, p, m, True, nblocks, 0, 0)
        assert none[2] == 0 and none[0] == none[1]
        if nblocks % 37 == 0 or nblocks <= 70:
            assert none[0] == (nblocks if nblocks <= 8 else round5_fan(m, nblocks)), nblocks
        for cus in CUS:
            for knob in (0, 1, 2):
                fan, fan5, turns, items = raw_plan(pkg, lib, p, m, True, nblocks, cus, knob)
                where = (m, nblocks, cus, knob)
                if knob:
                    assert (fan, fan5, turns, items) == none, where      # a forced kernel: exactly the plan of 0 CUs
                    continue
                assert fan == nblocks if nblocks <= 8 else 2 <= fan <= 64, where
                assert fan5 == none[0], where
                # the levels shrink by exactly ceil(count / fan) and end with at most fan items
                assert items[0] == nblocks and items[-1] <= max(fan, 1), where
                for a, b in zip(items, items[1:]):
                    assert a > fan and b == ceil_div(a, fan), where
                if turns:
                    chains = ceil_div(nblocks, fan)
                    assert chains >= cus and fan >= fan5 and turns == ceil_div(chains, cus), where
                    assert items[1] == chains, where
                    moved += fan != fan5
                else:
                    assert fan == fan5, where
                    # no turns were counted only where round 5's fan leaves level 0 below a chain per CU
                    assert nblocks <= 8 or ceil_div(nblocks, fan5) < cus, where
    assert moved > 0


def test_lds_resident_rows_never_take_the_streamed_model(pkg):
    lib = pkg.load_library()
    p = pkg.ChainPlan()
    differs = 0
    for m in (64, 2500, LDS_ROWS):
        for nblocks in list(range(1, 1200)) + [4096, 6143, 10000]:
            want = depth_fan(nblocks)
            for cus in (0,) + CUS:
                for knob in (0, 1, 2):
                    fan, fan5, turns, items = raw_plan(pkg, lib, p, m, False, nblocks, cus, knob)
                    assert (fan, fan5, turns) == (want, want, 0), (m, nblocks, cus, knob)
            differs += raw_plan(pkg, lib, p, m, True, nblocks, 256, 0)[0] != want
            plan = pkg.chain_plan_host(m, nblocks, 256, chain_wg=1)           # (streamed: None -> by the row count)
            assert all(l[5] == 0 for l in plan["launches"])                   # ... and no launch of theirs is on k_chain_wg
    assert differs > 0                                                         # (the flag is what decides: the models disagree)
    # by the row count alone (streamed=None): one row more and the turns of workgroups are counted
    assert pkg.chain_plan_host(LDS_ROWS + 1, 6143, 256)["turns"] >= 1
    resident = pkg.chain_plan_host(LDS_ROWS, 6143, 256)
    assert (resident["fan"], resident["turns"]) == (depth_fan(6143), 0)


def test_launches_follow_the_levels(pkg):
    for m, nblocks, cus in ((11300, 1280, 256), (11300, 1100, 256), (100000, 6143, 304), (11300, 60, 256), (11300, 5, 256), (11300, 1, 256)):
        p = pkg.chain_plan_host(m, nblocks, cus)
        items, fan = p["level_items"], p["fan"]
        top = len(items) - 1
        want = [(i, pkg.CHAIN_COMPOSE, items[i + 1], fan) for i in range(top)] + [(top, pkg.CHAIN_TOP, 1, items[top])] + \
               [(i, pkg.CHAIN_EXPAND, items[i + 1], fan) for i in reversed(range(top))]
        assert [l[:4] for l in p["launches"]] == want
        assert all(l[4] == 0 for l in p["launches"])
        assert [l[5] for l in p["launches"]] == [cus if l[2] >= cus else 0 for l in p["launches"]]      # (a workgroup a CU: resident = 1)


# ---- the rule and the cap on the workgroups

def test_the_rule_fires_at_a_chain_per_cu(pkg):
    for cus in CUS:
        for fan in (2, 4, 7):
            below = pkg.chain_plan_host(100000, (cus - 1) * fan, cus, chain_fan=fan)
            at = pkg.chain_plan_host(100000, (cus - 1) * fan + 1, cus, chain_fan=fan)
            assert level0(below) == [(cus - 1, 0)] * 2
            assert level0(at) == [(cus, cus)] * 2
    # a device that does not say how many CUs it has counts as one
    assert all(l[5] == 1 for l in pkg.chain_plan_host(100000, 600, 0, chain_fan=4)["launches"])


def test_workgroups_are_capped_by_residency_and_by_the_workspace(pkg):
    cus, fan = 256, 4
    for grid in (256, 257, 367, 512, 1000):
        for fit in (1, 100, 255, 256, 300, 5000, pkg.CHAIN_FIT_ANY):
            for resident in (0, 1, 2):
                p = pkg.chain_plan_host(100000, grid * fan, cus, chain_fan=fan, fit=fit, resident=resident)
                assert level0(p) == [(grid, min(grid, fit, cus * max(resident, 1)))] * 2, (grid, fit, resident)
    # no room for a workspace: the spread kernels, also under a forced knob
    for knob in (0, 1):
        p = pkg.chain_plan_host(100000, 2000, cus, chain_fan=fan, chain_wg=knob, fit=0)
        assert all(l[5] == 0 for l in p["launches"])
    p = pkg.chain_plan_host(100000, 2000, cus, chain_fan=fan, chain_wg=1, fit=3)
    assert [l[5] for l in p["launches"]] == [min(l[2], 3) for l in p["launches"]]


# ---- sharded ranks

@pytest.mark.parametrize("F", [2, 3, 4, 8])
def test_sharded_ranks_tile_the_blocks(pkg, F):
    blocks = list(range(1, 300)) + [511, 512, 513, 1000, 2049, 4095, 4096, 6143, 8184, 10000]
    for world in range(2, 9):
        for nblocks in blocks:
            plans = [pkg.chain_plan_sharded_host(nblocks, world, r, 256, chain_fan=F) for r in range(world)]
            p0 = plans[0]
            k, q, bpr, nh = p0["shard_k"], p0["shard_q"], p0["blocks_per_rank"], p0["n_hyper"]
            where = (F, world, nblocks)
            assert bpr == q * F ** k and bpr >= ceil_div(nblocks, world), where       # q F^k covers a rank's share
            assert 1 <= nh <= world and nh == ceil_div(nblocks, bpr), where
            at = 0
            for r, p in enumerate(plans):
                assert [p[f] for f in ("shard_k", "shard_q", "blocks_per_rank", "n_hyper", "fan")] == [k, q, bpr, nh, F], where
                assert p["b_lo"] == at, where                                           # the ranges tile
                assert r >= nh or p["b_lo"] % (F ** k) == 0, where                      # a rank with blocks starts at a multiple of F^k
                assert (p["b_hi"] > p["b_lo"]) == (r < nh), where                       # every active rank owns a block, no other does
                at = p["b_hi"]
                # the rank's items a level, and its launches: up, its composites, the hyper chain, and down again
                items = p["level_items"]
                assert len(items) == k + 1 and items[0] == p["b_hi"] - p["b_lo"], where
                lo, hi = p["b_lo"], p["b_hi"]
                for i in range(1, k + 1):
                    lo, hi = lo // F, ceil_div(hi, F)
                    assert items[i] == hi - lo, where
                hyper = (k + 1, pkg.CHAIN_TOP, 1, nh, 0)
                if r < nh:
                    assert items[k] <= q, where
                    up = [(i, pkg.CHAIN_COMPOSE, items[i + 1], F) for i in range(k)] + [(k, pkg.CHAIN_COMPOSE, 1, q)]
                    down = [(k, pkg.CHAIN_EXPAND, 1, q)] + [(i, pkg.CHAIN_EXPAND, items[i + 1], F) for i in reversed(range(k))]
                    assert [l[:4] for l in p["launches"]] == up + [hyper[:4]] + down, where
                else:
                    assert [l[:5] for l in p["launches"]] == [hyper], where
            assert at == nblocks, where


def test_sharded_first_chains_and_kernels(pkg):
    """A rank's launches start at its own first chain of every level, and take the kernel the rule gives their chain count."""
    cus = 256
    for world, nblocks in ((2, 2049), (2, 6144), (3, 3000), (8, 8184)):
        for r in range(world):
            p = pkg.chain_plan_sharded_host(nblocks, world, r, cus)
            F, k = p["fan"], p["shard_k"]
            for level, kind, chains, blocks, first, wgs in p["launches"]:
                if level < k:
                    assert first == p["b_lo"] // F ** (level + 1)
                elif level == k:
                    assert first == r
                assert wgs == (cus if chains >= cus else 0)
            forced = pkg.chain_plan_sharded_host(nblocks, world, r, cus, chain_wg=1)
            assert all(l[5] == min(l[2], cus) for l in forced["launches"])
            none = pkg.chain_plan_sharded_host(nblocks, world, r, cus, chain_wg=2)
            assert all(l[5] == 0 for l in none["launches"])


def test_a_sharded_rank_of_c4_reaches_the_rule(pkg):
    """BASELINE C4 (5,000,000 columns, 100,000 rows) over 2, 4 and 8 ranks of 256 CUs, the block counts block_geometry's sharded branch
    gives it (blocks of 814, 814 and 611 columns): a rank's level 0 launches 768, 384 and 256 chains at the fan of 4 -- at least a
    chain per CU, so it goes to k_chain_wg by the rule."""
    for world, nblocks, chains in ((2, 6143, 768), (4, 6143, 384), (8, 8184, 256)):
        p = pkg.chain_plan_sharded_host(nblocks, world, 0, 256)
        assert p["fan"] == 4 and level0(p)[0][0] == chains and level0(p)[0][1] == 256, (world, p)
