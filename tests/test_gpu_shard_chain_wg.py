"""Sharded ranks with phase B's chains on a workgroup each (k_chain_wg).  A rank's branch of phase B goes through the same launcher as
one GPU's, with what only it passes: a first chain that is not 0 (the rank's range of every level), the chain over its own composites
into its hyper key block, and an expansion that starts from the state the chain over the hyper key blocks left in front of it.  Forced
(FSEQ_CHAIN_WG=1) on the streamed shapes of tests/test_gpu_shard.py, and by the rule -- knob unset -- on the smallest alignment where one
rank's level 0 has at least a chain per CU and the other's has not.  The ranks are threads on the one GPU (ThreadWorld)."""
import importlib

import numpy as np
import pytest

import fso
from helpers import founder_mosaic
from test_gpu_shard import check_against_oracle, run_world

pytestmark = pytest.mark.gpu

MAX_COLUMNS = 30000


@pytest.fixture(scope="module")
def pkg():
    return importlib.import_module("founder-sequences_amd")


def check_block_states(pkg, ctxs, msa, B, fan, every):
    """Every rank's block states -- in front of its own blocks and behind the last of them, a sample and the ends of its range -- against
    the oracle's sweep; returns {(block, rank): (a, d)}."""
    m, n = msa.shape
    nblocks = ctxs[0].timings()["n_blocks"]
    assert ctxs[0].timings()["block_len"] == B
    asked = set()
    for r in range(len(ctxs)):
        plan = pkg.chain_plan_sharded_host(nblocks, len(ctxs), r, 1, chain_fan=fan)
        b_lo, b_hi = plan["b_lo"], plan["b_hi"]
        if b_hi > b_lo:
            asked |= {(b, r) for b in set(range(b_lo, b_hi + 1, every)) | {b_lo, b_lo + 1, b_hi - 1, b_hi}}
    p = fso.Pbwt(msa, debug=False)
    out = {}
    for b, r in sorted(asked):
        while p.idx < min(n, b * B):
            p.step()
        a, d = ctxs[r].debug_block_state(b)
        assert np.array_equal(a, p.a) and np.array_equal(d, p.d), (b, r)
        out[b, r] = (a, d)
    return out


def check_reports(pkg, ctxs, fan, knob):
    """Every rank's launches as fseq_debug_phase_b reports them against the plan of the rank; returns the reports."""
    world = len(ctxs)
    infos = [c.phase_b() for c in ctxs]
    for r, info in enumerate(infos):
        plan = pkg.chain_plan_sharded_host(info["nblocks"], world, r, info["cus"], chain_fan=fan, chain_wg=knob, fit=info["fit"], resident=info["resident"])
        assert info["fan"] == plan["fan"] and info["launches"] == plan["launches"], r
        assert not info["hand_armed"] and info["p2_groups_took_keys"] == 0, r          # a sharded rank never hands over
    return infos


def same_results(pkg, xs, ys):
    """Two worlds on the same input: traceback on every rank, boundary states on their owners."""
    for x, y in zip(xs, ys):
        assert x.result.max_segment_size == y.result.max_segment_size
        for f in ("lb", "rb", "segment_max_size", "segment_size"):
            assert np.array_equal(x.traceback()[f], y.traceback()[f]), f
        assert np.array_equal(x.reduced_traceback(), y.reduced_traceback())
    red = xs[0].reduced_traceback()
    for i in range(len(red)):
        owner = xs[0].shard_owner(int(red["rb"][i]))
        (a, d), (a2, d2) = xs[owner].boundary_state(i), ys[owner].boundary_state(i)
        assert np.array_equal(a, a2) and np.array_equal(d, d2), i


FORCED = [
    # world, fan (0: the 4 a sharded run takes), (m, n, L, K, Brec, mu, seed, kind, block_len)
    (2, 0, (12000, 3000, 20, 12, 120, 3e-4, 53, 0, 30)),
    (3, 0, (12000, 3000, 20, 12, 120, 3e-4, 53, 0, 30)),
    (4, 0, (12000, 3000, 20, 12, 120, 3e-4, 53, 0, 30)),
    (2, 2, (12000, 900, 10, 12, 200, 3e-4, 46, 0, 12)),
    (2, 3, (12000, 900, 10, 12, 200, 3e-4, 46, 0, 12)),
    (2, 8, (12000, 900, 10, 12, 200, 3e-4, 46, 0, 12)),
]


@pytest.mark.parametrize("world,fan,shape", FORCED, ids=["world%d_fan%d_n%d" % (w, f, s[1]) for w, f, s in FORCED])
def test_sharded_ranks_forced_onto_the_chain_per_workgroup_kernel(pkg, monkeypatch, world, fan, shape):
    m, n, L, K, Brec, mu, seed, kind, B = shape
    msa = fso.synth_msa(fso.synth_spec(seed, K, Brec, mu, kind), m, n)
    if fan:
        monkeypatch.setenv("FSEQ_CHAIN_FAN", str(fan))
    monkeypatch.setenv("FSEQ_CHAIN_WG", "1")
    wg = run_world(pkg, world, lambda c: c.set_sequences(msa), m, n, L, block_len=B)
    check_against_oracle(pkg, wg, msa, L)
    infos = check_reports(pkg, wg, fan, 1)
    for r, info in enumerate(infos):
        assert info["launches"] and all(l[5] >= 1 for l in info["launches"]), r         # every launch of every rank on k_chain_wg
        assert any(l[4] > 0 for l in info["launches"]) == (r > 0), r                     # ... from the rank's own first chain
    states = check_block_states(pkg, wg, msa, B, fan, 7)
    monkeypatch.setenv("FSEQ_CHAIN_WG", "2")
    spread = run_world(pkg, world, lambda c: c.set_sequences(msa), m, n, L, block_len=B)
    for r, info in enumerate(check_reports(pkg, spread, fan, 2)):
        assert all(l[5] == 0 for l in info["launches"]), r
        assert [l[:5] for l in info["launches"]] == [l[:5] for l in infos[r]["launches"]], r
    same_results(pkg, wg, spread)
    for (b, r), (a, d) in states.items():
        a2, d2 = spread[r].debug_block_state(b)
        assert np.array_equal(a, a2) and np.array_equal(d, d2), (b, r)


def test_a_sharded_rank_reaches_the_rule(pkg):
    """Knob unset, two ranks, 11,300 rows in blocks of 12 columns at L = 10 (the halo is min(L, 56) columns, so the blocks stand): the
    first block count at which rank 0's level 0 has more chains than the device CUs at the fan of 4 -- k_chain_wg in two turns -- while
    rank 1's stays below a chain per CU and keeps the spread kernels.  On 256 CUs: 2,049 blocks, 24,588 columns; rank 0 has 1,280
    blocks in 320 chains, rank 1 769 in 193.  The oracle takes about 5 s on that shape (4 threads)."""
    import torch
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    M, L, B, world = 11300, 10, 12, 2
    most = MAX_COLUMNS // B - 1

    def mixed(nblocks):
        plans = [pkg.chain_plan_sharded_host(nblocks, world, r, cus) for r in range(world)]
        on_wg = [[l for l in p["launches"] if l[5]] for p in plans]
        return plans if on_wg[0] and on_wg[0][0][2] > cus and not on_wg[1] and plans[1]["b_hi"] > plans[1]["b_lo"] else None

    found = next(((nb, mixed(nb)) for nb in [8 * cus + 1] + list(range(4 * cus, most + 1)) if nb <= most and mixed(nb)), None)
    if found is None:
        pytest.skip("%d CUs: no alignment of %d rows in blocks of %d columns below %d columns puts one of two ranks on the rule" % (cus, M, B, MAX_COLUMNS))
    nblocks, plans = found
    n = nblocks * B
    msa = founder_mosaic(12, M, n, brec=100, seed=1601)
    ctxs = run_world(pkg, world, lambda c: c.set_sequences(msa), M, n, L, block_len=B)
    assert ctxs[0].timings()["n_blocks"] == nblocks
    check_against_oracle(pkg, ctxs, msa, L)
    infos = check_reports(pkg, ctxs, 0, 0)
    for r, (info, plan) in enumerate(zip(infos, plans)):
        assert info["cus"] == cus
        assert [l[:5] for l in info["launches"]] == [l[:5] for l in plan["launches"]], r
        assert [bool(l[5]) for l in info["launches"]] == [bool(l[5]) for l in plan["launches"]], r
    # rank 0: exactly its level 0, up and down, on k_chain_wg, more chains than workgroups; rank 1: nothing
    chains = plans[0]["level_items"][1]
    assert [l[:5] for l in infos[0]["launches"] if l[5]] == [(0, pkg.CHAIN_COMPOSE, chains, 4, 0), (0, pkg.CHAIN_EXPAND, chains, 4, 0)]
    assert chains > cus
    assert all(l[5] == 0 for l in infos[1]["launches"])
    check_block_states(pkg, ctxs, msa, B, 0, 50)
