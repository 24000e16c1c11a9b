// fseq_chainplan.hpp -- the plan of phase B as values, made by pure functions: the fan of the recursion over the key blocks
// (block_geometry, csrc/fseq_path_setup.hip), the items of every level (the buffers of alloc_geometry_buffers), the launches of the way
// up, the top chain and the way down (long_phase_b, csrc/fseq_path_pass1.hip), which of them the rule sends to the chain-per-workgroup
// kernel k_chain_wg and on how many workgroups (chain_wg_groups), and a sharded rank's (k, q), block range and launches.
// Host only: no HIP header, no context -- plain C++17, so that the arithmetic is tested without a device (fseq_debug_chain_plan,
// fseq_debug_chain_plan_sharded, tests/test_chain_plan.py), as plan_reduced (fseq_redplan.hpp) and plan_length_scan (fseq_scanplan.hpp) are.
#pragma once

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

namespace fseq {

constexpr uint32_t CHAIN_SHARD_FAN = 4;      // the fan of a sharded rank's recursion where FSEQ_CHAIN_FAN names none

// one chain launch of phase B
enum ChainLaunchKind : uint32_t { CHAIN_COMPOSE = 0, CHAIN_TOP = 1, CHAIN_EXPAND = 2 };
struct ChainLaunch {
	uint32_t level = 0;          // the level whose key blocks the chains walk (0: the alignment's own blocks); sharded: shard_k for the chain over a
	                             // rank's composites, shard_k + 1 for the chain over the hyper key blocks
	uint32_t kind = 0;           // ChainLaunchKind: composition from the identity (way up), the top chain, expansion (way down)
	uint32_t chains = 0;         // the launch's chains ...
	uint32_t blocks = 0;         // ... of this many key blocks each (the last chain of a level may hold fewer)
	uint32_t first_chain = 0;    // the launch's first chain among the level's (a sharded rank's range starts behind the ranks before it)
	uint32_t workgroups = 0;     // workgroups of k_chain_wg; 0: the spread kernels (k_cm_*) -- LDS-resident rows: always 0
};

// ---- the rule: which kernel a streamed launch of `grid` chains takes.
// At least a chain per CU -> k_chain_wg; below that the spread kernels fill the chip and a chain per workgroup does not.
// knob (FSEQ_CHAIN_WG): 0 the rule, 1 every streamed launch, 2 none.  cus: what the device reports (below 1 counts as 1).
inline bool chain_wg_rule(uint32_t grid, int cus, int knob)
{
	if (knob >= 2) return false;
	return knob == 1 || grid >= (uint32_t) std::max(cus, 1);
}

// How many workgroups of k_chain_wg the launch gets; 0: the launch takes the spread kernels.  As many as the launch has chains, as are
// resident at once (`resident` a CU, below 1 counts as 1) and as the workspace holds (`fit`); a launch on more chains than that walks
// them in turns.  fit == 0 (only a forced launch on a few blocks finds room for none): the spread kernels.
inline uint32_t chain_wg_workgroups(uint32_t grid, int cus, int knob, size_t fit, int resident)
{
	if (!chain_wg_rule(grid, cus, knob)) return 0;
	return (uint32_t) std::min<size_t>(std::min<size_t>(grid, fit), (size_t) std::max(cus, 1) * (size_t) std::max(resident, 1));
}

// ---- the fan, not sharded
// [r5] streamed rows: the cost of fan g.  A step is a launch sequence over all the chains of a level (fseq_chainsort.hpp), bound by what
// it moves, not by its depth -- so the fan weighs the steps in all (the blocks of every level once on the way up, all but every chain's
// last on the way down: ~N (2g - 1) / (g - 1)) against the rounds of launches, (2g - 1) per level.
// [r14] turns != 0: level 0 on k_chain_wg instead, `turns` turns of workgroups of 2g - 1 steps each: a step 0.5 ms at 100,000 rows, a
// chain's step from the identity 0.4 more (block_geometry has the measurements).
inline double chain_stream_cost(uint32_t m, uint32_t nblocks, uint32_t g, uint64_t turns)
{
	double steps = 0, rounds = 0, own = 0;
	uint64_t cnt = nblocks;
	bool level0 = true;
	while (cnt > g)
	{
		if (level0 && turns) own = (double) turns * ((2.0 * g - 1.0) * 0.5 + 0.4) * ((double) m / 1e5);
		else
		{
			steps += (double) cnt * (2.0 * g - 1.0) / g;   // up: every item; down: all but the last of every group
			rounds += 2.0 * g - 1.0;
		}
		level0 = false;
		cnt = (cnt + g - 1) / g;
	}
	steps += (double) cnt; rounds += (double) cnt;           // the top chain
	return own + steps * 3.5e-3 * ((double) m / 1e5) + rounds * 0.05;
}

struct ChainFan {
	uint32_t fan = 0;        // the fan in force
	uint32_t fan5 = 0;       // the fan before the turns of workgroups were looked at: round 5's model on streamed rows, the depth model otherwise
	uint32_t turns = 0;      // the turns of workgroups the model counted for level 0 at `fan`; 0: it counted none (round 5's fan stands)
};

// m rows in nblocks blocks; streamed: the rows take the streamed kernels (select_kernels finds no LDS-resident configuration);
// cus: the device's CUs as the runtime reports them (0: it does not say); knob: FSEQ_CHAIN_WG; forced: FSEQ_CHAIN_FAN (0: none --
// a forced fan stands whatever the models say, and no turns are reported for it)
inline ChainFan plan_chain_fan(uint32_t m, bool streamed, uint32_t nblocks, int cus, int knob, uint32_t forced)
{
	ChainFan P;
	// Phase B is serial over key blocks, so it is applied recursively: compose groups of G blocks from the identity
	// (parallel), groups of G of those, ... until at most G are left, chain them, expand level by level.  Serial depth
	// = G steps per launch, 2 levels - 1 launches (+ about half a step of launch gap each): G = 4 for 100..10^4
	// blocks (1024 blocks: 9 launches of <= 4 steps instead of the 5 x 11 of a three-level chain).
	uint32_t best_g = nblocks, best_cost = ~0u;
	for (uint32_t g = 2; g <= 64 && g < std::max(3u, nblocks); ++g)
	{
		uint32_t lv = 1;
		for (uint64_t cap = g; cap < nblocks; cap *= g) ++lv;
		uint32_t const cost = (2u * lv - 1u) * (2u * g + 1u);
		if (cost < best_cost) { best_cost = cost; best_g = g; }
	}
	uint32_t turns = 0;
	if (streamed && nblocks > 8)
	{
		double best = 1e300;
		for (uint32_t g = 2; g <= 64 && g < nblocks; ++g)
		{
			double const cost = chain_stream_cost(m, nblocks, g, 0);
			if (cost < best) { best = cost; best_g = g; }
		}
		// [r14] Where that fan's level 0 has at least a chain per CU, the level goes to k_chain_wg: a workgroup a CU walks its chains one
		// after the other, so the level takes ceil(chains / CUs) turns of 2g - 1 steps, and a fan that leaves the last turn nearly empty
		// pays for it.  Only then, and only among the wider fans that keep level 0 on that kernel, the turns are counted.
		// FSEQ_CHAIN_WG=1 or 2 (tests): round 5's fan.
		int const ncu = knob == 0 ? cus : 0;
		if (ncu > 0 && ((uint64_t) nblocks + best_g - 1) / best_g >= (uint64_t) ncu && nblocks > best_g)
		{
			uint32_t const g5 = best_g;
			P.fan5 = g5;
			best = 1e300;
			for (uint32_t g = g5; g <= 64 && g < nblocks; ++g)
			{
				uint64_t const chains = ((uint64_t) nblocks + g - 1) / g;
				if (chains < (uint64_t) ncu) break;
				uint64_t const t = (chains + ncu - 1) / ncu;
				double const cost = chain_stream_cost(m, nblocks, g, t);
				if (cost < best) { best = cost; best_g = g; turns = (uint32_t) t; }
			}
		}
	}
	if (nblocks <= 8) best_g = std::max(1u, nblocks);        // one chain
	if (!P.fan5) P.fan5 = best_g;
	P.fan = best_g; P.turns = turns;
	if (forced) { P.fan = forced; P.turns = 0; }
	return P;
}

// the items of every level under fan `fan`: [0] the blocks, [i] the composites of fan items of level i - 1, until at most fan are left
// (those the top chain takes)
inline std::vector<uint32_t> chain_level_items(uint32_t nblocks, uint32_t fan)
{
	std::vector<uint32_t> items{nblocks};
	for (uint32_t cnt = nblocks; fan >= 2 && cnt > fan;)
	{
		cnt = (cnt + fan - 1) / fan;
		items.push_back(cnt);
	}
	return items;
}

// the launches of phase B on one GPU, in the order they are queued: up the levels, the top chain, down the levels.  streamed, cus, knob,
// fit, resident: as for chain_wg_workgroups (not streamed: every launch on the LDS-resident chain kernel, workgroups 0)
inline std::vector<ChainLaunch> chain_launches(std::vector<uint32_t> const &items, uint32_t fan, bool streamed, int cus, int knob, size_t fit, int resident)
{
	std::vector<ChainLaunch> out;
	size_t const top = items.size() - 1;
	auto put = [&](uint32_t level, uint32_t kind, uint32_t chains, uint32_t blocks) {
		ChainLaunch l;
		l.level = level; l.kind = kind; l.chains = chains; l.blocks = blocks;
		l.workgroups = streamed ? chain_wg_workgroups(chains, cus, knob, fit, resident) : 0u;
		out.push_back(l);
	};
	for (size_t i = 0; i < top; ++i) put((uint32_t) i, CHAIN_COMPOSE, items[i + 1], fan);
	put((uint32_t) top, CHAIN_TOP, 1, items[top]);
	for (size_t i = top; i-- > 0;) put((uint32_t) i, CHAIN_EXPAND, items[i + 1], fan);
	return out;
}

// ---- sharded: a rank is one hyper-block of phase B: q groups of F^k blocks, composed level by level with fan F (k launches of <= F
// serial steps up, the q composites into the hyper key block, and the same down again).  q F^k >= the blocks a rank needs; (k, q)
// with the fewest serial steps among those that keep every rank busy.
struct ShardChainPlan {
	uint32_t F = 0, k = 0, q = 0;
	uint32_t group = 0;          // F^k: the blocks of one of a rank's q groups
	uint32_t bpr = 0;            // q F^k: the blocks of a rank
	uint32_t n_super = 0;        // groups in all
	uint32_t n_hyper = 0;        // ranks that own blocks (<= world)
};

inline ShardChainPlan plan_chain_sharded(uint32_t nblocks, uint32_t world, uint32_t F)
{
	ShardChainPlan P;
	uint32_t const per = (nblocks + world - 1) / world;
	uint32_t best_k = 0, best_q = std::max(1u, per), best_cost = ~0u;
	{
		uint64_t pw = 1;
		for (uint32_t k = 0; pw <= per; ++k, pw *= F)
		{
			uint32_t const q = (uint32_t) ((per + pw - 1) / pw);
			uint64_t const bpr = (uint64_t) q * pw;
			bool const all_busy = bpr == per || bpr * (world - 1) < nblocks;      // the last rank still owns blocks
			uint32_t const cost = F * k + q;
			if ((all_busy || k == 0) && cost < best_cost) { best_cost = cost; best_k = k; best_q = q; }
		}
	}
	uint64_t pw = 1;
	for (uint32_t i = 0; i < best_k; ++i) pw *= F;
	P.F = F; P.k = best_k; P.q = best_q;
	P.group = (uint32_t) pw;
	P.bpr = (uint32_t) (best_q * pw);
	P.n_super = (nblocks + P.group - 1) / P.group;
	P.n_hyper = (nblocks + P.bpr - 1) / P.bpr;
	return P;
}

// the blocks [b_lo, b_hi) of a rank (empty behind the last rank that owns any)
inline void shard_block_range(ShardChainPlan const &P, uint32_t nblocks, uint32_t rank, uint32_t *b_lo, uint32_t *b_hi)
{
	*b_lo = (uint32_t) std::min<uint64_t>(nblocks, (uint64_t) rank * P.bpr);
	*b_hi = (uint32_t) std::min<uint64_t>(nblocks, (uint64_t) (rank + 1) * P.bpr);
}

// a rank's items of level i, 0 .. k: [lo[i], hi[i]) (rank boundaries are multiples of F^k blocks)
inline void shard_level_ranges(ShardChainPlan const &P, uint32_t b_lo, uint32_t b_hi, std::vector<uint32_t> &lo, std::vector<uint32_t> &hi)
{
	lo.assign(P.k + 1, 0); hi.assign(P.k + 1, 0);
	lo[0] = b_lo; hi[0] = b_hi;
	for (uint32_t i = 1; i <= P.k; ++i) { lo[i] = lo[i - 1] / P.F; hi[i] = (hi[i - 1] + P.F - 1) / P.F; }
}

// the launches of a rank's phase B, in the order they are queued: up its own range, its composites into its hyper key block, (the
// exchange,) the chain over the hyper key blocks -- every rank --, its composites from the state in front of it, down its own range.  A
// rank without blocks launches the chain over the hyper key blocks alone.
inline std::vector<ChainLaunch> shard_chain_launches(ShardChainPlan const &P, uint32_t nblocks, uint32_t rank, bool streamed, int cus, int knob, size_t fit,
                                                     int resident)
{
	std::vector<ChainLaunch> out;
	uint32_t b_lo, b_hi;
	shard_block_range(P, nblocks, rank, &b_lo, &b_hi);
	std::vector<uint32_t> lo, hi;
	shard_level_ranges(P, b_lo, b_hi, lo, hi);
	bool const have = rank < P.n_hyper;
	auto put = [&](uint32_t level, uint32_t kind, uint32_t chains, uint32_t blocks, uint32_t first) {
		if (!chains) return;
		ChainLaunch l;
		l.level = level; l.kind = kind; l.chains = chains; l.blocks = blocks; l.first_chain = first;
		l.workgroups = streamed ? chain_wg_workgroups(chains, cus, knob, fit, resident) : 0u;
		out.push_back(l);
	};
	for (uint32_t i = 0; have && i < P.k; ++i) put(i, CHAIN_COMPOSE, hi[i + 1] - lo[i + 1], P.F, lo[i + 1]);
	if (have) put(P.k, CHAIN_COMPOSE, 1, P.q, rank);
	put(P.k + 1, CHAIN_TOP, 1, P.n_hyper, 0);
	if (have)
	{
		put(P.k, CHAIN_EXPAND, 1, P.q, rank);
		for (uint32_t i = P.k; i-- > 0;) put(i, CHAIN_EXPAND, hi[i + 1] - lo[i + 1], P.F, lo[i + 1]);
	}
	return out;
}

} // namespace fseq
