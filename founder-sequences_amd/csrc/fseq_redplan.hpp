// fseq_redplan.hpp -- [r5] phase C on representative rows: the plan of one attempt as a value, made by a pure function.
// Which block runs on its representatives, on which configuration of the reduced column kernel, and whether the
// representatives pay at all is arithmetic on the counts k_reduce_prep left (fseq_reduced.hpp).  Host only: no HIP header, no
// context -- plain C++17, so that the arithmetic is tested without a device (fseq_debug_red_plan, tests/test_red_plan.py).
// red_plan (csrc/fseq_path_reduced.hip) is the stages around it.
#pragma once

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

namespace fseq {

constexpr uint32_t RED_NONE = 0xFFFFFFFFu;      // cnt[b]: block b is not reduced (more representatives than the kernel holds)
constexpr uint8_t RED_FORCE_FULL = 1, RED_FORCE_WIDE = 2;    // RedPlanInput::force[b]

// what planning needs of a configuration (ReducedSet, fseq_ctx.hpp).  fits: it fits this run's geometry (the LDS at this block
// length and symbol width, the 16-bit value ids: columns_fit_reduced)
// cls [r10]: its staged-column buffers may be sized for a class column of phase A at no cost (red_cls_direct below)
struct RedConfig { uint32_t rows, values, T, E; bool ew, fits; bool cls = false; };

// [r10] The direct-or-gather rule of a configuration: it stages phase A's class columns itself where buffers of the class width
// still fit the LDS and leave as many of its workgroups resident on a CU as the buffers sized for its rows do (lds_*: its LDS with
// either buffer, resident_*: workgroups per CU at that size); else its blocks are gathered into the reduced alignment as before.
inline bool red_cls_direct(size_t lds_cls, size_t lds_limit, uint32_t resident_rows, uint32_t resident_cls)
{
	return lds_cls <= lds_limit && resident_cls >= 1u && resident_cls >= resident_rows;
}

struct RedPlanInput {
	uint32_t m = 0, nblocks = 0;
	uint32_t b_lo = 0, b_hi = 0;             // my blocks (a rank of a sharded run; else all)
	std::vector<uint32_t> cnt;               // [nblocks] representatives of a block of mine (RED_NONE: not reduced)
	std::vector<uint8_t> force;              // [nblocks] 0, or what an earlier run on this input found: RED_FORCE_FULL -- the block's lists could not be proven on
	                                         // its representatives --, RED_FORCE_WIDE -- the block stays reduced but skips the slim configuration, which refused it
	std::vector<RedConfig> configs;          // ascending by the rows they hold
	bool reduced_always = false;             // FSEQ_REDUCED_ALWAYS: the representatives whenever some block has fewer of them than rows
	bool no_block_list = false;              // the first form of the streamed kernel runs the blocks on all rows: it takes no block list
};

enum class RedVerdict {
	Use,                                     // phase C by this plan
	Declined,                                // the representatives do not pay: the attempt takes the run on all rows with its stride states
	NoBlockList                              // some block would run on all rows, and the kernel on all rows takes no block list
};

struct RedBin { int config; uint32_t first, count; };     // blocks[first, first + count) run on configuration `config`

struct RedPlan {
	RedVerdict verdict = RedVerdict::Declined;
	std::vector<uint32_t> cnt;               // [block] representatives (RED_NONE: not reduced, or not a block of mine)
	std::vector<uint8_t> full;               // [block] 1: phase C runs the block on all rows
	std::vector<int> config_of;              // [block] configuration of a reduced block's phase C (-1: none)
	std::vector<int> config_snap_of;         // ... and of its sweeps in pass 2 (no lists: no list wave); also for a block that is `full`
	// [r10] [block] 1: the block's columns are staged from phase A's class columns where it has them -- every configuration it runs on
	// (phase C's unless `full`, pass 2's) takes the class width: the same source in both, the reduced stride states are in its ids;
	// gathered: listed blocks without it (the reduced alignment is needed for them)
	std::vector<uint8_t> from_cls;
	uint32_t gathered = 0;
	// what goes to d_red_blocks: [0, listed) every block with a count, ascending; then the configurations in use in ascending
	// index, each with its blocks ascending (bins); then [full_at, full_at + nfull) the blocks on all rows, ascending
	std::vector<uint32_t> blocks;
	std::vector<RedBin> bins;
	uint32_t full_at = 0, nfull = 0;
	uint32_t listed = 0, max_rows = 0;       // max_rows: the most representatives among the listed blocks
	uint32_t reduced_blocks = 0, rows_mean = 0;      // blocks in the bins; the mean of their counts
};

inline RedPlan plan_reduced(RedPlanInput const &in)
{
	RedPlan P;
	uint32_t const nbk = in.nblocks, m = in.m, my_blocks = in.b_hi - in.b_lo;
	size_t const nconf = in.configs.size();
	P.cnt.assign(nbk, RED_NONE);
	std::copy(in.cnt.begin() + in.b_lo, in.cnt.begin() + in.b_hi, P.cnt.begin() + in.b_lo);
	P.full.assign(nbk, 0);
	P.config_of.assign(nbk, -1);
	P.config_snap_of.assign(nbk, -1);
	P.from_cls.assign(nbk, 0);
	std::vector<uint8_t> usable(nconf), usable_snap(nconf);
	for (size_t i = 0; i < nconf; ++i)
	{
		RedConfig const &rs = in.configs[i];
		// (small blocks: one-wave workgroups for both; from 256 threads on phase C takes the configurations with a list wave,
		// pass 2's sweeps the others)
		usable[i] = rs.fits && (rs.T <= 128u || rs.ew);
		usable_snap[i] = rs.fits && !rs.ew;
	}
	std::vector<std::vector<uint32_t>> per(nconf);
	uint32_t n_full = 0;
	uint64_t sum_rows = 0;
	for (uint32_t b = in.b_lo; b < in.b_hi; ++b)
	{
		uint32_t const r = P.cnt[b];
		if (r != RED_NONE)
		{
			P.blocks.push_back(b);
			P.max_rows = std::max(P.max_rows, r);
			int cf = -1, cs = -1;
			// (a block the slim configuration refused -- more distinct start values than its table holds -- skips it)
			bool const wide = in.force[b] == RED_FORCE_WIDE;
			for (size_t i = 0; i < nconf; ++i) if (usable[i] && in.configs[i].rows >= r && !(wide && in.configs[i].values < in.configs[i].rows)) { cf = (int) i; break; }
			for (size_t i = 0; i < nconf; ++i) if (usable_snap[i] && in.configs[i].rows >= r) { cs = (int) i; break; }
			P.config_of[b] = cf;
			P.config_snap_of[b] = cs;
		}
		bool const full = r == RED_NONE || P.config_of[b] < 0 || in.force[b] == RED_FORCE_FULL || (uint64_t) r * 10u > (uint64_t) m * 7u;
		if (full) { P.full[b] = 1; ++n_full; }
		else { per[(size_t) P.config_of[b]].push_back(b); sum_rows += r; }
		if (r != RED_NONE)
		{
			bool const c_ok = full || in.configs[(size_t) P.config_of[b]].cls;
			bool const s_ok = P.config_snap_of[b] < 0 || in.configs[(size_t) P.config_snap_of[b]].cls;
			// (a block no configuration sweeps is read by nobody)
			P.from_cls[b] = (c_ok && s_ok && !(full && P.config_snap_of[b] < 0)) ? 1 : 0;
			if (!P.from_cls[b] && !(full && P.config_snap_of[b] < 0)) ++P.gathered;
		}
	}
	P.listed = (uint32_t) P.blocks.size();
	P.reduced_blocks = my_blocks - n_full;
	P.rows_mean = my_blocks > n_full ? (uint32_t) (sum_rows / (my_blocks - n_full)) : 0u;
	for (size_t i = 0; i < nconf; ++i)
	{
		auto const &v = per[i];
		if (v.empty()) continue;
		P.bins.push_back(RedBin{(int) i, (uint32_t) P.blocks.size(), (uint32_t) v.size()});
		P.blocks.insert(P.blocks.end(), v.begin(), v.end());
	}
	P.full_at = (uint32_t) P.blocks.size();
	for (uint32_t b = in.b_lo; b < in.b_hi; ++b) if (P.full[b]) P.blocks.push_back(b);
	P.nfull = n_full;
	// worth it?  The run on all rows is the tuned one (three workgroups per CU, stride states for pass 2), and a row of a small
	// reduced workgroup costs more than a row there: the representatives take over where they are clearly fewer -- rows to
	// update in all, a block on all rows counted as one and a half (its boundaries are reached from the block's start) -- below
	// a fifth of the rows (BASELINE C3 / C4 / C5: 8 / 7 / 6 %; C3's shape with ten times the mutations, 40 %: 11.4 ms against
	// 9.4 on all rows, tools/diversity_sweep.py; FSEQ_REDUCED_ALWAYS: tests)
	uint64_t const rows_all = sum_rows + (uint64_t) n_full * m * 3u / 2u;
	if ((!in.reduced_always && (rows_all * 5u > (uint64_t) my_blocks * m || (uint64_t) n_full * 4u > my_blocks)) || (uint64_t) n_full >= my_blocks)
		P.verdict = RedVerdict::Declined;
	else if (n_full && in.no_block_list)
		P.verdict = RedVerdict::NoBlockList;
	else
		P.verdict = RedVerdict::Use;
	return P;
}

} // namespace fseq
