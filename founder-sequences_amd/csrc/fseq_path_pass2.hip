// fseq_path_pass2.hip -- the segmentation path, pass 2: the (a, d) states at the merged boundaries, behind phase C on all rows
// (from the stride states) or behind the reduced phase C (one chain step from the block's boundary state).  It launches through
// KernelSet, Stream2Config, ChainSnapSet and the launchers of fseq_path_pass1.hip and fseq_path_reduced.hip, which all take the boundaries as one SnapArgs.
// (The units of the path and what crosses them: fseq_path.hpp.)
#include "fseq_path.hpp"
#include "fseq_stream2.hpp"      // (no name of it is used here since the launchers take SnapArgs; kept so that the unit's device code stays what it was)

namespace fseq {

namespace {

// sharded: R of SURVEY.md 8(d) is the sum of pass 2's cells over the ranks (one slot pair per rank); the run's last exchange
int pass2_sum_cells(fseq_ctx *c, LongRun &R, hipStream_t st)
{
	Shard const &sh = c->sh;
	if (!sh.on) return FSEQ_OK;
	uint32_t slots[2] = {(uint32_t) R.pass2_cells, (uint32_t) (R.pass2_cells >> 32)};
	std::vector<uint32_t> all(2 * sh.world);
	HIP_TRY(c, hipMemsetAsync(sh.xbuf, 0, all.size() * 4, st));
	HIP_TRY(c, hipMemcpyAsync(sh.xbuf + 2 * sh.rank, slots, 8, hipMemcpyHostToDevice, st));
	int rc;
	if ((rc = shard_exchange(c, all.size(), 0))) return rc;
	HIP_TRY(c, hipMemcpy(all.data(), sh.xbuf, all.size() * 4, hipMemcpyDeviceToHost));
	R.pass2_cells = 0;
	for (uint32_t g = 0; g < sh.world; ++g) R.pass2_cells += (uint64_t) all[2 * g] | ((uint64_t) all[2 * g + 1] << 32);
	c->sh.closed = true;
	return FSEQ_OK;
}

// ---- the sweeps' tasks (long_pass2_reduced below and fseq_debug_class_tables): a workgroup sweeps the tasks of one block that share a
// start column, on the configuration the plan sweeps the block with
struct SweepWg { uint32_t blk, first, count, start; };

// task i, column rb strictly inside block blk: onto the last workgroup of its configuration or a new one (the tasks come in ascending
// columns).  false: no configuration sweeps the block (it has no representatives)
bool sweep_add_task(fseq_ctx const *c, std::vector<std::vector<SweepWg>> &wgs, uint32_t blk, uint64_t rb, uint32_t i)
{
	RedPlan const &plan = c->red.plan;
	int const cf = blk < plan.config_snap_of.size() ? plan.config_snap_of[blk] : -1;
	if (cf < 0 || plan.cnt[blk] == RED_NONE) return false;
	// the sweep starts at the last state phase C dropped in front of the boundary (or at the block's first column)
	uint64_t start = c->red_ss_stride ? (rb - 1u) / c->red_ss_stride * c->red_ss_stride : 0u;
	// (a block that ran on all rows dropped none)
	if (start <= (uint64_t) blk * c->B || plan.full[blk]) start = (uint64_t) blk * c->B;
	auto &v = wgs[(size_t) cf];
	if (!v.empty() && v.back().blk == blk && v.back().start == (uint32_t) start) ++v.back().count;
	else v.push_back(SweepWg{blk, i, 1u, (uint32_t) start});
	return true;
}

// the launches of the configurations in use and what their workgroups read: hb[w] the block, hw[3 w ..] {first task, tasks, start column}
void sweep_launch_lists(std::vector<std::vector<SweepWg>> const &wgs, std::vector<RedLaunch> &ls, std::vector<uint32_t> &hb, std::vector<uint32_t> &hw)
{
	for (size_t cf = 0; cf < wgs.size(); ++cf)
	{
		if (wgs[cf].empty()) continue;
		ls.push_back(RedLaunch{(int) cf, (uint32_t) hb.size(), (uint32_t) wgs[cf].size()});
		for (auto const &w : wgs[cf]) { hb.push_back(w.blk); hw.push_back(w.first); hw.push_back(w.count); hw.push_back(w.start); }
	}
}

// the class tables at the task columns, configuration by configuration (RA: the tasks and the tables set by the caller)
int sweep_class_tables(fseq_ctx *c, std::vector<RedLaunch> ls, RedArgs const &RA)
{
	if (ls.empty()) return FSEQ_OK;
	std::stable_sort(ls.begin(), ls.end(), [](RedLaunch const &x, RedLaunch const &y) { return x.count > y.count; });
	return red_launch_all(c, ls, RA, ListArgs{(uint32_t) c->p.segment_length});       // (no lists: the segment length alone)
}

// ---- [r5] pass 2 behind the reduced phase C: a boundary inside a block is ONE chain step from the block's boundary state
// (k_chain_snap), keyed by the classes the block's representatives form at that column (k_columns_red with the class
// tables as its output); a boundary on a block border is that border's state.  Blocks without representatives (more than a
// configuration holds) replay their columns on all rows from the block's start (k_colblock<MODE_SNAP>).
int long_pass2_reduced(fseq_ctx *c, LongRun &R)
{
	FSEQ_LONG_LOCALS(c);
	size_t const S2all = c->segments.size();
	if (!S2all) return FSEQ_OK;
	RedPlan const &plan = c->red.plan;
	ChainSnapSet cs{};
	if (!c->use_stream)
	{
		if (!select_chain_snap(ks.T, ks.E, &cs)) return fail(c, FSEQ_E_UNSUPPORTED, "pass 2: no chain step for this configuration");
		HIP_TRY(c, cs.prepare());
	}
	c->snap_slot.assign(S2all, -1);
	// my tasks (sharded: a boundary belongs to the rank whose blocks hold the state in front of it), in the order of the boundaries
	std::vector<uint64_t> rbs;
	std::vector<uint32_t> task_blk, ncls0;
	// tasks of reduced blocks by configuration: workgroups {block, first task, count, start column}; tasks of the other blocks: old groups
	std::vector<std::vector<SweepWg>> wgs((size_t) reduced_config_count());
	std::vector<uint64_t> o_rbs, o_srcs;
	std::vector<uint2> o_grp;
	std::vector<uint32_t> o_slot;
	uint64_t cells = 0;
	for (size_t si = 0; si < S2all; ++si)
	{
		uint64_t const rb = c->segments[si].rb;
		if (sharded)
		{
			uint32_t const owner = (uint32_t) std::min<uint64_t>(rb / ((uint64_t) sh.bpr * c->B), sh.active - 1u);
			if (owner != sh.rank) continue;
		}
		size_t const i = rbs.size();
		c->snap_slot[si] = (int64_t) i;
		rbs.push_back(rb);
		bool const border = rb % c->B == 0;
		uint32_t const blk = border ? (uint32_t) (rb / c->B) : (uint32_t) std::min<uint64_t>(rb / c->B, c->nblocks - 1u);
		task_blk.push_back(blk);
		ncls0.push_back(0u);                                       // a border: the copy; else the sweep fills it in
		if (border) continue;
		if (!sweep_add_task(c, wgs, blk, rb, (uint32_t) i))
		{
			ncls0[i] = 0xFFFFFFFFu;                                // not this kernel's
			if (!o_srcs.empty() && o_srcs.back() == blk) ++o_grp.back().y;
			else { o_grp.push_back(make_uint2((uint32_t) o_rbs.size(), 1u)); o_srcs.push_back(blk); }
			o_rbs.push_back(rb); o_slot.push_back((uint32_t) i);
		}
	}
	size_t const S2 = rbs.size();
	if (!S2) { R.pass2_cells = 0; return pass2_sum_cells(c, R, st); }
	if ((rc = c->d_snap_a.ensure(c, S2 * (size_t) m))) return rc;
	if ((rc = c->d_snap_d.ensure(c, S2 * (size_t) m))) return rc;
	if ((rc = c->d_red_cls.ensure(c, S2 * (size_t) c->red_cap))) return rc;
	if ((rc = c->d_red_headd.ensure(c, S2 * (size_t) c->red_cap))) return rc;
	if ((rc = c->d_red_ncls.ensure(c, S2))) return rc;
	if ((rc = c->d_red_taskblk.ensure(c, S2))) return rc;
	if ((rc = c->d_red_wgtasks.ensure(c, 4 * S2 + 64))) return rc;
	if ((rc = c->d_red_p2grp.ensure(c, 2 * S2 + 2 + P2_STATS + P2_HAND))) return rc;
	if ((rc = c->d_cols.ensure(c, S2))) return rc;
	// streamed rows: the groups of the chain-step kernel, a block's tasks each (blocks with tasks of that kernel only), the
	// largest first, and behind them the counter the workgroups take them by
	std::vector<uint32_t> p2grp;
	if (c->use_stream)
	{
		std::vector<uint2> g;
		for (size_t i = 0; i < S2; ++i)
		{
			if (i == 0 || task_blk[i] != task_blk[i - 1]) g.push_back(make_uint2((uint32_t) i, 0u));
			++g.back().y;
		}
		size_t k = 0;
		for (auto const &x : g)
		{
			bool mine = false;
			for (uint32_t t = x.x; t < x.x + x.y; ++t) mine = mine || ncls0[t] == 0u;
			if (mine) g[k++] = x;
		}
		g.resize(k);
		std::stable_sort(g.begin(), g.end(), [](uint2 const &x, uint2 const &y) { return x.y > y.y; });
		for (auto const &x : g) { p2grp.push_back(x.x); p2grp.push_back(x.y); }
		p2grp.push_back(0u);
		p2grp.insert(p2grp.end(), P2_STATS + P2_HAND, 0u);                   // (the kernel's counters, zeroed with the counter)
	}
	// the task lists through pinned memory of their own (live until the synchronisation behind the kernels)
	std::vector<uint32_t> hb, hw;
	std::vector<RedLaunch> ls;
	sweep_launch_lists(wgs, ls, hb, hw);
	for (size_t cf = 0; cf < wgs.size(); ++cf)
	{
		if (wgs[cf].empty()) continue;
		for (auto const &w : wgs[cf]) cells += (rbs[w.first + w.count - 1u] - (uint64_t) w.start) * plan.cnt[w.blk];
		if (c->tune.debug)
		{
			// (worded like red_plan's report of phase C; a workgroup sweeps one block's tasks that share a start column)
			ReducedSet rs{};
			(void) reduced_config((int) cf, &rs);
			uint32_t tasks = 0;
			for (auto const &w : wgs[cf]) tasks += w.count;
			fprintf(stderr, "[fseq]   reduced pass 2: configuration of %u rows: %zu workgroups, %u tasks in blocks %u to %u (%u threads x %u rows)\n", rs.rows, wgs[cf].size(), tasks,
			        wgs[cf].front().blk, wgs[cf].back().blk, rs.T, rs.E);
		}
	}
	{
		size_t const need = S2 * 16 + hb.size() * 16 + p2grp.size() * 4 + 256 + (P2_STATS + P2_HAND) * 4;
		if (c->red_pin2_bytes < need)
		{
			if (c->h_red_pin2) (void) hipHostFree(c->h_red_pin2);
			c->h_red_pin2 = nullptr; c->red_pin2_bytes = 0;
			HIP_TRY(c, hipHostMalloc(reinterpret_cast<void **>(&c->h_red_pin2), need * 2, hipHostMallocDefault));
			c->red_pin2_bytes = need * 2;
		}
		uint8_t *pp = c->h_red_pin2;
		auto put = [&](void const *src, size_t bytes) { void *at = pp; memcpy(pp, src, bytes); pp += (bytes + 15) & ~size_t(15); return at; };
		HIP_TRY(c, hipMemcpyAsync(c->d_cols, put(rbs.data(), S2 * 8), S2 * 8, hipMemcpyHostToDevice, st));
		HIP_TRY(c, hipMemcpyAsync(c->d_red_taskblk, put(task_blk.data(), S2 * 4), S2 * 4, hipMemcpyHostToDevice, st));
		HIP_TRY(c, hipMemcpyAsync(c->d_red_ncls, put(ncls0.data(), S2 * 4), S2 * 4, hipMemcpyHostToDevice, st));
		if (!p2grp.empty())
			HIP_TRY(c, hipMemcpyAsync(c->d_red_p2grp, put(p2grp.data(), p2grp.size() * 4), p2grp.size() * 4, hipMemcpyHostToDevice, st));
		if (!hb.empty())
		{
			HIP_TRY(c, hipMemcpyAsync(c->d_red_wgtasks + 3 * S2, put(hb.data(), hb.size() * 4), hb.size() * 4, hipMemcpyHostToDevice, st));
			HIP_TRY(c, hipMemcpyAsync(c->d_red_wgtasks, put(hw.data(), hw.size() * 4), hw.size() * 4, hipMemcpyHostToDevice, st));
		}
	}
	uint32_t *const pin_stats = reinterpret_cast<uint32_t *>(c->h_red_pin2 + c->red_pin2_bytes - (P2_STATS + P2_HAND) * 4);      // (behind the task lists)
	c->p2_stats_have = false; c->p2_groups = 0;
	HIP_TRY(c, hipEventRecord(c->ev.pass2_begin, st));
	progress(c, FSEQ_STAGE_SAMPLES, 0, S2);
	RangeScope range_p2("fseq pass 2: boundary states (update_pbwt_task)");
	// the class tables at the task columns, configuration by configuration
	RedArgs RA;
	red_fill_args(c, RA);
	RA.task_rb = c->d_cols.as<unsigned long long const>();
	RA.cls = c->d_red_cls; RA.headd = c->d_red_headd; RA.ncls = c->d_red_ncls;
	RA.blocks = c->d_red_wgtasks + 3 * S2; RA.wg_tasks = c->d_red_wgtasks;
	if ((rc = sweep_class_tables(c, ls, RA))) return rc;
	// the states at my boundaries, from the blocks' boundary states
	SnapArgs tasks;
	tasks.A = msa_args(c);
	tasks.bstate_a = c->d_bstate_a; tasks.bstate_d = c->d_bstate_d; tasks.task_blk = c->d_red_taskblk;
	tasks.snap_a = c->d_snap_a; tasks.snap_d = c->d_snap_d; tasks.ss.snap_stride = c->snap_stride; tasks.keyed = scan_keyed(c);
	// one chain step per boundary (a copy for the borders)
	if (!c->use_stream)
		cs.launch(st, (uint32_t) S2, cs.lds, tasks, RA);
	else
	{
		// streamed rows: a block's tasks on one workgroup, the groups taken from a counter
		uint32_t const ngrp = (uint32_t) ((p2grp.size() - 1 - P2_STATS - P2_HAND) / 2);
		if (ngrp)
		{
			uint32_t *const stats = c->d_red_p2grp + 2 * (size_t) ngrp + 1;
			if ((rc = launch_chain_snap_grouped(c, ngrp, stats))) return rc;
			// (its counters come back with the synchronisation behind pass 2)
			HIP_TRY(c, hipMemcpyAsync(pin_stats, stats, (P2_STATS + P2_HAND) * 4, hipMemcpyDeviceToHost, st));
			c->p2_stats_have = true; c->p2_groups = ngrp;
		}
	}
	for (size_t i = 0; i < S2; ++i)
		if (ncls0[i] == 0u && rbs[i] % c->B != 0) cells += (uint64_t) m * 4u;      // (a step is ~4 digit passes over the rows)
	// the boundaries of blocks without representatives: their columns on all rows from the block's start
	if (!o_grp.empty())
	{
		size_t const So = o_rbs.size();
		DevTemp<uint32_t> tmp_a(c), tmp_d(c);
		DevTemp<uint64_t> d_orb(c), d_osrc(c);
		DevTemp<uint2> d_ogrp(c);
		if ((rc = tmp_a.alloc(So * (size_t) m)) || (rc = tmp_d.alloc(So * (size_t) m)) ||
		    (rc = d_orb.alloc(So)) || (rc = d_osrc.alloc(o_srcs.size())) || (rc = d_ogrp.alloc(o_grp.size()))) return rc;
		HIP_TRY(c, hipMemcpyAsync(d_orb, o_rbs.data(), So * 8, hipMemcpyHostToDevice, st));
		HIP_TRY(c, hipMemcpyAsync(d_osrc, o_srcs.data(), o_srcs.size() * 8, hipMemcpyHostToDevice, st));
		HIP_TRY(c, hipMemcpyAsync(d_ogrp, o_grp.data(), o_grp.size() * sizeof(uint2), hipMemcpyHostToDevice, st));
		// (from the blocks' start states: no stride states here)
		tasks.task_rb = d_orb; tasks.task_grp = d_ogrp; tasks.task_src = d_osrc; tasks.snap_a = tmp_a; tasks.snap_d = tmp_d;
		if (!c->use_stream) ks.snap(st, (uint32_t) o_grp.size(), ks.lds_snap, tasks);
		else launch_replay_stream(c, o_grp.size(), tasks);
		for (size_t j = 0; j < So; ++j)
		{
			HIP_TRY(c, hipMemcpyAsync(c->d_snap_a + (size_t) o_slot[j] * m, tmp_a + j * (size_t) m, (size_t) m * 4, hipMemcpyDeviceToDevice, st));
			HIP_TRY(c, hipMemcpyAsync(c->d_snap_d + (size_t) o_slot[j] * m, tmp_d + j * (size_t) m, (size_t) m * 4, hipMemcpyDeviceToDevice, st));
		}
		for (size_t g = 0; g < o_grp.size(); ++g) cells += (o_rbs[o_grp[g].x + o_grp[g].y - 1] - o_srcs[g] * c->B) * m;
		HIP_TRY(c, hipStreamSynchronize(st));
	}
	HIP_TRY(c, hipEventRecord(c->ev.pass2_end, st));
	HIP_TRY(c, hipGetLastError());
	HIP_TRY(c, hipStreamSynchronize(st));
	range_p2.end();
	if (c->p2_stats_have)
	{
		memcpy(c->p2_stats, pin_stats, sizeof(c->p2_stats));
		memcpy(c->p2_hand, pin_stats + P2_STATS, sizeof(c->p2_hand));
		if (c->tune.debug) fprintf(stderr, "[fseq] pass 2 chain steps: %u groups took the keys phase B handed over, %u gathered their own\n", c->p2_hand[0], c->p2_hand[1]);
	}
	progress(c, FSEQ_STAGE_SAMPLES, S2, S2);
	float f = 0;
	HIP_TRY(c, hipEventElapsedTime(&f, c->ev.pass2_begin, c->ev.pass2_end)); R.ms_p2 = f;
	R.pass2_cells = cells;
	return pass2_sum_cells(c, R, st);
}

} // namespace

// ---- pass 2: (a, d) at the merged boundaries
int long_pass2(fseq_ctx *c, LongRun &R)
{
	FSEQ_LONG_LOCALS(c);
	c->p2_stats_have = false;
	if (c->red_active) return long_pass2_reduced(c, R);
	uint64_t &pass2_cells = R.pass2_cells;
	double &ms_p2 = R.ms_p2;
	size_t const S2 = c->segments.size();
	// ---- pass 2: (a,d) at the merged boundaries (update_pbwt_task.cc:13-35)
	if (S2)
	{
		if ((rc = c->d_cols.ensure(c, S2))) return rc;
		// every boundary starts from the nearest exact state at or below it: a block boundary state
		// (phase B) or one of the states phase C dropped every snap_stride columns; boundaries that share
		// a start state share one sweep (boundaries ascending)
		// sharded: a boundary belongs to the rank whose blocks hold the state in front of it
		std::vector<uint64_t> rbs, srcs;
		std::vector<uint2> grp;
		uint64_t const sstr = c->snap_stride;
		std::vector<uint64_t> starts;
		std::vector<uint32_t> grp_blk;                            // block whose columns a group replays
		c->snap_slot.assign(S2, -1);
		for (size_t i = 0; i < S2; ++i)
		{
			uint64_t const rb = c->segments[i].rb;
			if (sharded)
			{
				uint32_t const owner = (uint32_t) std::min<uint64_t>(rb / ((uint64_t) sh.bpr * c->B), sh.active - 1u);
				if (owner != sh.rank) continue;
			}
			c->snap_slot[i] = (int64_t) rbs.size();
			rbs.push_back(rb);
			// (states in id form belong to the block that made them: the boundary behind the last column starts inside the last block)
			uint64_t const blk = std::min<uint64_t>(rb / c->B, c->ss_ids ? c->nblocks - 1u : c->nblocks);
			uint64_t const q = rb / sstr;
			uint64_t src = blk, p0 = blk * c->B;
			if (c->d_ss_a && q >= 1 && q * sstr > p0) { src = q | (1ull << 63); p0 = q * sstr; }
			if (grp.empty() || srcs.back() != src) { grp.push_back(make_uint2((uint32_t) (rbs.size() - 1), 1u)); srcs.push_back(src); starts.push_back(p0); grp_blk.push_back((uint32_t) blk); }
			else ++grp.back().y;
		}
		for (size_t g = 0; g < grp.size(); ++g)
			pass2_cells += (rbs[grp[g].x + grp[g].y - 1] - starts[g]) * m;
		size_t const S2m = rbs.size();                            // boundaries that are mine (all of them when not sharded)
		if ((rc = c->d_snap_a.ensure(c, S2m * (size_t) m))) return rc;
		if ((rc = c->d_snap_d.ensure(c, S2m * (size_t) m))) return rc;
		if ((rc = c->d_src.ensure(c, srcs.size()))) return rc;
		if ((rc = c->d_grp.ensure(c, grp.size()))) return rc;
		{
			// (through the pinned stage: it stays untouched until the synchronisation behind the kernel)
			if ((rc = pin_reserve(c, (srcs.size() + S2m + grp.size()) * 8 + 256))) return rc;
			uint64_t *const psrc = pin_take<uint64_t>(c, srcs.size());
			uint64_t *const prb = pin_take<uint64_t>(c, S2m);
			uint2 *const pgrp = pin_take<uint2>(c, grp.size());
			std::copy(srcs.begin(), srcs.end(), psrc);
			std::copy(rbs.begin(), rbs.end(), prb);
			std::copy(grp.begin(), grp.end(), pgrp);
			if (!srcs.empty()) HIP_TRY(c, hipMemcpyAsync(c->d_src, psrc, srcs.size() * 8, hipMemcpyHostToDevice, st));
			if (S2m) HIP_TRY(c, hipMemcpyAsync(c->d_cols, prb, S2m * 8, hipMemcpyHostToDevice, st));
			if (!grp.empty()) HIP_TRY(c, hipMemcpyAsync(c->d_grp, pgrp, grp.size() * sizeof(uint2), hipMemcpyHostToDevice, st));
		}
		HIP_TRY(c, hipEventRecord(c->ev.pass2_begin, st));
		progress(c, FSEQ_STAGE_SAMPLES, 0, S2);
		RangeScope range_p2("fseq pass 2: boundary states (update_pbwt_task)");
		// the states at my boundaries, every group swept from its block's boundary state or a stride state
		SnapArgs tasks;
		tasks.A = msa_args(c);
		tasks.bstate_a = c->d_bstate_a; tasks.bstate_d = c->d_bstate_d; tasks.task_rb = c->d_cols; tasks.task_grp = c->d_grp; tasks.task_src = c->d_src;
		tasks.snap_a = c->d_snap_a; tasks.snap_d = c->d_snap_d; tasks.ss = stride_states(c); tasks.keyed = scan_keyed(c);
		if (!grp.empty() && c->use_stream && c->ss_ids)
		{
			// pass 2 on phase C's tile step (fseq_stream2.hpp, S2_SNAP): one workgroup per block that has boundaries, the block's
			// groups one after the other in the block's own workspace (where V and D0 of its id space still are)
			std::vector<uint32_t> wgb;
			std::vector<uint2> wgg;
			std::vector<uint64_t> wgw;                             // columns a workgroup replays
			for (size_t g = 0; g < grp.size(); ++g)
			{
				if (wgb.empty() || wgb.back() != grp_blk[g]) { wgb.push_back(grp_blk[g]); wgg.push_back(make_uint2((uint32_t) g, 1u)); wgw.push_back(0); }
				else ++wgg.back().y;
				wgw.back() += rbs[grp[g].x + grp[g].y - 1] - starts[g] + 2;      // (+ the loads of the start state and the snapshots)
			}
			{
				// the longest first: the workgroups are handed out in launch order, and a long one at the end would run alone
				std::vector<uint32_t> order(wgb.size());
				for (uint32_t i = 0; i < order.size(); ++i) order[i] = i;
				std::stable_sort(order.begin(), order.end(), [&](uint32_t x, uint32_t y) { return wgw[x] > wgw[y]; });
				std::vector<uint32_t> b2(wgb.size());
				std::vector<uint2> g2(wgg.size());
				for (size_t i = 0; i < order.size(); ++i) { b2[i] = wgb[order[i]]; g2[i] = wgg[order[i]]; }
				wgb.swap(b2); wgg.swap(g2);
			}
			if ((rc = c->d_wgblk.ensure(c, wgb.size()))) return rc;
			if ((rc = c->d_wggrp.ensure(c, wgb.size()))) return rc;
			// (pageable sources: the runtime stages them before the call returns)
			HIP_TRY(c, hipMemcpyAsync(c->d_wgblk, wgb.data(), wgb.size() * 4, hipMemcpyHostToDevice, st));
			HIP_TRY(c, hipMemcpyAsync(c->d_wggrp, wgg.data(), wgg.size() * sizeof(uint2), hipMemcpyHostToDevice, st));
			tasks.ws = c->d_ws; tasks.wg_block = c->d_wgblk; tasks.wg_groups = c->d_wggrp; tasks.bs_w = c->d_bs_w; tasks.bs_h = c->d_bs_h;
			c->s2.launch_snap(st, (uint32_t) wgb.size(), c->s2_lds, tasks);
			HIP_TRY(c, hipStreamSynchronize(st));                 // (wgb / wgg must outlive their copies)
		}
		else if (c->use_stream) launch_replay_stream(c, grp.size(), tasks);
		else if (!grp.empty()) ks.snap(st, (uint32_t) grp.size(), ks.lds_snap, tasks);
		HIP_TRY(c, hipEventRecord(c->ev.pass2_end, st));
		HIP_TRY(c, hipGetLastError());
		HIP_TRY(c, hipStreamSynchronize(st));
		range_p2.end();
		progress(c, FSEQ_STAGE_SAMPLES, S2, S2);
		float f = 0;
		HIP_TRY(c, hipEventElapsedTime(&f, c->ev.pass2_begin, c->ev.pass2_end)); ms_p2 = f;
		if ((rc = pass2_sum_cells(c, R, st))) return rc;
	}

	return FSEQ_OK;
}

} // namespace fseq

using namespace fseq;

extern "C" {

// pass 2's sweeps at caller-chosen columns of the last run (include/fseq_debug.h): the same task construction and launches as
// long_pass2_reduced, on buffers of this call's own
int fseq_debug_class_tables(fseq_ctx *c, uint64_t const *columns, uint32_t count, uint32_t *cls, uint32_t *headd, uint32_t *ncls)
{
	if (!c || !columns || !count || !cls || !headd || !ncls) return FSEQ_E_ARG;
	if (int const rc0 = need_result(c, true)) return rc0;
	if (!c->red_active || c->sh.on) return fail(c, FSEQ_E_UNSUPPORTED, "class tables: the last run did not go through the representatives on one rank");
	FSEQ_LONG_LOCALS(c);
	(void) hipSetDevice(p.device);
	uint32_t const cap = c->red_cap;
	std::vector<std::vector<SweepWg>> wgs((size_t) reduced_config_count());
	std::vector<uint32_t> task_blk(count);
	for (uint32_t i = 0; i < count; ++i)
	{
		uint64_t const rb = columns[i];
		if (rb == 0 || rb >= n || rb % c->B == 0 || (i && rb <= columns[i - 1])) return fail(c, FSEQ_E_ARG, "class tables: ascending columns strictly inside blocks");
		task_blk[i] = (uint32_t) (rb / c->B);
		if (!sweep_add_task(c, wgs, task_blk[i], rb, i)) return fail(c, FSEQ_E_UNSUPPORTED, "class tables: a column of a block without representatives");
	}
	std::vector<RedLaunch> ls;
	std::vector<uint32_t> hb, hw;
	sweep_launch_lists(wgs, ls, hb, hw);
	DevTemp<uint64_t> d_rb(c);
	DevTemp<uint32_t> d_wg(c), d_blk(c), d_cls(c), d_headd(c), d_ncls(c);
	if ((rc = d_rb.alloc(count)) || (rc = d_wg.alloc(hw.size())) || (rc = d_blk.alloc(hb.size())) || (rc = d_cls.alloc((size_t) count * cap)) ||
	    (rc = d_headd.alloc((size_t) count * cap)) || (rc = d_ncls.alloc(count))) return rc;
	HIP_TRY(c, hipMemcpyAsync(d_rb, columns, (size_t) count * 8, hipMemcpyHostToDevice, st));
	HIP_TRY(c, hipMemcpyAsync(d_wg, hw.data(), hw.size() * 4, hipMemcpyHostToDevice, st));
	HIP_TRY(c, hipMemcpyAsync(d_blk, hb.data(), hb.size() * 4, hipMemcpyHostToDevice, st));
	HIP_TRY(c, hipMemsetAsync(d_cls, 0xFF, (size_t) count * cap * 4, st));
	HIP_TRY(c, hipMemsetAsync(d_headd, 0xFF, (size_t) count * cap * 4, st));
	HIP_TRY(c, hipMemsetAsync(d_ncls, 0, (size_t) count * 4, st));
	HIP_TRY(c, hipStreamSynchronize(st));                         // (the lists are pageable memory of this call)
	RedArgs RA;
	red_fill_args(c, RA);
	RA.task_rb = d_rb.as<unsigned long long const>();
	RA.cls = d_cls; RA.headd = d_headd; RA.ncls = d_ncls;
	RA.blocks = d_blk; RA.wg_tasks = d_wg;
	if ((rc = sweep_class_tables(c, ls, RA))) return rc;
	HIP_TRY(c, hipStreamSynchronize(st));
	// by rows: the class of a row is the class of its block key (phase A's rank of the row in the block)
	std::vector<uint32_t> tab(cap), hd(cap), rank(m);
	HIP_TRY(c, hipMemcpy(ncls, d_ncls, (size_t) count * 4, hipMemcpyDeviceToHost));
	for (uint32_t i = 0; i < count; ++i)
	{
		if (i == 0 || task_blk[i] != task_blk[i - 1]) HIP_TRY(c, hipMemcpy(rank.data(), c->d_rank + (size_t) task_blk[i] * m, (size_t) m * 4, hipMemcpyDeviceToHost));
		HIP_TRY(c, hipMemcpy(tab.data(), d_cls + (size_t) i * cap, (size_t) cap * 4, hipMemcpyDeviceToHost));
		HIP_TRY(c, hipMemcpy(hd.data(), d_headd + (size_t) i * cap, (size_t) cap * 4, hipMemcpyDeviceToHost));
		for (uint32_t r = 0; r < m; ++r) cls[(size_t) i * m + r] = rank[r] < cap ? tab[rank[r]] : 0xFFFFFFFFu;
		for (uint32_t r = 0; r < m; ++r) headd[(size_t) i * m + r] = r < cap ? hd[r] : 0xFFFFFFFFu;
	}
	return FSEQ_OK;
}

} // extern "C"
