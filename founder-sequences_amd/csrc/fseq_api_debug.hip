// fseq_api_debug.hip -- the entry points of include/fseq_debug.h (what the tests and tools look at behind a run; the
// range-minimum query's is with the DP, csrc/fseq_path_dp.hip) and the row-sharded conformance sweep of include/fseq.h.
// The one unit that includes fseq_rowshard.hpp.
#include "fseq_path.hpp"
#include "fseq_dp.hpp"           // the round schedule (fseq_debug_dp_schedule)
#include "fseq_rowshard.hpp"
#include "fseq_tbcheck.hpp"      // the chain a caller's lb array must hold (fseq_debug_merge_on_lists)

using namespace fseq;

namespace {

// one workgroup of the packed local pass (fseq_localpass.hpp, what partition_step's PL branch runs): thread t takes the
// positions [t * E, (t + 1) * E) and writes their new values and its four tail maxima
template <int E>
__global__ __launch_bounds__(1024) void k_local_pass_debug(uint32_t const *d_in, uint32_t const *s_in, uint32_t *dnew_out, uint32_t *tails_out)
{
	uint32_t const t = threadIdx.x;
	uint32_t d[E], s[E], dnew[E], run[4];
#pragma unroll
	for (int e = 0; e < E; ++e) { d[e] = d_in[t * E + e]; s[e] = s_in[t * E + e]; }
	local_pass_packed<E>(d, s, dnew, run);
#pragma unroll
	for (int e = 0; e < E; ++e) dnew_out[t * E + e] = dnew[e];
#pragma unroll
	for (int x = 0; x < 4; ++x) tails_out[t * 4 + x] = run[x];
}

} // namespace

extern "C" {

int fseq_debug_local_pass(int device, uint32_t threads, uint32_t rows_per_thread, uint32_t const *d, uint32_t const *s, uint32_t *dnew, uint32_t *tails)
{
	uint32_t const E = rows_per_thread;
	if (!d || !s || !dnew || !tails || threads == 0 || threads > 1024 || threads % 64 != 0 || (E != 11 && E != 12 && E != 15)) return FSEQ_E_ARG;
	size_t const n = (size_t) threads * E;
	// what the kernels guarantee the pass: values below 2^16, symbols 0 .. 4, an unused position (4) with the value 0
	for (size_t i = 0; i < n; ++i)
		if (d[i] > 0xFFFFu || s[i] > 4u || (s[i] == 4u && d[i] != 0u)) return FSEQ_E_ARG;
	if (hipSetDevice(device) != hipSuccess) return FSEQ_E_HIP;
	uint32_t *g_d = nullptr, *g_s = nullptr, *g_o = nullptr, *g_t = nullptr;
	int rc = FSEQ_E_HIP;
	do
	{
		if (hipMalloc((void **) &g_d, n * 4) != hipSuccess || hipMalloc((void **) &g_s, n * 4) != hipSuccess) break;
		if (hipMalloc((void **) &g_o, n * 4) != hipSuccess || hipMalloc((void **) &g_t, (size_t) threads * 16) != hipSuccess) break;
		if (hipMemcpy(g_d, d, n * 4, hipMemcpyHostToDevice) != hipSuccess || hipMemcpy(g_s, s, n * 4, hipMemcpyHostToDevice) != hipSuccess) break;
		if (E == 11) hipLaunchKernelGGL(k_local_pass_debug<11>, dim3(1), dim3(threads), 0, 0, g_d, g_s, g_o, g_t);
		else if (E == 12) hipLaunchKernelGGL(k_local_pass_debug<12>, dim3(1), dim3(threads), 0, 0, g_d, g_s, g_o, g_t);
		else hipLaunchKernelGGL(k_local_pass_debug<15>, dim3(1), dim3(threads), 0, 0, g_d, g_s, g_o, g_t);
		if (hipGetLastError() != hipSuccess || hipDeviceSynchronize() != hipSuccess) break;
		if (hipMemcpy(dnew, g_o, n * 4, hipMemcpyDeviceToHost) != hipSuccess || hipMemcpy(tails, g_t, (size_t) threads * 16, hipMemcpyDeviceToHost) != hipSuccess) break;
		rc = FSEQ_OK;
	} while (false);
	(void) hipFree(g_d); (void) hipFree(g_s); (void) hipFree(g_o); (void) hipFree(g_t);
	return rc;
}

int fseq_debug_set_tuning(fseq_ctx *c, char const *name, char const *value)
{
	if (!c || !name) return FSEQ_E_ARG;
	// sharded: the input was laid out for the block partition of the knobs in force when it was set, and every rank must
	// plan the same partition -- the knobs of a sharded run are set (identically on every rank) before the input
	if (c->sh.on && c->have_input) return fail(c, FSEQ_E_ARG, "sharded run: set tuning knobs before the input is set (identically on every rank)");
	if (!c->tune.set(name, value)) return fail(c, FSEQ_E_ARG, "unknown tuning knob");
	// (the scan's knob is read by fseq_scan_segment_lengths alone: no geometry, no kernel and no result depends on it)
	if (!strcmp(name, "FSEQ_SCAN_REBUILD")) return FSEQ_OK;
	// (... and the matcher's by the match entries alone: the run, its result and its buffers stay)
	if (!strcmp(name, "FSEQ_MATCH_SPLIT") || !strcmp(name, "FSEQ_MATCH_OVERLAP") || !strcmp(name, "FSEQ_MATCH_STAGE_BYTES")) return FSEQ_OK;
	// (... and the graph writer's by fseq_write_block_graph alone)
	if (!strcmp(name, "FSEQ_GRAPH_BATCH")) return FSEQ_OK;
	// (... and the key width of the graph threading by fseq_graph_thread_rows / fseq_graph_thread_held_out alone)
	if (!strcmp(name, "FSEQ_GRAPH_THREAD_KEY_BITS")) return FSEQ_OK;
	// (... and the batch of packed representatives by fseq_graph_nearest_rows / fseq_graph_nearest_held_out alone)
	if (!strcmp(name, "FSEQ_GRAPH_NEAREST_BATCH")) return FSEQ_OK;
	// (the geometry and the kernel choice may depend on it: the work buffers of an earlier run were sized for the old one)
	(void) hipSetDevice(c->p.device);
	if (c->stream) (void) hipStreamSynchronize(c->stream);
	free_work(c);
	// (what the last run saw belongs to the old geometry: a block the tree or the trie ranked then may be given up now)
	forget_run_history(c);
	return FSEQ_OK;
}

int fseq_debug_pass2_paths(fseq_ctx *c, uint32_t *by_runs, uint32_t *by_sort, uint32_t *copies, uint32_t *max_runs, uint32_t *runs_hist)
{
	if (!c) return FSEQ_E_ARG;
	if (int const rc = need_result(c)) return rc;
	uint32_t const none[P2_STATS] = {};
	uint32_t const *s = c->p2_stats_have ? c->p2_stats : none;
	if (by_runs) *by_runs = s[0];
	if (by_sort) *by_sort = s[1];
	if (copies) *copies = s[2];
	if (max_runs) *max_runs = s[3];
	if (runs_hist) std::copy(s + 4, s + 4 + P2_HIST, runs_hist);
	return FSEQ_OK;
}

namespace {

bool put_launches(std::vector<ChainLaunch> const &ls, fseq_chain_launch_info *out, uint32_t *n)
{
	if (ls.size() > FSEQ_DEBUG_CHAIN_LAUNCHES) return false;
	for (size_t i = 0; i < ls.size(); ++i) out[i] = fseq_chain_launch_info{ls[i].level, ls[i].kind, ls[i].chains, ls[i].blocks, ls[i].first_chain, ls[i].workgroups};
	*n = (uint32_t) ls.size();
	return true;
}

} // namespace

int fseq_debug_chain_plan(uint32_t m, int streamed, uint32_t nblocks, uint32_t cus, int chain_wg, uint32_t chain_fan, uint64_t fit, uint32_t resident,
                          fseq_chain_plan *plan)
{
	if (!plan || 0 == m || 0 == nblocks || chain_wg < 0 || chain_wg > 2 || 1 == chain_fan || cus > 0x7FFFFFFFu || resident > 0x7FFFFFFFu) return FSEQ_E_ARG;
	*plan = fseq_chain_plan{};
	// (as block_geometry asks: the CUs count only where the turns could be looked at)
	ChainFan const f = plan_chain_fan(m, streamed != 0, nblocks, (int) cus, chain_wg, chain_fan);
	std::vector<uint32_t> const items = chain_level_items(nblocks, f.fan);
	if (items.size() > FSEQ_DEBUG_CHAIN_LEVELS) return FSEQ_E_ARG;
	plan->fan = f.fan; plan->fan_round5 = f.fan5; plan->turns = f.turns;
	plan->n_levels = (uint32_t) items.size();
	std::copy(items.begin(), items.end(), plan->level_items);
	size_t const fit_ = (size_t) std::min<uint64_t>(fit, SIZE_MAX);
	if (!put_launches(chain_launches(items, f.fan, streamed != 0, (int) cus, chain_wg, fit_, (int) resident), plan->launches, &plan->n_launches)) return FSEQ_E_ARG;
	return FSEQ_OK;
}

int fseq_debug_chain_plan_sharded(uint32_t nblocks, uint32_t world, uint32_t rank, uint32_t chain_fan, int streamed, uint32_t cus, int chain_wg, uint64_t fit,
                                  uint32_t resident, fseq_chain_plan *plan)
{
	if (!plan || 0 == nblocks || 0 == world || world > 4096u || rank >= world || chain_wg < 0 || chain_wg > 2 || 1 == chain_fan || cus > 0x7FFFFFFFu
	    || resident > 0x7FFFFFFFu)
		return FSEQ_E_ARG;
	*plan = fseq_chain_plan{};
	ShardChainPlan const S = plan_chain_sharded(nblocks, world, chain_fan ? chain_fan : CHAIN_SHARD_FAN);
	if (S.k + 1 > FSEQ_DEBUG_CHAIN_LEVELS) return FSEQ_E_ARG;
	plan->fan = plan->fan_round5 = S.F;
	plan->shard_k = S.k; plan->shard_q = S.q; plan->blocks_per_rank = S.bpr; plan->n_hyper = S.n_hyper;
	shard_block_range(S, nblocks, rank, &plan->b_lo, &plan->b_hi);
	std::vector<uint32_t> lo, hi;
	shard_level_ranges(S, plan->b_lo, plan->b_hi, lo, hi);
	plan->n_levels = S.k + 1;
	for (uint32_t i = 0; i <= S.k; ++i) plan->level_items[i] = hi[i] - lo[i];
	size_t const fit_ = (size_t) std::min<uint64_t>(fit, SIZE_MAX);
	if (!put_launches(shard_chain_launches(S, nblocks, rank, streamed != 0, (int) cus, chain_wg, fit_, (int) resident), plan->launches, &plan->n_launches))
		return FSEQ_E_ARG;
	return FSEQ_OK;
}

int fseq_debug_phase_b(fseq_ctx *c, fseq_phase_b_info *info)
{
	if (!c || !info) return FSEQ_E_ARG;
	if (int const rc = need_result(c)) return rc;
	static_assert(sizeof(info->cw_stats) == CW_STATS * 4, "fseq_phase_b_info::cw_stats holds the counters of k_chain_wg");
	*info = fseq_phase_b_info{};
	info->cus = (uint32_t) std::max(device_cus(c), 0);
	info->nblocks = c->nblocks; info->fan = c->chain_fan;
	if (!put_launches(c->pb_launches, info->launches, &info->n_launches)) return fail(c, FSEQ_E_UNSUPPORTED, "fseq_debug_phase_b: more launches than the report holds");
	info->resident = c->use_stream ? (uint32_t) std::max(c->cw_resident, 0) : 0u;
	info->fit = c->pb_fit;
	info->hand_armed = c->pb_hand;
	info->stats_kept = c->pb_cw_stats_have;
	if (c->pb_cw_stats_have) std::copy(c->pb_cw_stats, c->pb_cw_stats + CW_STATS, info->cw_stats);
	if (c->p2_stats_have)
	{
		info->p2_groups = c->p2_groups; info->p2_groups_took_keys = c->p2_hand[0]; info->p2_groups_gathered = c->p2_hand[1];
	}
	return FSEQ_OK;
}

int fseq_debug_class_columns(fseq_ctx *c, uint32_t *from_classes, uint32_t *from_alignment, uint32_t block, uint32_t *have, uint32_t *nkeys, uint64_t *ldc,
                             uint8_t *out, uint64_t out_bytes)
{
	if (!c) return FSEQ_E_ARG;
	if (int const rc = need_result(c)) return rc;
	(void) hipSetDevice(c->p.device);
	uint32_t const b_lo = c->sh.on ? c->sh.b_lo : 0u, b_hi = c->sh.on ? c->sh.b_hi : c->nblocks;
	std::vector<uint32_t> flags;
	if (c->cls_read)
	{
		flags.assign(c->nblocks, 0u);
		if (b_hi > b_lo) HIP_TRY(c, hipMemcpy(flags.data() + b_lo, c->d_cls_have + b_lo, (size_t) (b_hi - b_lo) * 4, hipMemcpyDeviceToHost));
	}
	uint32_t n_cls = 0, n_msa = 0;
	if (c->red_active && !c->red_direct && c->red.plan.cnt.size() == c->nblocks)
		for (uint32_t b = b_lo; b < b_hi; ++b)
			if (c->red.plan.cnt[b] != RED_NONE) ++(c->cls_read && flags[b] ? n_cls : n_msa);
	if (from_classes) *from_classes = n_cls;
	if (from_alignment) *from_alignment = n_msa;
	if (block == UINT32_MAX) return FSEQ_OK;
	if (block < b_lo || block >= b_hi) return fail(c, FSEQ_E_ARG, "fseq_debug_class_columns: not a block of this context");
	uint32_t h = 0;
	if (c->cls_on && c->d_cls && c->d_cls_have) HIP_TRY(c, hipMemcpy(&h, c->d_cls_have + block, 4, hipMemcpyDeviceToHost));
	if (have) *have = h;
	if (nkeys) { *nkeys = 0; if (c->d_nkeys) HIP_TRY(c, hipMemcpy(nkeys, c->d_nkeys + block, 4, hipMemcpyDeviceToHost)); }
	if (ldc) *ldc = c->cls_on ? c->cls_ld : 0;
	if (out && h)
	{
		uint64_t const k0 = (uint64_t) block * c->B, k1 = std::min<uint64_t>(c->p.n, k0 + c->B);
		if (out_bytes < (k1 - k0) * c->cls_ld) return fail(c, FSEQ_E_ARG, "fseq_debug_class_columns: the buffer is smaller than the block's class columns");
		HIP_TRY(c, hipMemcpy(out, c->d_cls + (size_t) k0 * c->cls_ld, (size_t) (k1 - k0) * c->cls_ld, hipMemcpyDeviceToHost));
	}
	return FSEQ_OK;
}

int fseq_debug_column_sources(fseq_ctx *c, uint32_t *staged, uint32_t *gathered, uint32_t block, uint32_t *block_staged)
{
	if (!c) return FSEQ_E_ARG;
	if (int const rc = need_result(c)) return rc;
	(void) hipSetDevice(c->p.device);
	uint32_t const b_lo = c->sh.on ? c->sh.b_lo : 0u, b_hi = c->sh.on ? c->sh.b_hi : c->nblocks;
	uint32_t n_staged = 0, n_gathered = 0, mine = 0;
	RedPlan const &P = c->red.plan;
	if (c->red_active && !c->red_direct && P.cnt.size() == c->nblocks)
	{
		std::vector<uint32_t> have(c->nblocks, 0u);
		if (c->cls_staged && b_hi > b_lo) HIP_TRY(c, hipMemcpy(have.data() + b_lo, c->d_cls_have + b_lo, (size_t) (b_hi - b_lo) * 4, hipMemcpyDeviceToHost));
		for (uint32_t b = b_lo; b < b_hi; ++b)
		{
			if (P.cnt[b] == RED_NONE) continue;
			bool const st = c->cls_staged && P.from_cls[b] && have[b];
			++(st ? n_staged : n_gathered);
			if (b == block) mine = st ? 1u : 0u;
		}
	}
	if (staged) *staged = n_staged;
	if (gathered) *gathered = n_gathered;
	if (block_staged) *block_staged = mine;
	return FSEQ_OK;
}

int fseq_debug_dp(fseq_ctx *c, uint32_t *lb, uint32_t *max_size, uint32_t *size)
{
	if (!c) return FSEQ_E_ARG;
	if (int const rc = need_result(c)) return rc;
	(void) hipSetDevice(c->p.device);
	if (lb) HIP_TRY(c, hipMemcpy(lb, c->dp.LB, c->dp_size * 4, hipMemcpyDeviceToHost));
	if (max_size) HIP_TRY(c, hipMemcpy(max_size, c->dp.M, c->dp_size * 4, hipMemcpyDeviceToHost));
	if (size) HIP_TRY(c, hipMemcpy(size, c->dp.SZ, c->dp_size * 4, hipMemcpyDeviceToHost));
	return FSEQ_OK;
}

int fseq_debug_dp_owned(fseq_ctx *c, uint64_t *first, uint64_t *last, int *final_cell, int *whole_arrays)
{
	if (!c || !c->have_result || c->res.short_path) return FSEQ_E_ARG;
	uint64_t lo = 0, hi = c->dp_size;
	int fin = 1, whole = 1;
	if (c->sh.on)
	{
		Shard const &sh = c->sh;
		bool const have = sh.rank < sh.active && sh.rank < c->own_lo.size();
		lo = have ? c->own_lo[sh.rank] : 0; hi = have ? c->own_hi[sh.rank] : 0;
		fin = have && sh.rank + 1u == sh.active ? 1 : 0;
		whole = c->dp_window_mode ? 0 : 1;
	}
	if (first) *first = lo;
	if (last) *last = hi;
	if (final_cell) *final_cell = fin;
	if (whole_arrays) *whole_arrays = whole;
	return FSEQ_OK;
}

int fseq_debug_ranges(uint64_t *pushes, uint64_t *pops, int *with_roctx)
{
	if (pushes) *pushes = g_range_pushes.load(std::memory_order_relaxed);
	if (pops) *pops = g_range_pops.load(std::memory_order_relaxed);
#ifdef FSEQ_WITH_ROCTX
	if (with_roctx) *with_roctx = 1;
#else
	if (with_roctx) *with_roctx = 0;
#endif
	return FSEQ_OK;
}

int fseq_debug_clock(fseq_ctx *c, double *ghz, uint32_t *workgroups)
{
	if (!c || !ghz) return FSEQ_E_ARG;
#ifdef FSEQ_CLOCK_STAMPS
	(void) hipSetDevice(c->p.device);
	std::vector<unsigned long long> st((size_t) FSEQ_CLOCK_SLOTS * 4);
	HIP_TRY(c, hipMemcpyFromSymbol(st.data(), HIP_SYMBOL(g_clock_stamps), st.size() * 8));
	std::vector<double> f;
	for (uint32_t i = 0; i < FSEQ_CLOCK_SLOTS; ++i)
	{
		unsigned long long const t0 = st[4 * i], r0 = st[4 * i + 1], t1 = st[4 * i + 2], r1 = st[4 * i + 3];
		if (t1 > t0 && r1 > r0) f.push_back((double) (t1 - t0) / (double) (r1 - r0) * 0.1);      // cycles per 10 ns = GHz x 10
	}
	if (f.empty()) return fail(c, FSEQ_E_ARG, "no clock stamps: run a long-path segmentation first");
	std::nth_element(f.begin(), f.begin() + f.size() / 2, f.end());
	*ghz = f[f.size() / 2];
	if (workgroups) *workgroups = (uint32_t) f.size();
	return FSEQ_OK;
#else
	(void) workgroups;
	*ghz = 0.0;
	return fail(c, FSEQ_E_UNSUPPORTED, "built without -DFSEQ_CLOCK_STAMPS (the product kernels execute no stamp)");
#endif
}

int fseq_debug_block_state(fseq_ctx *c, uint64_t block_idx, uint32_t *a_out, uint32_t *d_out)
{
	if (!c || !c->have_result || c->res.short_path || block_idx > c->nblocks) return FSEQ_E_ARG;
	if (c->sh.on && (block_idx < c->sh.b_lo || block_idx > c->sh.b_hi)) return fail(c, FSEQ_E_ARG, "block state held by another rank");
	(void) hipSetDevice(c->p.device);
	size_t const m = c->p.m;
	if (a_out) HIP_TRY(c, hipMemcpy(a_out, c->d_bstate_a + block_idx * m, m * 4, hipMemcpyDeviceToHost));
	if (d_out) HIP_TRY(c, hipMemcpy(d_out, c->d_bstate_d + block_idx * m, m * 4, hipMemcpyDeviceToHost));
	return FSEQ_OK;
}

int fseq_debug_column_list(fseq_ctx *c, uint64_t col, uint32_t *values, uint32_t *counts,
                           uint32_t *n_entries, uint32_t *cnt0, uint32_t *complete)
{
	// (behind a scan over segment lengths there is no result, but the lists of its last long-path entry are held)
	if (!c || !(c->scan_lists || (c->have_result && !c->res.short_path)) || col >= c->p.n) return FSEQ_E_ARG;
	if (c->lw.on && (col < c->lw.col_lo || col >= c->lw.col_hi)) return fail(c, FSEQ_E_ARG, "the list of this column is not held: the run kept its lists in windows (fseq_set_list_memory)");
	(void) hipSetDevice(c->p.device);
	uint4 h;
	HIP_TRY(c, hipMemcpy(&h, c->d_hdr + col, sizeof(h), hipMemcpyDeviceToHost));
	std::vector<uint2> e(h.x);
	if (h.x) HIP_TRY(c, hipMemcpy(e.data(), c->d_ent + col * (size_t) c->stride, h.x * sizeof(uint2), hipMemcpyDeviceToHost));
	for (uint32_t i = 0; i < h.x; ++i)
	{
		if (values) values[i] = e[i].x;
		if (counts) counts[i] = e[i].y;
	}
	if (n_entries) *n_entries = h.x;
	if (cnt0) *cnt0 = h.y;
	if (complete) *complete = h.z;
	return FSEQ_OK;
}

int fseq_debug_list_windows(fseq_ctx *c, uint64_t *bytes_held, uint64_t *columns_per_window, uint32_t *windows, uint32_t *merge_windows)
{
	if (!c || !c->have_result) return FSEQ_E_ARG;
	fseq_ctx::ListWindows const &W = c->lw;
	bool const lists = !c->res.short_path;
	if (bytes_held) *bytes_held = W.on ? W.bytes : lists ? (uint64_t) c->d_ent.cap * sizeof(uint2) : 0;
	if (columns_per_window) *columns_per_window = W.on ? (uint64_t) W.wb * c->B : lists ? held_hi(c) - held_lo(c) : 0;
	if (windows) *windows = W.on ? W.nwin : lists ? 1u : 0u;
	if (merge_windows) *merge_windows = W.on ? W.merge_windows : 0u;
	return FSEQ_OK;
}

int fseq_debug_dp_schedule(uint64_t segment_length, uint64_t n, uint64_t col_hi, uint32_t *n_rounds, uint32_t *cells_per_round,
                           uint32_t *rounds_within, int *pipelined)
{
	if (0 == segment_length || n < 2 * segment_length || n >= 0xFFFFFFF0ull) return FSEQ_E_ARG;
	DpSchedule const S = dp_schedule((uint32_t) segment_length, (uint32_t) n);
	if (n_rounds) *n_rounds = S.nrounds;
	if (cells_per_round) *cells_per_round = S.RL;
	if (rounds_within) *rounds_within = dp_rounds_within(S, col_hi);
	if (pipelined) *pipelined = S.pipe ? 1 : 0;
	return FSEQ_OK;
}

// ---- phase D on caller-supplied lists (tests/test_gpu_dp_lists.py): the host's check of the lists, then the production launchers
int fseq_debug_dp_lists_check(uint32_t m, uint64_t n, uint64_t L, uint32_t stride, uint32_t const *ent, uint32_t const *hdr, uint64_t *bad_column,
                              uint32_t *rule)
{
	auto refuse = [&](uint64_t k, uint32_t r) {
		if (bad_column) *bad_column = k;
		if (rule) *rule = r;
		return FSEQ_E_ARG;
	};
	if (!ent || !hdr || 0 == m || 0 == L || n < 2 * L || n >= 0xFFFFFFF0ull || 0 == stride || n * stride > (1ull << 28)) return refuse(~0ull, 0u);
	// the columns a cell reads: end - 1 of every cell end in [L, n - L], and n - 1 (the final cell)
	for (uint64_t k = L - 1; k < n; k = (k + 1 == n - L ? n - 1 : k + 1))
	{
		uint32_t const *const h = hdr + 4 * k, *const e = ent + 2 * k * stride;
		uint32_t const nent = h[0];
		if (nent < 1 || nent > stride) return refuse(k, 1u);
		if (e[0] != k + 1) return refuse(k, 2u);
		uint64_t sum = e[1];
		for (uint32_t i = 1; i < nent; ++i)
		{
			if (e[2 * i] >= e[2 * i - 2]) return refuse(k, 3u);
			if (e[2 * i + 1] < 1) return refuse(k, 5u);
			sum += e[2 * i + 1];
		}
		// (descending from k + 1 >= 1: a value 0 can only stand last)
		bool const zero_last = e[2 * (nent - 1)] == 0;
		bool const full = sum == m;
		if (zero_last && (e[2 * (nent - 1) + 1] != h[1] || !full)) return refuse(k, 4u);
		if (!zero_last && full && h[1] != 0) return refuse(k, 4u);
		if (sum != h[3] || sum > m) return refuse(k, 6u);
		if (h[2] > 1 || (h[2] == 1) != full || h[1] > m) return refuse(k, 7u);
	}
	if (bad_column) *bad_column = ~0ull;
	if (rule) *rule = 0;
	return FSEQ_OK;
}

namespace {

// what the entries on caller-supplied lists refuse before the device is touched (who: "DP on lists", "merge on lists")
int lists_refused(fseq_ctx *c, char const *who, uint32_t list_cap, uint32_t const *ent, uint32_t const *hdr)
{
	char what[200];
	auto no = [&](int code, char const *why) {
		snprintf(what, sizeof(what), "%s: %s", who, why);
		return fail(c, code, what);
	};
	if (c->sh.on) return no(FSEQ_E_UNSUPPORTED, "not for sharded contexts (a rank holds the lists of its own columns)");
	if (c->lw.budget) return no(FSEQ_E_UNSUPPORTED, "not under a list memory budget (every list is held)");
	if (!c->have_input) return fail(c, FSEQ_E_ARG, "no input set");
	if (c->in.open) return fail(c, FSEQ_E_ARG, "a chunked input is under way (fseq_input_begin without fseq_input_end)");
	fseq_params const &p = c->p;
	if (p.n < 2 * p.segment_length) return no(FSEQ_E_ARG, "the short path (n < 2L) has no DP");
	if (list_cap > 0x00FFFFFFu) return no(FSEQ_E_ARG, "list capacity out of range");
	uint64_t bad = 0;
	uint32_t rule = 0;
	if (fseq_debug_dp_lists_check(p.m, p.n, p.segment_length, (list_cap + 3) & ~1u, ent, hdr, &bad, &rule))
	{
		snprintf(what, sizeof(what), "%s: the list of column %lld breaks rule %u of fseq_debug_dp_lists_check", who, (long long) bad, rule);
		return fail(c, FSEQ_E_ARG, what);
	}
	return FSEQ_OK;
}

// the context holds no result from here on, and its lists are the caller's: nothing of a run may answer for them
int lists_onto_context(fseq_ctx *c, uint32_t list_cap, uint32_t const *ent, uint32_t const *hdr)
{
	(void) hipSetDevice(c->p.device);
	c->have_result = false;
	c->scan_lists = false;
	c->free_match();
	c->lw.on = false; c->lw.merge_windows = 0;
	int rc;
	if (!c->kernels_ready && (rc = prepare_geometry(c))) return rc;
	if ((rc = ensure_work_buffers(c, list_cap, false))) return rc;
	hipStream_t st = c->stream;
	HIP_TRY(c, hipStreamSynchronize(st));
	HIP_TRY(c, hipMemcpyAsync(c->d_ent, ent, (size_t) c->p.n * c->stride * sizeof(uint2), hipMemcpyHostToDevice, st));
	HIP_TRY(c, hipMemcpyAsync(c->d_hdr, hdr, (size_t) c->p.n * sizeof(uint4), hipMemcpyHostToDevice, st));
	return FSEQ_OK;
}

} // namespace

int fseq_debug_dp_on_lists(fseq_ctx *c, uint32_t list_cap, uint32_t const *ent, uint32_t const *hdr, uint32_t const *cuts, uint32_t n_cuts,
                           uint32_t *lb, uint32_t *max_size, uint32_t *size, fseq_dp_lists_info *info)
{
	if (!c) return FSEQ_E_ARG;
	if (!ent || !hdr || !info || (n_cuts && !cuts) || 0 == list_cap) return fail(c, FSEQ_E_ARG, "DP on lists: lists, a capacity and an info are needed");
	int rc;
	if ((rc = lists_refused(c, "DP on lists", list_cap, ent, hdr))) return rc;
	fseq_params const &p = c->p;
	uint64_t const n = p.n, L = p.segment_length;
	DpSchedule const S = dp_schedule((uint32_t) L, (uint32_t) n);
	for (uint32_t i = 0; i < n_cuts; ++i)
		if (cuts[i] == 0 || cuts[i] >= S.nrounds || (i && cuts[i] <= cuts[i - 1]))
			return fail(c, FSEQ_E_ARG, "DP on lists: the cut rounds ascend strictly inside (0, rounds)");
	if ((rc = lists_onto_context(c, list_cap, ent, hdr))) return rc;
	hipStream_t st = c->stream;
	HIP_TRY(c, hipMemsetAsync(path_words(c)->dp, 0, sizeof(PathWords::dp), st));
	HIP_TRY(c, hipMemsetAsync(c->dp.M, 0, c->dp_size * 4, st));
	HIP_TRY(c, hipMemsetAsync(c->dp.LB, 0, c->dp_size * 4, st));
	HIP_TRY(c, hipMemsetAsync(c->dp.SZ, 0, c->dp_size * 4, st));
	HIP_TRY(c, hipMemsetAsync(c->dp.K, 0, (c->dp_size + 64) * 8, st));
	HIP_TRY(c, hipMemsetAsync(c->dp.Tb, 0, (size_t) 32 * c->dp.tstride * 4, st));
	HIP_TRY(c, hipMemsetAsync(c->dp.Tbv, 0, (size_t) 32 * c->dp.tstride * 4, st));
	HIP_TRY(c, hipMemsetAsync(c->d_Mprev, 0, c->dp_size * 4, st));
	*info = fseq_dp_lists_info{};
	if (n_cuts == 0)
	{
		DpProof proof;
		bool unproven = false;
		if ((rc = long_dp_on_lists(c, &proof, &unproven))) return rc;
		info->unproven = unproven ? 1u : 0u;
		info->dp_chunks = proof.dp_chunks;
		info->dp_sweeps = proof.dp_sweeps;
		info->launches = proof.dp_chunks ? 0u : 1u;
	}
	else
	{
		uint32_t r_lo = 0;
		for (uint32_t i = 0; i <= n_cuts; ++i)
		{
			uint32_t const r_hi = i < n_cuts ? cuts[i] : S.nrounds;
			launch_dp_serial(c, DP_PARTIAL, st, r_lo, r_hi);
			r_lo = r_hi;
		}
		HIP_TRY(c, hipGetLastError());
		uint32_t words[4] = {0, 0, 0, 0};
		HIP_TRY(c, hipMemcpyAsync(words, path_words(c)->dp, sizeof(PathWords::dp), hipMemcpyDeviceToHost, st));
		HIP_TRY(c, hipStreamSynchronize(st));
		info->unproven = words[0] & 1u;
		info->launches = n_cuts + 1u;
	}
	if (lb) HIP_TRY(c, hipMemcpy(lb, c->dp.LB, c->dp_size * 4, hipMemcpyDeviceToHost));
	if (max_size) HIP_TRY(c, hipMemcpy(max_size, c->dp.M, c->dp_size * 4, hipMemcpyDeviceToHost));
	if (size) HIP_TRY(c, hipMemcpy(size, c->dp.SZ, c->dp_size * 4, hipMemcpyDeviceToHost));
	return FSEQ_OK;
}

// ---- the traceback and the greedy merge on caller-supplied DP arrays and lists (tests/test_gpu_merge_lists.py): the host's
// checks of the lists and of the chain (fseq_tbcheck.hpp), then follow_traceback and the merge as a run calls them
int fseq_debug_merge_on_lists(fseq_ctx *c, uint32_t list_cap, uint32_t const *ent, uint32_t const *hdr, uint32_t const *lb, uint32_t const *max_size,
                              uint32_t const *size, uint32_t flags, uint64_t const *col_splits, uint32_t n_splits, fseq_dp_arg *traceback,
                              uint64_t *n_traceback, uint32_t *tau, uint64_t *n_tau, fseq_segment *segments, uint64_t *n_segments, fseq_merge_lists_info *info)
{
	if (!c) return FSEQ_E_ARG;
	if (!ent || !hdr || !lb || !max_size || !size || 0 == list_cap) return fail(c, FSEQ_E_ARG, "merge on lists: lists, a capacity and the three DP arrays are needed");
	int rc;
	if ((rc = lists_refused(c, "merge on lists", list_cap, ent, hdr))) return rc;
	uint64_t const n = c->p.n, L = c->p.segment_length;
	uint64_t bad = 0;
	if (int const why = tb_chain_check(lb, n, L, &bad, nullptr))
	{
		char what[200];
		if (why == TB_CHAIN_LB) snprintf(what, sizeof(what), "merge on lists: the lb of chain entry %lld is neither 0 nor in L .. the entry", (long long) bad);
		else snprintf(what, sizeof(what), "merge on lists: the chain from entry n - L has not ended at entry %lld, n / L + 2 entries on", (long long) bad);
		return fail(c, FSEQ_E_ARG, what);
	}
	if (flags & ~1u) return fail(c, FSEQ_E_ARG, "merge on lists: unknown flags");
	MergeProbe probe;
	probe.separate = (flags & 1u) != 0;
	if (n_splits && (!col_splits || !probe.separate)) return fail(c, FSEQ_E_ARG, "merge on lists: column splits go with flag bit 0 (thresholds from launches of their own)");
	probe.bounds.push_back(0);
	for (uint32_t i = 0; i < n_splits; ++i)
	{
		if (col_splits[i] <= probe.bounds.back() || col_splits[i] >= n) return fail(c, FSEQ_E_ARG, "merge on lists: the column splits ascend strictly inside (0, n)");
		probe.bounds.push_back(col_splits[i]);
	}
	probe.bounds.push_back(n);
	if ((rc = lists_onto_context(c, list_cap, ent, hdr))) return rc;
	hipStream_t st = c->stream;
	HIP_TRY(c, hipMemcpyAsync(c->dp.LB, lb, c->dp_size * 4, hipMemcpyHostToDevice, st));
	HIP_TRY(c, hipMemcpyAsync(c->dp.M, max_size, c->dp_size * 4, hipMemcpyHostToDevice, st));
	HIP_TRY(c, hipMemcpyAsync(c->dp.SZ, size, c->dp_size * 4, hipMemcpyHostToDevice, st));
	bool overflow = false;
	rc = probe_traceback_and_merge(c, &probe, &overflow);
	if (FSEQ_OK == rc)
	{
		size_t const S = c->traceback.size(), R = overflow ? 0 : c->segments.size();
		if (n_traceback) *n_traceback = S;
		if (traceback) std::copy(c->traceback.begin(), c->traceback.end(), traceback);
		if (n_tau) *n_tau = probe.tau.size();
		for (size_t j = 0; tau && j < probe.tau.size(); ++j) { tau[2 * j] = probe.tau[j].x; tau[2 * j + 1] = probe.tau[j].y; }
		if (n_segments) *n_segments = R;
		if (segments) std::copy(c->segments.begin(), c->segments.begin() + R, segments);
		if (info) *info = fseq_merge_lists_info{overflow ? 1u : 0u, probe.separate ? 1u : 0u, probe.threshold_launches, probe.count_launches};
	}
	// nothing of this call is a run's: no result, no traceback, no segments (the size of the traceback's first copy alone stays, as after a run)
	c->traceback.clear();
	c->segments.clear();
	c->tau_host.clear();
	if (rc) return rc;
	// (a run writes the entries its cells own and finds 0 in the others, n - 2L + 1 .. n - L - 1: the caller's words go)
	HIP_TRY(c, hipMemsetAsync(c->dp.LB, 0, c->dp_size * 4, st));
	HIP_TRY(c, hipMemsetAsync(c->dp.M, 0, c->dp_size * 4, st));
	HIP_TRY(c, hipMemsetAsync(c->dp.SZ, 0, c->dp_size * 4, st));
	HIP_TRY(c, hipStreamSynchronize(st));
	return FSEQ_OK;
}

// ---- row-sharded pBWT sweep: the north-star partition as a conformance path (fseq_rowshard.hpp) ------------------
uint64_t fseq_rowshard_xbuf_words(uint32_t m, uint32_t bits, uint32_t world)
{
	if (!m || !world || (bits != 2 && bits != 4 && bits != 8)) return 0;
	uint32_t const bsh = bits == 2 ? 2u : bits == 4 ? 1u : 0u;
	uint64_t const cw = (sym_bytes(m, bsh) + 3u) / 4u;
	return 2 * (cw + 2ull * m) + (uint64_t) RS_SLOT * world + 64;
}

int fseq_rowshard_rows(uint32_t m, uint32_t bits, uint32_t rank, uint32_t world, uint32_t *row_lo, uint32_t *row_hi)
{
	if (!m || !world || rank >= world || !row_lo || !row_hi || (bits != 2 && bits != 4 && bits != 8)) return FSEQ_E_ARG;
	uint32_t const bsh = bits == 2 ? 2u : bits == 4 ? 1u : 0u;
	uint64_t const cw = (sym_bytes(m, bsh) + 3u) / 4u, rpw = 32u / bits;
	*row_lo = (uint32_t) std::min<uint64_t>(m, cw * rank / world * rpw);
	*row_hi = (uint32_t) std::min<uint64_t>(m, cw * (rank + 1) / world * rpw);
	return FSEQ_OK;
}

int fseq_rowshard_pbwt(fseq_rowshard const *A, uint32_t *a_out, uint32_t *d_out, uint32_t *pos_lo, uint32_t *pos_hi,
                       double *ms, uint64_t *n_exchanges)
{
	if (!A || !A->m || !A->world || A->rank >= A->world || !A->d_cols || !a_out || !d_out) return FSEQ_E_ARG;
	if ((A->bits != 2 && A->bits != 4 && A->bits != 8) || A->sigma < 1 || A->sigma > (1u << A->bits)) return FSEQ_E_ARG;
	uint32_t const m = A->m, G = A->world, g = A->rank;
	uint32_t const bsh = A->bits == 2 ? 2u : A->bits == 4 ? 1u : 0u;
	uint64_t const cw = (sym_bytes(m, bsh) + 3u) / 4u;
	if (A->ld % 4 || A->ld < cw * 4) return FSEQ_E_ARG;
	if (A->ncols > 0xFFFFFFFEull) return FSEQ_E_ARG;
	if (G > 1 && (!A->xbuf || !A->fn)) return FSEQ_E_ARG;
	if (!A->xbuf || A->xbuf_words < fseq_rowshard_xbuf_words(m, A->bits, G)) return FSEQ_E_ARG;
	if (hipSetDevice(A->device) != hipSuccess) return FSEQ_E_HIP;
	uint32_t nbits = 1;
	while ((1u << nbits) < A->sigma) ++nbits;
	uint32_t const npass = (nbits + 1) / 2;
	uint64_t const reg = cw + 2ull * m;
	uint32_t *const xb = static_cast<uint32_t *>(A->xbuf);
	uint32_t *const slots = xb + 2 * reg;
	auto C_ = [&](uint32_t r) { return xb + r * reg; };
	auto A_ = [&](uint32_t r) { return xb + r * reg + cw; };
	auto D_ = [&](uint32_t r) { return xb + r * reg + cw + m; };
	uint32_t const p_lo = (uint32_t) ((uint64_t) m * g / G), p_hi = (uint32_t) ((uint64_t) m * (g + 1) / G), ml = p_hi - p_lo;
	uint32_t const w_lo = (uint32_t) (cw * g / G), w_hi = (uint32_t) (cw * (g + 1) / G);
	hipStream_t st = nullptr;
	if (hipStreamCreateWithFlags(&st, hipStreamNonBlocking) != hipSuccess) return FSEQ_E_HIP;
	uint64_t nex = 0;
	bool ok = true;
	auto H = [&](hipError_t e) { if (e != hipSuccess) ok = false; return e == hipSuccess; };
	auto xch = [&](uint64_t off, uint64_t count) {
		++nex;
		if (G == 1 || !ok) return;
		if (!H(hipStreamSynchronize(st))) return;
		if (A->fn(A->user, off, count, 0) != 0) ok = false;
	};
	auto contrib = [&](uint64_t k, uint32_t r) {
		H(hipMemsetAsync(C_(r), 0, cw * 4, st));
		if (w_hi > w_lo)
			hipLaunchKernelGGL(k_rs_contrib, dim3((w_hi - w_lo + 255u) / 256u), dim3(256), 0, st,
			                   reinterpret_cast<uint32_t const *>(static_cast<uint8_t const *>(A->d_cols) + k * A->ld), w_lo, w_hi, C_(r));
	};
	double const t0 = now_ms();
	hipLaunchKernelGGL(k_rs_init, dim3((m + 255u) / 256u), dim3(256), 0, st, A_(0), D_(0), m);
	uint32_t colreg = 0, adreg = 0;
	if (A->ncols)
	{
		contrib(0, 0);
		xch(0, cw);                                              // X0 of column 0
	}
	for (uint64_t k = 0; k < A->ncols && ok; ++k)
		for (uint32_t pass = 0; pass < npass && ok; ++pass)
		{
			uint8_t const *col = reinterpret_cast<uint8_t const *>(C_(colreg));
			H(hipMemsetAsync(slots, 0, (size_t) RS_SLOT * G * 4, st));
			hipLaunchKernelGGL(k_rs_sweep<false>, dim3(1), dim3(ST), 0, st, col, A_(adreg) + p_lo, D_(adreg) + p_lo, ml, bsh, pass,
			                   (uint32_t) (k + 1), slots, g, G, (uint32_t *) nullptr, (uint32_t *) nullptr);
			xch(2 * reg, (uint64_t) RS_SLOT * G);                   // X1 + X2
			uint32_t const r2 = 1u - adreg;
			H(hipMemsetAsync(A_(r2), 0, (size_t) 2 * m * 4, st));
			hipLaunchKernelGGL(k_rs_sweep<true>, dim3(1), dim3(ST), 0, st, col, A_(adreg) + p_lo, D_(adreg) + p_lo, ml, bsh, pass,
			                   (uint32_t) (k + 1), slots, g, G, A_(r2), D_(r2));
			if (pass + 1 == npass && k + 1 < A->ncols)
			{
				contrib(k + 1, r2);
				xch(r2 * reg, reg);                                  // X3 + X0 of the next column
				colreg = r2;
			}
			else
				xch(r2 * reg + cw, 2ull * m);                        // X3
			adreg = r2;
		}
	if (ok) H(hipStreamSynchronize(st));
	double const t1 = now_ms();
	if (ok && ml)
	{
		H(hipMemcpy(a_out + p_lo, A_(adreg) + p_lo, (size_t) ml * 4, hipMemcpyDeviceToHost));
		H(hipMemcpy(d_out + p_lo, D_(adreg) + p_lo, (size_t) ml * 4, hipMemcpyDeviceToHost));
	}
	(void) hipStreamDestroy(st);
	if (pos_lo) *pos_lo = p_lo;
	if (pos_hi) *pos_hi = p_hi;
	if (ms) *ms = t1 - t0;
	if (n_exchanges) *n_exchanges = nex;
	return ok ? FSEQ_OK : FSEQ_E_HIP;
}

int fseq_debug_alphabet(fseq_ctx *c, uint32_t *sigma, uint32_t *bits, uint8_t *code_to_byte)
{
	if (!c || !sigma || !bits) return FSEQ_E_ARG;
	if (!c->have_input) return fail(c, FSEQ_E_ARG, "alphabet: the context holds no input");
	*sigma = c->sigma;
	*bits = 8u >> c->bsh;
	if (code_to_byte) memcpy(code_to_byte, c->code_to_byte, 256);
	return FSEQ_OK;
}

int fseq_debug_device_bytes(fseq_ctx *c, uint64_t *now, uint64_t *peak, int reset_peak)
{
	if (!c || !now || !peak) return FSEQ_E_ARG;
	*now = c->alloc_total;
	*peak = c->alloc_peak;
	if (reset_peak) c->alloc_peak = c->alloc_total;
	return FSEQ_OK;
}

} // extern "C"
