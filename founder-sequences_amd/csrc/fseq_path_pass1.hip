// fseq_path_pass1.hip -- the segmentation path, pass 1: phase A (the key blocks; the short path's one block), phase B (the
// boundary states), the list capacity, phase C's launchers on all rows (on the blocks' representatives: csrc/fseq_path_reduced.hip).
// The attempt that queues them is csrc/fseq_path_attempt.hip.  The one unit that instantiates k_colblock_stream<> and
// k_columns_stream<> and that includes fseq_chainsort.hpp: pass 2 replays columns and takes its streamed chain steps through
// the launchers here -- and so do the two debug entries at the end, which run those steps' kernels on constructed states
// (fseq_debug_pass2_step, fseq_debug_chain_launch, include/fseq_debug.h: the kernels of a header are one unit's).
// (The units of the path and what crosses them: fseq_path.hpp.)
#include "fseq_path.hpp"
#include "fseq_kernels.hpp"
#include "fseq_stream.hpp"
#include "fseq_stream2.hpp"
#include "fseq_chainsort.hpp"
#include "fseq_blockkeys.hpp"
#include "fseq_blocktrie.hpp"

namespace fseq {

std::atomic<uint64_t> g_range_pushes{0}, g_range_pops{0};

// ---- launches: LDS-resident kernels, or their HBM-streamed counterparts for large m
// grid workgroups = the blocks starting at column col0, col0 + B, ...; rank / keyd / nkeys point at the first of them
// phase B and pass 2 work on absolute divergences (column numbers <= n): their partition steps scan keys while n fits
// the configuration's key shift (FSEQ_PLAIN_SCAN: never)
uint32_t scan_keyed(fseq_ctx const *c)
{
	if (c->use_stream || c->tune.plain_scan) return 0u;
	return (c->p.n < (1ull << c->ks.scan_shift) && !c->tune.occurrence_keys) ? 1u : c->p.n < (1ull << 25) ? 2u : 0u;       // row-count keys, occurrence keys, has-based scan
}

namespace {

// streamed rows: occurrence keys while every column number fits 25 bits (FSEQ_PLAIN_SCAN: the has-based scan)
bool stream_keyed(fseq_ctx const *c) { return c->p.n < (1ull << 25) && !c->tune.plain_scan; }

// one launch of the streamed column sweep, the context's workspace behind the alignment: MODE_RANK (phase A) writes the key
// blocks, MODE_SNAP (pass 2) the states at the boundaries tasks.task_rb
template <int MODE>
void launch_colblock_stream(fseq_ctx *c, uint32_t grid, MsaArgs const &A, PhaseAArgs const &K, SnapArgs const &S)
{
	// (K.only: the per-block filter goes in the start-state slot, which the rank mode does not use otherwise)
	hipLaunchKernelGGL((stream_keyed(c) ? k_colblock_stream<MODE, true> : k_colblock_stream<MODE, false>), dim3(grid), dim3(ST), stream_lds_bytes(sym_bytes(A.m, A.bsh), c->stream_staged), c->stream,
	                   A.msa, A.ld, A.m, A.n, A.B, A.nblocks, A.npass, A.bsh, c->d_ws.base, (uint32_t) c->stream_staged, K.rank, K.keyd, K.nkeys, MODE == MODE_RANK ? K.only : S.bstate_a, S.bstate_d,
	                   S.task_rb, S.task_grp, S.snap_a, S.snap_d, S.task_src, S.ss.snap_stride, (uint32_t const *) S.ss.ss_a, (uint32_t const *) S.ss.ss_d, K.col0, S.ss.ss_pack);
}

// phase A as a column sweep over the blocks of K
void launch_rank(fseq_ctx *c, PhaseAArgs const &K)
{
	if (!K.nblk) return;
	if (c->use_stream) launch_colblock_stream<MODE_RANK>(c, K.nblk, K.A, K, SnapArgs{});
	else c->ks.rank(c->stream, K.nblk, c->ks.lds_colblock, K);
}

// phase A in key space, streamed rows (fseq_blockkeys.hpp): the blocks of K in turn on `groups` workgroups
void launch_blockkeys_stream(fseq_ctx *c, uint32_t groups, PhaseAArgs const &K)
{
	MsaArgs const &A = K.A;
	hipLaunchKernelGGL(k_blockkeys_stream, dim3(groups), dim3(1024), c->bk_lds, c->stream, A.msa, A.ld, A.m, A.n, A.B, A.bsh, K.nblk, K.rank, K.keyd, K.nkeys, K.col0,
	                   static_cast<uint32_t *>(K.work), K.work_per, K.cap_words, K.counters, K.wide, K.todo, K.only);
}

} // namespace

void launch_replay_stream(fseq_ctx *c, size_t groups, SnapArgs const &tasks)
{
	// the streamed sweep needs 4m workspace words per workgroup: as many groups per launch as d_ws holds
	size_t const cap = std::max<size_t>(1, c->d_ws.cap / (4 * (size_t) c->p.m));
	SnapArgs S = tasks;
	for (size_t g0 = 0; g0 < groups; g0 += cap)
	{
		S.task_grp = tasks.task_grp + g0; S.task_src = tasks.task_src + g0;
		launch_colblock_stream<MODE_SNAP>(c, (uint32_t) std::min(cap, groups - g0), S.A, PhaseAArgs{}, S);
	}
}

namespace {

// one chain launch on streamed rows: a chain step as a radix sort by rank + range maxima (fseq_chainsort.hpp), every sweep of a
// step a launch over (parts) x (chains): a chain of G blocks is G rounds of them.  A is complete but for the step, the pass and
// the chain count: the rows (m), the workspace of `grid` chains (ws) and their histograms (hist) are the caller's
// (phase B: launch_chain; tests: fseq_debug_chain_launch)
void launch_chain_stream(hipStream_t st, uint32_t grid, ChainMultiArgs A)
{
	uint32_t const m = A.m, nparts = chainmulti_parts(m), npass = chainmulti_passes(m);
	A.step = 0; A.pass = 0;
	A.nchains = grid;
	uint32_t const grid_y = (grid + 7u) & ~7u;       // (cm_wg: the workgroups of a chain on one XCD)
	dim3 const by_row((m + CM_WG - 1u) / CM_WG, grid_y), by_part((nparts + CM_WG / WAVE - 1u) / (CM_WG / WAVE), grid_y);
	hipLaunchKernelGGL(k_cm_init, by_row, dim3(CM_WG), 0, st, A);
	for (uint32_t s_ = 0; s_ < A.G; ++s_)
	{
		A.step = s_;
		for (uint32_t ps = 0; ps < npass; ++ps)
		{
			A.pass = ps;
			hipLaunchKernelGGL(k_cm_count, by_part, dim3(CM_WG), 0, st, A);
			hipLaunchKernelGGL(k_cm_offsets, dim3(grid), dim3(ST), 0, st, A);
			hipLaunchKernelGGL(k_cm_scatter, by_part, dim3(CM_WG), 0, st, A);
		}
		hipLaunchKernelGGL(k_cm_output, by_row, dim3(CM_WG), 0, st, A);
	}
	if (A.out_rank) hipLaunchKernelGGL(k_cm_emit, dim3(grid), dim3(ST), stream_lds_bytes(0, false), st, A, A.G);
}

// the same launch with a chain per workgroup (k_chain_wg, fseq_chainsort.hpp): `wgs` workgroups with a workspace of
// chainwg_ws_words(m) words each take the `grid` chains by a fixed stride; A as for launch_chain_stream (ws and hist are not used);
// stats: CW_STATS device words the kernel adds to, or nullptr
void launch_chain_wg(hipStream_t st, uint32_t grid, uint32_t wgs, ChainMultiArgs A, uint32_t *ws, uint32_t run_cap, uint32_t *stats)
{
	A.step = 0; A.pass = 0;
	A.nchains = grid;
	hipLaunchKernelGGL(k_chain_wg, dim3(wgs), dim3(ST), chainwg_lds_bytes(), st, A, ws, run_cap, stats);
}

// FSEQ_CHAIN_RUN_CAP: the most runs of equal key a step of k_chain_wg may form and still be moved by runs (0: every step sorts
// its rows; unset: what the kernel's LDS holds)
uint32_t chain_run_cap(fseq_ctx const *c)
{
	return c->tune.chain_run_cap < 0 ? CW_RUN_CAP : std::min<uint32_t>((uint32_t) c->tune.chain_run_cap, CW_RUN_CAP);
}

// How many workgroups of k_chain_wg a launch of `grid` chains gets; 0: the launch takes the spread kernels.  The rule: at least
// a chain per CU (chain_wg_rule, fseq_chainplan.hpp).  Below that the spread kernels fill the chip and a chain per workgroup does not
// (the upper levels of the recursion, the top chain, BASELINE C4cols50k and C4slice at round 5's fan, which they keep:
// block_geometry); from there on every CU has a chain of its own, a step costs no launch, and the kernel moves runs.  A sharded
// rank's level 0 reaches the rule as well where the rank has at least 4 x CUs blocks (fan 4): BASELINE C4 on 2, 4 and 8 ranks of
// 256 CUs launches 768, 384 and 256 chains there (fseq_debug_chain_plan_sharded).  FSEQ_CHAIN_WG: 1 every streamed launch, 2 none.
uint32_t chain_wg_groups(fseq_ctx *c, uint32_t grid)
{
	if (c->tune.chain_wg >= 2) return 0;             // (no device is asked)
	// as many as are resident at once (one a CU: its LDS) and as the workspace holds.  d_ws is a workspace of 9 m + B + 16 words per
	// block, a launch by the rule has CUs x fan blocks below it and fan >= 2: it holds a workgroup a CU (13 m + 90,000 words each)
	// from 18,000 rows on, and below that the launch takes fewer workgroups and more turns; only a forced launch on a few blocks
	// can find room for none, and takes the spread kernels
	size_t const fit = c->d_ws.cap / chainwg_ws_words(c->p.m);
	return chain_wg_workgroups(grid, device_cus(c), c->tune.chain_wg, fit, c->cw_resident);
}

// one chain launch of phase B (A: the level's key blocks, the start states, what comes out -- ChainMultiArgs); the launch
// adds the rows and, streamed rows, its workspace.  level, kind: for the context's record of the launch (fseq_debug_phase_b)
void launch_chain(fseq_ctx *c, uint32_t grid, ChainMultiArgs A, uint32_t level, ChainLaunchKind kind)
{
	if (!grid) return;
	A.m = c->p.m;
	uint32_t const wgs = c->use_stream ? chain_wg_groups(c, grid) : 0u;
	{
		ChainLaunch rec;
		rec.level = level; rec.kind = kind; rec.chains = grid; rec.blocks = A.G; rec.first_chain = A.grp0; rec.workgroups = wgs;
		c->pb_launches.push_back(rec);
	}
	if (c->use_stream)
		if (wgs)
		{
			if (c->tune.debug)
				fprintf(stderr, "[fseq] phase B: %u chains of %u blocks on %u workgroups of their own (%zu bytes of LDS, at most %u runs)\n", grid, A.G, wgs,
				        chainwg_lds_bytes(), chain_run_cap(c));
			launch_chain_wg(c->stream, grid, wgs, A, c->d_ws.base, chain_run_cap(c), c->d_cw_stats.base);
			return;
		}
	// streamed rows: ensure_work_buffers sized d_ws and d_cshist for the widest launch of phase B (a chain per chain_fan blocks,
	// plus one, in d_cshist; chainsort_ws_words(m) <= 8.25 m + 80 words <= the 9 m + B + 16 of every block's workspace)
	if (c->use_stream)
	{
		A.ws = c->d_ws.base; A.hist = c->d_cshist;
		launch_chain_stream(c->stream, grid, A);
	}
	else
		c->ks.chain(c->stream, grid, c->ks.lds_chain, A, scan_keyed(c));
}

} // namespace

int prepare_stream_kernels(fseq_ctx *c, size_t lds)
{
	HIP_TRY(c, allow_lds(k_colblock_stream<MODE_RANK>, lds));
	HIP_TRY(c, allow_lds(k_colblock_stream<MODE_SNAP>, lds));
	HIP_TRY(c, allow_lds(k_colblock_stream<MODE_RANK, true>, lds));
	HIP_TRY(c, allow_lds(k_colblock_stream<MODE_SNAP, true>, lds));
	HIP_TRY(c, allow_lds(k_columns_stream<19>, lds));
	HIP_TRY(c, allow_lds(k_columns_stream<0>, lds));
	HIP_TRY(c, allow_lds(k_chain_snap_grouped, pass2_lds_bytes()));
	HIP_TRY(c, allow_lds(k_cm_emit, stream_lds_bytes(0, false)));
	HIP_TRY(c, allow_lds(k_chain_wg, chainwg_lds_bytes()));
	if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&c->cw_resident, k_chain_wg, (int) ST, chainwg_lds_bytes()) != hipSuccess) c->cw_resident = 1;
	return FSEQ_OK;
}
int prepare_stream2_prologue(fseq_ctx *c)
{
	HIP_TRY(c, allow_lds(k_columns_stream2_prologue, stream_lds_bytes(0, true)));
	return FSEQ_OK;
}
int prepare_blockkeys_stream(fseq_ctx *c)
{
	HIP_TRY(c, allow_lds(k_blockkeys_stream, c->bk_lds));
	return FSEQ_OK;
}
size_t chain_hist_words(uint32_t m) { return (size_t) chainmulti_parts(m) * CS_BINS; }

// FSEQ_P2_RUN_CAP: the most runs of equal class a task of pass 2's streamed chain step may form and still be moved by runs
// (0: every task sorts its rows; unset: what the kernel's LDS holds)
uint32_t pass2_run_cap(fseq_ctx const *c)
{
	return c->tune.p2_run_cap < 0 ? P2_RUN_CAP : std::min<uint32_t>((uint32_t) c->tune.p2_run_cap, P2_RUN_CAP);
}

// streamed rows: pass 2's chain step by runs or as a radix sort, + range maxima, in a workspace per workgroup (fseq_chainsort.hpp),
// a block's tasks on one workgroup, the ngrp groups of d_red_p2grp taken from the counter behind them; stats: P2_STATS zeroed
// device words (fseq_debug_pass2_paths) and P2_HAND more behind them (the groups that took phase B's keys, the groups that gathered)
int launch_chain_snap_grouped(fseq_ctx *c, uint32_t ngrp, uint32_t *stats)
{
	uint32_t const m = c->p.m;
	hipStream_t st = c->stream;
	if (c->red_cap > P2_CLS_CAP) return fail(c, FSEQ_E_UNSUPPORTED, "pass 2: more representatives a block than the class table in LDS holds");
	int ncu = 0;
	(void) hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, c->p.device);
	size_t const fit = c->d_ws.cap / pass2_ws_words(m);
	uint32_t const grid = (uint32_t) std::min<size_t>(std::min<size_t>(ngrp, fit), (size_t) std::max(ncu, 1) * 2u);
	if (!grid) return fail(c, FSEQ_E_OOM, "pass 2: the workspace holds no chain step");
	if (c->tune.debug)
	{
		int resident = 0;
		(void) hipOccupancyMaxActiveBlocksPerMultiprocessor(&resident, k_chain_snap_grouped, (int) ST, pass2_lds_bytes());
		fprintf(stderr, "[fseq] pass 2 chain steps: %u groups on %u workgroups (the workspace holds %zu, a CU %d), %zu bytes of LDS, at most %u runs\n", ngrp, grid, fit,
		        resident, pass2_lds_bytes(), pass2_run_cap(c));
	}
	// phase B's keys where it handed them over for the boundary states in force (FSEQ_P2_KEYS=2: none)
	bool const hand = c->p2keys_live && c->tune.p2_keys != 2 && c->d_p2keys.base && c->d_p2keys_flag.base;
	hipLaunchKernelGGL(k_chain_snap_grouped, dim3(grid), dim3(ST), pass2_lds_bytes(), st, c->d_bstate_a, c->d_bstate_d, c->d_rank, m, c->d_red_taskblk, c->d_red_cls,
	                   c->d_red_headd, c->d_red_ncls, c->red_cap, c->d_red_p2grp.as<uint2 const>(), ngrp, c->d_red_p2grp + 2 * (size_t) ngrp,
	                   c->d_snap_a, c->d_snap_d, c->d_ws.base, pass2_run_cap(c), stats, hand ? c->d_p2keys.base : (uint16_t const *) nullptr,
	                   hand ? c->d_p2keys_flag.base : (uint32_t const *) nullptr, stats + P2_STATS);
	return FSEQ_OK;
}

// ---- phase A: the key blocks of my column blocks (independent of the list capacity)
int long_phase_a(fseq_ctx *c, LongRun &R)
{
	FSEQ_LONG_LOCALS(c);
	// 4-bit symbols, LDS-resident rows: the codes present in every column I hold, once per input (k_columns takes a column with at
	// most four of them in one digit pass)
	if (c->bsh == 1u && c->npass == 2u && !c->use_stream && !c->tune.no_dense_columns && !c->colmask_ready && held_hi(c) > held_lo(c)
	    && c->d_msa_own && (c->ld & 3u) == 0)                  // (own columns: padded past their last byte, whole words can be read)
	{
		uint64_t const lo = held_lo(c), hi = held_hi(c);
		if ((rc = c->d_colmask.alloc_range(c, (size_t) lo, (size_t) hi, 1))) return rc;
		HIP_TRY(c, hipMemsetAsync(&path_words(c)->dense_columns, 0, 4, st));
		hipLaunchKernelGGL(k_column_presence, dim3((uint32_t) std::min<uint64_t>(hi - lo, 8192)), dim3(256), 0, st, c->d_msa, c->ld, sym_bytes(m, c->bsh), lo, hi, c->d_colmask,
		                   &path_words(c)->dense_columns);
		// (once per input: one column in twenty with at most four codes, and phase C is the kernel with the one-pass branch)
		uint32_t n_dense = 0;
		HIP_TRY(c, hipMemcpyAsync(&n_dense, &path_words(c)->dense_columns, 4, hipMemcpyDeviceToHost, st));
		HIP_TRY(c, hipStreamSynchronize(st));
		c->colmask_use = (uint64_t) n_dense * 20u >= hi - lo;
		c->colmask_ready = true;
	}
	HIP_TRY(c, hipEventRecord(c->ev.a_begin, st));
	progress(c, FSEQ_STAGE_TRACEBACK, 0, n);
	FSEQ_RANGE_PUSH("fseq pass 1: phases A + B (block keys, boundary states)");
	R.range_ab_open = true;                  // (popped in long_phase_b; run_long_path pops it when a phase fails in between)
	bool const keyspace = R.keyspace = c->bk_cap_words && my_blocks && !c->tune.phase_a_classic;
	// The key-space tree hands the blocks whose merges would slice past their budget to the column sweep (fseq_blockkeys.hpp,
	// BK_ABORT): per-block flags, the sweep launched over my blocks with the flags as its filter.  What the last run on this
	// input saw decides what is launched now (the input has not changed, so neither has the outcome): no block given up ->
	// the tree alone; most of them -> the sweep alone; else both.  FSEQ_BLOCKKEYS_CAP (tests of the slices): the tree slices
	// as often as it takes.
	bool const limited = keyspace && !c->tune.blockkeys_cap;
	bool const tree = keyspace && !(limited && c->bk_given_up >= 0 && 2u * (uint32_t) c->bk_given_up > my_blocks);
	bool const sweep_after = limited && !(tree && c->bk_given_up == 0);
	R.tree_alone = tree && limited && !sweep_after;
	R.tree_ran = tree;
	uint32_t *todo = nullptr;
	if (limited)
	{
		if ((rc = c->d_todo.ensure(c, my_blocks))) return rc;
		todo = c->d_todo;
		HIP_TRY(c, hipMemsetAsync(todo, tree ? 0 : 0x01, (size_t) my_blocks * 4, st));     // (no tree: every block is the sweep's)
	}
	if (keyspace) HIP_TRY(c, hipMemsetAsync(&path_words(c)->phase_a, 0, sizeof(PhaseACounters), st));
	// The trie over 32-bit group words first (fseq_blocktrie.hpp) -- it reads the block once and ranks only its distinct keys --
	// and the key-space tree for the blocks it gives up (too many distinct keys for its tables).  As with the tree and the
	// sweep, what the last run on this input saw decides what is launched: nothing given up -> the trie alone; most blocks ->
	// no trie.  The tests of the tree's slices (FSEQ_BLOCKKEYS_CAP, _NO_LIMIT) keep the tree.
	uint32_t const bt_bits = 8u >> c->bsh, bt_T = blocktrie_threads(m, c->use_stream);
	// (LDS-resident rows: from 6,145 rows on -- BASELINE C5's 10,000: phase A 7.3 -> 5.9 ms; on C3's 2,504 rows a level of the trie is
	// a dozen barriers for 157 busy threads and the tree is as fast, 1.31 against 1.36 ms; FSEQ_BLOCKTRIE_ALWAYS: tests)
	bool const trie = tree && limited && (uint64_t) m <= (uint64_t) (32u / bt_bits) * bt_T * 32u && c->B < 65536u && !c->tune.no_blocktrie
	                  && (c->use_stream || m > 12u * 512u || c->tune.blocktrie_always)
	                  && (c->ld & 3u) == 0 && (reinterpret_cast<uintptr_t>(c->d_msa) & 3u) == 0
	                  && !(c->bt_given_up >= 0 && 2u * (uint32_t) c->bt_given_up > my_blocks);
	bool const tree_after = tree && !(trie && c->bt_given_up == 0);
	c->cls_on = c->cls_every = c->cls_read = c->cls_staged = false;
	R.trie_ran = trie;
	R.trie_alone = trie && !tree_after;
	// my key blocks, and what the key-space tree works with; the trie hands the tree its blocks, the tree hands the sweep its own
	PhaseAArgs keys;
	keys.A = msa_args(c);
	keys.rank = c->d_rank + (size_t) b_lo * m; keys.keyd = c->d_keyd + (size_t) b_lo * m; keys.nkeys = c->d_nkeys + b_lo;
	keys.col0 = (uint64_t) b_lo * c->B; keys.nblk = my_blocks;
	keys.T = c->bk_T; keys.cap_words = c->bk_cap_words; keys.counters = &path_words(c)->phase_a.tree_sliced; keys.todo = todo;
	keys.wide = (c->tune.blockkeys_wide ? 1u : 0u) | (c->tune.blockkeys_single ? 2u : 0u);
	if (trie)
	{
		int ncu = 0;
		(void) hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, c->p.device);
		uint32_t const per_cu = (uint32_t) std::max<size_t>(1, std::min<size_t>(2048u / bt_T, (160u * 1024u) / blocktrie_lds(bt_T)));
		uint32_t const groups = std::min<uint32_t>(my_blocks, (uint32_t) std::max(1, ncu) * per_cu);
		size_t const per = (blocktrie_ws_words(m, c->B, bt_bits, bt_T) + 15) & ~size_t(15);
		if ((rc = c->d_btws.ensure(c, per * groups))) return rc;
		if ((rc = c->d_only.ensure(c, my_blocks))) return rc;
		HIP_TRY(c, hipMemsetAsync(c->d_only, 0, (size_t) my_blocks * 4, st));
		PhaseAArgs T = keys;
		T.T = bt_T; T.work = c->d_btws; T.work_per = per; T.counters = &path_words(c)->phase_a.trie_given_up; T.todo = c->d_only;
		// The class columns of the blocks the trie ranks (its phase 3): what phase C's reduced alignment is gathered from instead of
		// reading the alignment a second time.  Only where somebody will read them: streamed rows (LDS-resident row counts take the
		// representatives' symbols from the alignment's own columns), the reduced phase C not switched off or declined on this input.
		// The buffer is the largest the reduced path adds (12 T classes a column: 3 KB at 2 bits, 15 GB on BASELINE C4), so it must fit
		// the context's memory budget and, without one, a quarter of what is free -- the lists and the reduced states are allocated
		// after it and must not fail for it.  Where it does not fit, or the allocation fails, the alignment is read as before.
		if (c->use_stream && c->tune.class_columns && !c->tune.no_reduced && n >= 2 * L && !(c->red.memory.declined && !c->tune.reduced_always) && !c->red.memory.cls_unread)
		{
			size_t const ldc = ((size_t) sym_bytes((uint32_t) BT_PER * bt_T, c->bsh) + 15) & ~size_t(15);
			uint64_t const k_lo = (uint64_t) b_lo * c->B, k_hi = std::min<uint64_t>(n, (uint64_t) b_hi * c->B);
			size_t const need = (size_t) (k_hi - k_lo) * ldc + 64;
			bool ok = c->d_cls.cap >= need;
			if (!ok)
			{
				size_t const held = c->d_cls.base ? c->d_cls.cap : 0;
				size_t free_b = 0, total_b = 0;
				bool fits = hipMemGetInfo(&free_b, &total_b) == hipSuccess && need <= (free_b + held) / 4;
				if (c->mem_budget && c->alloc_total - std::min(c->alloc_total, held) + need > c->mem_budget) fits = false;
				if (fits) ok = c->d_cls.try_alloc(c, need);        // (no room after all: not an error of the run)
				else if (c->d_cls.base) c->d_cls.release(c);
				if (c->tune.debug && !ok) fprintf(stderr, "[fseq] phase A: no room for %zu bytes of class columns: the reduced alignment from the alignment\n", need);
			}
			if (ok && (rc = c->d_cls_have.ensure(c, c->nblocks))) return rc;
			if (ok)
			{
				c->cls_ld = ldc;
				c->d_cls.rebase((ptrdiff_t) ((size_t) k_lo * ldc));
				HIP_TRY(c, hipMemsetAsync(c->d_cls_have + b_lo, 0, (size_t) my_blocks * 4, st));
				T.cls = c->d_cls; T.ldc = ldc; T.cls_have = c->d_cls_have + b_lo;
				c->cls_on = true; c->cls_every = !tree_after;
			}
		}
		HIP_TRY(c, launch_blocktrie(st, groups, T));
		keys.only = c->d_only;
	}
	if (tree_after && c->use_stream)
	{
		// phase A in key space, streamed rows: one workgroup per CU with its own workspace, blocks round-robin
		int ncu = 0;
		(void) hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, c->p.device);
		uint32_t const groups = std::min<uint32_t>(my_blocks, (uint32_t) std::max(1, ncu));
		size_t const per = (blockkeys_stream_ws_words(m, c->B, c->bsh) + 15) & ~size_t(15);
		if ((rc = c->d_bkws.ensure(c, per * groups))) return rc;
		keys.work = c->d_bkws; keys.work_per = per;
		launch_blockkeys_stream(c, groups, keys);
	}
	else if (tree_after)
	{
		// phase A in key space (fseq_blockkeys.hpp)
		size_t const per = (blockkeys_scratch_halfwords(m, c->B, c->bsh) + 7) & ~size_t(7);
		if (c->bk_per_block != per) c->d_bk.release(c);
		if ((rc = c->d_bk.ensure(c, per * my_blocks))) return rc;
		c->bk_per_block = per;
		keys.work = c->d_bk; keys.work_per = per;
		launch_blockkeys(st, my_blocks, c->bk_lds, keys);
	}
	if (!keyspace || sweep_after)
	{
		// (the sweep takes what the tree gave up; without a tree, every block)
		keys.only = keyspace && tree ? todo : nullptr;
		launch_rank(c, keys);
	}
	HIP_TRY(c, hipEventRecord(c->ev.a_end_b_begin, st));
	if (sharded && c->tune.inject_failure_rank >= 0 && (uint32_t) c->tune.inject_failure_rank == sh.rank)
		return fail(c, FSEQ_E_OOM, "injected failure (FSEQ_INJECT_FAILURE_RANK)");
	if (sync_at(c, 'A')) { fprintf(stderr, "[fseq] phase A queued\n"); HIP_TRY(c, hipStreamSynchronize(st)); fprintf(stderr, "[fseq] phase A done\n"); }
	if (c->tune.check_phase_a)
	{
		// diagnostic: the key blocks must be well-formed before anything indexes with them (ranks < nkeys <= m, the
		// divergence in front of a key inside the block's columns)
		HIP_TRY(c, hipStreamSynchronize(st));
		std::vector<uint32_t> rk(m), kd(m);
		for (uint32_t b = b_lo; b < b_hi; ++b)
		{
			uint32_t nk = 0;
			HIP_TRY(c, hipMemcpy(&nk, c->d_nkeys + b, 4, hipMemcpyDeviceToHost));
			HIP_TRY(c, hipMemcpy(rk.data(), c->d_rank + (size_t) b * m, (size_t) m * 4, hipMemcpyDeviceToHost));
			HIP_TRY(c, hipMemcpy(kd.data(), c->d_keyd + (size_t) b * m, (size_t) m * 4, hipMemcpyDeviceToHost));
			uint64_t const k0 = (uint64_t) b * c->B, k1 = std::min<uint64_t>(n, k0 + c->B);
			uint32_t bad_r = 0, bad_k = 0;
			for (uint32_t i = 0; i < m; ++i) if (rk[i] >= nk) ++bad_r;
			for (uint32_t j = 0; j < nk && j < m; ++j) if (kd[j] <= k0 || kd[j] > k1) ++bad_k;
			if (nk == 0 || nk > m || bad_r || bad_k)
			{
				char what[200];
				snprintf(what, sizeof(what), "phase A check: block %u has %u keys (m = %u), %u ranks out of range, %u key divergences outside (%llu, %llu]",
				         b, nk, m, bad_r, bad_k, (unsigned long long) k0, (unsigned long long) k1);
				return fail(c, FSEQ_E_HIP, what);
			}
		}
	}
	return FSEQ_OK;
}

// What an attempt read back of phase A's counters (fseq_path_attempt.hip: every attempt, whatever its verdict -- phase A runs once
// a run, so every attempt of a run reads the same): the run's figures, and what the next run's phase A launches
int phase_a_take_counts(fseq_ctx *c, LongRun const &R, PhaseACounters counts)
{
	FSEQ_LONG_LOCALS(c);
	if (!R.keyspace) return FSEQ_OK;
	if (!R.tree_ran) counts.tree_given_up = my_blocks;       // (no tree this time: every block went to the column sweep, as last time)
	c->tm.phase_a_fallbacks = counts.tree_sliced;
	c->tm.phase_a_given_up = counts.tree_given_up;
	// (the tree ran alone because no block was given up last time; the same input gives the same outcome)
	if (R.tree_alone && counts.tree_given_up != 0u) return fail(c, FSEQ_E_HIP, "internal: the key-space tree gave up blocks it ranked in the run before");
	c->bk_given_up = (int) counts.tree_given_up;
	if (R.trie_ran)
	{
		if (R.trie_alone && counts.trie_given_up != 0u) return fail(c, FSEQ_E_HIP, "internal: the block trie gave up blocks it ranked in the run before");
		c->bt_given_up = (int) counts.trie_given_up;
		c->tm.phase_a_trie_given_up = counts.trie_given_up;
	}
	return FSEQ_OK;
}

// the short path's phase A: one block [0, n), ranked in key space (fseq_blockkeys.hpp); FSEQ_PHASE_A_CLASSIC: the per-column sweep
int short_phase_a(fseq_ctx *c, uint32_t *d_rank, uint32_t *d_keyd, uint32_t *d_nkeys)
{
	fseq_params const &p = c->p;
	uint32_t const m = p.m;
	int rc;
	PhaseAArgs keys;
	keys.A = msa_args(c, p.n, (uint32_t) p.n, 1);
	keys.rank = d_rank; keys.keyd = d_keyd; keys.nkeys = d_nkeys; keys.nblk = 1;
	keys.T = c->bk_T; keys.cap_words = c->bk_cap_words;
	keys.wide = (c->tune.blockkeys_wide ? 1u : 0u) | (c->tune.blockkeys_single ? 2u : 0u);
	if (c->bk_cap_words && !c->tune.phase_a_classic)
	{
		if (c->use_stream)
		{
			size_t const per = (blockkeys_stream_ws_words(m, (uint32_t) p.n, c->bsh) + 15) & ~size_t(15);
			if ((rc = c->d_bkws.ensure(c, per))) return rc;
			keys.work = c->d_bkws; keys.work_per = per;
			launch_blockkeys_stream(c, 1, keys);
		}
		else
		{
			size_t const per = (blockkeys_scratch_halfwords(m, (uint32_t) p.n, c->bsh) + 7) & ~size_t(7);
			if (c->bk_per_block != per) c->d_bk.release(c);
			if ((rc = c->d_bk.ensure(c, per))) return rc;
			c->bk_per_block = per;
			keys.work = c->d_bk; keys.work_per = per;
			launch_blockkeys(c->stream, 1, c->bk_lds, keys);
		}
	}
	else
	{
		// the 16-bit LDS kernels keep block-relative divergences in 16 bits: one block of 65536 columns or more would wrap
		if (!c->use_stream && c->ks.cap > 7168u && p.n > 65535u)
			return fail(c, FSEQ_E_UNSUPPORTED, "short path by column sweep: more than 65535 columns with 16-bit LDS state (unset FSEQ_PHASE_A_CLASSIC)");
		launch_rank(c, keys);
	}
	return FSEQ_OK;
}

// ---- phase B: the exact boundary state of every block
int long_phase_b(fseq_ctx *c, LongRun &R)
{
	FSEQ_LONG_LOCALS(c);
	(void) R;
	bool hand = false;                                            // phase B hands the keys of level 0's expansion to pass 2 (below)
	// level 0: my key blocks and boundary states; level i: the composites of chain_fan key blocks of level i - 1 (fseq_ctx::levels)
	auto rank_of = [&](size_t i) { return i ? c->levels[i - 1].rank : c->d_rank; };
	auto keyd_of = [&](size_t i) { return i ? c->levels[i - 1].keyd : c->d_keyd; };
	auto nkeys_of = [&](size_t i) { return i ? c->levels[i - 1].nkeys : c->d_nkeys; };
	auto sa_of = [&](size_t i) { return i ? c->levels[i - 1].state_a : c->d_bstate_a; };
	auto sd_of = [&](size_t i) { return i ? c->levels[i - 1].state_d : c->d_bstate_d; };
	auto count_of = [&](size_t i) { return i ? c->levels[i - 1].count : c->nblocks; };
	// the key blocks of level i in chains of G, the launch's first chain grp0
	auto chains_of = [&](size_t i, uint32_t G, uint32_t grp0) {
		ChainMultiArgs A{};
		A.rank = rank_of(i); A.keyd = keyd_of(i); A.nkeys = nkeys_of(i); A.nb_total = count_of(i); A.G = G;
		A.cols_per_block = i ? c->levels[i - 1].cols : (uint64_t) c->B; A.grp0 = grp0;
		return A;
	};
	// compose level i: every chain, from the identity, into one key block of level i + 1
	auto compose = [&](size_t i, uint32_t G, uint32_t grp0 = 0) {
		ChainMultiArgs A = chains_of(i, G, grp0);
		A.out_rank = rank_of(i + 1); A.out_keyd = keyd_of(i + 1); A.out_nkeys = nkeys_of(i + 1);
		return A;
	};
	// expand level i: the state in front of each of its key blocks, every chain from the state level i + 1 holds for it (the
	// top level: from the identity, unless the caller names a start)
	auto expand = [&](size_t i, uint32_t G, uint32_t grp0 = 0) {
		ChainMultiArgs A = chains_of(i, G, grp0);
		if (i < c->levels.size()) { A.start_a = sa_of(i + 1); A.start_d = sd_of(i + 1); }
		A.out_state_a = sa_of(i); A.out_state_d = sd_of(i);
		// (the alignment's own blocks: the kernel that walks a chain on one workgroup hands its keys to pass 2)
		if (i == 0 && hand) { A.hand_keys = c->d_p2keys.base; A.hand_flag = c->d_p2keys_flag.base; }
		return A;
	};
	// [r15] The expansion of level 0 steps through block b from bstate_a[b] with rank[b]: its keys are the r pass 2's streamed chain
	// step gathers for the block, so k_chain_wg stores them (16 bits a row, a flag per block) and pass 2 reads them.  Only where both
	// ends exist -- streamed rows on one GPU, that launch on k_chain_wg by the rule, pass 2 (as far as known here) on the blocks'
	// representatives -- and where the device has room: a failed allocation is no error, pass 2 then gathers as before.  The flags are
	// cleared in front of every phase B: a context is reused across inputs, lengths and identity-reduced uploads
	c->p2keys_live = false;
	c->pb_launches.clear(); c->pb_hand = false; c->pb_cw_stats_have = false;
	c->pb_fit = c->use_stream ? c->d_ws.cap / chainwg_ws_words(m) : 0;
	if (c->use_stream && !sharded && c->tune.p2_keys != 2 && !c->tune.no_reduced && n >= 2 * L && !(c->red.memory.declined && !c->tune.reduced_always)
	    && chain_wg_groups(c, c->levels.empty() ? 1u : count_of(1)))
	{
		size_t const need = (size_t) c->nblocks * m;
		hand = (c->d_p2keys.cap >= need || c->d_p2keys.try_alloc(c, need)) && (c->d_p2keys_flag.cap >= c->nblocks || c->d_p2keys_flag.try_alloc(c, c->nblocks));
		if (hand) HIP_TRY(c, hipMemsetAsync(c->d_p2keys_flag.base, 0, (size_t) c->nblocks * 4, st));
		else if (c->tune.debug) fprintf(stderr, "[fseq] phase B: no room for the keys it could hand to pass 2 (%zu bytes): pass 2 gathers its own\n", need * 2);
	}
	// FSEQ_DEBUG: the chain-per-workgroup kernel keeps its counters (zeroed here, read and printed below); else it keeps none
	if (c->use_stream && c->tune.debug && c->tune.chain_wg < 2)
	{
		if ((rc = c->d_cw_stats.ensure(c, CW_STATS))) return rc;
		HIP_TRY(c, hipMemsetAsync(c->d_cw_stats.base, 0, CW_STATS * 4, st));
	}
	else if (c->d_cw_stats.base) c->d_cw_stats.release(c);
	if (!sharded)
	{
		// phase B: up the levels -- compose groups of G key blocks of a level into one key block of the next
		// (parallel, from the identity) --, chain the few key blocks of the top level (one workgroup), down the levels --
		// expand every group from the boundary state the level above gave it (parallel)
		uint32_t const G = c->chain_fan;
		size_t const top = c->levels.size();
		for (size_t i = 0; i < top; ++i) launch_chain(c, count_of(i + 1), compose(i, G), (uint32_t) i, CHAIN_COMPOSE);
		launch_chain(c, 1, expand(top, count_of(top)), (uint32_t) top, CHAIN_TOP);
		for (size_t i = top; i-- > 0;) launch_chain(c, count_of(i + 1), expand(i, G), (uint32_t) i, CHAIN_EXPAND);
	}
	else
	{
		// Sharded phase B: rank r is hyper-block r.  Up the levels over my own block range (fan F, as on one GPU), my
		// last composites into my hyper key block, exchange the W hyper key blocks (the one collective of pass 1's column
		// work), chain them (every rank, same result), then down again from the state in front of my hyper-block.
		uint32_t const F = c->chain_fan, NH = c->n_hyper, K = c->shard_k, Q = c->shard_q;
		bool const have = sh.rank < NH;
		// my items of level i: [lo_i, hi_i) (rank boundaries are multiples of F^K blocks)
		std::vector<uint32_t> lo(K + 1), hi(K + 1);
		lo[0] = b_lo; hi[0] = b_hi;
		for (uint32_t i = 1; i <= K; ++i) { lo[i] = lo[i - 1] / F; hi[i] = (hi[i - 1] + F - 1) / F; }
		// the hyper key blocks (d_h*): Q composites of level K into mine, and -- every rank -- the chain over all NH of them
		ChainMultiArgs mine = chains_of(K, Q, sh.rank), hyper{};
		mine.out_rank = c->d_hrank; mine.out_keyd = c->d_hkeyd; mine.out_nkeys = c->d_hnkeys;
		hyper.rank = c->d_hrank; hyper.keyd = c->d_hkeyd; hyper.nkeys = c->d_hnkeys; hyper.nb_total = hyper.G = NH; hyper.cols_per_block = (uint64_t) sh.bpr * c->B;
		hyper.out_state_a = c->d_hstate_a; hyper.out_state_d = c->d_hstate_d;
		for (uint32_t i = 0; have && i < K; ++i) launch_chain(c, hi[i + 1] - lo[i + 1], compose(i, F, lo[i + 1]), i, CHAIN_COMPOSE);
		if (have) launch_chain(c, 1, mine, K, CHAIN_COMPOSE);
		{
			// xbuf: [hrank NH x m][hkeyd NH x m][hnkeys NH]
			size_t const w = (size_t) NH * m;
			HIP_TRY(c, hipMemsetAsync(sh.xbuf, 0, (2 * w + NH) * 4, st));
			if (have)
			{
				HIP_TRY(c, hipMemcpyAsync(sh.xbuf + (size_t) sh.rank * m, c->d_hrank + (size_t) sh.rank * m, (size_t) m * 4, hipMemcpyDeviceToDevice, st));
				HIP_TRY(c, hipMemcpyAsync(sh.xbuf + w + (size_t) sh.rank * m, c->d_hkeyd + (size_t) sh.rank * m, (size_t) m * 4, hipMemcpyDeviceToDevice, st));
				HIP_TRY(c, hipMemcpyAsync(sh.xbuf + 2 * w + sh.rank, c->d_hnkeys + sh.rank, 4, hipMemcpyDeviceToDevice, st));
			}
			if ((rc = shard_exchange(c, 2 * w + NH, 0))) return rc;
			HIP_TRY(c, hipMemcpyAsync(c->d_hrank, sh.xbuf, w * 4, hipMemcpyDeviceToDevice, st));
			HIP_TRY(c, hipMemcpyAsync(c->d_hkeyd, sh.xbuf + w, w * 4, hipMemcpyDeviceToDevice, st));
			HIP_TRY(c, hipMemcpyAsync(c->d_hnkeys, sh.xbuf + 2 * w, (size_t) NH * 4, hipMemcpyDeviceToDevice, st));
		}
		launch_chain(c, 1, hyper, K + 1, CHAIN_TOP);
		if (have)
		{
			// (my hyper-block starts from the state the chain over the hyper key blocks left in front of it)
			ChainMultiArgs top = expand(K, Q, sh.rank);
			top.start_a = c->d_hstate_a; top.start_d = c->d_hstate_d;
			launch_chain(c, 1, top, K, CHAIN_EXPAND);
			for (uint32_t i = K; i-- > 0;) launch_chain(c, hi[i + 1] - lo[i + 1], expand(i, F, lo[i + 1]), i, CHAIN_EXPAND);
			// the state behind my last block = in front of the next rank's hyper-block (or behind the whole alignment,
			// which the expansion has written itself): my halo block starts from it
			if (b_hi < c->nblocks)
			{
				HIP_TRY(c, hipMemcpyAsync(c->d_bstate_a + (size_t) b_hi * m, c->d_hstate_a + (size_t) (sh.rank + 1u) * m, (size_t) m * 4, hipMemcpyDeviceToDevice, st));
				HIP_TRY(c, hipMemcpyAsync(c->d_bstate_d + (size_t) b_hi * m, c->d_hstate_d + (size_t) (sh.rank + 1u) * m, (size_t) m * 4, hipMemcpyDeviceToDevice, st));
			}
		}
	}
	c->p2keys_live = c->pb_hand = hand;
	HIP_TRY(c, hipEventRecord(c->ev.b_end, st));
	HIP_TRY(c, hipGetLastError());
	FSEQ_RANGE_POP();
	R.range_ab_open = false;
	progress(c, FSEQ_STAGE_TRACEBACK, n / 5, n);                  // (phases A and B queued: about a fifth of pass 1)
	if (c->d_cw_stats.base)
	{
		uint32_t (&s)[CW_STATS] = c->pb_cw_stats;
		HIP_TRY(c, hipMemcpyAsync(s, c->d_cw_stats.base, sizeof(s), hipMemcpyDeviceToHost, st));
		HIP_TRY(c, hipStreamSynchronize(st));
		c->pb_cw_stats_have = true;
		fprintf(stderr, "[fseq] phase B chain steps on a workgroup of their own: %u by runs, %u by the sort of the rows, %u from the identity; most runs %u; by run count (<= 2^b):", s[0], s[1], s[2], s[3]);
		for (uint32_t b = 0; b < P2_HIST; ++b) fprintf(stderr, " %u", s[4 + b]);
		fprintf(stderr, "\n");
	}
	if (sync_at(c, 'B')) { fprintf(stderr, "[fseq] phase B queued\n"); HIP_TRY(c, hipStreamSynchronize(st)); fprintf(stderr, "[fseq] phase B done\n"); }
	return FSEQ_OK;
}

// ---- the list capacity X: what the caller asked for, what worked last time, or an estimate from the boundary states
int long_list_capacity(fseq_ctx *c, LongRun &R)
{
	FSEQ_LONG_LOCALS(c);
	uint32_t &X = R.X;
	if (!p.list_cap && !c->X_hint)
	{
		// first run on this input: size the lists from the block boundary states (k_boundary_recent)
		// (sharded: every rank looks at its own boundaries, the ranks then agree on the largest estimate)
		std::vector<uint32_t> recent(my_blocks ? my_blocks + 1 : 0);
		if (my_blocks)
		{
			hipLaunchKernelGGL(k_boundary_recent, dim3(my_blocks + 1), dim3(256), 0, st, c->d_bstate_d, m, n, c->B, (uint32_t) L, c->d_recent, b_lo);
			HIP_TRY(c, hipMemcpyAsync(recent.data(), c->d_recent, recent.size() * 4, hipMemcpyDeviceToHost, st));
		}
		HIP_TRY(c, hipStreamSynchronize(st));
		recent.erase(std::remove(recent.begin(), recent.end(), 0xFFFFFFFFu), recent.end());
		if (!recent.empty())
		{
			std::nth_element(recent.begin(), recent.begin() + recent.size() / 2, recent.end());
			uint64_t const med = recent[recent.size() / 2];
			// (a quarter above the median, to the next multiple of 64 -- not the next 2^k - 1: the lists of BASELINE C4 are
			// 5,000,000 x (X + 3) x 8 bytes, and what they do not take goes to the stride states of pass 2)
			uint64_t const want = med + med / 4;
			if (X < want) X = (uint32_t) (((want + 63) & ~63ull) - 1);
			if (c->tune.debug)
				fprintf(stderr, "[fseq] list capacity estimate: %zu boundaries, median recent count %llu -> X = %u\n",
				        recent.size(), (unsigned long long) med, X);
		}
	}
	if (sharded)
	{
		HIP_TRY(c, hipMemcpyAsync(sh.xbuf, &X, 4, hipMemcpyHostToDevice, st));
		if ((rc = shard_exchange(c, 1, 1))) return rc;
		HIP_TRY(c, hipMemcpy(&X, sh.xbuf, 4, hipMemcpyDeviceToHost));
	}
	if (X >= m) X = m;

	return FSEQ_OK;
}

namespace {

// streamed rows, the first form of the column kernel (KS: bits of the keys its partition steps scan; 0: the has-based scan)
template <int KS>
void launch_columns_stream(fseq_ctx *c, uint32_t grid, ColumnsArgs const &C)
{
	MsaArgs const &A = C.A;
	hipLaunchKernelGGL(k_columns_stream<KS>, dim3(grid), dim3(ST), stream_lds_bytes(sym_bytes(A.m, A.bsh), c->stream_staged), c->stream, A.msa, A.ld, A.m, A.n, A.B, A.npass, A.bsh, C.ws, (uint32_t) c->stream_staged,
	                   C.bstate_a, C.bstate_d, C.lists.L, C.lists.X, C.lists.stride, C.lists.ent, C.lists.hdr, C.ss.snap_stride, C.ss.ss_a, C.ss.ss_d, C.block0, C.done_host, C.epoch, C.ss.ss_pack);
}

} // namespace

// ---- phase C on all rows of the blocks b0 .. b0 + nb - 1
// (list [r5]: workgroup i owns block list[i] instead of b0 + i -- the blocks the reduced phase C hands to the run on all rows)
void launch_columns(fseq_ctx *c, uint32_t b0, uint32_t nb, uint32_t const *list)
{
	FSEQ_LONG_LOCALS(c);
	// columns phase C covers here: all, or my blocks plus the halo block's first columns (the lists my last DP round reads)
	ColumnsArgs C;
	C.A = msa_args(c, sharded ? sh.c_end : n, c->B, c->nblocks);
	C.bstate_a = c->d_bstate_a; C.bstate_d = c->d_bstate_d; C.lists = list_args(c); C.ss = stride_states(c); C.ws = c->d_ws;
	C.block0 = b0; C.blocklist = list;                         // (done_host, epoch: nothing on the path waits for single blocks from the host)
	if (c->colmask_ready && c->colmask_use) C.colmask = c->d_colmask;
	if (c->use_stream && c->s2.T)
	{
		uint32_t pack_abits = 1;
		while ((1u << pack_abits) < m) ++pack_abits;
		hipLaunchKernelGGL(k_columns_stream2_prologue, dim3(nb), dim3(ST), stream_lds_bytes(0, true), st, m, C.A.n, C.A.B, C.ws, C.bstate_a, C.bstate_d, b0, pack_abits,
		                   c->ss_ids ? c->d_bs_w : (uint32_t *) nullptr, c->ss_ids ? c->d_bs_h : (uint8_t *) nullptr, list);
		c->s2.launch(st, nb, c->s2_lds, C);
	}
	else if (c->use_stream && (uint64_t) m + c->B < (1u << 19) && !c->tune.stream_plain_scan) launch_columns_stream<19>(c, nb, C);
	else if (c->use_stream) launch_columns_stream<0>(c, nb, C);
	else ks.columns(st, nb, c->lds_columns, C);
}

} // namespace fseq

using namespace fseq;

namespace {

// the device buffers of one debug call: freed when the call returns, whichever way
struct DebugBuffers {
	std::vector<void *> held;
	~DebugBuffers() { for (void *p : held) (void) hipFree(p); }
	// `words` device words, every byte `fill` (0 or 0xFF); nullptr where the allocation or the fill fails
	uint32_t *words(size_t words, int fill)
	{
		void *p = nullptr;
		if (hipMalloc(&p, std::max<size_t>(1, words) * 4) != hipSuccess) return nullptr;
		held.push_back(p);
		if (hipMemset(p, fill, std::max<size_t>(1, words) * 4) != hipSuccess) return nullptr;
		return static_cast<uint32_t *>(p);
	}
	uint32_t *copy(uint32_t const *src, size_t n, size_t at = 0, size_t total = 0)
	{
		uint32_t *p = words(std::max(total, at + n), 0);
		if (p && n && hipMemcpy(p + at, src, n * 4, hipMemcpyHostToDevice) != hipSuccess) return nullptr;
		return p;
	}
};

constexpr uint32_t DEBUG_M_MIN = 11265, DEBUG_M_MAX = 589824;      // streamed rows: more than the LDS kernels hold, up to what the build accepts

// count rows of m words, every one a permutation of 0 .. m - 1
bool rows_are_permutations(uint32_t const *a, size_t count, uint32_t m)
{
	std::vector<uint8_t> seen(m);
	for (size_t b = 0; b < count; ++b)
	{
		std::fill(seen.begin(), seen.end(), 0);
		for (uint32_t i = 0; i < m; ++i)
		{
			uint32_t const v = a[b * m + i];
			if (v >= m || seen[v]) return false;
			seen[v] = 1;
		}
	}
	return true;
}

// one chain launch on constructed key blocks: the spread kernels (workgroups == 0), or k_chain_wg on `workgroups` workgroups
int debug_chain_launch(int device, uint32_t m, uint32_t nb_total, uint32_t G, uint64_t cols_per_block, uint32_t const *rank, uint32_t const *keyd,
                       uint32_t const *nkeys, uint32_t first_chain, uint32_t chains, uint32_t const *start_a, uint32_t const *start_d,
                       uint32_t run_cap, uint32_t workgroups, uint32_t *out_state_a, uint32_t *out_state_d, uint32_t *out_rank, uint32_t *out_keyd,
                       uint32_t *out_nkeys, uint32_t *stats, uint16_t *hand_keys = nullptr, uint32_t *hand_flag = nullptr)
{
	// ---- everything an index is formed from, before the first HIP call
	bool const want_states = out_state_a != nullptr, want_keys = out_rank != nullptr;
	if (!rank || !keyd || !nkeys || (!want_states && !want_keys)) return FSEQ_E_ARG;
	if (want_states != (out_state_d != nullptr) || want_keys != (out_keyd != nullptr) || want_keys != (out_nkeys != nullptr)) return FSEQ_E_ARG;
	if ((start_a != nullptr) != (start_d != nullptr)) return FSEQ_E_ARG;
	// (the entry that hands keys over takes any m from 65 on: the kernel's sweeps at a few rows a wave, and waves without any)
	if (m < (hand_keys ? 65u : DEBUG_M_MIN) || m > DEBUG_M_MAX || !nb_total || nb_total > 4096u) return FSEQ_E_ARG;
	if ((hand_keys != nullptr) != (hand_flag != nullptr) || (hand_keys && !workgroups)) return FSEQ_E_ARG;
	if (!G || G > nb_total) return FSEQ_E_ARG;                            // (a chain of more steps than blocks only queues idle launches)
	uint32_t const nchains_all = (nb_total + G - 1u) / G;
	if (!chains || first_chain >= nchains_all || chains > nchains_all - first_chain) return FSEQ_E_ARG;
	for (uint32_t b = 0; b < nb_total; ++b)
	{
		if (!nkeys[b] || nkeys[b] > m) return FSEQ_E_ARG;
		for (uint32_t i = 0; i < m; ++i)
			if (rank[(size_t) b * m + i] >= nkeys[b]) return FSEQ_E_ARG;
	}
	if (start_a && !rows_are_permutations(start_a, chains, m)) return FSEQ_E_ARG;

	if (hipSetDevice(device) != hipSuccess) return FSEQ_E_HIP;
	DebugBuffers B;
	// (the kernels index start states and composite key blocks by the chain's number in the level, first_chain + its number in the launch)
	size_t const blocks = (size_t) nb_total * m, per_chain = (size_t) (first_chain + chains) * m, at = (size_t) first_chain * m;
	ChainMultiArgs A{};
	A.m = m; A.nb_total = nb_total; A.G = G; A.cols_per_block = cols_per_block; A.grp0 = first_chain;
	A.rank = B.copy(rank, blocks); A.keyd = B.copy(keyd, blocks); A.nkeys = B.copy(nkeys, nb_total);
	uint32_t *d_wg_ws = nullptr, *d_stats = nullptr;
	if (workgroups)
	{
		d_wg_ws = B.words((size_t) workgroups * chainwg_ws_words(m), 0); d_stats = B.words(CW_STATS, 0);
		if (!d_wg_ws || !d_stats) return FSEQ_E_OOM;
		if (allow_lds(k_chain_wg, chainwg_lds_bytes()) != hipSuccess) return FSEQ_E_HIP;
	}
	else
	{
		A.ws = B.words((size_t) chains * chainsort_ws_words(m), 0);
		A.hist = B.words((size_t) chains * chainmulti_parts(m) * CS_BINS, 0);
		if (!A.ws || !A.hist) return FSEQ_E_OOM;
	}
	if (!A.rank || !A.keyd || !A.nkeys) return FSEQ_E_OOM;
	if (start_a)
	{
		A.start_a = B.copy(start_a, (size_t) chains * m, at); A.start_d = B.copy(start_d, (size_t) chains * m, at);
		if (!A.start_a || !A.start_d) return FSEQ_E_OOM;
	}
	if (want_states)
	{
		A.out_state_a = B.words(blocks + m, 0xFF); A.out_state_d = B.words(blocks + m, 0xFF);
		if (!A.out_state_a || !A.out_state_d) return FSEQ_E_OOM;
	}
	if (want_keys)
	{
		A.out_rank = B.words(per_chain, 0xFF); A.out_keyd = B.words(per_chain, 0xFF); A.out_nkeys = B.words(first_chain + chains, 0xFF);
		if (!A.out_rank || !A.out_keyd || !A.out_nkeys) return FSEQ_E_OOM;
		if (allow_lds(k_cm_emit, stream_lds_bytes(0, false)) != hipSuccess) return FSEQ_E_HIP;
	}
	if (hand_keys)
	{
		// the caller's array goes up as it is (what the kernel leaves alone comes back unchanged), the flags start clear
		size_t const bytes = blocks * 2;
		void *p = B.words((bytes + 3) / 4, 0);
		A.hand_flag = B.words(nb_total, 0);
		if (!p || !A.hand_flag) return FSEQ_E_OOM;
		A.hand_keys = static_cast<uint16_t *>(p);
		if (hipMemcpy(A.hand_keys, hand_keys, bytes, hipMemcpyHostToDevice) != hipSuccess) return FSEQ_E_HIP;
	}
	if (workgroups) launch_chain_wg(0, chains, workgroups, A, d_wg_ws, run_cap, d_stats);
	else launch_chain_stream(0, chains, A);
	if (hipGetLastError() != hipSuccess || hipDeviceSynchronize() != hipSuccess) return FSEQ_E_HIP;
	if (workgroups && hipMemcpy(stats, d_stats, CW_STATS * 4, hipMemcpyDeviceToHost) != hipSuccess) return FSEQ_E_HIP;
	if (want_states && (hipMemcpy(out_state_a, A.out_state_a, (blocks + m) * 4, hipMemcpyDeviceToHost) != hipSuccess
	                    || hipMemcpy(out_state_d, A.out_state_d, (blocks + m) * 4, hipMemcpyDeviceToHost) != hipSuccess))
		return FSEQ_E_HIP;
	if (want_keys && (hipMemcpy(out_rank, A.out_rank + at, (size_t) chains * m * 4, hipMemcpyDeviceToHost) != hipSuccess
	                  || hipMemcpy(out_keyd, A.out_keyd + at, (size_t) chains * m * 4, hipMemcpyDeviceToHost) != hipSuccess
	                  || hipMemcpy(out_nkeys, A.out_nkeys + first_chain, (size_t) chains * 4, hipMemcpyDeviceToHost) != hipSuccess))
		return FSEQ_E_HIP;
	if (hand_keys && (hipMemcpy(hand_keys, A.hand_keys, blocks * 2, hipMemcpyDeviceToHost) != hipSuccess
	                  || hipMemcpy(hand_flag, A.hand_flag, (size_t) nb_total * 4, hipMemcpyDeviceToHost) != hipSuccess))
		return FSEQ_E_HIP;
	return FSEQ_OK;
}

// one launch of pass 2's streamed chain step on constructed states; hand_keys / hand_flag (both or neither): phase B's hand-over
int debug_pass2_step(int device, uint32_t m, uint32_t nblocks, uint32_t const *a0, uint32_t const *d0, uint32_t const *rank, uint32_t cap,
                     uint32_t ntasks, uint32_t const *task_blk, uint32_t const *cls, uint32_t const *headd, uint32_t const *ncls,
                     uint32_t run_cap, uint32_t workgroups, uint16_t const *hand_keys, uint32_t const *hand_flag, uint32_t *snap_a, uint32_t *snap_d,
                     uint32_t *stats, uint32_t *hand_stats);

} // namespace

extern "C" {

int fseq_debug_pass2_step(int device, uint32_t m, uint32_t nblocks, uint32_t const *a0, uint32_t const *d0, uint32_t const *rank, uint32_t cap,
                          uint32_t ntasks, uint32_t const *task_blk, uint32_t const *cls, uint32_t const *headd, uint32_t const *ncls,
                          uint32_t run_cap, uint32_t workgroups, uint32_t *snap_a, uint32_t *snap_d, uint32_t *stats)
{
	return debug_pass2_step(device, m, nblocks, a0, d0, rank, cap, ntasks, task_blk, cls, headd, ncls, run_cap, workgroups, nullptr, nullptr, snap_a, snap_d,
	                        stats, nullptr);
}

int fseq_debug_pass2_step_keys(int device, uint32_t m, uint32_t nblocks, uint32_t const *a0, uint32_t const *d0, uint32_t const *rank, uint32_t cap,
                               uint32_t ntasks, uint32_t const *task_blk, uint32_t const *cls, uint32_t const *headd, uint32_t const *ncls,
                               uint32_t run_cap, uint32_t workgroups, uint16_t const *hand_keys, uint32_t const *hand_flag, uint32_t *snap_a,
                               uint32_t *snap_d, uint32_t *stats, uint32_t *hand_stats)
{
	if (!hand_keys || !hand_flag || !hand_stats) return FSEQ_E_ARG;
	return debug_pass2_step(device, m, nblocks, a0, d0, rank, cap, ntasks, task_blk, cls, headd, ncls, run_cap, workgroups, hand_keys, hand_flag, snap_a,
	                        snap_d, stats, hand_stats);
}

int fseq_debug_chain_launch_wg_keys(int device, uint32_t m, uint32_t nb_total, uint32_t G, uint64_t cols_per_block, uint32_t const *rank,
                                    uint32_t const *keyd, uint32_t const *nkeys, uint32_t first_chain, uint32_t chains, uint32_t const *start_a,
                                    uint32_t const *start_d, uint32_t run_cap, uint32_t workgroups, uint32_t *out_state_a, uint32_t *out_state_d,
                                    uint32_t *out_rank, uint32_t *out_keyd, uint32_t *out_nkeys, uint32_t *stats, uint16_t *hand_keys, uint32_t *hand_flag)
{
	if (!stats || run_cap > CW_RUN_CAP || !workgroups || workgroups > 1024u || !hand_keys || !hand_flag) return FSEQ_E_ARG;
	return debug_chain_launch(device, m, nb_total, G, cols_per_block, rank, keyd, nkeys, first_chain, chains, start_a, start_d, run_cap, workgroups,
	                          out_state_a, out_state_d, out_rank, out_keyd, out_nkeys, stats, hand_keys, hand_flag);
}

} // extern "C"

namespace {

int debug_pass2_step(int device, uint32_t m, uint32_t nblocks, uint32_t const *a0, uint32_t const *d0, uint32_t const *rank, uint32_t cap,
                     uint32_t ntasks, uint32_t const *task_blk, uint32_t const *cls, uint32_t const *headd, uint32_t const *ncls,
                     uint32_t run_cap, uint32_t workgroups, uint16_t const *hand_keys, uint32_t const *hand_flag, uint32_t *snap_a, uint32_t *snap_d,
                     uint32_t *stats, uint32_t *hand_stats)
{
	// ---- everything an index is formed from, before the first HIP call
	if (!a0 || !d0 || !rank || !task_blk || !cls || !headd || !ncls || !snap_a || !snap_d || !stats) return FSEQ_E_ARG;
	if (m < DEBUG_M_MIN || m > DEBUG_M_MAX || !nblocks || nblocks > 4096u || !ntasks || ntasks > 4096u) return FSEQ_E_ARG;
	if (!cap || cap > P2_CLS_CAP || run_cap > P2_RUN_CAP || !workgroups || workgroups > 1024u) return FSEQ_E_ARG;
	if (!rows_are_permutations(a0, nblocks, m)) return FSEQ_E_ARG;
	for (size_t i = 0; i < (size_t) nblocks * m; ++i)
		if (rank[i] >= cap) return FSEQ_E_ARG;
	// the groups: consecutive tasks of one block (a block's tasks lie together: it forms one group)
	std::vector<uint2> groups;
	{
		std::vector<uint8_t> block_seen(nblocks);
		for (uint32_t t = 0; t < ntasks; ++t)
		{
			if (task_blk[t] >= nblocks) return FSEQ_E_ARG;
			if (t && task_blk[t] == task_blk[t - 1]) { ++groups.back().y; continue; }
			if (block_seen[task_blk[t]]) return FSEQ_E_ARG;
			block_seen[task_blk[t]] = 1;
			groups.push_back(make_uint2(t, 1u));
		}
	}
	for (uint32_t t = 0; t < ntasks; ++t)
	{
		uint32_t const D = ncls[t];
		if (D == 0u || D == 0xFFFFFFFFu) continue;
		if (D > cap) return FSEQ_E_ARG;
		// (the kernel loads all cap entries of the class table into LDS and looks any of them up)
		for (uint32_t j = 0; j < cap; ++j)
			if (cls[(size_t) t * cap + j] >= D) return FSEQ_E_ARG;
	}
	// (a handed-over key is a rank of the block: the class table is looked up at it.  Only behind a set flag: what lies behind a
	// clear one is never read, whatever it holds)
	for (uint32_t b = 0; hand_keys && b < nblocks; ++b)
		for (size_t i = 0; hand_flag[b] && i < m; ++i)
			if (hand_keys[(size_t) b * m + i] >= cap) return FSEQ_E_ARG;
	// largest first, the counter behind them (long_pass2_reduced)
	std::stable_sort(groups.begin(), groups.end(), [](uint2 x, uint2 y) { return x.y > y.y; });
	uint32_t const ngrp = (uint32_t) groups.size();
	std::vector<uint32_t> grp_words(2 * (size_t) ngrp + 1, 0u);
	for (uint32_t g = 0; g < ngrp; ++g) { grp_words[2 * g] = groups[g].x; grp_words[2 * g + 1] = groups[g].y; }

	if (hipSetDevice(device) != hipSuccess) return FSEQ_E_HIP;
	DebugBuffers B;
	size_t const states = (size_t) nblocks * m, outs = (size_t) ntasks * m, tables = (size_t) ntasks * cap;
	uint32_t *d_a0 = B.copy(a0, states), *d_d0 = B.copy(d0, states), *d_rank = B.copy(rank, states);
	uint32_t *d_blk = B.copy(task_blk, ntasks), *d_cls = B.copy(cls, tables), *d_headd = B.copy(headd, tables), *d_ncls = B.copy(ncls, ntasks);
	uint32_t *d_grp = B.copy(grp_words.data(), grp_words.size());
	uint32_t *d_sa = B.words(outs, 0xFF), *d_sd = B.words(outs, 0xFF), *d_stats = B.words(P2_STATS, 0);
	uint32_t *d_ws = B.words((size_t) workgroups * pass2_ws_words(m), 0);
	uint16_t *d_hk = nullptr;
	uint32_t *d_hf = nullptr, *d_hs = nullptr;
	if (hand_keys)
	{
		void *p = B.words((states * 2 + 3) / 4, 0);
		d_hf = B.copy(hand_flag, nblocks); d_hs = B.words(P2_HAND, 0);
		if (!p || !d_hf || !d_hs) return FSEQ_E_OOM;
		d_hk = static_cast<uint16_t *>(p);
		if (hipMemcpy(d_hk, hand_keys, states * 2, hipMemcpyHostToDevice) != hipSuccess) return FSEQ_E_HIP;
	}
	if (!d_a0 || !d_d0 || !d_rank || !d_blk || !d_cls || !d_headd || !d_ncls || !d_grp || !d_sa || !d_sd || !d_stats || !d_ws) return FSEQ_E_OOM;
	if (allow_lds(k_chain_snap_grouped, pass2_lds_bytes()) != hipSuccess) return FSEQ_E_HIP;
	hipLaunchKernelGGL(k_chain_snap_grouped, dim3(workgroups), dim3(ST), pass2_lds_bytes(), 0, d_a0, d_d0, d_rank, m, d_blk, d_cls, d_headd, d_ncls, cap,
	                   reinterpret_cast<uint2 const *>(d_grp), ngrp, d_grp + 2 * (size_t) ngrp, d_sa, d_sd, d_ws, run_cap, d_stats, d_hk, d_hf, d_hs);
	if (hipGetLastError() != hipSuccess || hipDeviceSynchronize() != hipSuccess) return FSEQ_E_HIP;
	if (hipMemcpy(snap_a, d_sa, outs * 4, hipMemcpyDeviceToHost) != hipSuccess || hipMemcpy(snap_d, d_sd, outs * 4, hipMemcpyDeviceToHost) != hipSuccess
	    || hipMemcpy(stats, d_stats, P2_STATS * 4, hipMemcpyDeviceToHost) != hipSuccess)
		return FSEQ_E_HIP;
	if (hand_stats && hipMemcpy(hand_stats, d_hs, P2_HAND * 4, hipMemcpyDeviceToHost) != hipSuccess) return FSEQ_E_HIP;
	return FSEQ_OK;
}

} // namespace

extern "C" {

int fseq_debug_chain_launch(int device, uint32_t m, uint32_t nb_total, uint32_t G, uint64_t cols_per_block, uint32_t const *rank, uint32_t const *keyd,
                            uint32_t const *nkeys, uint32_t first_chain, uint32_t chains, uint32_t const *start_a, uint32_t const *start_d,
                            uint32_t *out_state_a, uint32_t *out_state_d, uint32_t *out_rank, uint32_t *out_keyd, uint32_t *out_nkeys)
{
	return debug_chain_launch(device, m, nb_total, G, cols_per_block, rank, keyd, nkeys, first_chain, chains, start_a, start_d, 0, 0,
	                          out_state_a, out_state_d, out_rank, out_keyd, out_nkeys, nullptr);
}

int fseq_debug_chain_launch_wg(int device, uint32_t m, uint32_t nb_total, uint32_t G, uint64_t cols_per_block, uint32_t const *rank, uint32_t const *keyd,
                               uint32_t const *nkeys, uint32_t first_chain, uint32_t chains, uint32_t const *start_a, uint32_t const *start_d,
                               uint32_t run_cap, uint32_t workgroups, uint32_t *out_state_a, uint32_t *out_state_d, uint32_t *out_rank,
                               uint32_t *out_keyd, uint32_t *out_nkeys, uint32_t *stats)
{
	if (!stats || run_cap > CW_RUN_CAP || !workgroups || workgroups > 1024u) return FSEQ_E_ARG;
	return debug_chain_launch(device, m, nb_total, G, cols_per_block, rank, keyd, nkeys, first_chain, chains, start_a, start_d, run_cap, workgroups,
	                          out_state_a, out_state_d, out_rank, out_keyd, out_nkeys, stats);
}

} // extern "C"
