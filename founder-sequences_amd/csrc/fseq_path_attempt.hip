// fseq_path_attempt.hip -- the segmentation path: one attempt at a list capacity -- phase C and the DP behind phases A and B,
// as stages with one verdict --, the list windows an attempt under a list budget runs in, the loop over attempts, and the
// short path.  Host code only: the unit instantiates no kernel and reaches every one through the launchers of the other
// units (fseq_path.hpp).
#include "fseq_path.hpp"
#include "fseq_dpschedule.hpp"   // the round schedule (list windows, the attempt)

namespace fseq {

namespace {

// ---- a list budget (fseq_set_list_memory): pass 1's lists in windows of wb consecutive column blocks.  Window w = blocks
// [lo_w, hi_w) holds the lists of the columns [lo_w B - H, hi_w B) in one buffer (d_ent rebased to (lo_w B - H) stride:
// the kernels address lists as they always do); phase C writes the window's own columns, the DP runs the rounds whose
// lists are all there, and the last H columns move to the front for the next window.  H: the columns in front of a window
// that its first DP round still reads.

// DP rounds [.., r) that the lists of the columns < hi_w B feed: every regular round that reads no later column (its cells
// read the lists of the columns e0 - 1 .. e0 + len - 2: dp_rounds_within); the drain round and the final cell wait for the
// last window (the drain round's loads read column n - L, which an earlier window's buffer need not hold)
uint32_t window_round_hi(fseq_ctx const *c, DpSchedule const &S, uint32_t hi_w)
{
	if (hi_w >= c->nblocks) return S.nrounds;
	return std::min(dp_rounds_within(S, (uint64_t) hi_w * c->B), S.nreg);
}

// the window shape at list capacity X: the most blocks a window may have with the halo its rounds need beside them
int plan_list_windows(fseq_ctx *c, uint32_t X)
{
	fseq_ctx::ListWindows &W = c->lw;
	W.on = false;
	W.merge_windows = 0;
	uint64_t const n = c->p.n, L = c->p.segment_length, B = c->B, nb = c->nblocks;
	if (!W.budget || c->sh.on || n < 2 * L) return FSEQ_OK;
	uint64_t const stride = (X + 3) & ~1u, per_col = stride * sizeof(uint2), pad = 256 * sizeof(uint2);
	if (n * per_col + pad <= W.budget) return FSEQ_OK;              // every list fits: the run as without a budget
	DpSchedule const S = dp_schedule((uint32_t) L, (uint32_t) n);
	uint64_t const cols = W.budget > pad ? (W.budget - pad) / per_col : 0;
	// the halo that windows of wb blocks need: how far in front of a window the lowest column lies that its rounds read
	auto halo_of = [&](uint64_t wb) {
		uint64_t need = 0;
		uint32_t r_lo = 0;
		for (uint64_t lo = 0; lo < nb; lo += wb)
		{
			uint64_t const hi = std::min(nb, lo + wb);
			uint32_t const r_hi = window_round_hi(c, S, (uint32_t) hi);
			if (r_hi > r_lo)
			{
				uint64_t const first = (uint64_t) dp_round(S, r_lo).e0 - 1u;     // the lowest column the window's rounds read
				if (lo * B > first) need = std::max(need, lo * B - first);
				r_lo = r_hi;
			}
		}
		return need;
	};
	auto take = [&](uint64_t wb, uint64_t H) {
		W.on = true;
		W.wb = (uint32_t) wb; W.H = (uint32_t) H;
		W.nwin = (uint32_t) ((nb + wb - 1) / wb);
		W.bytes = (H + wb * B) * per_col + pad;
		return FSEQ_OK;
	};
	uint64_t H = S.RL;                                              // (a first guess, raised to what the windows' rounds read)
	for (int it = 0; it < 64; ++it)
	{
		uint64_t const wb = cols > H ? std::min<uint64_t>(nb, (cols - H) / B) : 0;
		// (the halo moves to the front in one copy: a window must be at least as wide as the halo)
		if (wb == 0 || wb * B < H) break;
		uint64_t const need = halo_of(wb);
		if (need <= H) return take(wb, H);
		H = need;
	}
	// The halo is no monotonic function of the window width: the drain round and the final cell wait for the last window and
	// read from column n - L on, so the last window's halo is its start minus n - L -- up to L columns, and a few blocks more
	// or less per window move that start anywhere.  Where the iteration above has run into a halo that leaves no window (or
	// has not settled), every width is tried, the widest first.
	uint64_t const wb_most = cols > S.RL ? std::min<uint64_t>(nb, (cols - S.RL) / B) : 0;
	for (uint64_t wb = wb_most; wb >= 1; --wb)
	{
		uint64_t const Hw = std::max<uint64_t>(S.RL, halo_of(wb));
		if (Hw + wb * B <= cols && wb * B >= Hw) return take(wb, Hw);
	}
	// no width fits: the refusal names the least shape that would (one window of all blocks is a shape, so there is one)
	uint64_t wb_least = nb, H_least = S.RL;
	for (uint64_t wb = 1; wb < nb; ++wb)
	{
		uint64_t const Hw = std::max<uint64_t>(S.RL, halo_of(wb));
		if (wb * B >= Hw && Hw + wb * B < H_least + wb_least * B) { wb_least = wb; H_least = Hw; }
	}
	char what[320];
	snprintf(what, sizeof(what), "list memory budget of %llu bytes holds no window: one window of %llu column block(s) of %llu columns plus a halo of %llu columns "
	         "at list capacity %u needs %llu bytes", (unsigned long long) W.budget, (unsigned long long) wb_least, (unsigned long long) B, (unsigned long long) H_least, X,
	         (unsigned long long) ((H_least + wb_least * B) * per_col + pad));
	return fail(c, FSEQ_E_OOM, what);
}

} // namespace

// the buffer holds window [lo_w, ..): column k at d_ent + k * stride
void set_list_window(fseq_ctx *c, uint32_t lo_w)
{
	c->d_ent.rebase(((int64_t) lo_w * c->B - (int64_t) c->lw.H) * (int64_t) c->stride);
}

// phase C (lists, headers, stride states) of the blocks [lo, hi): on their representatives where this attempt's plan put
// them (the plan's block lists ascend within every configuration, so a window's blocks are one stretch of each), else on
// all rows
int window_phase_c(fseq_ctx *c, uint32_t lo, uint32_t hi)
{
	if (!c->red_active)
	{
		launch_columns(c, lo, hi - lo);
		return FSEQ_OK;
	}
	RedPlan const &plan = c->red.plan;
	uint32_t const *const h_blocks = plan.blocks.data();             // (what d_red_blocks holds)
	auto stretch = [&](uint32_t first, uint32_t count) {
		uint32_t const *const b = h_blocks + first, *const e = b + count;
		uint32_t const *const a = std::lower_bound(b, e, lo), *const z = std::lower_bound(b, e, hi);
		return std::make_pair(first + (uint32_t) (a - b), (uint32_t) (z - a));
	};
	RedArgs RA;
	red_fill_args(c, RA);
	std::vector<RedLaunch> ls;
	for (auto const &bin : plan.bins)
	{
		auto const r = stretch(bin.first, bin.count);
		if (r.second) ls.push_back(RedLaunch{bin.config, r.first, r.second});
	}
	std::stable_sort(ls.begin(), ls.end(), [](RedLaunch const &x, RedLaunch const &y) { return x.count > y.count; });
	int rc;
	if ((rc = red_launch_all(c, ls, RA, list_args(c)))) return rc;
	auto const f = stretch(plan.full_at, plan.nfull);
	if (f.second) launch_columns(c, 0, f.second, c->d_red_blocks + f.first);
	return FSEQ_OK;
}

namespace {

// pass 1 + the DP window by window (queued on the context's stream; overflow lands in d_flags as for the whole-array DP)
int long_windows_cd(fseq_ctx *c, DpSchedule const &S)
{
	FSEQ_LONG_LOCALS(c);
	fseq_ctx::ListWindows &W = c->lw;
	while (W.ev.size() < 2 * (size_t) W.nwin)
	{
		hipEvent_t e = nullptr;
		HIP_TRY(c, hipEventCreate(&e));
		W.ev.push_back(e);
	}
	// (the entries no cell writes -- between the last regular cell and the final one -- read 0, as after dp_spec_reset)
	HIP_TRY(c, hipMemsetAsync(c->dp.M, 0, c->dp_size * 4, st));
	HIP_TRY(c, hipMemsetAsync(c->dp.LB, 0, c->dp_size * 4, st));
	HIP_TRY(c, hipMemsetAsync(c->dp.SZ, 0, c->dp_size * 4, st));
	uint32_t r_lo = 0, w = 0, lo = 0;
	for (; lo < c->nblocks; lo += W.wb, ++w)
	{
		uint32_t const hi = std::min(c->nblocks, lo + W.wb);
		if (lo && W.H)
			HIP_TRY(c, hipMemcpyAsync(c->d_ent.base, c->d_ent.base + (size_t) W.wb * c->B * c->stride, (size_t) W.H * c->stride * sizeof(uint2), hipMemcpyDeviceToDevice, st));
		set_list_window(c, lo);
		if ((rc = window_phase_c(c, lo, hi))) return rc;
		uint32_t const r_hi = window_round_hi(c, S, hi);
		HIP_TRY(c, hipEventRecord(W.ev[2 * (size_t) w], st));
		if (r_hi > r_lo)
		{
			launch_dp_serial(c, DP_PARTIAL, st, r_lo, r_hi);
			r_lo = r_hi;
		}
		HIP_TRY(c, hipEventRecord(W.ev[2 * (size_t) w + 1], st));
	}
	HIP_TRY(c, hipGetLastError());
	uint32_t const lo_last = (W.nwin - 1u) * W.wb;
	W.col_lo = (uint64_t) lo_last * c->B; W.col_hi = n;
	if (c->tune.debug)
		fprintf(stderr, "[fseq] list windows: %u windows of %u blocks (%llu columns) + a halo of %u columns, %.2f GB of lists at X = %u\n", W.nwin, W.wb,
		        (unsigned long long) W.wb * c->B, W.H, W.bytes / 1e9, c->X);
	return FSEQ_OK;
}

// ---- one attempt at the list capacity R.X: phase C and the DP queued behind phases A and B, one read-back, one verdict
enum class Attempt {
	Stands,                                  // the DP's result is proven: on to pass 2
	Again,                                   // the same capacity once more: with a fresh plan, or the flagged blocks on all rows
	Overflow                                 // a list was too short to prove a cell: a larger capacity
};

// what the stages of an attempt share
struct AttemptState {
	double t0 = 0;                           // (FSEQ_DEBUG: the attempt's marks)
	bool red_candidate = false;              // phase C may run on the blocks' representatives
	bool windowed = false, use_spec = false; // the lists in column windows; the DP as speculative sweeps
	DpSchedule S{};
	SpecPlan spec;
	uint32_t spec_overflow = 0, spec_sweeps = 0;
};

void mark(fseq_ctx const *c, AttemptState const &A, char const *what)
{
	if (c->tune.debug) fprintf(stderr, "[fseq]   attempt +%.3f ms %s\n", now_ms() - A.t0, what);
}

// stage 1: what an attempt settles before it queues anything: the list windows' plan, the work buffers, the DP's words
// cleared, the DP's schedule and chunk plan
int attempt_prepare(fseq_ctx *c, LongRun const &R, AttemptState &A)
{
	FSEQ_LONG_LOCALS(c);
	// [r5] phase C on representative rows: the default wherever the lists are consumed by the speculative DP behind phase C
	// (sharded: a rank's own blocks; its halo block has no state behind it to take the classes from and runs on all rows)
	A.red_candidate = !c->tune.no_reduced && n >= 2 * L;
	A.t0 = now_ms();
	// a list budget the lists at this capacity exceed: pass 1 and the DP in column windows (long_windows_cd)
	if ((rc = plan_list_windows(c, R.X))) return rc;
	A.windowed = c->lw.on;
	if ((rc = ensure_work_buffers(c, R.X, !A.red_candidate))) return rc;
	mark(c, A, "lists allocated");
	// the DP's words, and in a diagnostic build what it writes behind the production words; never phase A's counters, which
	// were written on this stream before and are read at the attempt's end
	HIP_TRY(c, hipMemsetAsync(path_words(c)->dp, 0, sizeof(PathWords::dp), st));
#if defined(FSEQ_DP_STAMPS) || defined(FSEQ_DP_STATS)
	HIP_TRY(c, hipMemsetAsync(path_words(c)->dp_stamps, 0, sizeof(PathWords) - offsetof(PathWords, dp_stamps), st));
#endif
	if (c->tune.poison_lists)
	{
		// tests of what the DP reads: a list or a header that phase C has not written (a column outside a window's buffer, a
		// block no launch covered) must not look right by accident
		HIP_TRY(c, hipMemsetAsync(c->d_ent.base, 0xFF, c->d_ent.cap * sizeof(uint2), st));
		HIP_TRY(c, hipMemsetAsync(c->d_hdr, 0xFF, (size_t) n * sizeof(uint4), st));
	}
	A.S = dp_schedule((uint32_t) L, (uint32_t) n);
	// the DP as chunk-speculative sweeps over the whole chip once every list is written (fseq_dpspec.hpp); the serial kernel for
	// inputs too short for three chunks (and FSEQ_DP_SERIAL), and window by window under a list budget
	A.spec = spec_plan(c, A.S);
	A.use_spec = !A.windowed && (sharded || A.spec.nchunks() > 0);
	if (sharded && A.spec.nchunks() < 1) return fail(c, FSEQ_E_UNSUPPORTED, "sharded run: no DP chunk plan");
	return FSEQ_OK;
}

// stage 2: phase C (lists, headers, stride states) of every block of mine, on the blocks' representatives where this attempt's
// plan takes them (red_plan).  What is launched:
//
//                      the whole alignment              list windows                   a rank's blocks + its halo block
//   representatives    red_columns, then the plan's     window by window:              red_columns, the plan's all-rows list,
//   (a plan in use)    all-rows list in one launch      window_phase_c, then the DP    then the halo block on all rows
//   all rows           window_phase_c(0, nblocks):      rounds its lists feed          one launch: my blocks and the halo
//                      one launch over every block      (long_windows_cd)              block
//
// The whole alignment on its representatives is not window_phase_c(0, nblocks): a window queues the configurations' launches in
// a stable order by block count (it holds a stretch of every configuration), red_columns the largest workgroups first, and the
// order of the launches in a stream is behaviour here.  A sharded run has no windows (plan_list_windows).
// FSEQ_SYNC_PHASES=C waits behind the last launch of every case.
int attempt_phase_c(fseq_ctx *c, LongRun const &R, AttemptState const &A)
{
	FSEQ_LONG_LOCALS(c);
	c->red_active = false;
	if (A.red_candidate)
	{
		if ((rc = red_plan(c, R.X, &c->red_active))) return rc;
		mark(c, A, "reduced plan");
		if (!c->red_active && (rc = ensure_work_buffers(c, R.X, true))) return rc;      // (the stride states after all)
	}
	uint32_t const halo = sharded && sh.c_end > sh.c_hi ? 1u : 0u;      // the block behind mine for as far as the halo reaches (k_columns stops at n_c)
	if (A.windowed)
	{
		// (phase C of a window, then the DP rounds its lists feed -- the DP is queued here, inside phase C's events)
		if ((rc = long_windows_cd(c, A.S))) return rc;
	}
	else if (c->red_active)
	{
		if ((rc = red_columns(c))) return rc;
		mark(c, A, "reduced columns queued");
		// the blocks that run on all rows, in one launch (no stride states: pass 2 reaches their boundaries from the block's start)
		if (c->red.plan.nfull) launch_columns(c, 0, c->red.plan.nfull, c->d_red_blocks + c->red.plan.full_at);
		if (halo) launch_columns(c, b_hi, 1u);
	}
	else if (!sharded)
	{
		if ((rc = window_phase_c(c, 0, c->nblocks))) return rc;
	}
	else if (my_blocks)
		launch_columns(c, b_lo, my_blocks + halo);
	if (sync_at(c, 'C')) { fprintf(stderr, "[fseq] phase C queued\n"); HIP_TRY(c, hipStreamSynchronize(st)); fprintf(stderr, "[fseq] phase C done\n"); }
	return FSEQ_OK;
}

// stage 3, sharded: the ranks agree on whether the attempt stands BEFORE the DP's exchanges: a rank whose lists could not be
// proven on the representatives (or whose plan's counts have changed) makes every rank run the attempt again.  *again: they do
int attempt_shard_agreement(fseq_ctx *c, LongRun &R, bool *again)
{
	FSEQ_LONG_LOCALS(c);
	RedFlags mine{0u, 0u};
	if (c->red_active)
	{
		HIP_TRY(c, hipMemcpyAsync(&mine, red_flags(c), sizeof(mine), hipMemcpyDeviceToHost, st));
		HIP_TRY(c, hipStreamSynchronize(st));
	}
	uint32_t word = (mine.unproven ? 1u : 0u) | (mine.plan_stale ? 2u : 0u);
	HIP_TRY(c, hipMemcpyAsync(sh.xbuf, &word, 4, hipMemcpyHostToDevice, st));
	if ((rc = shard_exchange(c, 1, 1))) return rc;
	uint32_t all = 0;
	HIP_TRY(c, hipMemcpy(&all, sh.xbuf, 4, hipMemcpyDeviceToHost));
	*again = all != 0;
	if (!all) return FSEQ_OK;
	if (mine.plan_stale) c->red.memory.forget_plan();
	if (mine.unproven)
	{
		uint32_t cnt = 0, wide = 0;
		if ((rc = red_take_invalid(c, b_lo, b_hi, &cnt, &wide))) return rc;
		c->red.memory.forget_plan();
		R.redone += cnt;
	}
	return FSEQ_OK;
}

// stage 4: the DP behind phase C: the speculative sweeps, or the serial kernel over every round; nothing for windows, whose
// rounds stage 2 has queued.  skip: the ranks send the attempt round again (stage 3) -- it waits for the reset all the same,
// as the next attempt queues one anew
int attempt_queue_dp(fseq_ctx *c, AttemptState &A, bool skip)
{
	hipStream_t st = c->stream;
	if (A.use_spec) HIP_TRY(c, hipStreamWaitEvent(st, c->ev.dp_reset, 0));      // the DP arrays were reset beside phase C
	if (skip) return FSEQ_OK;
	if (A.use_spec) return run_dp_spec(c, A.S, A.spec, st, &A.spec_overflow, &A.spec_sweeps, true);
	if (!A.windowed) launch_dp_serial(c, DP_WHOLE, st, 0u, A.S.nrounds);
	return FSEQ_OK;
}

// the attempt's share of the phases' times, whatever its verdict (the stream has been synchronised: every event is complete)
int attempt_times(fseq_ctx *c, LongRun &R, AttemptState const &A)
{
	float f = 0;
	HIP_TRY(c, hipEventElapsedTime(&f, c->ev.c_begin, c->ev.c_end)); R.ms_c += f;
	HIP_TRY(c, hipEventElapsedTime(&f, c->ev.dp_begin, c->ev.dp_end)); R.ms_dp += f;
	for (uint32_t w = 0; A.windowed && w < c->lw.nwin; ++w)
	{
		// (the windows' DP launches ran between phase C's events)
		HIP_TRY(c, hipEventElapsedTime(&f, c->lw.ev[2 * (size_t) w], c->lw.ev[2 * (size_t) w + 1]));
		R.ms_c -= f; R.ms_dp += f;
	}
	return FSEQ_OK;
}

// stage 5: the words into their pinned mirror and one synchronisation; the verdict; then, whatever it is, phase A's counts and
// the times.  agreed_again: the ranks have decided (stage 3) and no DP ran
int attempt_decide(fseq_ctx *c, LongRun &R, AttemptState const &A, bool agreed_again, Attempt *verdict)
{
	FSEQ_LONG_LOCALS(c);
	if ((rc = pin_reserve(c, 64))) return rc;
	AttemptWords *const h = pin_take<AttemptWords>(c, 1);
	*h = AttemptWords{};
	if (!agreed_again) HIP_TRY(c, hipMemcpyAsync(h->dp, path_words(c)->dp, sizeof(h->dp), hipMemcpyDeviceToHost, st));
	if (R.keyspace) HIP_TRY(c, hipMemcpyAsync(&h->phase_a, &path_words(c)->phase_a, sizeof(h->phase_a), hipMemcpyDeviceToHost, st));
	if (c->red_active && !sharded) HIP_TRY(c, hipMemcpyAsync(&h->red, red_flags(c), sizeof(h->red), hipMemcpyDeviceToHost, st));      // (sharded: agreed on before the DP)
	HIP_TRY(c, hipStreamSynchronize(st));
	*verdict = agreed_again ? Attempt::Again : ((h->dp[0] & 1u) != 0 || A.spec_overflow != 0) ? Attempt::Overflow : Attempt::Stands;
	if (c->red_active && h->red.plan_stale)
	{
		// (the counts are not what the plan was made from: plan afresh)
		c->red.memory.forget_plan();
		*verdict = Attempt::Again;
	}
	else if (c->red_active && h->red.unproven)
	{
		uint32_t cnt = 0, wide = 0;
		if ((rc = red_take_invalid(c, 0, c->nblocks, &cnt, &wide))) return rc;
		if (c->tune.debug) fprintf(stderr, "[fseq] reduced phase C: the lists of %u blocks reach below what their representatives vouch for: those blocks again on all rows\n", cnt - wide);
		if (c->tune.debug && wide) fprintf(stderr, "[fseq] reduced phase C: %u blocks hold more distinct start values than the slim configuration's table: those blocks again on the next configuration\n", wide);
		if (cnt) { R.redone += cnt; *verdict = Attempt::Again; }
	}
	if ((rc = phase_a_take_counts(c, R, h->phase_a))) return rc;
	return attempt_times(c, R, A);
}

#if defined(FSEQ_DP_STAMPS) || defined(FSEQ_DP_STATS)
// stage 6, diagnostic builds: what the serial DP of an attempt that was not sent round again left behind the production words
int attempt_dump_diagnostics(fseq_ctx *c)
{
#ifdef FSEQ_DP_STAMPS
	{
		unsigned long long stamps[96];
		HIP_TRY(c, hipMemcpy(stamps, path_words(c)->dp_stamps, sizeof(stamps), hipMemcpyDeviceToHost));
		for (int w = 0; w < 16; ++w)
		{
			unsigned long long const *q = stamps + 48 + 3 * w;
			double const nr = (double) (stamps[3 * w + 2] ? stamps[3 * w + 2] : 1);
			fprintf(stderr, "[dp stamps] wave %2d cycles/round: barrier 1 = %.0f, update = %.0f, barrier 2 = %.0f\n", w, q[0] / nr, q[1] / nr, q[2] / nr);
		}
		for (int w = 0; w < 16; ++w)
		{
			unsigned long long const *q = stamps + 3 * w;
			double const nr = (double) (q[2] ? q[2] : 1);
			fprintf(stderr, "[dp stamps] wave %2d rounds=%llu cycles/round: work=%.0f waits=%.0f\n", w, q[2], q[0] / nr, q[1] / nr);
		}
	}
#endif
#ifdef FSEQ_DP_STATS
	{
		uint32_t hist[34];
		HIP_TRY(c, hipMemcpy(hist, path_words(c)->dp_hist, sizeof(hist), hipMemcpyDeviceToHost));
		fprintf(stderr, "[dp stats] list entries a cell needed (cell-pair path; last = more than 32):");
		for (int i = 0; i < 34; ++i) fprintf(stderr, " %u", hist[i]);
		fprintf(stderr, "\n");
	}
#endif
	return FSEQ_OK;
}
#endif

// stages 1 to 5 in turn: the attempt up to its verdict.  What a run (long_attempt) and a scan over segment lengths
// (long_attempts_to_proof) share
int attempt_to_verdict(fseq_ctx *c, LongRun &R, AttemptState &A, Attempt *verdict)
{
	FSEQ_LONG_LOCALS(c);
	if ((rc = attempt_prepare(c, R, A))) return rc;
	HIP_TRY(c, hipEventRecord(c->ev.c_begin, st));
	RangeScope range_cd("fseq pass 1: phases C + D (column updates + lists, segmentation DP)");
	if (A.use_spec)
	{
		// the arrays the speculative DP starts from are reset on the second stream while phase C runs
		if ((rc = dp_spec_reset(c, A.spec, c->stream2))) return rc;
		HIP_TRY(c, hipEventRecord(c->ev.dp_reset, c->stream2));
	}
	if ((rc = attempt_phase_c(c, R, A))) return rc;
	bool again = false;
	if (sharded && A.red_candidate && (rc = attempt_shard_agreement(c, R, &again))) return rc;
	HIP_TRY(c, hipEventRecord(c->ev.c_end, st));
	HIP_TRY(c, hipEventRecord(c->ev.dp_begin, st));
	if ((rc = attempt_queue_dp(c, A, again))) return rc;
	HIP_TRY(c, hipEventRecord(c->ev.dp_end, st));
	HIP_TRY(c, hipGetLastError());
	mark(c, A, "DP queued");
	return attempt_decide(c, R, A, again, verdict);
}

// the ordinary retry rule behind a verdict of overflow: twice the capacity and one, at most every row
int attempt_grow_capacity(fseq_ctx *c, LongRun &R)
{
	uint32_t const m = c->p.m;
	if (R.X >= m) return fail(c, FSEQ_E_HIP, "internal: divergence lists complete but DP flagged overflow");
	R.X = (uint32_t) std::min<uint64_t>(m, (uint64_t) R.X * 2 + 1);
	++R.retries;
	if (c->tune.debug) fprintf(stderr, "[fseq] divergence lists too short, retry %u with X = %u\n", R.retries, R.X);
	return FSEQ_OK;
}

// the stages in turn; stage 7, behind a verdict that is not "again": the traceback and the merge (which may still find a list too short)
int long_attempt(fseq_ctx *c, LongRun &R, Attempt *verdict)
{
	FSEQ_LONG_LOCALS(c);
	AttemptState A;
	if ((rc = attempt_to_verdict(c, R, A, verdict))) return rc;
	if (*verdict == Attempt::Again) return FSEQ_OK;
#if defined(FSEQ_DP_STAMPS) || defined(FSEQ_DP_STATS)
	if ((rc = attempt_dump_diagnostics(c))) return rc;
#endif
	progress(c, FSEQ_STAGE_TRACEBACK, n, n);
	RangeScope range_tb("fseq traceback + find_segments_greedy");
	double const th0 = now_ms();
	bool overflow = *verdict == Attempt::Overflow;
	c->tm.dp_sweeps = A.spec_sweeps;
	c->tm.dp_chunks = A.use_spec ? A.spec.nchunks() : 0u;

	if (!overflow && (rc = long_traceback_and_merge(c, th0, &overflow))) return rc;
	R.ms_host += now_ms() - th0;
	range_tb.end();
	if (!overflow) progress(c, FSEQ_STAGE_MERGE, c->traceback.size(), c->traceback.size());
	if (c->tune.debug) fprintf(stderr, "[fseq] host: traceback + merge %.3f ms\n", now_ms() - th0);
	*verdict = overflow ? Attempt::Overflow : Attempt::Stands;
	return FSEQ_OK;
}

} // namespace

// ---- what a scan over segment lengths shares with a run (csrc/fseq_lengthscan.hip)
// Attempts at the context's segment length, from the capacity R.X on, until the DP's result is proven; they stop at the verdict:
// no traceback, merge or pass 2.  Phases A and B of R are behind the stream.
int long_attempts_to_proof(fseq_ctx *c, LongRun &R, DpProof *proof)
{
	int rc;
	for (Attempt verdict = Attempt::Again; verdict != Attempt::Stands;)
	{
		AttemptState A;
		if ((rc = attempt_to_verdict(c, R, A, &verdict))) return rc;
		if (verdict == Attempt::Overflow && (rc = attempt_grow_capacity(c, R))) return rc;
		proof->dp_chunks = A.use_spec ? A.spec.nchunks() : 0u;
		proof->dp_sweeps = A.spec_sweeps;
	}
	HIP_TRY(c, hipMemcpy(&proof->max_segment_size, c->dp.M + (c->dp_size - 1), 4, hipMemcpyDeviceToHost));
	return FSEQ_OK;
}

// The DP alone on the lists the context holds, in the form a run at the context's segment length chooses (the speculative sweeps,
// or the serial kernel where the input is too short for three chunks): its words cleared, the schedule and the chunk plan of this
// length, and the words and the final cell's entry back in one round trip.  *unproven: a list was too short to prove a cell.
int long_dp_on_lists(fseq_ctx *c, DpProof *proof, bool *unproven)
{
	FSEQ_LONG_LOCALS(c);
	HIP_TRY(c, hipMemsetAsync(path_words(c)->dp, 0, sizeof(PathWords::dp), st));
	DpSchedule const S = dp_schedule((uint32_t) L, (uint32_t) n);
	SpecPlan const spec = spec_plan(c, S);
	uint32_t spec_overflow = 0;
	proof->dp_chunks = spec.nchunks();
	proof->dp_sweeps = 0;
	if (spec.nchunks() > 0) { if ((rc = run_dp_spec(c, S, spec, st, &spec_overflow, &proof->dp_sweeps))) return rc; }
	else launch_dp_serial(c, DP_WHOLE, st, 0u, S.nrounds);
	HIP_TRY(c, hipGetLastError());
	if ((rc = pin_reserve(c, 64))) return rc;
	uint32_t *const h = pin_take<uint32_t>(c, 8);
	HIP_TRY(c, hipMemcpyAsync(h, path_words(c)->dp, sizeof(PathWords::dp), hipMemcpyDeviceToHost, st));
	HIP_TRY(c, hipMemcpyAsync(h + 4, c->dp.M + (c->dp_size - 1), 4, hipMemcpyDeviceToHost, st));
	HIP_TRY(c, hipStreamSynchronize(st));
	*unproven = (h[0] & 1u) != 0 || spec_overflow != 0;
	proof->max_segment_size = h[4];
	return FSEQ_OK;
}

int run_long_path(fseq_ctx *c, fseq_result *res)
{
	FSEQ_LONG_LOCALS(c);
	LongRun R;
	R.X = p.list_cap ? p.list_cap : std::max(FSEQ_X_FLOOR, c->X_hint);
	c->tm = fseq_timings{};
	c->tm.block_len = c->B;
	c->tm.n_blocks = c->nblocks;
	double const t_begin = now_ms();

	// (FSEQ_DEBUG: where the host's wall time of a run goes -- a first run on a context allocates, loads code objects, plans)
	auto mark = [&](char const *what) { if (c->tune.debug) fprintf(stderr, "[fseq] +%.3f ms %s\n", now_ms() - t_begin, what); };
	if ((rc = ensure_work_buffers(c, 0))) return rc;
	mark("work buffers");
	auto close_ab = [&](int code) { if (R.range_ab_open) { FSEQ_RANGE_POP(); R.range_ab_open = false; } return code; };
	if ((rc = long_phase_a(c, R))) return close_ab(rc);
	mark("phase A queued");
	if ((rc = long_phase_b(c, R))) return close_ab(rc);
	mark("phase B queued");
	if ((rc = long_list_capacity(c, R))) return rc;
	mark("list capacity");
	// (sharded: the thresholds are the same on every rank, so every rank takes the same way here)
	for (Attempt verdict = Attempt::Again; verdict != Attempt::Stands;)
	{
		if ((rc = long_attempt(c, R, &verdict))) return rc;
		mark("attempt done");
		switch (verdict)
		{
		case Attempt::Stands: break;
		case Attempt::Again: break;            // (the same capacity; the blocks that were flagged run on all rows now)
		case Attempt::Overflow:
			if ((rc = attempt_grow_capacity(c, R))) return rc;
			break;
		}
	}
	c->X_hint = R.X;                         // later runs on this context start with the capacity that worked
	c->res.segment_count = c->segments.size();
	if ((rc = long_pass2(c, R))) return rc;
	mark("pass 2 done");
	uint32_t const X = R.X, retries = R.retries;
	double const ms_c = R.ms_c, ms_dp = R.ms_dp, ms_host = R.ms_host, ms_p2 = R.ms_p2;
	uint64_t const pass2_cells = R.pass2_cells;
	size_t const S2 = c->segments.size();
	{
		float f = 0;
		HIP_TRY(c, hipEventElapsedTime(&f, c->ev.a_begin, c->ev.a_end_b_begin)); c->tm.ms_phase_a = f;
		HIP_TRY(c, hipEventElapsedTime(&f, c->ev.a_end_b_begin, c->ev.b_end)); c->tm.ms_phase_b = f;
	}
	c->tm.ms_phase_c = ms_c;
	c->tm.ms_dp = ms_dp;
	c->tm.ms_pass2 = ms_p2;
	c->tm.ms_host = ms_host;
	c->tm.ms_colstep_kernels = c->tm.ms_phase_a + ms_c + ms_p2;
	c->tm.colstep_launches = 2 + retries + (S2 ? 1 : 0);
	c->tm.colstep_cells = (uint64_t) m * n * (2 + retries) + pass2_cells;
	c->tm.pass2_cells = pass2_cells;
	c->tm.list_cap_used = X;
	c->tm.retries = retries;
	c->tm.reduced_redone = R.redone;
	if (!c->red_active) { c->tm.reduced_blocks = 0; c->tm.reduced_rows_mean = 0; }
	c->tm.ms_total = now_ms() - t_begin;
	c->have_result = true;
	*res = c->res;
	if (!(c->res.max_segment_size < m))
		return fail(c, FSEQ_E_NO_REDUCTION, "Unable to reduce the number of sequences; the maximum segment size is equal to the number of input sequences.");
	return FSEQ_OK;
}

// segmentation_sp_context::process (segmentation_sp_context.cc:21-28): one sweep over all n columns
// from the identity; the distinct rows are the block keys of a single block [0, n).
int run_short_path(fseq_ctx *c, fseq_result *res)
{
	fseq_params const &p = c->p;
	uint32_t const m = p.m;
	hipStream_t st = c->stream;
	int rc;
	c->tm = fseq_timings{};
	double const t_begin = now_ms();
	DevTemp<uint32_t> d_rank(c), d_keyd(c), d_nk(c);
	if ((rc = d_rank.alloc(m)) || (rc = d_keyd.alloc(m)) || (rc = d_nk.alloc(4))) return rc;
	if (c->use_stream && !c->d_ws && (rc = c->d_ws.alloc(c, (size_t) 4 * m))) return rc;
	if ((rc = short_phase_a(c, d_rank, d_keyd, d_nk))) return rc;
	std::vector<uint32_t> rank(m);
	uint32_t nk = 0;
	hipError_t e1 = hipMemcpyAsync(rank.data(), d_rank, (size_t) m * 4, hipMemcpyDeviceToHost, st);
	hipError_t e2 = hipMemcpyAsync(&nk, d_nk, 4, hipMemcpyDeviceToHost, st);
	hipError_t e3 = hipStreamSynchronize(st);
	release_all(c, d_rank, d_keyd, d_nk);                          // (not held through the host's part below)
	if (e1 != hipSuccess) return fail(c, FSEQ_E_HIP, "short path copy", e1);
	if (e2 != hipSuccess) return fail(c, FSEQ_E_HIP, "short path copy", e2);
	if (e3 != hipSuccess) return fail(c, FSEQ_E_HIP, "short path sync", e3);
	// identical rows keep ascending row-id order in the pBWT, so a run's first row is its smallest id
	c->sp_first.assign(nk, 0xFFFFFFFFu);
	c->sp_len.assign(nk, 0);
	for (uint32_t r = 0; r < m; ++r)
	{
		uint32_t const k = rank[r];
		if (c->sp_first[k] == 0xFFFFFFFFu) c->sp_first[k] = r;
		++c->sp_len[k];
	}
	c->res = fseq_result{};
	c->res.max_segment_size = nk;
	c->res.short_path = 1;
	c->traceback.clear();
	c->segments.clear();
	c->tm.colstep_launches = 1;
	c->tm.colstep_cells = (uint64_t) m * p.n;
	c->tm.ms_total = now_ms() - t_begin;
	c->have_result = true;
	*res = c->res;
	if (!(nk < m))
		return fail(c, FSEQ_E_NO_REDUCTION, "Unable to reduce the number of sequences; the maximum segment size is equal to the number of input sequences.");
	return FSEQ_OK;
}

} // namespace fseq
