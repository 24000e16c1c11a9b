// fseq_path_dp.hip -- the segmentation path, phase D and what follows it: the chunk-speculative DP driver and the serial DP's
// launcher, the tracebacks, the greedy merge of the traceback's segments (whole lists, or list windows), and the debug entry
// points of the range-minimum query and of the traceback by parts.  The one unit that instantiates k_dp<> and includes
// fseq_dpspec.hpp.
// (The units of the path and what crosses them: fseq_path.hpp.)
#include "fseq_path.hpp"
#include "fseq_kernels.hpp"
#include "fseq_dp.hpp"
#include "fseq_dpspec.hpp"
#include "fseq_tbcheck.hpp"

namespace fseq {

namespace {

// one launcher per traceback kernel, on plain pointers (a run's buffers, or fseq_debug_traceback_parts' own)
void launch_tb_windows(hipStream_t st, uint32_t const *LB, uint32_t dp_size, uint32_t L, uint32_t *exit_next, uint32_t *exit_cnt, uint32_t vlo, uint32_t vhi)
{
	uint32_t const nwin = (dp_size + TB_WIN - 1u) / TB_WIN;
	hipLaunchKernelGGL(k_tb_windows, dim3(nwin), dim3(256), 0, st, LB, dp_size, L, exit_next, exit_cnt, vlo, vhi);
}

void launch_tb_chain_part(hipStream_t st, uint32_t const *exit_next, uint32_t const *exit_cnt, uint32_t start, uint32_t off0, uint32_t vlo, uint2 *head, uint32_t nwin,
                          uint32_t *count, uint32_t *word)
{
	hipLaunchKernelGGL(k_tb_chain_part, dim3(1), dim3(64), 0, st, exit_next, exit_cnt, start, off0, vlo, head, nwin, count, word);
}

void launch_tb_emit(hipStream_t st, uint32_t const *LB, uint32_t const *M, uint32_t const *SZ, uint32_t dp_size, uint32_t L, uint2 const *head, uint32_t *count,
                    uint4 *out, uint32_t cap, uint32_t vlo)
{
	uint32_t const nwin = (dp_size + TB_WIN - 1u) / TB_WIN;
	hipLaunchKernelGGL(k_tb_emit, dim3(nwin), dim3(256), 0, st, LB, M, SZ, dp_size, L, head, count, out, cap, vlo);
}

// The host's side of a traceback followed part by part: which part the chain stands in, the running offset into the whole
// list, and what a part's two words (k_tb_chain_part) may say.  lo[g] = part g's first entry, ascending.
struct TbPartWalk {
	uint32_t const *lo;
	uint32_t parts;
	size_t cap;
	uint32_t cur, off = 0, hops = 0;
	bool ended = false;
	TbPartWalk(uint32_t const *lo_, uint32_t parts_, uint32_t start, size_t cap_) : lo(lo_), parts(parts_), cap(cap_), cur(start) {}
	uint32_t owner() const
	{
		uint32_t g = parts - 1u;
		while (g > 0 && cur < lo[g]) --g;
		return g;
	}
	// part g reported w = {1 + the entry the chain continues at (0: it ended there), its entries}: nullptr, or why the walk ends here
	char const *take(uint32_t g, uint32_t const *w)
	{
		off += w[1];
		if (w[1] == 0 || off > cap || ++hops > parts) return "internal: the sharded traceback chain does not descend";
		if (w[0] == 0) { ended = true; return nullptr; }
		if (w[0] - 1u >= lo[g]) return "internal: the sharded traceback chain left a rank upwards";
		cur = w[0] - 1u;
		return nullptr;
	}
};

// follow_traceback (segmentation_lp_context.cc:191-224): the lb chain is followed on the device, window by window
// (k_tb_windows / k_tb_chain / k_tb_emit, fseq_kernels.hpp); the S visited entries come back in one small copy.
// Scratch: Mprev (exit pointers) and the first words of K (hop counts) -- both are free once the DP is done.

// The same when every rank of a sharded run holds the lb's of its own entries only (run_dp_spec, windows): the chain is
// followed rank by rank -- the owner of the entry it stands at walks its part and tells the others where it left and
// how many entries it visited (two words) --, every rank emits its entries at their place in the whole list, and the
// S x 16 bytes are gathered: one small exchange per rank the chain passes through instead of the lb and size arrays.
int follow_traceback_sharded(fseq_ctx *c, hipStream_t st)
{
	Shard const &sh = c->sh;
	uint32_t const L = (uint32_t) c->p.segment_length, dp_size = (uint32_t) c->dp_size;
	size_t const cap = (size_t) (c->p.n / L + 2);
	uint32_t const nwin = (dp_size + TB_WIN - 1u) / TB_WIN;
	int rc;
	if ((rc = c->d_tb.ensure(c, cap + nwin / 2 + 2))) return rc;
	uint2 *d_head = reinterpret_cast<uint2 *>(c->d_tb + cap);
	uint32_t *d_count = reinterpret_cast<uint32_t *>(d_head + nwin);
	uint32_t *d_exit_next = c->d_Mprev, *d_exit_cnt = c->dp.K.as<uint32_t>();
	// my part: my entries, and the final cell's (the last entry of the array) on the last active rank
	bool const have = sh.rank < sh.active && c->own_hi[sh.rank] > c->own_lo[sh.rank];
	uint32_t const vlo = have ? c->own_lo[sh.rank] : 0u, vhi = have ? (sh.rank + 1u == sh.active ? dp_size : c->own_hi[sh.rank]) : 0u;
	HIP_TRY(c, hipMemsetAsync(d_count, 0, 16, st));
	if (have) launch_tb_windows(st, c->dp.LB, dp_size, L, d_exit_next, d_exit_cnt, vlo, vhi);
	TbPartWalk walk(c->own_lo.data(), sh.active, dp_size - 1u, cap);
	uint32_t my_cnt = 0, my_off = 0;
	while (!walk.ended)
	{
		uint32_t const g = walk.owner();
		HIP_TRY(c, hipMemsetAsync(sh.xbuf, 0, 16, st));
		if (g == sh.rank) launch_tb_chain_part(st, d_exit_next, d_exit_cnt, walk.cur, walk.off, vlo, d_head, nwin, d_count, sh.xbuf);
		if ((rc = shard_exchange(c, 4, 0))) return rc;
		uint32_t w[4];
		HIP_TRY(c, hipMemcpy(w, sh.xbuf, 16, hipMemcpyDeviceToHost));
		if (g == sh.rank) { my_cnt = w[1]; my_off = walk.off; }
		if (char const *why = walk.take(g, w)) return fail(c, FSEQ_E_HIP, why);   // (ended: the chain ended on rank g)
	}
	size_t const S = walk.off;
	if (my_cnt) launch_tb_emit(st, c->dp.LB, c->dp.M, c->dp.SZ, dp_size, L, d_head, d_count, c->d_tb, (uint32_t) cap, vlo);
	// gather: every rank's entries sit at their final offsets of its own d_tb; word 4 S: "the chain ended in lb == 0"
	if (4 * S + 2 > sh.xwords) return fail(c, FSEQ_E_ARG, "exchange buffer too small (fseq_shard_xbuf_words)");
	HIP_TRY(c, hipMemsetAsync(sh.xbuf, 0, (4 * S + 1) * 4, st));
	if (my_cnt)
	{
		// (the chain visits a rank once, so my entries are one range of the list: d_tb[my_off .. my_off + my_cnt))
		HIP_TRY(c, hipMemcpyAsync(sh.xbuf + 4 * (size_t) my_off, c->d_tb + my_off, (size_t) my_cnt * sizeof(uint4), hipMemcpyDeviceToDevice, st));
		HIP_TRY(c, hipMemcpyAsync(sh.xbuf + 4 * S, d_count + 1, 4, hipMemcpyDeviceToDevice, st));
	}
	if ((rc = shard_exchange(c, 4 * S + 1, 0))) return rc;
	std::vector<uint4> h(S);
	uint32_t ok = 0;
	HIP_TRY(c, hipMemcpyAsync(h.data(), sh.xbuf, S * sizeof(uint4), hipMemcpyDeviceToHost, st));
	HIP_TRY(c, hipMemcpyAsync(&ok, sh.xbuf + 4 * S, 4, hipMemcpyDeviceToHost, st));
	HIP_TRY(c, hipStreamSynchronize(st));
	HIP_TRY(c, hipGetLastError());
	if (ok != 1u || S == 0) return fail(c, FSEQ_E_HIP, "internal: the traceback chain does not descend to lb == 0");
	c->tau_host.clear();
	c->tb_guess = S;
	c->traceback.resize(S);
	for (size_t j = 0; j < S; ++j)
	{
		uint4 const e = h[S - 1 - j];                        // the kernels list the last segment first
		c->traceback[j] = fseq_dp_arg{e.y, (uint64_t) e.x + L, e.z, e.w};
	}
	return FSEQ_OK;
}

int follow_traceback(fseq_ctx *c, hipStream_t st)
{
	if (c->sh.on && c->dp_window_mode) return follow_traceback_sharded(c, st);
	uint32_t const L = (uint32_t) c->p.segment_length, dp_size = (uint32_t) c->dp_size;
	size_t const cap = (size_t) (c->p.n / L + 2);           // a segment is at least L columns long
	uint32_t const nwin = (dp_size + TB_WIN - 1u) / TB_WIN;
	int rc;
	if ((rc = c->d_tb.ensure(c, cap + nwin / 2 + 2))) return rc;   // out[cap] | head[nwin] (uint2) | count[4]
	uint2 *d_head = reinterpret_cast<uint2 *>(c->d_tb + cap);
	uint32_t *d_count = reinterpret_cast<uint32_t *>(d_head + nwin);
	uint32_t *d_exit_next = c->d_Mprev, *d_exit_cnt = c->dp.K.as<uint32_t>();
	HIP_TRY(c, hipMemsetAsync(d_count, 0, 16, st));
	launch_tb_windows(st, c->dp.LB, dp_size, L, d_exit_next, d_exit_cnt, 0u, 0xFFFFFFFFu);            // (the whole array is one part)
	hipLaunchKernelGGL(k_tb_chain, dim3(1), dim3(64), 0, st, d_exit_next, d_exit_cnt, dp_size, d_head, nwin, d_count);
	launch_tb_emit(st, c->dp.LB, c->dp.M, c->dp.SZ, dp_size, L, d_head, d_count, c->d_tb, (uint32_t) cap, 0u);
	// the count and -- in the same round trip -- as many entries as the last run of this context had (a second copy
	// only when there are more this time)
	size_t const guess = std::min(cap, c->tb_guess ? c->tb_guess + 16 : (size_t) 4096);
	if ((rc = pin_reserve(c, guess * (sizeof(uint4) + sizeof(uint2)) + 256))) return rc;
	uint32_t *const cnt = pin_take<uint32_t>(c, 4);
	uint4 *const hp = pin_take<uint4>(c, guess);
	uint2 *const taup = pin_take<uint2>(c, guess);
	std::vector<uint4> h;
	// not sharded: the merge thresholds of the traceback boundaries (k_seg_tau_tb) ride along -- one workgroup per
	// POSSIBLE entry, those behind the count return at once (list windows: the lists are gone, merge_windowed takes them)
	c->tau_host.clear();
	bool const tau_tb = !c->sh.on && !c->lw.on;
	if (tau_tb)
	{
		if ((rc = c->d_tau.ensure(c, cap))) return rc;
		hipLaunchKernelGGL(k_seg_tau_tb, dim3((uint32_t) cap), dim3(64), 0, st, c->d_tb.as<uint4 const>(), d_count, L, c->stride, c->d_ent, c->d_hdr, c->d_tau);
		HIP_TRY(c, hipMemcpyAsync(taup, c->d_tau, guess * sizeof(uint2), hipMemcpyDeviceToHost, st));
	}
	HIP_TRY(c, hipMemcpyAsync(cnt, d_count, 16, hipMemcpyDeviceToHost, st));
	HIP_TRY(c, hipMemcpyAsync(hp, c->d_tb, guess * sizeof(uint4), hipMemcpyDeviceToHost, st));
	HIP_TRY(c, hipStreamSynchronize(st));
	HIP_TRY(c, hipGetLastError());
	h.assign(hp, hp + std::min<size_t>(guess, cnt[0]));
	if (tau_tb) c->tau_host.assign(taup, taup + std::min<size_t>(guess, cnt[0]));
	if (cnt[1] != 1u || cnt[0] == 0 || cnt[0] > cap) return fail(c, FSEQ_E_HIP, "internal: the traceback chain does not descend to lb == 0");
	size_t const S = cnt[0];
	if (S > guess)
	{
		h.resize(S);
		HIP_TRY(c, hipMemcpy(h.data() + guess, c->d_tb + guess, (S - guess) * sizeof(uint4), hipMemcpyDeviceToHost));
		if (!c->tau_host.empty())
		{
			c->tau_host.resize(S);
			HIP_TRY(c, hipMemcpy(c->tau_host.data() + guess, c->d_tau + guess, (S - guess) * sizeof(uint2), hipMemcpyDeviceToHost));
		}
	}
	if (!c->tau_host.empty()) c->tau_host.resize(S);
	c->tb_guess = S;
	c->traceback.resize(S);
	for (size_t j = 0; j < S; ++j)
	{
		uint4 const e = h[S - 1 - j];                        // the kernels list the last segment first
		c->traceback[j] = fseq_dp_arg{e.y, (uint64_t) e.x + L, e.z, e.w};
	}
	return FSEQ_OK;
}

uint32_t Wx_for_debug(fseq_ctx const *c, uint32_t L) { return c->tune.shard_dp_window ? (uint32_t) c->tune.shard_dp_window : std::max<uint32_t>(2u * DPW, 16u * L); }

// "every rank contributes its own slice": zero the buffer, copy my words [lo, hi) of src in, all-reduce (sum), copy
// everything back over dst -- an all-gather of unequal slices through the one primitive
int shard_gather_u32(fseq_ctx *c, uint32_t *d_array, uint64_t total, uint64_t lo, uint64_t hi, uint64_t extra = ~0ull)
{
	if (!c->sh.on) return FSEQ_OK;
	hipStream_t st = c->stream;
	HIP_TRY(c, hipMemsetAsync(c->sh.xbuf, 0, total * 4, st));
	if (hi > lo) HIP_TRY(c, hipMemcpyAsync(c->sh.xbuf + lo, d_array + lo, (hi - lo) * 4, hipMemcpyDeviceToDevice, st));
	if (extra != ~0ull) HIP_TRY(c, hipMemcpyAsync(c->sh.xbuf + extra, d_array + extra, 4, hipMemcpyDeviceToDevice, st));
	int rc = shard_exchange(c, total, 0);
	if (rc) return rc;
	HIP_TRY(c, hipMemcpyAsync(d_array, c->sh.xbuf, total * 4, hipMemcpyDeviceToDevice, st));
	return FSEQ_OK;
}

} // namespace

SpecPlan spec_plan(fseq_ctx *c, DpSchedule const &S)
{
	SpecPlan P;
#if defined(FSEQ_DP_STAMPS) || defined(FSEQ_DP_STATS)
	if (!c->sh.on) return P;                 // the diagnostic builds instrument the serial kernel
#endif
	if (c->tune.dp_serial && !c->sh.on) return P;
	int ncu = 0;
	(void) hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, c->p.device);
	if (ncu < 1) ncu = 1;
	// one chunk per CU, but chunks of at least max(400, 8L) entries (the sweeps of shorter chunks are cheaper but more of
	// them are needed; BASELINE C2, L = 50: 96 chunks of 21 rounds 0.32 ms in 3 sweeps, 250 of 8 rounds 0.20 ms in 4,
	// 334 of 6 rounds 0.27 ms)
	uint32_t const min_entries = std::max<uint32_t>(400u, 8u * S.L);
	uint32_t forced = 0;
	if (c->tune.dp_spec_rounds) forced = (uint32_t) c->tune.dp_spec_rounds;   // tests: any chunk length
	auto cut = [&](uint32_t lo, uint32_t hi) {
		// rounds [lo, hi) of one rank into chunks
		if (hi <= lo) return;
		uint32_t rpc = std::max<uint32_t>((hi - lo + (uint32_t) ncu - 1u) / (uint32_t) ncu, (min_entries + S.RL - 1u) / S.RL);
		if (forced) rpc = forced;
		for (uint32_t r = lo; r < hi; r += rpc) P.r0.push_back(r);
	};
	if (!c->sh.on)
	{
		cut(0, S.nreg);
		P.r0.push_back(S.nreg);
		uint32_t const nch = P.nchunks();
		if ((nch < 3u && !forced) || nch < 2u || nch > 65535u) { P.r0.clear(); return P; }
		P.mine_lo = 0; P.mine_hi = nch;
		return P;
	}
	Shard const &sh = c->sh;
	uint32_t prev = 0;
	for (uint32_t g = 0; g < sh.active; ++g)
	{
		// rounds whose first column (L + r RL - 1) lies in rank g's columns; the last active rank takes the rest
		uint64_t const hi_col = std::min<uint64_t>(c->p.n, (uint64_t) (g + 1) * sh.bpr * c->B);
		uint32_t r_hi = S.nreg;
		if (g + 1 < sh.active)
		{
			uint64_t const need = hi_col + 1 > S.L ? hi_col + 1 - S.L : 0;      // first round with L + r RL - 1 >= hi_col
			r_hi = (uint32_t) std::min<uint64_t>(S.nreg, (need + S.RL - 1) / S.RL);
		}
		if (r_hi < prev) r_hi = prev;
		if (g == sh.rank) P.mine_lo = (uint32_t) P.r0.size();
		P.rank_lo.push_back((uint32_t) P.r0.size());
		cut(prev, r_hi);
		if (g == sh.rank) P.mine_hi = (uint32_t) P.r0.size();
		prev = r_hi;
	}
	P.rank_lo.push_back((uint32_t) P.r0.size());
	P.r0.push_back(S.nreg);
	if (sh.rank >= sh.active) P.mine_lo = P.mine_hi = P.nchunks();
	return P;
}

// The arrays a run of the speculative DP starts from (nothing here depends on phases A-C: run_long_path queues it on
// the second stream while phase C runs)
int dp_spec_reset(fseq_ctx *c, SpecPlan const &P, hipStream_t s)
{
	uint32_t const nch = P.nchunks();
	int rc;
	if ((rc = c->d_spec.ensure(c, (size_t) 7 * nch + 16))) return rc;
	if ((rc = c->d_chunk_r0.ensure(c, nch + 1u))) return rc;
	HIP_TRY(c, hipMemcpyAsync(c->d_chunk_r0, P.r0.data(), (size_t) (nch + 1u) * 4, hipMemcpyHostToDevice, s));
	HIP_TRY(c, hipMemsetAsync(c->dp.M, 0, c->dp_size * 4, s));
	HIP_TRY(c, hipMemsetAsync(c->d_Mprev, 0, c->dp_size * 4, s));
	HIP_TRY(c, hipMemsetAsync(c->d_spec, 0, ((size_t) 7 * nch + 16) * 4, s));
	HIP_TRY(c, hipMemsetAsync(c->d_spec, 0x01, (size_t) nch * 4, s));         // d_active != 0: every chunk runs in sweep 1
	if (c->sh.on)
	{
		// LB / SZ are gathered over the ranks at the end: what nobody writes must be 0 everywhere
		HIP_TRY(c, hipMemsetAsync(c->dp.LB, 0, c->dp_size * 4, s));
		HIP_TRY(c, hipMemsetAsync(c->dp.SZ, 0, c->dp_size * 4, s));
	}
	return FSEQ_OK;
}

// Phase D as chunk-speculative sweeps on the whole chip (fseq_dpspec.hpp).  Leaves M / LB / SZ exactly as
// k_dp<DP_WHOLE> would (on every rank of a sharded run); *overflow = some cell's list was too short.
// reset_done: dp_spec_reset has been queued (on any stream `st` already waits for).
int run_dp_spec(fseq_ctx *c, DpSchedule const &S, SpecPlan const &P, hipStream_t st, uint32_t *overflow, uint32_t *sweeps_out, bool reset_done)
{
	fseq_params const &p = c->p;
	uint32_t const m = p.m, n = (uint32_t) p.n, L = (uint32_t) p.segment_length;
	uint32_t const nch = P.nchunks();
	bool const sharded = c->sh.on;
	int rc;
	if (!reset_done && (rc = dp_spec_reset(c, P, st))) return rc;
	uint32_t *d_active = c->d_spec, *d_changed = d_active + nch, *d_tailmin = d_changed + nch, *d_floor = d_tailmin + nch,
	         *d_lift = d_floor + nch, *d_ovf = d_lift + nch;
	SpecCtl *d_ctl = reinterpret_cast<SpecCtl *>(d_ovf + 2 * (size_t) nch);      // (ovf: {list too short, lowest entry read} per chunk)
	SpecGeom G;
	G.chunk_r0 = c->d_chunk_r0;
	G.RL = S.RL;
	G.nchunks = nch;
	G.NR = n - 2u * L + 1u;
	G.t_final = n - L;
	G.win = std::max<uint32_t>(256u, 4u * L);
	if (c->tune.dp_spec_win) G.win = (uint32_t) c->tune.dp_spec_win;
	uint32_t const ncomplete = G.NR / 64u;
	uint32_t const grid_c = (uint32_t) ((c->dp_size + 255) / 256);          // 4 blocks of 64 entries per workgroup, incl. the final cell's

	DpSpecArgs SP;
	SP.chunk_r0 = c->d_chunk_r0; SP.nchunks = nch; SP.chunk0 = P.mine_lo; SP.active = d_active; SP.ovf = d_ovf;
	SP.ctl = reinterpret_cast<uint32_t const *>(d_ctl);
	uint32_t const mine = P.mine_hi - P.mine_lo;
	// my entries: the chunks [mine_lo, mine_hi) are consecutive rounds
	uint64_t const t_lo = mine ? (uint64_t) P.r0[P.mine_lo] * S.RL : 0, t_hi = mine ? (P.mine_hi == nch ? G.NR : (uint64_t) P.r0[P.mine_hi] * S.RL) : 0;
	uint64_t const t_extra = (mine && P.mine_hi == nch) ? G.t_final : ~0ull;
	auto sweep = [&](bool fresh) {
		SP.fresh = fresh ? 1u : 0u;
		if (mine)
			hipLaunchKernelGGL(k_dp<DP_SPEC>, dim3(mine), dim3(1024), dp_lds_bytes(), st, c->dp, c->d_ent, c->d_hdr, c->stride, m, n, L,
			                   path_words(c)->dp, 0u, 0u, SP);
	};
	auto compare = [&](bool first) {
		hipLaunchKernelGGL(k_spec_scan, dim3(nch), dim3(256), 0, st, c->dp.M, c->d_Mprev, G, d_active, d_changed, d_tailmin, d_ctl);
		hipLaunchKernelGGL(k_spec_decide, dim3(1), dim3(64), 0, st, nch, first ? 1u : 0u, d_changed, d_tailmin, d_floor, d_lift, d_active, d_ovf, d_ctl);
	};
	auto rebuild = [&]() {
		hipLaunchKernelGGL(k_spec_rebuild, dim3(grid_c), dim3(256), 0, st, c->dp, c->d_Mprev, G, d_lift, d_ctl);
		hipLaunchKernelGGL(k_spec_table, dim3((ncomplete + 255u) / 256u), dim3(256), 0, st, c->dp, ncomplete, d_ctl);
	};
	uint32_t max_sweeps = 12;
	if (c->tune.dp_spec_max_sweeps) max_sweeps = (uint32_t) c->tune.dp_spec_max_sweeps;
	SpecCtl h{};
	// "list too short" of my chunks lo .. hi - 1 (ovf words are {flag, lowest entry read} pairs)
	auto own_overflow = [&](std::vector<uint32_t> const &ovf2, uint32_t lo, uint32_t hi) {
		uint32_t o = 0;
		for (uint32_t k = lo; k < hi; ++k) o |= ovf2[2 * (size_t) k] ? 1u : 0u;
		return o;
	};
	// ---- sharded: who owns which entries, and whether a rank keeps windows or whole arrays
	c->dp_window_mode = false;
	c->dp_exchange_words = 0;
	std::vector<uint32_t> win_lo, win_off;                    // window in front of rank g: entries [win_lo[g], own_lo[g]) at xbuf + win_off[g]
	uint64_t win_total = 0;
	if (sharded)
	{
		Shard const &sh = c->sh;
		c->own_lo.assign(sh.world, 0); c->own_hi.assign(sh.world, 0);
		for (uint32_t g = 0; g < sh.active; ++g)
		{
			uint32_t const c_lo = P.rank_lo[g], c_hi = P.rank_lo[g + 1];
			c->own_lo[g] = P.r0[c_lo] * S.RL;
			c->own_hi[g] = c_hi == nch ? G.NR : P.r0[c_hi] * S.RL;
			if (c_hi <= c_lo) c->own_hi[g] = c->own_lo[g];
		}
		// A chunk reads entries in front of it through its LDS ring (the DPW entries in front of its first cell) and, rarely,
		// straight from memory: both stay within a few thousand entries on every input measured (the candidates of a cell end
		// where the cumulative count of its list passes the cell's value).  So a rank keeps, of the other ranks' keys, a WINDOW
		// in front of its own entries, the sweeps report the lowest entry they read (k_dp: ovf words), and a sweep that looked
		// below the window makes the run start again with whole-array exchanges (exactness never rests on the window).
		uint32_t Wx = std::max<uint32_t>(2u * DPW, 16u * L);
		if (c->tune.shard_dp_window) Wx = (uint32_t) c->tune.shard_dp_window;
		win_lo.assign(sh.world, 0); win_off.assign(sh.world, 0);
		uint64_t off = 2ull * nch + 2;                          // [changed nch][tailmin nch][below][pad]
		for (uint32_t g = 1; g < sh.active; ++g)
		{
			uint32_t const th = c->own_lo[g];
			win_lo[g] = th > Wx ? ((th - Wx) & ~63u) : 0u;       // (whole 64-blocks: the block minima of the window are then right too)
			win_off[g] = (uint32_t) off;
			off += th - win_lo[g];
		}
		win_total = off;
		c->dp_window_mode = !c->tune.shard_dp_full && !c->shard_dp_full_sticky && 2 * win_total < c->dp_size && win_total + 1 <= c->sh.xwords;
	}
	sweep(true);
	uint32_t done_sweeps = 1;
	std::vector<uint32_t> ovf_early;
	if (!sharded)
	{
		// every kernel returns at once when the iteration has converged, so sweeps are queued ahead of the
		// host's look at the control word: three further sweeps first (the measured common case needs three in
		// all), then one at a time
		uint32_t batch = 3;
		while (true)
		{
			for (uint32_t i = 0; i < batch && done_sweeps < max_sweeps; ++i)
			{
				compare(done_sweeps == 1);
				rebuild();
				sweep(false);
				++done_sweeps;
			}
			compare(done_sweeps == 1);
			if ((rc = pin_reserve(c, sizeof(h) + (size_t) nch * 8 + 64))) return rc;
			auto *const hpin = pin_take<std::remove_reference_t<decltype(h)>>(c, 1);
			uint32_t *const opin = pin_take<uint32_t>(c, 2 * (size_t) nch);
			HIP_TRY(c, hipMemcpyAsync(hpin, d_ctl, sizeof(h), hipMemcpyDeviceToHost, st));
			// (the chunks' "list too short" words in the same round trip: final if the iteration has converged)
			HIP_TRY(c, hipMemcpyAsync(opin, d_ovf, (size_t) nch * 8, hipMemcpyDeviceToHost, st));
			HIP_TRY(c, hipStreamSynchronize(st));
			HIP_TRY(c, hipGetLastError());
			h = *hpin;
			ovf_early.assign(opin, opin + 2 * (size_t) nch);
			if (h.done || done_sweeps >= max_sweeps) break;
			// the compare just queued has already chosen the next sweep's active set and lifts
			rebuild();
			sweep(false);
			++done_sweeps;
			batch = 1;
		}
	}
	else if (!c->dp_window_mode)
	{
		// sharded, whole arrays: after every sweep the ranks exchange the keys of their chunks; compare / lift / rebuild then run
		// on the whole arrays on every rank (same inputs, same results), the next sweep again on the rank's own chunks
		while (true)
		{
			if ((rc = shard_gather_u32(c, c->dp.M, c->dp_size, t_lo, t_hi, t_extra))) return rc;
			c->dp_exchange_words += c->dp_size;
			compare(done_sweeps == 1);
			HIP_TRY(c, hipMemcpyAsync(&h, d_ctl, sizeof(h), hipMemcpyDeviceToHost, st));
			HIP_TRY(c, hipStreamSynchronize(st));
			HIP_TRY(c, hipGetLastError());
			if (h.done) break;                   // no serial fallback here: after sweep k the chunks 0..k-1 are exact, so this ends
			if (done_sweeps > nch + 2u) return fail(c, FSEQ_E_HIP, "internal: speculative DP did not converge");
			rebuild();
			sweep(false);
			++done_sweeps;
		}
	}
	else
	{
		// sharded, windows: after every sweep ONE exchange carries what the others need of a rank -- "changed" and the tail
		// minimum of each of its chunks (the lifts follow from those on every rank alike), whether one of its chunks read
		// below its window, and the keys in the window in front of every other rank's entries (a rank contributes the part
		// of each window it owns).  compare (of its own chunks) / decide / lift / rebuild run on every rank; what a rank holds
		// outside its entries and its window is never read.
		Shard const &sh = c->sh;
		uint32_t *const xb = sh.xbuf;
		uint32_t const my_valid_lo = sh.rank < sh.active ? win_lo[sh.rank] : 0u;
		while (true)
		{
			HIP_TRY(c, hipMemsetAsync(xb, 0, (size_t) win_total * 4, st));
			if (mine)
				hipLaunchKernelGGL(k_spec_scan, dim3(mine), dim3(256), 0, st, c->dp.M, c->d_Mprev, G, d_active, xb, xb + nch, d_ctl,
				                   P.mine_lo, (uint32_t const *) d_ovf, my_valid_lo, xb + 2 * (size_t) nch);
			for (uint32_t g = 1; mine && g < sh.active; ++g)
			{
				uint64_t const a = std::max<uint64_t>(win_lo[g], t_lo), b = std::min<uint64_t>(c->own_lo[g], t_hi);
				if (b > a) HIP_TRY(c, hipMemcpyAsync(xb + win_off[g] + (a - win_lo[g]), c->dp.M + a, (b - a) * 4, hipMemcpyDeviceToDevice, st));
			}
			if ((rc = shard_exchange(c, win_total, 0))) return rc;
			c->dp_exchange_words += win_total;
			HIP_TRY(c, hipMemcpyAsync(d_changed, xb, (size_t) 2 * nch * 4, hipMemcpyDeviceToDevice, st));      // changed | tailmin are adjacent
			if (sh.rank >= 1 && sh.rank < sh.active && c->own_lo[sh.rank] > win_lo[sh.rank])
				HIP_TRY(c, hipMemcpyAsync(c->dp.M + win_lo[sh.rank], xb + win_off[sh.rank], (size_t) (c->own_lo[sh.rank] - win_lo[sh.rank]) * 4, hipMemcpyDeviceToDevice, st));
			hipLaunchKernelGGL(k_spec_decide, dim3(1), dim3(64), 0, st, nch, done_sweeps == 1 ? 1u : 0u, d_changed, d_tailmin, d_floor, d_lift, d_active, d_ovf, d_ctl);
			uint32_t below = 0;
			HIP_TRY(c, hipMemcpyAsync(&h, d_ctl, sizeof(h), hipMemcpyDeviceToHost, st));
			HIP_TRY(c, hipMemcpyAsync(&below, xb + 2 * (size_t) nch, 4, hipMemcpyDeviceToHost, st));
			HIP_TRY(c, hipStreamSynchronize(st));
			HIP_TRY(c, hipGetLastError());
			if (below)
			{
				// some rank's sweep read a key it does not hold: nothing of this run is trusted; whole arrays from here on
				// (every rank sees the same word, so every rank takes this way)
				if (c->tune.debug) fprintf(stderr, "[fseq] sharded DP: a sweep read below its window (%u entries): again with whole-array exchanges\n", Wx_for_debug(c, L));
				c->shard_dp_full_sticky = true;
				return run_dp_spec(c, S, P, st, overflow, sweeps_out, false);
			}
			if (h.done) break;
			if (done_sweeps > nch + 2u) return fail(c, FSEQ_E_HIP, "internal: speculative DP did not converge");
			rebuild();
			sweep(false);
			++done_sweeps;
		}
	}
	if (!h.done)
	{
		// bounded (one GPU only): finish serially behind the last chunk known to be exact (its masks and samples are rebuilt first)
		rebuild();
		uint32_t const first_dirty = std::min(h.first_changed + 1u, nch);
		uint32_t const r0 = first_dirty < nch ? P.r0[first_dirty] : S.nreg;
		HIP_TRY(c, hipMemsetAsync(path_words(c)->dp, 0, sizeof(PathWords::dp), st));
		launch_dp_serial(c, DP_PARTIAL, st, r0, S.nrounds);
		// overflow: the serial part reports through d_flags, the frozen chunks through their own words
		std::vector<uint32_t> ovf(2 * (size_t) nch);
		uint32_t fl[4] = {0, 0, 0, 0};
		HIP_TRY(c, hipMemcpyAsync(ovf.data(), d_ovf, (size_t) nch * 8, hipMemcpyDeviceToHost, st));
		HIP_TRY(c, hipMemcpyAsync(fl, path_words(c)->dp, sizeof(fl), hipMemcpyDeviceToHost, st));
		HIP_TRY(c, hipStreamSynchronize(st));
		HIP_TRY(c, hipGetLastError());
		*overflow = (fl[0] & 1u) | own_overflow(ovf, P.mine_lo, std::min(P.mine_hi, h.first_changed + 1u));
		if (c->tune.debug) fprintf(stderr, "[fseq] speculative DP: not converged after %u sweeps, serial from round %u\n", done_sweeps, r0);
	}
	else
	{
		// the chunks' "list too short" words are written by their owners only
		std::vector<uint32_t> ovf(2 * (size_t) nch);
		if (ovf_early.size() == 2 * (size_t) nch) ovf = ovf_early;           // (read together with the control word that said "done")
		else
		{
			HIP_TRY(c, hipMemcpyAsync(ovf.data(), d_ovf, (size_t) nch * 8, hipMemcpyDeviceToHost, st));
			HIP_TRY(c, hipStreamSynchronize(st));
		}
		*overflow = own_overflow(ovf, P.mine_lo, P.mine_hi);
	}
	if (sharded)
	{
		if (!c->dp_window_mode)
		{
			// lb and size of every entry from the rank that computed it (frozen chunks: from the sweep that last ran them)
			if ((rc = shard_gather_u32(c, c->dp.LB, c->dp_size, t_lo, t_hi, t_extra))) return rc;
			if ((rc = shard_gather_u32(c, c->dp.SZ, c->dp_size, t_lo, t_hi, t_extra))) return rc;
			c->dp_exchange_words += 2 * c->dp_size;
		}
		uint32_t o = *overflow;
		HIP_TRY(c, hipMemcpyAsync(c->sh.xbuf, &o, 4, hipMemcpyHostToDevice, st));
		if ((rc = shard_exchange(c, 1, 1))) return rc;
		HIP_TRY(c, hipMemcpy(&o, c->sh.xbuf, 4, hipMemcpyDeviceToHost));
		*overflow = o;
	}
	if (sweeps_out) *sweeps_out = h.done ? h.sweeps : done_sweeps + 1000u;
	if (c->tune.debug)
		fprintf(stderr, "[fseq] speculative DP: %u chunks (mine %u..%u), %u sweeps compared, done=%u%s, %.2f MB exchanged by the sweeps\n", nch, P.mine_lo, P.mine_hi, h.sweeps, h.done,
		        sharded ? (c->dp_window_mode ? ", windows" : ", whole arrays") : "", c->dp_exchange_words * 4 / 1e6);
	return FSEQ_OK;
}

int prepare_dp_kernels(fseq_ctx *c)
{
	HIP_TRY(c, allow_lds(k_dp<DP_WHOLE>, dp_lds_bytes()));
	HIP_TRY(c, allow_lds(k_dp<DP_PARTIAL>, dp_lds_bytes()));
	HIP_TRY(c, allow_lds(k_dp<DP_SPEC>, dp_lds_bytes()));
	return FSEQ_OK;
}

void launch_dp_serial(fseq_ctx *c, int mode, hipStream_t st, uint32_t r_lo, uint32_t r_hi)
{
	hipLaunchKernelGGL((mode == DP_WHOLE ? k_dp<DP_WHOLE> : k_dp<DP_PARTIAL>), dim3(1), dim3(1024), dp_lds_bytes(), st, c->dp, c->d_ent, c->d_hdr, c->stride, c->p.m, (uint32_t) c->p.n,
	                   (uint32_t) c->p.segment_length, path_words(c)->dp, r_lo, r_hi, DpSpecArgs{});
}

bool shard_dp_plan_ok(fseq_ctx *c)
{
	// every rank that owns blocks must own at least one regular DP round, and the last one the final cell's column
	DpSchedule const S = dp_schedule((uint32_t) c->p.segment_length, (uint32_t) c->p.n);
	SpecPlan const P = spec_plan(c, S);
	bool ok = P.nchunks() >= 1;
	if (ok && c->sh.rank < c->sh.active && P.mine_hi <= P.mine_lo) ok = false;
	// (the plan is the same on every rank: check every rank's share here so that all ranks fail together)
	for (uint32_t g = 0; ok && g < c->sh.active; ++g)
	{
		Shard probe = c->sh; probe.rank = g;
		Shard const keep = c->sh; c->sh = probe;
		SpecPlan const Q = spec_plan(c, S);
		c->sh = keep;
		if (Q.mine_hi <= Q.mine_lo) ok = false;
		if (g + 1 == c->sh.active && Q.mine_hi != Q.nchunks()) ok = false;
	}
	return ok;
}

namespace {

// the merge thresholds of the `count` boundary columns in d_cols, from the lists of the columns [col_lo, col_hi), into d_tau ...
void launch_seg_tau(fseq_ctx *c, size_t count, uint64_t col_lo, uint64_t col_hi, uint32_t max_seg)
{
	hipLaunchKernelGGL(k_seg_tau, dim3((uint32_t) count), dim3(64), 0, c->stream, c->d_cols, col_lo, col_hi, max_seg, c->stride, c->d_ent, c->d_hdr, c->d_tau);
}

// ... and the merged sizes of the `count` (column, lb) pairs in d_cols: returns where on the device they land
uint32_t *launch_seg_count(fseq_ctx *c, size_t count, uint64_t col_lo, uint64_t col_hi)
{
	uint32_t *d_cnt = c->d_tau.as<uint32_t>();
	hipLaunchKernelGGL(k_seg_count, dim3((uint32_t) count), dim3(64), 0, c->stream, c->d_cols, c->d_cols + count, col_lo, col_hi, c->stride, c->d_ent, c->d_hdr, d_cnt);
	return d_cnt;
}

// The walk of find_segments_greedy (lp.cc:335-390) over the traceback's boundaries, a step per boundary.  Its test
// #{d_rb > current_lb} <= max_segment_size (:363-364) holds exactly for current_lb >= tau_rb (k_seg_tau): boundary j then joins
// the segment in front of it, else the segment is cut there.  A merged segment's size is the count at its last joined boundary
// (:366): emit() notes in `ask` which segments wait for theirs; how and when the counts are asked for is the caller's.
struct MergeWalk {
	enum Step { JOIN, CUT, UNDECIDED };
	struct Pending { size_t seg, j; uint64_t lb; };      // segment, its last boundary, the lb it was counted from
	fseq_ctx *c;
	uint64_t current_lb = 0, prev_size;
	bool prev_size_pending = false;
	size_t prev = 0;
	std::vector<Pending> ask;
	explicit MergeWalk(fseq_ctx *c_) : c(c_), prev_size(c_->traceback[0].segment_size) {}
	void emit()
	{
		if (prev_size_pending) ask.push_back(Pending{c->segments.size(), prev, current_lb});
		c->segments.push_back(fseq_segment{current_lb, c->traceback[prev].rb, (uint32_t) prev_size, 0});
	}
	Step step(size_t j, uint2 const t)
	{
		bool const fits = t.y != SEG_TAU_NEVER && current_lb >= t.x;
		if (!fits && t.y == SEG_TAU_OPEN) return UNDECIDED;            // the list ended before it could tell
		if (fits)
			prev_size_pending = true;                                   // prev_size = the count at boundary j (:366)
		else
		{
			emit();
			prev_size = c->traceback[j].segment_size;
			prev_size_pending = false;
			current_lb = c->traceback[prev].rb;
		}
		prev = j;
		return fits ? JOIN : CUT;
	}
};

// find_segments_greedy (lp.cc:335-390) when the lists are gone after a windowed pass 1: a second pass over the windows that
// hold a traceback boundary's column rb - 1 writes their lists again (same plan, same kernels: the same lists), takes the
// thresholds of the window's boundaries (k_seg_tau), advances the walk over them -- current_lb depends on earlier boundaries
// only -- and counts the merged size at every boundary that joins the segment before it at the walk's current_lb
// (k_seg_count; the last such count of a segment is its size).  *overflow: a list ended before a threshold could be told.
int merge_windowed(fseq_ctx *c, bool *overflow)
{
	FSEQ_LONG_LOCALS(c);
	fseq_ctx::ListWindows &W = c->lw;
	size_t const S = c->traceback.size();
	uint32_t const max_seg = c->traceback.back().segment_max_size;
	if ((rc = c->d_cols.ensure(c, 2 * S))) return rc;
	if ((rc = c->d_tau.ensure(c, S))) return rc;
	if ((rc = pin_reserve(c, S * 28 + 256))) return rc;
	uint64_t *const qc = pin_take<uint64_t>(c, 2 * S);
	uint2 *const tau = pin_take<uint2>(c, S);
	uint32_t *const cnt = pin_take<uint32_t>(c, S);
	std::vector<uint32_t> size_at(S, 0);                 // merged size at boundary j (for the boundaries that join)
	MergeWalk walk(c);
	size_t j = 1;
	W.merge_windows = 0;
	for (uint32_t lo = 0; lo < c->nblocks && j < S; lo += W.wb)
	{
		uint32_t const hi = std::min(c->nblocks, lo + W.wb);
		uint64_t const col_lo = (uint64_t) lo * c->B, col_hi = std::min<uint64_t>(n, (uint64_t) hi * c->B);
		size_t j_hi = j;
		while (j_hi < S && c->traceback[j_hi].rb - 1 < col_hi) ++j_hi;
		if (j_hi == j) continue;                          // (no boundary in this window: its lists are not needed)
		set_list_window(c, lo);
		W.col_lo = W.col_hi = 0;                          // (the buffer is being rewritten)
		if ((rc = window_phase_c(c, lo, hi))) return rc;
		++W.merge_windows;
		size_t const q = j_hi - j;
		for (size_t i = 0; i < q; ++i) qc[i] = c->traceback[j + i].rb - 1;
		HIP_TRY(c, hipMemcpyAsync(c->d_cols, qc, q * 8, hipMemcpyHostToDevice, st));
		launch_seg_tau(c, q, col_lo, col_hi, max_seg);
		HIP_TRY(c, hipMemcpyAsync(tau, c->d_tau, q * sizeof(uint2), hipMemcpyDeviceToHost, st));
		HIP_TRY(c, hipStreamSynchronize(st));
		HIP_TRY(c, hipGetLastError());
		W.col_lo = col_lo; W.col_hi = col_hi;
		// the walk over this window's boundaries; the joins ask for the count at their column with the current_lb of the moment
		size_t nq = 0;
		for (; j < j_hi; ++j)
		{
			MergeWalk::Step const step = walk.step(j, tau[j - (j_hi - q)]);
			if (step == MergeWalk::UNDECIDED) { *overflow = true; return FSEQ_OK; }
			if (step == MergeWalk::JOIN) { qc[nq] = c->traceback[j].rb - 1; qc[S + nq] = walk.current_lb; cnt[nq] = (uint32_t) j; ++nq; }
		}
		if (nq)
		{
			std::vector<uint32_t> const js(cnt, cnt + nq);
			HIP_TRY(c, hipMemcpyAsync(c->d_cols, qc, nq * 8, hipMemcpyHostToDevice, st));
			HIP_TRY(c, hipMemcpyAsync(c->d_cols + nq, qc + S, nq * 8, hipMemcpyHostToDevice, st));
			HIP_TRY(c, hipMemcpyAsync(cnt, launch_seg_count(c, nq, col_lo, col_hi), nq * 4, hipMemcpyDeviceToHost, st));
			HIP_TRY(c, hipStreamSynchronize(st));
			HIP_TRY(c, hipGetLastError());
			for (size_t i = 0; i < nq; ++i) size_at[js[i]] = cnt[i];
		}
	}
	if (j < S) return fail(c, FSEQ_E_HIP, "internal: a traceback boundary lies in no list window");
	walk.emit();
	for (MergeWalk::Pending const &a : walk.ask) c->segments[a.seg].segment_size = size_at[a.j];
	if (c->tune.debug) fprintf(stderr, "[fseq] merge: %u of %u list windows written again\n", W.merge_windows, W.nwin);
	return FSEQ_OK;
}

// find_segments_greedy over the traceback follow_traceback left on the context: the second half of long_traceback_and_merge.
// probe (fseq_debug_merge_on_lists alone; a run passes none): where the thresholds and counts are taken from, and what was taken.
int merge_traceback(fseq_ctx *c, bool *overflow_out, MergeProbe *probe)
{
	FSEQ_LONG_LOCALS(c);
	uint32_t const max_seg = c->traceback.back().segment_max_size;
	c->res.max_segment_size = max_seg;
	c->res.dp_segment_count = c->traceback.size();
	c->res.short_path = 0;
	size_t const S = c->traceback.size();

	// ---- find_segments_greedy (lp.cc:335-390, MergeWalk): tau comes from the list of column rb - 1 where that list lives
	// (k_seg_tau: one number per traceback boundary instead of the lists; sharded: every rank for its columns).
	c->segments.clear();
	if (!(max_seg < m)) return FSEQ_OK;
	if (c->lw.on) return merge_windowed(c, overflow_out);
	uint64_t const own_lo = held_lo(c), own_hi = sharded ? sh.c_hi : n;      // columns whose lists I answer for
	std::vector<uint2> tau(S);
	bool const separate = probe && probe->separate;
	if (S > 1 && c->tau_host.size() == S && !separate)
		tau = c->tau_host;                                          // came back with the traceback
	else if (S > 1)
	{
		if ((rc = c->d_cols.ensure(c, 2 * S))) return rc;
		if ((rc = c->d_tau.ensure(c, S))) return rc;
		std::vector<uint64_t> cols(S);
		for (size_t j = 0; j < S; ++j) cols[j] = c->traceback[j].rb - 1;
		HIP_TRY(c, hipMemcpyAsync(c->d_cols, cols.data(), S * 8, hipMemcpyHostToDevice, st));
		if (separate)
		{
			// one launch per column range, summed word by word: what the exchange of a sharded run does with the ownership rule's zeros
			std::vector<uint2> part(S);
			for (size_t r = 0; r + 1 < probe->bounds.size(); ++r)
			{
				launch_seg_tau(c, S, probe->bounds[r], probe->bounds[r + 1], max_seg);
				HIP_TRY(c, hipMemcpyAsync(part.data(), c->d_tau, S * 8, hipMemcpyDeviceToHost, st));
				HIP_TRY(c, hipStreamSynchronize(st));
				for (size_t j = 0; j < S; ++j) { tau[j].x += part[j].x; tau[j].y += part[j].y; }
				++probe->threshold_launches;
			}
		}
		else
		{
			launch_seg_tau(c, S, own_lo, own_hi, max_seg);
			if (sharded)
			{
				HIP_TRY(c, hipMemcpyAsync(sh.xbuf, c->d_tau, S * 8, hipMemcpyDeviceToDevice, st));
				if ((rc = shard_exchange(c, 2 * S, 0))) return rc;
				HIP_TRY(c, hipMemcpyAsync(tau.data(), sh.xbuf, S * 8, hipMemcpyDeviceToHost, st));
			}
			else
				HIP_TRY(c, hipMemcpyAsync(tau.data(), c->d_tau, S * 8, hipMemcpyDeviceToHost, st));
		}
		HIP_TRY(c, hipStreamSynchronize(st));
		HIP_TRY(c, hipGetLastError());
	}
	if (separate) probe->tau = tau;
	// the walk itself; the merged sizes are asked for afterwards
	MergeWalk walk(c);
	for (size_t j = 1; j < S; ++j)
		if (walk.step(j, tau[j]) == MergeWalk::UNDECIDED) { *overflow_out = true; return FSEQ_OK; }
	walk.emit();
	size_t const Q = walk.ask.size();
	if (!Q) return FSEQ_OK;
	if ((rc = pin_reserve(c, Q * 20 + 64))) return rc;
	uint64_t *const qc = pin_take<uint64_t>(c, 2 * Q);
	for (size_t i = 0; i < Q; ++i) { qc[i] = c->traceback[walk.ask[i].j].rb - 1; qc[Q + i] = walk.ask[i].lb; }
	uint32_t *const cnt = pin_take<uint32_t>(c, Q);
	if ((rc = c->d_cols.ensure(c, 2 * Q))) return rc;
	if ((rc = c->d_tau.ensure(c, Q))) return rc;
	HIP_TRY(c, hipMemcpyAsync(c->d_cols, qc, 2 * Q * 8, hipMemcpyHostToDevice, st));
	if (separate)
	{
		std::vector<uint32_t> sum(Q, 0u);
		for (size_t r = 0; r + 1 < probe->bounds.size(); ++r)
		{
			HIP_TRY(c, hipMemcpyAsync(cnt, launch_seg_count(c, Q, probe->bounds[r], probe->bounds[r + 1]), Q * 4, hipMemcpyDeviceToHost, st));
			HIP_TRY(c, hipStreamSynchronize(st));
			for (size_t i = 0; i < Q; ++i) sum[i] += cnt[i];
			++probe->count_launches;
		}
		std::copy(sum.begin(), sum.end(), cnt);
	}
	else
	{
		uint32_t *const d_cnt = launch_seg_count(c, Q, own_lo, own_hi);
		if (sharded)
		{
			HIP_TRY(c, hipMemcpyAsync(sh.xbuf, d_cnt, Q * 4, hipMemcpyDeviceToDevice, st));
			if ((rc = shard_exchange(c, Q, 0))) return rc;
			HIP_TRY(c, hipMemcpyAsync(cnt, sh.xbuf, Q * 4, hipMemcpyDeviceToHost, st));
		}
		else
			HIP_TRY(c, hipMemcpyAsync(cnt, d_cnt, Q * 4, hipMemcpyDeviceToHost, st));
	}
	HIP_TRY(c, hipStreamSynchronize(st));
	HIP_TRY(c, hipGetLastError());
	for (size_t i = 0; i < Q; ++i) c->segments[walk.ask[i].seg].segment_size = cnt[i];
	return FSEQ_OK;
}

} // namespace

// ---- follow_traceback and find_segments_greedy for one attempt (the lists held their own so far): the traceback on
// the device, the merge walk over one threshold per traceback boundary on the host.  *overflow_out: a threshold or a merged
// size needed more of a list than it holds.
int long_traceback_and_merge(fseq_ctx *c, double th0, bool *overflow_out)
{
	*overflow_out = false;
	if (int const rc = follow_traceback(c, c->stream)) return rc;
	if (c->tune.debug) fprintf(stderr, "[fseq] host: traceback walk + gather %.3f ms\n", now_ms() - th0);
	return merge_traceback(c, overflow_out, nullptr);
}

// the same two halves on the DP arrays and lists a caller laid over the context (fseq_debug_merge_on_lists)
int probe_traceback_and_merge(fseq_ctx *c, MergeProbe *probe, bool *overflow_out)
{
	*overflow_out = false;
	if (int const rc = follow_traceback(c, c->stream)) return rc;
	if (!probe->separate) probe->tau = c->tau_host;          // what rode with the traceback, whether or not a merge reads it
	return merge_traceback(c, overflow_out, probe);
}

} // namespace fseq

using namespace fseq;

extern "C" {

int fseq_debug_rmq(int device, uint32_t const *keys, uint32_t count, uint32_t const *beg, uint32_t const *end, uint32_t n_queries,
                   uint32_t *index_hbm, uint32_t *index_lds)
{
	if (!keys || !count || (n_queries && (!beg || !end || !index_hbm))) return FSEQ_E_ARG;
	for (uint32_t q = 0; q < n_queries; ++q)
		if (beg[q] >= end[q] || end[q] > count) return FSEQ_E_ARG;
	if (hipSetDevice(device) != hipSuccess) return FSEQ_E_HIP;
	DpArrays A{};
	A.tstride = count / 64 + 2;
	uint32_t *d_prev = nullptr, *d_lift = nullptr, *d_r0 = nullptr;
	uint2 *d_q = nullptr, *d_out = nullptr;
	SpecCtl *d_ctl = nullptr;
	int rc = FSEQ_E_HIP;
	auto A_free = [&]() {
		(void) hipFree(A.M); (void) hipFree(A.K); (void) hipFree(A.Tb); (void) hipFree(A.Tbv); (void) hipFree(d_prev); (void) hipFree(d_lift);
		(void) hipFree(d_r0); (void) hipFree(d_q); (void) hipFree(d_out); (void) hipFree(d_ctl);
	};
	std::vector<uint2> hq(n_queries), ho(n_queries);
	for (uint32_t q = 0; q < n_queries; ++q) hq[q] = make_uint2(beg[q], end[q]);
	uint32_t const r0[2] = {0u, count};                       // one "chunk" of `count` rounds of one entry
	do
	{
		if (hipMalloc((void **) &A.M, ((size_t) count + 64) * 4) != hipSuccess) break;
		if (hipMalloc((void **) &A.K, ((size_t) count + 64) * 8) != hipSuccess) break;
		if (hipMalloc((void **) &A.Tb, (size_t) 32 * A.tstride * 4) != hipSuccess) break;
		if (hipMalloc((void **) &A.Tbv, (size_t) 32 * A.tstride * 4) != hipSuccess) break;
		if (hipMalloc((void **) &d_prev, ((size_t) count + 64) * 4) != hipSuccess) break;
		if (hipMalloc((void **) &d_lift, 16) != hipSuccess) break;
		if (hipMalloc((void **) &d_r0, 16) != hipSuccess) break;
		if (hipMalloc((void **) &d_q, std::max<size_t>(1, n_queries) * 8) != hipSuccess) break;
		if (hipMalloc((void **) &d_out, std::max<size_t>(1, n_queries) * 8) != hipSuccess) break;
		if (hipMalloc((void **) &d_ctl, sizeof(SpecCtl)) != hipSuccess) break;
		if (hipMemcpy(A.M, keys, (size_t) count * 4, hipMemcpyHostToDevice) != hipSuccess) break;
		if (hipMemset(d_lift, 0, 16) != hipSuccess || hipMemset(d_ctl, 0, sizeof(SpecCtl)) != hipSuccess) break;
		if (hipMemcpy(d_r0, r0, 8, hipMemcpyHostToDevice) != hipSuccess) break;
		if (n_queries && hipMemcpy(d_q, hq.data(), (size_t) n_queries * 8, hipMemcpyHostToDevice) != hipSuccess) break;
		SpecGeom G;
		G.chunk_r0 = d_r0; G.RL = 1; G.nchunks = 1; G.NR = count; G.t_final = count + 32u; G.win = 1;
		hipLaunchKernelGGL(k_spec_rebuild, dim3((count + 255u) / 256u), dim3(256), 0, 0, A, d_prev, G, d_lift, d_ctl);
		hipLaunchKernelGGL(k_spec_table, dim3((count / 64u + 255u) / 256u + 1u), dim3(256), 0, 0, A, count / 64u, d_ctl);
		size_t const lds = (size_t) DPW * 12 + (size_t) DP_LEVELS * DP_TRN * 8 + 64;
		if (allow_lds(k_debug_rmq, lds) != hipSuccess) break;
		hipLaunchKernelGGL(k_debug_rmq, dim3(1), dim3(1024), lds, 0, A, count, d_q, n_queries, d_out);
		if (hipGetLastError() != hipSuccess || hipDeviceSynchronize() != hipSuccess) break;
		if (n_queries && hipMemcpy(ho.data(), d_out, (size_t) n_queries * 8, hipMemcpyDeviceToHost) != hipSuccess) break;
		for (uint32_t q = 0; q < n_queries; ++q) { index_hbm[q] = ho[q].x; if (index_lds) index_lds[q] = ho[q].y; }
		rc = FSEQ_OK;
	} while (false);
	A_free();
	return rc;
}

// The traceback as a sharded run in window mode follows it, part by part in one process: follow_traceback_sharded's launchers
// and walk; in place of the exchange, part g's two words are read back and handed to the walk.  The chain only descends, so
// the parts are served from the last one down: each makes its view and its windows, the one the chain stands in follows its
// share and emits it.
int fseq_debug_traceback_parts(int device, uint64_t n, uint64_t segment_length, uint32_t const *lb, uint32_t const *max_size, uint32_t const *size,
                               uint32_t const *part_lo, uint32_t n_parts, uint32_t const *foreign, fseq_dp_arg *traceback, uint64_t *n_traceback,
                               uint32_t *part_entries, uint32_t *part_windows, uint64_t *bad_entry)
{
	if (bad_entry) *bad_entry = ~0ull;
	if (!lb || !max_size || !size || !part_lo || 0 == n_parts || n_parts > 64) return FSEQ_E_ARG;
	if (tb_chain_check(lb, n, segment_length, bad_entry, nullptr) != TB_CHAIN_OK) return FSEQ_E_ARG;
	uint32_t const L = (uint32_t) segment_length, dp_size = (uint32_t) (n - segment_length + 1);
	if (part_lo[0] != 0) return FSEQ_E_ARG;
	for (uint32_t g = 1; g < n_parts; ++g)
		if (part_lo[g] <= part_lo[g - 1] || part_lo[g] >= dp_size) return FSEQ_E_ARG;
	if (hipSetDevice(device) != hipSuccess) return FSEQ_E_HIP;
	size_t const cap = (size_t) (n / L + 2);
	uint32_t const nwin = (dp_size + TB_WIN - 1u) / TB_WIN;
	uint32_t *d_view = nullptr, *d_M = nullptr, *d_SZ = nullptr, *d_next = nullptr, *d_cnt = nullptr, *d_count = nullptr, *d_word = nullptr;
	uint2 *d_head = nullptr;
	uint4 *d_out = nullptr;
	auto free_all = [&]() {
		(void) hipFree(d_view); (void) hipFree(d_M); (void) hipFree(d_SZ); (void) hipFree(d_next); (void) hipFree(d_cnt); (void) hipFree(d_count);
		(void) hipFree(d_word); (void) hipFree(d_head); (void) hipFree(d_out);
	};
	std::vector<uint32_t> view(dp_size), ents(n_parts, 0u), wins(n_parts, 0u);
	std::vector<uint4> h(cap);
	TbPartWalk walk(part_lo, n_parts, dp_size - 1u, cap);
	uint32_t ended_in_zero = 0;
	int rc = FSEQ_E_HIP;
	do
	{
		size_t const words = (size_t) dp_size * 4;
		if (hipMalloc((void **) &d_view, words) != hipSuccess || hipMalloc((void **) &d_M, words) != hipSuccess || hipMalloc((void **) &d_SZ, words) != hipSuccess) break;
		if (hipMalloc((void **) &d_next, words) != hipSuccess || hipMalloc((void **) &d_cnt, words) != hipSuccess) break;
		if (hipMalloc((void **) &d_count, 16) != hipSuccess || hipMalloc((void **) &d_word, 16) != hipSuccess) break;
		if (hipMalloc((void **) &d_head, (size_t) nwin * sizeof(uint2)) != hipSuccess || hipMalloc((void **) &d_out, cap * sizeof(uint4)) != hipSuccess) break;
		if (hipMemcpy(d_M, max_size, words, hipMemcpyHostToDevice) != hipSuccess || hipMemcpy(d_SZ, size, words, hipMemcpyHostToDevice) != hipSuccess) break;
		bool failed = false;
		for (uint32_t g = n_parts; g-- > 0 && !failed;)
		{
			failed = true;
			uint32_t const vlo = part_lo[g], vhi = g + 1u < n_parts ? part_lo[g + 1u] : dp_size;
			// the part's view: its own entries, and what it holds of the others' (nothing it may follow)
			for (uint32_t t = 0; t < dp_size; ++t) view[t] = (t >= vlo && t < vhi) ? lb[t] : foreign ? foreign[t] : 0xFFFFFFFFu;
			if (hipMemcpy(d_view, view.data(), words, hipMemcpyHostToDevice) != hipSuccess) break;
			if (hipMemset(d_count, 0, 16) != hipSuccess || hipMemset(d_word, 0, 16) != hipSuccess) break;
			launch_tb_windows(nullptr, d_view, dp_size, L, d_next, d_cnt, vlo, vhi);
			bool const mine = !walk.ended && walk.owner() == g;
			uint32_t const off0 = walk.off;
			if (mine)
			{
				launch_tb_chain_part(nullptr, d_next, d_cnt, walk.cur, off0, vlo, d_head, nwin, d_count, d_word);
				launch_tb_emit(nullptr, d_view, d_M, d_SZ, dp_size, L, d_head, d_count, d_out, (uint32_t) cap, vlo);
			}
			if (hipGetLastError() != hipSuccess || hipDeviceSynchronize() != hipSuccess) break;
			if (mine)
			{
				uint32_t w[4], cnt[4];
				if (hipMemcpy(w, d_word, 16, hipMemcpyDeviceToHost) != hipSuccess || hipMemcpy(cnt, d_count, 16, hipMemcpyDeviceToHost) != hipSuccess) break;
				if (walk.take(g, w)) break;                                   // (the refusals of a sharded run)
				if (hipMemcpy(h.data() + off0, d_out + off0, (size_t) w[1] * sizeof(uint4), hipMemcpyDeviceToHost) != hipSuccess) break;
				ents[g] = w[1]; wins[g] = cnt[2];
				ended_in_zero |= cnt[1];
			}
			failed = false;
		}
		if (failed || !walk.ended || ended_in_zero != 1u || walk.off == 0) break;
		size_t const S = walk.off;
		if (n_traceback) *n_traceback = S;
		for (size_t j = 0; traceback && j < S; ++j)
		{
			uint4 const e = h[S - 1 - j];                             // the kernels list the last segment first
			traceback[j] = fseq_dp_arg{e.y, (uint64_t) e.x + L, e.z, e.w};
		}
		if (part_entries) std::copy(ents.begin(), ents.end(), part_entries);
		if (part_windows) std::copy(wins.begin(), wins.end(), part_windows);
		rc = FSEQ_OK;
	} while (false);
	free_all();
	return rc;
}

} // extern "C"
