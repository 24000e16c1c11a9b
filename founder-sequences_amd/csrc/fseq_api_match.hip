// fseq_api_match.hip -- the part of the C ABI (include/fseq.h) that validates founders: every input row matched against
// them on the device.
//
// replaces: match-sequences-to-founders (match_founder_sequences.cc:108-259, match-sequences-to-founders/cmdline.ggo), which
// reads the rows and the founders from files and matches on host threads.  Here the rows are the alignment the context
// already holds; the kernels are in fseq_match.hpp.  A translation unit of its own: it is built beside the others and
// touches nothing of the segmentation's state.
#include "fseq_ctx.hpp"
#include "fseq_match.hpp"
#include "fseq_exceptions.hpp"

using namespace fseq;

namespace {

int refuse_common(fseq_ctx *c, uint32_t K)
{
	if (c->sh.on) return fail(c, FSEQ_E_UNSUPPORTED, "match: sharded context: a rank holds its own columns only (match on an unsharded context)");
	if (!c->have_input || !c->d_msa) return fail(c, FSEQ_E_ARG, "match: no alignment resident on the device");
	if (K > MT_MAX_FOUNDERS)
	{
		char what[160];
		snprintf(what, sizeof(what), "match: %u founders, the kernels hold the live sets of at most %u", K, MT_MAX_FOUNDERS);
		return fail(c, FSEQ_E_UNSUPPORTED, what);
	}
	if (c->p.n >= 0xFFFFFFFFull) return fail(c, FSEQ_E_UNSUPPORTED, "match: the per-row counters are 32 bits wide (n < 2^32 - 1)");
	return FSEQ_OK;
}

// A.kept set: the restored form of the walk (source positions, gap steps), a kernel of its own per variant; A.exc_off set as
// well: the restored form for query rows, which reads their exception cells
template <bool WRITE, bool RST, bool EXC>
hipError_t launch_walk_as(fseq_ctx *c, MatchShape const &s, MatchWalkArgs const &A)
{
	void (*k)(MatchWalkArgs) = nullptr;
	switch (s.WR)
	{
		case 1: k = k_match_walk<1, WRITE, RST, EXC>; break;
		case 2: k = k_match_walk<2, WRITE, RST, EXC>; break;
		case 4: k = k_match_walk<4, WRITE, RST, EXC>; break;
		case 8: k = k_match_walk<8, WRITE, RST, EXC>; break;
		default: k = k_match_walk<0, WRITE, RST, EXC>; break;
	}
	hipError_t const e = allow_lds(k, s.lds);
	if (e != hipSuccess) return e;
	hipLaunchKernelGGL(k, dim3((A.m + MT_T - 1u) / MT_T), dim3(MT_T), s.lds, c->stream, A);
	return hipGetLastError();
}

template <bool WRITE>
hipError_t launch_walk(fseq_ctx *c, MatchShape const &s, MatchWalkArgs const &A)
{
	if (!A.kept) return launch_walk_as<WRITE, false, false>(c, s, A);
	return A.exc_off ? launch_walk_as<WRITE, true, true>(c, s, A) : launch_walk_as<WRITE, true, false>(c, s, A);
}

// the rows a match walks where they are not the alignment's: the queries of fseq_match_rows, the held-out rows
struct MatchRows { uint8_t const *cols; size_t ld; uint32_t m, bsh; };
// ... and, for the restored walk of such rows, their exception cells (csrc/fseq_exceptions.hpp)
struct MatchExceptions { uint64_t const *off; uint32_t const *cols; };

// both walks over the founders' columns in c->match.fcols; ev[0] has been recorded in front of the kernel that wrote them.
// ms_device = ev[0] .. ev[1] (the founders' columns, the counting walk, the scan) + ev[2] .. ev[3] (the writing walk): the host's
// wait for the totals and the allocation of the output between the two are not in it.
// restored: the pieces in the source's co-ordinates, the identity columns of c->idn between the kept columns accounted for.
// R: the rows walked (nullptr: the alignment's); X: restored query rows' exception cells
int run_match(fseq_ctx *c, MatchShape const &s, uint64_t min_len, fseq_match_summary *out, bool restored = false, MatchRows const *R = nullptr,
              MatchExceptions const *X = nullptr)
{
	auto &mt = c->match;
	hipStream_t st = c->stream;
	uint32_t const m = R ? R->m : c->p.m;
	int rc;
	if ((rc = mt.cnt.ensure(c, 3 * (size_t) m)) || (rc = mt.off.ensure(c, (size_t) m + 1 + 4))) return rc;
	uint64_t *const d_tot = mt.off + (m + 1);
	MatchWalkArgs A{};
	A.msa = R ? R->cols : c->d_msa; A.ld = R ? R->ld : c->ld; A.m = m; A.n = c->p.n; A.bsh = R ? R->bsh : c->bsh; A.sigma = c->sigma;
	A.fcols = mt.fcols; A.K = s.K; A.Kp = s.Kp; A.W = s.W; A.Wk = s.Wk; A.TC = s.TC; A.min_len = min_len;
	A.cnt = mt.cnt; A.off = mt.off;
	if (restored) { A.kept = c->idn.kept; A.n_src = c->idn.n_src; }
	if (restored && X) { A.exc_off = X->off; A.exc_cols = X->cols; }
	hipError_t e = launch_walk<false>(c, s, A);
	if (e != hipSuccess) return fail(c, FSEQ_E_HIP, "match: counting walk", e);
	hipLaunchKernelGGL(k_match_scan, dim3(1), dim3(MT_SCAN_T), 0, st, mt.cnt, m, mt.off, d_tot);
	HIP_TRY(c, hipGetLastError());
	uint64_t tot[4] = {0, 0, 0, 0};
	HIP_TRY(c, hipEventRecord(mt.ev[1], st));
	HIP_TRY(c, hipMemcpyAsync(tot, d_tot, sizeof(tot), hipMemcpyDeviceToHost, st));
	HIP_TRY(c, hipStreamSynchronize(st));
	HIP_TRY(c, hipGetLastError());
	// exactly sized output (grow-only buffers: a smaller result keeps what is there)
	if ((rc = mt.pieces.ensure(c, (size_t) tot[0])) || (rc = mt.sets.ensure(c, (size_t) tot[0] * s.W))) return rc;
	A.pieces = mt.pieces; A.sets = mt.sets;
	HIP_TRY(c, hipEventRecord(mt.ev[2], st));
	e = launch_walk<true>(c, s, A);
	if (e != hipSuccess) return fail(c, FSEQ_E_HIP, "match: writing walk", e);
	HIP_TRY(c, hipEventRecord(mt.ev[3], st));
	HIP_TRY(c, hipStreamSynchronize(st));
	HIP_TRY(c, hipGetLastError());
	float ms0 = 0.f, ms1 = 0.f;
	HIP_TRY(c, hipEventElapsedTime(&ms0, mt.ev[0], mt.ev[1]));
	HIP_TRY(c, hipEventElapsedTime(&ms1, mt.ev[2], mt.ev[3]));
	mt.sum = fseq_match_summary{tot[0], tot[1], tot[2], tot[3], s.K, s.W, (double) ms0 + (double) ms1};
	mt.split_info = fseq_match_split_info{1u, (m + MT_T - 1u) / MT_T, 0u, 0u, 0u, 0u};
	mt.have = true;
	*out = mt.sum;
	return FSEQ_OK;
}

template <bool WRITE, bool RST, bool EXC>
hipError_t launch_split_as(fseq_ctx *c, MatchShape const &s, MatchSplitArgs const &A, dim3 grid)
{
	void (*k)(MatchSplitArgs) = nullptr;
	switch (s.WR)
	{
		case 1: k = k_match_walk_split<1, WRITE, RST, EXC>; break;
		case 2: k = k_match_walk_split<2, WRITE, RST, EXC>; break;
		case 4: k = k_match_walk_split<4, WRITE, RST, EXC>; break;
		case 8: k = k_match_walk_split<8, WRITE, RST, EXC>; break;
		default: k = k_match_walk_split<0, WRITE, RST, EXC>; break;
	}
	hipError_t const e = allow_lds(k, s.lds);
	if (e != hipSuccess) return e;
	hipLaunchKernelGGL(k, grid, dim3(MT_T), s.lds, c->stream, A);
	return hipGetLastError();
}

// A.w.kept / A.w.exc_off set: the restored forms, as launch_walk
template <bool WRITE>
hipError_t launch_split(fseq_ctx *c, MatchShape const &s, MatchSplitArgs const &A, dim3 grid)
{
	if (!A.w.kept) return launch_split_as<WRITE, false, false>(c, s, A, grid);
	return A.w.exc_off ? launch_split_as<WRITE, true, true>(c, s, A, grid) : launch_split_as<WRITE, true, false>(c, s, A, grid);
}

// run_match with the columns split into plan.G segments (csrc/fseq_match.hpp): counting walk over (row groups x G), the check,
// the counting walk of the flagged groups unsplit, the scan per (row, g); then both writing walks.  No launch depends on a
// count the host has not read: the fall-back launches cover every group and the workgroups beyond the list return at once.
// G = 1 is the unsplit walk through the same kernel, without the check.  ms_device as run_match.
// restored: as run_match; the plan's segments and overlap are then counted in the context's (kept) columns, and head / tail
// hold source positions.  X: restored query rows' exception cells
int run_match_split(fseq_ctx *c, MatchShape const &s, MatchRows const &R, MatchSplitPlan const &plan, uint64_t min_len, fseq_match_summary *out,
                    bool restored = false, MatchExceptions const *X = nullptr)
{
	auto &mt = c->match;
	hipStream_t st = c->stream;
	uint32_t const m = R.m, G = plan.G, groups = (m + MT_T - 1u) / MT_T;
	size_t const slots = (size_t) m * G;
	int rc;
	if ((rc = mt.cnt.ensure(c, 3 * slots)) || (rc = mt.off.ensure(c, slots + 1 + 4)) || (rc = mt.split.ensure(c, 2 * slots + 2 * (size_t) groups + 2))) return rc;
	uint64_t *const d_tot = mt.off + (slots + 1);
	uint32_t *const d_head = mt.split, *const d_tail = d_head + slots, *const d_flag = d_tail + slots, *const d_list = d_flag + groups, *const d_info = d_list + groups;
	MatchSplitArgs A{};
	A.w.msa = R.cols; A.w.ld = R.ld; A.w.m = m; A.w.n = c->p.n; A.w.bsh = R.bsh; A.w.sigma = c->sigma;
	A.w.fcols = mt.fcols; A.w.K = s.K; A.w.Kp = s.Kp; A.w.W = s.W; A.w.Wk = s.Wk; A.w.TC = s.TC; A.w.min_len = min_len;
	A.w.cnt = mt.cnt; A.w.off = mt.off;
	if (restored) { A.w.kept = c->idn.kept; A.w.n_src = c->idn.n_src; }
	if (restored && X) { A.w.exc_off = X->off; A.w.exc_cols = X->cols; }
	A.G = G; A.GS = G; A.overlap = plan.overlap; A.head = d_head; A.tail = d_tail;
	MatchSplitArgs F = A;                                          // the fall-back: one segment, into slot 0 of the G
	F.G = 1; F.list = d_list; F.nlist = d_info;
	HIP_TRY(c, hipMemsetAsync(d_info, 0, 2 * sizeof(uint32_t), st));
	hipError_t e = launch_split<false>(c, s, A, dim3(groups, G));
	if (e != hipSuccess) return fail(c, FSEQ_E_HIP, "match: split counting walk", e);
	if (G > 1)
	{
		hipLaunchKernelGGL(k_match_split_check, dim3(groups), dim3(MT_T), 0, st, d_head, d_tail, m, G, (uint32_t *) mt.cnt, d_flag, d_list, d_info);
		HIP_TRY(c, hipGetLastError());
		e = launch_split<false>(c, s, F, dim3(groups));
		if (e != hipSuccess) return fail(c, FSEQ_E_HIP, "match: counting walk of the flagged groups", e);
	}
	hipLaunchKernelGGL(k_match_scan_split, dim3(1), dim3(MT_SCAN_T), 0, st, mt.cnt, m, G, mt.off, d_tot);
	HIP_TRY(c, hipGetLastError());
	uint64_t tot[4] = {0, 0, 0, 0};
	uint32_t info[2] = {0, 0};
	HIP_TRY(c, hipEventRecord(mt.ev[1], st));
	HIP_TRY(c, hipMemcpyAsync(tot, d_tot, sizeof(tot), hipMemcpyDeviceToHost, st));
	HIP_TRY(c, hipMemcpyAsync(info, d_info, sizeof(info), hipMemcpyDeviceToHost, st));
	HIP_TRY(c, hipStreamSynchronize(st));
	HIP_TRY(c, hipGetLastError());
	if ((rc = mt.pieces.ensure(c, (size_t) tot[0])) || (rc = mt.sets.ensure(c, (size_t) tot[0] * s.W))) return rc;
	A.w.pieces = F.w.pieces = mt.pieces; A.w.sets = F.w.sets = mt.sets;
	if (G > 1) A.flag = d_flag;
	HIP_TRY(c, hipEventRecord(mt.ev[2], st));
	if (info[0] < groups)
	{
		e = launch_split<true>(c, s, A, dim3(groups, G));
		if (e != hipSuccess) return fail(c, FSEQ_E_HIP, "match: split writing walk", e);
	}
	if (info[0])
	{
		e = launch_split<true>(c, s, F, dim3(info[0]));
		if (e != hipSuccess) return fail(c, FSEQ_E_HIP, "match: writing walk of the flagged groups", e);
	}
	HIP_TRY(c, hipEventRecord(mt.ev[3], st));
	HIP_TRY(c, hipStreamSynchronize(st));
	HIP_TRY(c, hipGetLastError());
	float ms0 = 0.f, ms1 = 0.f;
	HIP_TRY(c, hipEventElapsedTime(&ms0, mt.ev[0], mt.ev[1]));
	HIP_TRY(c, hipEventElapsedTime(&ms1, mt.ev[2], mt.ev[3]));
	mt.sum = fseq_match_summary{tot[0], tot[1], tot[2], tot[3], s.K, s.W, (double) ms0 + (double) ms1};
	mt.split_info = fseq_match_split_info{G, groups, info[0], 0u, plan.overlap, info[1]};
	mt.have = true;
	*out = mt.sum;
	return FSEQ_OK;
}

// FSEQ_MATCH_SPLIT set: fseq_match_founders, fseq_match_founder_rows and fseq_match_founders_restored walk the alignment's rows
// split as it says
int run_match_as_tuned(fseq_ctx *c, MatchShape const &s, uint64_t min_len, fseq_match_summary *out, bool restored = false)
{
	if (!c->tune.match_split) return run_match(c, s, min_len, out, restored);
	MatchSplitPlan const plan = match_split_plan(c->p.n, c->p.m, 0, (uint32_t) c->tune.match_split, (uint64_t) c->tune.match_overlap, false);
	return run_match_split(c, s, MatchRows{c->d_msa, c->ld, c->p.m, c->bsh}, plan, min_len, out, restored);
}

int begin_match(fseq_ctx *c, MatchShape const &s)
{
	auto &mt = c->match;
	mt.have = false;                                              // (a failed match leaves no result behind)
	mt.exc_from = 0;
	for (auto &e : mt.ev)
		if (!e) HIP_TRY(c, hipEventCreate(&e));
	return mt.fcols.ensure(c, (size_t) c->p.n * s.Kp);
}

// digits of v at p, returns the end
inline char *put_u64(char *p, uint64_t v)
{
	char tmp[20];
	int k = 0;
	do { tmp[k++] = (char) ('0' + v % 10); v /= 10; } while (v);
	while (k) *p++ = tmp[--k];
	return p;
}

// the refusals of a match by permutations; X: the founders
int check_permutations(fseq_ctx *c, bool restored, size_t &X)
{
	if (c->sh.on) return refuse_common(c, 0);
	if (!c->have_result || c->res.short_path) return fail(c, FSEQ_E_ARG, "match: permutations need a finished long-path run (short path: hand the rows of fseq_short_path_runs to fseq_match_founder_rows)");
	X = c->res.max_segment_size;
	size_t const S = c->segments.size();
	if (!X || !S) return fail(c, FSEQ_E_ARG, "match: no segments (segmentation failed or was not run)");
	int rc = refuse_common(c, (uint32_t) X);
	if (rc) return rc;
	if (restored && c->idn.n_src >= 0xFFFFFFFFull) return fail(c, FSEQ_E_UNSUPPORTED, "match: the per-row counters are 32 bits wide (source n < 2^32 - 1)");
	for (size_t i = 0; i < S; ++i)
		if (c->segments[i].lb != (i ? c->segments[i - 1].rb : 0u) || (i + 1 == S && c->segments[i].rb != c->p.n))
			return fail(c, FSEQ_E_ARG, "match: the merged segments do not tile the columns");
	return FSEQ_OK;
}

// what the kernels that lay out the founders' columns read: the caller holds it until the walks behind them have run
struct FounderTemps {
	DevTemp<uint32_t> perm;
	DevTemp<uint64_t> rb;
	DevTemp<uint8_t> raw, lut;
	std::vector<uint64_t> rbs;
	explicit FounderTemps(fseq_ctx *c) : perm(c), rb(c), raw(c), lut(c) {}
};

// the founders' columns (c->match.fcols, after begin_match) from the permutations of the run; records ev[0] in front of the kernel
int cols_from_permutations(fseq_ctx *c, uint32_t const *permutations, MatchShape const &s, FounderTemps &T)
{
	size_t const X = s.K, S = c->segments.size();
	int rc;
	hipStream_t st = c->stream;
	auto &d_perm = T.perm;
	auto &d_rb = T.rb;
	if ((rc = d_perm.alloc(S * X)) || (rc = d_rb.alloc(S))) return rc;
	auto &rbs = T.rbs;
	rbs.resize(S);
	for (size_t i = 0; i < S; ++i) rbs[i] = c->segments[i].rb;
	// '-' as k_founders prints it for a slot without a row: its code if the alphabet has one, otherwise a code no row has
	uint32_t gap = MT_NOCODE;
	for (uint32_t k = 0; k < c->sigma; ++k) if (c->code_to_byte[k] == (uint8_t) '-') gap = k;
	HIP_TRY(c, hipMemcpyAsync(d_perm, permutations, S * X * 4, hipMemcpyHostToDevice, st));
	HIP_TRY(c, hipMemcpyAsync(d_rb, rbs.data(), S * 8, hipMemcpyHostToDevice, st));
	HIP_TRY(c, hipEventRecord(c->match.ev[0], st));
	hipLaunchKernelGGL(k_match_founders_cols, dim3((uint32_t) ((c->p.n + 63) / 64)), dim3(256), 0, st, c->d_msa, c->ld, c->p.m, (uint64_t) c->p.n, c->bsh,
	                   d_perm, (uint32_t) X, d_rb, (uint32_t) S, gap, s.Kp, c->match.fcols);
	HIP_TRY(c, hipGetLastError());
	return FSEQ_OK;
}

// ... from K raw rows
int cols_from_rows(fseq_ctx *c, uint8_t const *const *founders, MatchShape const &s, FounderTemps &T)
{
	hipStream_t st = c->stream;
	uint64_t const n = c->p.n;
	uint32_t const K = s.K;
	int rc;
	auto &d_raw = T.raw;
	auto &d_lut = T.lut;
	if ((rc = d_raw.alloc((size_t) K * n)) || (rc = d_lut.alloc(256))) return rc;
	uint8_t code_of[256];
	memset(code_of, (int) MT_NOCODE, sizeof(code_of));             // (a byte outside the alphabet matches nothing)
	for (uint32_t k = 0; k < c->sigma; ++k) code_of[c->code_to_byte[k]] = (uint8_t) k;
	for (uint32_t f = 0; f < K; ++f)
		HIP_TRY(c, hipMemcpyAsync(d_raw + (size_t) f * n, founders[f], n, hipMemcpyHostToDevice, st));
	HIP_TRY(c, hipMemcpyAsync(d_lut, code_of, 256, hipMemcpyHostToDevice, st));
	HIP_TRY(c, hipStreamSynchronize(st));                         // (code_of and the caller's rows are read until here; not part of ms_device)
	HIP_TRY(c, hipEventRecord(c->match.ev[0], st));
	hipLaunchKernelGGL(k_match_founder_rows, dim3((uint32_t) ((n + 63) / 64)), dim3(256), 0, st, d_raw, n, K, s.Kp, d_lut, c->match.fcols);
	HIP_TRY(c, hipGetLastError());
	return FSEQ_OK;
}

// fseq_match_founders and, restored, fseq_match_founders_restored: the founders' columns from the permutations of the run
int match_permutations(fseq_ctx *c, uint32_t const *permutations, uint64_t min_segment_length, fseq_match_summary *out, bool restored)
{
	size_t X = 0;
	int rc = check_permutations(c, restored, X);
	if (rc) return rc;
	(void) hipSetDevice(c->p.device);
	MatchShape const s = match_shape((uint32_t) X, c->sigma, c->bsh);
	FounderTemps T(c);
	if ((rc = begin_match(c, s)) || (rc = cols_from_permutations(c, permutations, s, T))) return rc;
	return run_match_as_tuned(c, s, min_segment_length, out, restored);
}

constexpr size_t MT_QUERY_STAGE_BYTES = (size_t) 64 << 20;

} // namespace

// the queries of fseq_match_rows (and of fseq_graph_thread_rows, csrc/fseq_api_graph.hip) onto the device: column chunks of raw
// bytes through a bounded temporary, packed by k_match_pack_rows into dst at `bsh` / `ld`
int fseq::upload_queries(fseq_ctx *c, uint8_t const *const *rows, uint32_t n_rows, uint32_t bsh, size_t ld, DevBuf<uint8_t> &dst)
{
	hipStream_t st = c->stream;
	uint64_t const n = c->p.n;
	int rc;
	if ((rc = dst.ensure(c, (size_t) n * ld))) return rc;
	// columns of a chunk: a multiple of 16 (the kernel loads 16 bytes of a row), of 64 where the rows leave the room
	uint64_t cw = MT_QUERY_STAGE_BYTES / n_rows;
	cw = cw >= 64 ? cw & ~uint64_t(63) : cw & ~uint64_t(15);
	if (!cw) return fail(c, FSEQ_E_UNSUPPORTED, "match: more query rows than 16 columns of them fit the upload's 64 MiB");
	cw = std::min<uint64_t>(cw, (n + 15) & ~uint64_t(15));
	DevTemp<uint8_t> d_stage(c), d_lut(c);
	if ((rc = d_stage.alloc((size_t) n_rows * cw)) || (rc = d_lut.alloc(256))) return rc;
	uint8_t code_of[256];
	memset(code_of, (int) (c->sigma & 0xFFu), sizeof(code_of));    // (a byte outside the alphabet: the code above the alphabet's; with 256 codes there is no such byte)
	for (uint32_t k = 0; k < c->sigma; ++k) code_of[c->code_to_byte[k]] = (uint8_t) k;
	std::vector<uint8_t> stage;
	try { stage.assign((size_t) n_rows * cw, 0); } catch (std::bad_alloc const &) { return fail(c, FSEQ_E_OOM, "match: host staging of the query rows"); }
	HIP_TRY(c, hipMemcpyAsync(d_lut, code_of, 256, hipMemcpyHostToDevice, st));
	for (uint64_t c0 = 0; c0 < n; c0 += cw)
	{
		uint32_t const w = (uint32_t) std::min<uint64_t>(cw, n - c0);
		for (uint32_t q = 0; q < n_rows; ++q) memcpy(stage.data() + (size_t) q * cw, rows[q] + c0, w);
		HIP_TRY(c, hipMemcpyAsync(d_stage, stage.data(), stage.size(), hipMemcpyHostToDevice, st));
		hipLaunchKernelGGL(k_match_pack_rows, dim3((w + MT_PACK_COLS - 1u) / MT_PACK_COLS, (n_rows + MT_T - 1u) / MT_T), dim3(MT_T), 0, st,
		                   d_stage, (size_t) cw, n_rows, c0, w, d_lut, bsh, (uint8_t *) dst, ld);
		HIP_TRY(c, hipGetLastError());
		HIP_TRY(c, hipStreamSynchronize(st));                     // (the staging is filled again)
	}
	return FSEQ_OK;
}

// the queries of fseq_match_rows_restored (and of fseq_graph_thread_rows_restored, csrc/fseq_api_graph.hip), n_src raw bytes
// each: column chunks of the SOURCE through the same bounded staging; k_match_pack_rows_kept packs a chunk's kept columns into
// their reduced positions of dst, k_exc_bits_rows marks the chunk's identity columns in which a query differs from row 0 in a
// bit matrix of this call, from which exc_off / exc_cols are made (csrc/fseq_exceptions.hpp).  Every query byte crosses to the
// device once
int fseq::upload_queries_restored(fseq_ctx *c, uint8_t const *const *rows, uint32_t n_rows, uint32_t bsh, size_t ld, DevBuf<uint8_t> &dst,
                                  DevBuf<uint64_t> &exc_off, DevBuf<uint32_t> &exc_cols, uint64_t *exc_total)
{
	hipStream_t st = c->stream;
	uint64_t const n = c->p.n, n_src = c->idn.n_src;
	size_t const nw = (size_t) ((n_src + 31u) / 32u);
	int rc;
	if ((rc = dst.ensure(c, (size_t) n * ld))) return rc;
	// columns of a chunk: a multiple of 64 (a lane of k_exc_bits_rows owns a word of 32 columns; FSEQ_MATCH_STAGE_BYTES: at least 64)
	uint64_t cw = ((c->tune.match_stage ? (size_t) c->tune.match_stage : MT_QUERY_STAGE_BYTES) / n_rows) & ~uint64_t(63);
	if (c->tune.match_stage) cw = std::max<uint64_t>(cw, 64);
	if (!cw) return fail(c, FSEQ_E_UNSUPPORTED, "match: more query rows than 64 columns of them fit the upload's 64 MiB");
	cw = std::min<uint64_t>(cw, (n_src + 63) & ~uint64_t(63));
	DevTemp<uint8_t> d_stage(c), d_lut(c);
	DevTemp<uint32_t> d_bits(c);
	if ((rc = d_stage.alloc((size_t) n_rows * cw)) || (rc = d_lut.alloc(256)) || (rc = d_bits.alloc((size_t) n_rows * nw))) return rc;
	uint8_t code_of[256];
	memset(code_of, (int) (c->sigma & 0xFFu), sizeof(code_of));    // (a byte outside the alphabet: the code above the alphabet's)
	for (uint32_t k = 0; k < c->sigma; ++k) code_of[c->code_to_byte[k]] = (uint8_t) k;
	std::vector<uint8_t> stage;
	std::vector<uint32_t> kept;
	try { stage.assign((size_t) n_rows * cw, 0); kept.resize((size_t) n); } catch (std::bad_alloc const &) { return fail(c, FSEQ_E_OOM, "match: host staging of the query rows"); }
	HIP_TRY(c, hipMemcpyAsync(kept.data(), c->idn.kept, (size_t) n * 4, hipMemcpyDeviceToHost, st));
	HIP_TRY(c, hipMemcpyAsync(d_lut, code_of, 256, hipMemcpyHostToDevice, st));
	HIP_TRY(c, hipStreamSynchronize(st));
	for (uint64_t c0 = 0; c0 < n_src; c0 += cw)
	{
		uint32_t const w = (uint32_t) std::min<uint64_t>(cw, n_src - c0);
		for (uint32_t q = 0; q < n_rows; ++q) memcpy(stage.data() + (size_t) q * cw, rows[q] + c0, w);
		HIP_TRY(c, hipMemcpyAsync(d_stage, stage.data(), stage.size(), hipMemcpyHostToDevice, st));
		uint64_t const j_lo = (uint64_t) (std::lower_bound(kept.begin(), kept.end(), (uint32_t) c0) - kept.begin());
		uint64_t const j_hi = (uint64_t) (std::lower_bound(kept.begin(), kept.end(), (uint32_t) (c0 + w)) - kept.begin());
		if (j_hi > j_lo)
			hipLaunchKernelGGL(k_match_pack_rows_kept, dim3((uint32_t) ((j_hi - j_lo + MT_PACK_COLS - 1u) / MT_PACK_COLS), (n_rows + MT_T - 1u) / MT_T), dim3(MT_T), 0, st,
			                   (uint8_t const *) d_stage, (size_t) cw, n_rows, c0, j_lo, j_hi, (uint32_t const *) c->idn.kept, (uint8_t const *) d_lut, bsh, (uint8_t *) dst, ld);
		uint64_t const lanes = (uint64_t) n_rows * ((w + 31u) / 32u);
		hipLaunchKernelGGL(k_exc_bits_rows, dim3((uint32_t) ((lanes + EX_T - 1u) / EX_T)), dim3(EX_T), 0, st, (uint8_t const *) d_stage, (size_t) cw, n_rows, c0, w,
		                   (uint8_t const *) c->idn.ref, (uint8_t const *) c->idn.mask, n_src, (uint32_t *) d_bits, nw);
		HIP_TRY(c, hipGetLastError());
		HIP_TRY(c, hipStreamSynchronize(st));                     // (the staging is filled again)
	}
	return exc_lists_from_bits(c, st, d_bits, nw, n_rows, exc_off, exc_cols, exc_total);
}

namespace {

// fseq_match_held_out_restored / fseq_match_rows_restored behind their refusals: the restored walk over the query rows R, split
// along the kept columns as the knobs say or, without them, as fseq_match_rows chooses by itself; where that choice is one
// segment, the unsplit kernel walks
int match_queries_restored(fseq_ctx *c, uint32_t const *permutations, MatchShape const &s, MatchRows const &R, MatchExceptions const &X, int from,
                           uint64_t min_segment_length, fseq_match_summary *out)
{
	FounderTemps T(c);
	int rc = cols_from_permutations(c, permutations, s, T);
	if (rc) return rc;
	int cus = 0;
	(void) hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, c->p.device);
	MatchSplitPlan const plan = match_split_plan(c->p.n, R.m, (uint32_t) std::max(cus, 1), (uint32_t) c->tune.match_split, (uint64_t) c->tune.match_overlap, true);
	rc = (c->tune.match_split || plan.G > 1u) ? run_match_split(c, s, R, plan, min_segment_length, out, true, &X) : run_match(c, s, min_segment_length, out, true, &R, &X);
	if (rc) return rc;
	c->match.exc_from = from;
	c->match.exc_rows = R.m;
	return FSEQ_OK;
}

} // namespace

extern "C" {

int fseq_match_founders(fseq_ctx *c, uint32_t const *permutations, uint64_t min_segment_length, fseq_match_summary *out)
{
	if (!c || !permutations || !out) return FSEQ_E_ARG;
	return match_permutations(c, permutations, min_segment_length, out, false);
}

// the founders' columns are the reduced context's (k_match_founders_cols, n_kept x Kp): the identity columns, in which every
// restored founder carries row 0's byte as every row does, exist only as the gaps between the source positions in idn.kept
int fseq_match_founders_restored(fseq_ctx *c, uint32_t const *permutations, uint64_t min_segment_length, fseq_match_summary *out)
{
	if (!c || !permutations || !out) return FSEQ_E_ARG;
	if (!c->idn.have) return fail(c, FSEQ_E_ARG, "not a context made by fseq_create_without_identity_columns");
	return match_permutations(c, permutations, min_segment_length, out, true);
}

int fseq_match_founder_rows(fseq_ctx *c, uint8_t const *const *founders, uint32_t K, uint64_t min_segment_length, fseq_match_summary *out)
{
	if (!c || !founders || !out || 0 == K) return FSEQ_E_ARG;
	for (uint32_t f = 0; f < K; ++f)
		if (!founders[f]) return fail(c, FSEQ_E_ARG, "match: null founder row");
	int rc = refuse_common(c, K);
	if (rc) return rc;
	(void) hipSetDevice(c->p.device);
	MatchShape const s = match_shape(K, c->sigma, c->bsh);
	FounderTemps T(c);
	if ((rc = begin_match(c, s)) || (rc = cols_from_rows(c, founders, s, T))) return rc;
	return run_match_as_tuned(c, s, min_segment_length, out);
}

int fseq_match_rows(fseq_ctx *c, uint32_t const *permutations, uint8_t const *const *founders, uint32_t K,
                    uint8_t const *const *rows, uint32_t n_rows, uint64_t min_segment_length, fseq_match_summary *out)
{
	if (!c || !out) return FSEQ_E_ARG;
	if ((permutations != nullptr) == (founders != nullptr && K != 0)) return fail(c, FSEQ_E_ARG, "match: give either the permutations of the run or K founder rows");
	if (permutations && (founders || K)) return fail(c, FSEQ_E_ARG, "match: give either the permutations of the run or K founder rows");
	if (!rows || 0 == n_rows) return fail(c, FSEQ_E_ARG, "match: no query rows");
	for (uint32_t q = 0; q < n_rows; ++q)
		if (!rows[q]) return fail(c, FSEQ_E_ARG, "match: null query row");
	for (uint32_t f = 0; founders && f < K; ++f)
		if (!founders[f]) return fail(c, FSEQ_E_ARG, "match: null founder row");
	if (c->idn.have) return fail(c, FSEQ_E_ARG, "match: query rows on a context made by fseq_create_without_identity_columns (its columns are the kept ones of a longer source)");
	size_t X = K;
	int rc = permutations ? check_permutations(c, false, X) : refuse_common(c, K);
	if (rc) return rc;
	(void) hipSetDevice(c->p.device);
	// the queries' packing: the narrowest that leaves the code `sigma` free for a byte outside the alphabet
	uint32_t const sigma = c->sigma, bsh = sigma + 1u <= 4u ? 2u : sigma + 1u <= 16u ? 1u : 0u;
	size_t const ld = ((((size_t) n_rows + (1u << bsh) - 1u) >> bsh) + 15) & ~size_t(15);
	MatchShape const s = match_shape((uint32_t) X, sigma, bsh);
	if ((rc = begin_match(c, s)) || (rc = upload_queries(c, rows, n_rows, bsh, ld, c->match.qrows))) return rc;
	FounderTemps T(c);
	if ((rc = permutations ? cols_from_permutations(c, permutations, s, T) : cols_from_rows(c, founders, s, T))) return rc;
	int cus = 0;
	(void) hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, c->p.device);
	MatchSplitPlan const plan = match_split_plan(c->p.n, n_rows, (uint32_t) std::max(cus, 1), (uint32_t) c->tune.match_split, (uint64_t) c->tune.match_overlap, true);
	return run_match_split(c, s, MatchRows{c->match.qrows, ld, n_rows, bsh}, plan, min_segment_length, out);
}

// fseq_match_rows with the context's own held-out buffer (fseq_create_without_rows, csrc/fseq_api_rowsplit.hip) as the queries:
// they are on the device already, column-major and packed at the alignment's width, so nothing is uploaded or packed
int fseq_match_held_out(fseq_ctx *c, uint32_t const *permutations, uint8_t const *const *founders, uint32_t K, uint64_t min_segment_length,
                        fseq_match_summary *out)
{
	if (!c || !out) return FSEQ_E_ARG;
	if ((permutations != nullptr) == (founders != nullptr && K != 0)) return fail(c, FSEQ_E_ARG, "match: give either the permutations of the run or K founder rows");
	if (permutations && (founders || K)) return fail(c, FSEQ_E_ARG, "match: give either the permutations of the run or K founder rows");
	for (uint32_t f = 0; founders && f < K; ++f)
		if (!founders[f]) return fail(c, FSEQ_E_ARG, "match: null founder row");
	if (!c->hold.have) return fail(c, FSEQ_E_ARG, "not a context made by fseq_create_without_rows");
	size_t X = K;
	int rc = permutations ? check_permutations(c, false, X) : refuse_common(c, K);
	if (rc) return rc;
	(void) hipSetDevice(c->p.device);
	MatchShape const s = match_shape((uint32_t) X, c->sigma, c->bsh);
	if ((rc = begin_match(c, s))) return rc;
	FounderTemps T(c);
	if ((rc = permutations ? cols_from_permutations(c, permutations, s, T) : cols_from_rows(c, founders, s, T))) return rc;
	int cus = 0;
	(void) hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, c->p.device);
	uint32_t const n_held = c->hold.n_held;
	MatchSplitPlan const plan = match_split_plan(c->p.n, n_held, (uint32_t) std::max(cus, 1), (uint32_t) c->tune.match_split, (uint64_t) c->tune.match_overlap, true);
	return run_match_split(c, s, MatchRows{c->hold.cols, c->hold.ld, n_held, c->bsh}, plan, min_segment_length, out);
}

// the held-out rows' kept columns (c->hold.cols) walked at their source positions, with the exception cells the context was made
// with (fseq_create_without_identity_columns_held): nothing is uploaded, packed or scanned for
int fseq_match_held_out_restored(fseq_ctx *c, uint32_t const *permutations, uint64_t min_segment_length, fseq_match_summary *out)
{
	if (!c || !permutations || !out) return FSEQ_E_ARG;
	if (!c->idn.have || !c->hold.have_exc) return fail(c, FSEQ_E_ARG, "not a context made by fseq_create_without_identity_columns_held");
	size_t X = 0;
	int rc = check_permutations(c, true, X);
	if (rc) return rc;
	(void) hipSetDevice(c->p.device);
	MatchShape const s = match_shape((uint32_t) X, c->sigma, c->bsh);
	if ((rc = begin_match(c, s))) return rc;
	return match_queries_restored(c, permutations, s, MatchRows{c->hold.cols, c->hold.ld, c->hold.n_held, c->bsh}, MatchExceptions{c->hold.exc_off, c->hold.exc_cols}, 1,
	                              min_segment_length, out);
}

int fseq_match_rows_restored(fseq_ctx *c, uint32_t const *permutations, uint8_t const *const *rows, uint32_t n_rows, uint64_t min_segment_length,
                             fseq_match_summary *out)
{
	if (!c || !permutations || !out) return FSEQ_E_ARG;
	if (!rows || 0 == n_rows) return fail(c, FSEQ_E_ARG, "match: no query rows");
	for (uint32_t q = 0; q < n_rows; ++q)
		if (!rows[q]) return fail(c, FSEQ_E_ARG, "match: null query row");
	if (!c->idn.have) return fail(c, FSEQ_E_ARG, "not a context made by fseq_create_without_identity_columns");
	size_t X = 0;
	int rc = check_permutations(c, true, X);
	if (rc) return rc;
	(void) hipSetDevice(c->p.device);
	// the queries' packing: the narrowest that leaves the code `sigma` free for a byte outside the alphabet
	uint32_t const sigma = c->sigma, bsh = sigma + 1u <= 4u ? 2u : sigma + 1u <= 16u ? 1u : 0u;
	size_t const ld = ((((size_t) n_rows + (1u << bsh) - 1u) >> bsh) + 15) & ~size_t(15);
	MatchShape const s = match_shape((uint32_t) X, sigma, bsh);
	if ((rc = begin_match(c, s)) || (rc = upload_queries_restored(c, rows, n_rows, bsh, ld, c->match.qrows, c->match.exc_off, c->match.exc_cols, &c->match.exc_total))) return rc;
	return match_queries_restored(c, permutations, s, MatchRows{c->match.qrows, ld, n_rows, bsh}, MatchExceptions{c->match.exc_off, c->match.exc_cols}, 2,
	                              min_segment_length, out);
}

int fseq_get_match_exceptions(fseq_ctx *c, uint64_t *offsets, uint32_t *columns, uint64_t *total)
{
	if (!c) return FSEQ_E_ARG;
	if (!c->match.have || !c->match.exc_from)
		return fail(c, FSEQ_E_ARG, "the last match on this context is not a restored match of query rows (fseq_match_held_out_restored / fseq_match_rows_restored)");
	bool const own = c->match.exc_from == 2;
	uint64_t const all = own ? c->match.exc_total : c->hold.exc_total;
	(void) hipSetDevice(c->p.device);
	if (offsets) HIP_TRY(c, hipMemcpy(offsets, own ? (uint64_t *) c->match.exc_off : (uint64_t *) c->hold.exc_off, ((size_t) c->match.exc_rows + 1) * 8, hipMemcpyDeviceToHost));
	if (columns && all) HIP_TRY(c, hipMemcpy(columns, own ? (uint32_t *) c->match.exc_cols : (uint32_t *) c->hold.exc_cols, (size_t) all * 4, hipMemcpyDeviceToHost));
	if (total) *total = all;
	return FSEQ_OK;
}

int fseq_debug_match_split(fseq_ctx *c, fseq_match_split_info *info)
{
	if (!c || !info) return FSEQ_E_ARG;
	if (!c->match.have) return fail(c, FSEQ_E_ARG, "no match on this context (fseq_match_founders / fseq_match_founder_rows / fseq_match_rows)");
	*info = c->match.split_info;
	return FSEQ_OK;
}

int fseq_get_match(fseq_ctx *c, fseq_match_piece *pieces, uint32_t *founder_sets)
{
	if (!c) return FSEQ_E_ARG;
	if (!c->match.have) return fail(c, FSEQ_E_ARG, "no match on this context (fseq_match_founders / fseq_match_founder_rows)");
	(void) hipSetDevice(c->p.device);
	size_t const P = (size_t) c->match.sum.pieces, W = c->match.sum.set_words;
	if (pieces && P) HIP_TRY(c, hipMemcpy(pieces, c->match.pieces, P * sizeof(fseq_match_piece), hipMemcpyDeviceToHost));
	if (founder_sets && P) HIP_TRY(c, hipMemcpy(founder_sets, c->match.sets, P * W * 4, hipMemcpyDeviceToHost));
	return FSEQ_OK;
}

int fseq_write_match(fseq_ctx *c, char const *path)
{
	if (!c) return FSEQ_E_ARG;
	if (!c->match.have) return fail(c, FSEQ_E_ARG, "no match on this context (fseq_match_founders / fseq_match_founder_rows)");
	size_t const P = (size_t) c->match.sum.pieces, W = c->match.sum.set_words;
	std::vector<fseq_match_piece> pieces;
	std::vector<uint32_t> sets;
	try { pieces.resize(P); sets.resize(P * W); } catch (std::bad_alloc const &) { return fail(c, FSEQ_E_OOM, "match report buffers"); }
	int const rc = fseq_get_match(c, pieces.data(), sets.data());
	if (rc) return rc;
	FILE *f = (path && strcmp(path, "-") != 0) ? fopen(path, "wb") : stdout;
	if (!f) return fail(c, FSEQ_E_ARG, "cannot open the match output file");
	// match_founder_sequences.cc:220, :125-136
	bool ok = fputs("SEQUENCE_INDEX\tLB\tRB\tFOUNDER_INDICES\n", f) >= 0;
	std::vector<char> buf;
	size_t const flush_at = (size_t) 4 << 20;
	buf.reserve(flush_at + 64 + (size_t) c->match.sum.n_founders * 5);
	for (size_t i = 0; i < P && ok; ++i)
	{
		size_t const at = buf.size();
		buf.resize(at + 64 + (size_t) pieces[i].n_founders * 5);     // (three numbers, and an index of at most four digits plus a comma per founder)
		char *p = buf.data() + at;
		p = put_u64(p, pieces[i].row); *p++ = '\t';
		p = put_u64(p, pieces[i].lb); *p++ = '\t';
		p = put_u64(p, pieces[i].rb); *p++ = '\t';
		bool first = true;
		for (size_t w = 0; w < W; ++w)
			for (uint32_t v = sets[i * W + w]; v; v &= v - 1u)
			{
				if (!first) *p++ = ',';
				first = false;
				p = put_u64(p, w * 32u + (uint32_t) __builtin_ctz(v));
			}
		*p++ = '\n';
		buf.resize((size_t) (p - buf.data()));
		if (buf.size() >= flush_at) { ok = fwrite(buf.data(), 1, buf.size(), f) == buf.size(); buf.clear(); }
	}
	if (ok && !buf.empty()) ok = fwrite(buf.data(), 1, buf.size(), f) == buf.size();
	fflush(f);
	if (f != stdout) fclose(f);
	if (!ok) return fail(c, FSEQ_E_ARG, "writing the match output file failed");
	return FSEQ_OK;
}

} // extern "C"
