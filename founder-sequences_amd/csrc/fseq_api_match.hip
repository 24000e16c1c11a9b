// fseq_api_match.hip -- the part of the C ABI (include/fseq.h) that validates founders: every input row matched against
// them on the device.
//
// replaces: match-sequences-to-founders (match_founder_sequences.cc:108-259, match-sequences-to-founders/cmdline.ggo), which
// reads the rows and the founders from files and matches on host threads.  Here the rows are the alignment the context
// already holds; the kernels are in fseq_match.hpp.  A translation unit of its own: it is built beside the others and
// touches nothing of the segmentation's state.
#include "fseq_ctx.hpp"
#include "fseq_match.hpp"

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

// A.kept set: the restored form of the walk (source positions, gap steps), a kernel of its own per variant
template <bool WRITE, bool RST>
hipError_t launch_walk_as(fseq_ctx *c, MatchShape const &s, MatchWalkArgs const &A)
{
	void (*k)(MatchWalkArgs) = nullptr;
	switch (s.WR)
	{
		case 1: k = k_match_walk<1, WRITE, RST>; break;
		case 2: k = k_match_walk<2, WRITE, RST>; break;
		case 4: k = k_match_walk<4, WRITE, RST>; break;
		case 8: k = k_match_walk<8, WRITE, RST>; break;
		default: k = k_match_walk<0, WRITE, RST>; break;
	}
	hipError_t const e = allow_lds(k, s.lds);
	if (e != hipSuccess) return e;
	hipLaunchKernelGGL(k, dim3((c->p.m + MT_T - 1u) / MT_T), dim3(MT_T), s.lds, c->stream, A);
	return hipGetLastError();
}

template <bool WRITE>
hipError_t launch_walk(fseq_ctx *c, MatchShape const &s, MatchWalkArgs const &A)
{
	return A.kept ? launch_walk_as<WRITE, true>(c, s, A) : launch_walk_as<WRITE, false>(c, s, A);
}

// both walks over the founders' columns in c->match.fcols; ev[0] has been recorded in front of the kernel that wrote them.
// ms_device = ev[0] .. ev[1] (the founders' columns, the counting walk, the scan) + ev[2] .. ev[3] (the writing walk): the host's
// wait for the totals and the allocation of the output between the two are not in it.
// restored: the pieces in the source's co-ordinates, the identity columns of c->idn between the kept columns accounted for
int run_match(fseq_ctx *c, MatchShape const &s, uint64_t min_len, fseq_match_summary *out, bool restored = false)
{
	auto &mt = c->match;
	hipStream_t st = c->stream;
	uint32_t const m = c->p.m;
	int rc;
	if ((rc = mt.cnt.ensure(c, 3 * (size_t) m)) || (rc = mt.off.ensure(c, (size_t) m + 1 + 4))) return rc;
	uint64_t *const d_tot = mt.off + (m + 1);
	MatchWalkArgs A{};
	A.msa = c->d_msa; A.ld = c->ld; A.m = m; A.n = c->p.n; A.bsh = c->bsh; A.sigma = c->sigma;
	A.fcols = mt.fcols; A.K = s.K; A.Kp = s.Kp; A.W = s.W; A.Wk = s.Wk; A.TC = s.TC; A.min_len = min_len;
	A.cnt = mt.cnt; A.off = mt.off;
	if (restored) { A.kept = c->idn.kept; A.n_src = c->idn.n_src; }
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
	mt.have = true;
	*out = mt.sum;
	return FSEQ_OK;
}

int begin_match(fseq_ctx *c, MatchShape const &s)
{
	auto &mt = c->match;
	mt.have = false;                                              // (a failed match leaves no result behind)
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

// fseq_match_founders and, restored, fseq_match_founders_restored: the founders' columns from the permutations of the run
int match_permutations(fseq_ctx *c, uint32_t const *permutations, uint64_t min_segment_length, fseq_match_summary *out, bool restored)
{
	if (c->sh.on) return refuse_common(c, 0);
	if (!c->have_result || c->res.short_path) return fail(c, FSEQ_E_ARG, "match: permutations need a finished long-path run (short path: hand the rows of fseq_short_path_runs to fseq_match_founder_rows)");
	size_t const X = c->res.max_segment_size, S = c->segments.size();
	if (!X || !S) return fail(c, FSEQ_E_ARG, "match: no segments (segmentation failed or was not run)");
	int rc = refuse_common(c, (uint32_t) X);
	if (rc) return rc;
	if (restored && c->idn.n_src >= 0xFFFFFFFFull) return fail(c, FSEQ_E_UNSUPPORTED, "match: the per-row counters are 32 bits wide (source n < 2^32 - 1)");
	for (size_t i = 0; i < S; ++i)
		if (c->segments[i].lb != (i ? c->segments[i - 1].rb : 0u) || (i + 1 == S && c->segments[i].rb != c->p.n))
			return fail(c, FSEQ_E_ARG, "match: the merged segments do not tile the columns");
	(void) hipSetDevice(c->p.device);
	MatchShape const s = match_shape((uint32_t) X, c->sigma, c->bsh);
	if ((rc = begin_match(c, s))) return rc;
	hipStream_t st = c->stream;
	DevTemp<uint32_t> d_perm(c);
	DevTemp<uint64_t> d_rb(c);
	if ((rc = d_perm.alloc(S * X)) || (rc = d_rb.alloc(S))) return rc;
	std::vector<uint64_t> rbs(S);
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
	return run_match(c, s, min_segment_length, out, restored);
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
	if ((rc = begin_match(c, s))) return rc;
	hipStream_t st = c->stream;
	uint64_t const n = c->p.n;
	DevTemp<uint8_t> d_raw(c), d_lut(c);
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
	return run_match(c, s, min_segment_length, out);
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
