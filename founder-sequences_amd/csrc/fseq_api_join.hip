// fseq_api_join.hip -- the part of the C ABI (include/fseq.h) behind the segmentation: segment joining and the output files.
//
// replaces: join_context (join_context.cc:51-356) with greedy_matcher (greedy_matcher.cc:31-465), bipartite_matcher
// (bipartite_matcher.cc:17-151, create_segment_texts_task.cc, merge_segments_task.cc) and the random joiner, and the writers
// of --output-founders / --output-segments (join_context.cc:333-356, segmentation_dp_arg.cc:13-104).  Host C++ as in the
// reference (fseq_join.hpp), with the greedy joiner's data-parallel front -- class tables and co-occurrence edges -- on the
// device where the boundary states are (fseq_joinprep.hpp), and the score of a join (fseq_joinscore.hpp).  A translation unit of its own since round 4: nothing here
// touches the column kernels, and csrc/fseq_api.hip no longer carries the joiners.
#include "fseq_ctx.hpp"
#include "fseq_join.hpp"
#include "fseq_joinprep.hpp"
#include "fseq_joinbip.hpp"
#include "fseq_joinbipw.hpp"
#include "fseq_joinscore.hpp"
#include "fseq_joinscore_host.hpp"
#include "fseq_segfile.hpp"
#include "fseq_restored_bounds.hpp"

using namespace fseq;

// Boundary states (segments x m x 8 bytes) from which fseq_join_greedy takes the wide front by itself when max_segment_size is
// above JP_MAX_CLASSES: the smallest swept size from which it beat the host joiner at every larger one, and never below
// 16 MiB (profiles/join_wide.txt, tools/join_wide_probe.py).
static constexpr uint64_t JOIN_WIDE_MIN_BYTES = 16ull << 20;

// The wide device front of fseq_join_greedy (fseq_joinprep.hpp): what greedy_match_prepared takes, for any X up to 65,535.
// *done = false with FSEQ_OK: the caller goes on to the host joiner (a failed device allocation, implausible tables, a right
// segment of more than JW_CELLS classes, 2^32 edges or more -- the offsets are 32-bit words), with the error text cleared.
static int join_greedy_wide(fseq_ctx *c, uint32_t *permutations, double t0, bool *done)
{
	*done = false;
	size_t const m = c->p.m, S = c->segments.size();
	uint32_t const X = c->res.max_segment_size;
	hipStream_t st = c->stream;
	DevTemp<uint16_t> d_of(c);
	DevTemp<uint32_t> d_rep(c), d_size(c), d_count(c), d_start(c), d_off(c), d_ne(c);
	DevTemp<uint64_t> d_rb(c);
	DevTemp<unsigned long long> d_total(c);
	DevTemp<uint2> d_edges(c);
	auto no_room = [&](int rc) { if (rc == FSEQ_E_OOM) { c->err.clear(); return (int) FSEQ_OK; } return rc; };      // (the host joiner needs no device memory)
	int rc;
	if ((rc = d_of.alloc(S * m)) || (rc = d_rep.alloc(S * X)) || (rc = d_size.alloc(S * X)) || (rc = d_count.alloc(S)) ||
	    (rc = d_start.alloc(S * ((size_t) X + 1))) || (rc = d_off.alloc(S)) || (rc = d_ne.alloc(S)) || (rc = d_rb.alloc(S)) || (rc = d_total.alloc(1)))
		return no_room(rc);
	std::vector<uint64_t> rbs(S);
	for (size_t i = 0; i < S; ++i) rbs[i] = c->segments[i].rb;
	size_t const lds = (size_t) JW_CELLS * 4;
	uint32_t const pairs = (uint32_t) (S - 1);
	hipError_t e = hipMemcpyAsync(d_rb, rbs.data(), S * 8, hipMemcpyHostToDevice, st);
	if (e == hipSuccess) e = hipMemsetAsync(d_rep, 0, S * X * 4, st);
	if (e == hipSuccess) e = allow_lds(k_join_edges_wide<false>, lds);
	if (e == hipSuccess) e = allow_lds(k_join_edges_wide<true>, lds);
	if (e != hipSuccess) return fail(c, FSEQ_E_HIP, "join preparation", e);
	hipLaunchKernelGGL(k_join_classes_wide, dim3((uint32_t) S), dim3(JW_T), 0, st, c->d_snap_a, c->d_snap_d, d_rb, (uint32_t) m, X, d_of, d_rep, d_size, d_count, d_start);
	// the counting pass and the scan: the edge array is allocated at exactly the total
	if (pairs)
		hipLaunchKernelGGL(k_join_edges_wide<false>, dim3(pairs), dim3(JW_T), lds, st, c->d_snap_a, d_of, d_count, d_start, (uint32_t) m, X, d_ne, d_off, (uint2 *) nullptr, (uint64_t) 0);
	hipLaunchKernelGGL(k_join_scan, dim3(1), dim3(JW_T), 0, st, d_ne, pairs, d_off, d_total);
	std::vector<uint32_t> count(S);
	unsigned long long total = 0;
	e = hipMemcpyAsync(count.data(), d_count, S * 4, hipMemcpyDeviceToHost, st);
	if (e == hipSuccess) e = hipMemcpyAsync(&total, d_total, 8, hipMemcpyDeviceToHost, st);
	if (e == hipSuccess) e = hipStreamSynchronize(st);
	if (e == hipSuccess) e = hipGetLastError();
	if (e != hipSuccess) return fail(c, FSEQ_E_HIP, "join preparation", e);
	bool sane = total <= 0xFFFFFFFFull;
	for (size_t i = 0; sane && i < S; ++i) sane = count[i] >= 1 && count[i] <= X && (0 == i || count[i] <= JW_CELLS);
	if (!sane) return FSEQ_OK;                                // (the host joiner builds its own tables from the boundary states)
	if ((rc = d_edges.alloc((size_t) total))) return no_room(rc);
	if (pairs && total)
		hipLaunchKernelGGL(k_join_edges_wide<true>, dim3(pairs), dim3(JW_T), lds, st, c->d_snap_a, d_of, d_count, d_start, (uint32_t) m, X, d_ne, d_off, d_edges, (uint64_t) total);
	std::vector<uint32_t> rep(S * X), size(S * X), off(S), ne(S), edge_words(2 * (size_t) total + 2);
	e = hipMemcpyAsync(rep.data(), d_rep, S * X * 4, hipMemcpyDeviceToHost, st);
	if (e == hipSuccess) e = hipMemcpyAsync(size.data(), d_size, S * X * 4, hipMemcpyDeviceToHost, st);
	if (e == hipSuccess && pairs) e = hipMemcpyAsync(off.data(), d_off, (size_t) pairs * 4, hipMemcpyDeviceToHost, st);
	if (e == hipSuccess && pairs) e = hipMemcpyAsync(ne.data(), d_ne, (size_t) pairs * 4, hipMemcpyDeviceToHost, st);
	if (e == hipSuccess && total) e = hipMemcpyAsync(edge_words.data(), d_edges, (size_t) total * 8, hipMemcpyDeviceToHost, st);
	if (e == hipSuccess) e = hipStreamSynchronize(st);
	if (e == hipSuccess) e = hipGetLastError();
	release_all(c, d_of, d_rep, d_size, d_count, d_start, d_off, d_ne, d_rb, d_total, d_edges);      // (not held through the host's part)
	if (e != hipSuccess) return fail(c, FSEQ_E_HIP, "join preparation", e);
	double const t1 = now_ms();
	JoinProfile prof;
	greedy_match_prepared(c->p.m, X, S, count.data(), rep.data(), size.data(), edge_words.data(), off.data(), ne.data(), permutations, &prof);
	c->jp = fseq_join_profile{t1 - t0, prof.ms_classes, prof.ms_edges, prof.ms_draw, now_ms() - t0,
	                          (uint64_t) S * (2ull * X + 3) * 4 + (uint64_t) total * 8};
	*done = true;
	return FSEQ_OK;
}

// Boundary states from which fseq_join_bipartite takes the wide form by itself when max_segment_size is above JP_MAX_CLASSES:
// the smallest swept size from which it beat the host joiner at every larger one was 4.2 MB, so the floor of 16 MiB decides
// (profiles/join_bip_wide.txt, tools/join_bip_wide_probe.py; the sweep ends at 17 MB, BASELINE C4 ran through the wide form alone).
static constexpr uint64_t JOIN_BIP_WIDE_MIN_BYTES = 16ull << 20;

// The wide device form of fseq_join_bipartite (fseq_joinbipw.hpp), for any X up to JBW_MAX_TEXTS.  *done = false with
// FSEQ_OK: the caller goes on to the host joiner (a failed device allocation -- not one slab --, implausible class counts),
// with the error text cleared.
static int join_bipartite_wide(fseq_ctx *c, uint32_t *permutations, bool *done)
{
	*done = false;
	(void) hipSetDevice(c->p.device);
	double const t0 = now_ms();
	size_t const m = c->p.m, S = c->segments.size();
	uint32_t const X = c->res.max_segment_size;
	uint32_t const pairs = (uint32_t) (S - 1);
	hipStream_t st = c->stream;
	DevTemp<uint16_t> d_of(c), d_tpos(c), d_src(c), d_match(c);
	DevTemp<uint32_t> d_rep(c), d_size(c), d_count(c), d_start(c), d_min(c), d_reprow(c), d_perm(c), d_slabs(c);
	DevTemp<uint64_t> d_rb(c);
	auto no_room = [&](int rc) { if (rc == FSEQ_E_OOM) { c->err.clear(); return (int) FSEQ_OK; } return rc; };      // (the host joiner needs no device memory)
	int rc;
	if ((rc = d_of.alloc(S * m)) || (rc = d_tpos.alloc(S * X)) || (rc = d_src.alloc(S * X)) || (rc = d_match.alloc(S * X)) ||
	    (rc = d_rep.alloc(S * X)) || (rc = d_size.alloc(S * X)) || (rc = d_count.alloc(S)) || (rc = d_start.alloc(S * ((size_t) X + 1))) ||
	    (rc = d_min.alloc(S * X)) || (rc = d_reprow.alloc(S * X)) || (rc = d_perm.alloc(S * X)) || (rc = d_rb.alloc(S)))
		return no_room(rc);
	size_t const lds_texts = bip_texts_wide_lds_bytes(X), lds_match = bip_match_wide_lds_bytes(X);
	// G slabs = persistent workgroups: the pairs, what the CUs hold at once (two workgroups a CU while their LDS allows it),
	// FSEQ_JOIN_BIP_SLABS, and half of what is free on the device and of what is left of the context's memory budget
	uint32_t G = 0;
	if (pairs)
	{
		int ncu = 0;
		if (hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, c->p.device) != hipSuccess || ncu < 1) { (void) hipGetLastError(); ncu = 1; }
		size_t const slab = (size_t) X * X * 4;
		size_t free_b = 0, total_b = 0;
		if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) { (void) hipGetLastError(); free_b = slab; }
		uint64_t room = free_b / 2;
		if (c->mem_budget) room = std::min<uint64_t>(room, (c->mem_budget > c->alloc_total ? c->mem_budget - c->alloc_total : 0) / 2);
		uint64_t g = std::min<uint64_t>(pairs, (uint64_t) ncu * (2 * lds_match <= JBW_LDS_CU ? 2u : 1u));
		if (c->tune.join_bip_slabs > 0) g = std::min<uint64_t>(g, (uint64_t) c->tune.join_bip_slabs);
		g = std::max<uint64_t>(1, std::min<uint64_t>(g, room / slab));
		while (g && !d_slabs.try_alloc(c, (size_t) g * X * X)) g /= 2;
		if (!g) return FSEQ_OK;                                   // (no slab: the host joiner)
		G = (uint32_t) g;
		if (c->tune.debug) fprintf(stderr, "[fseq] bipartite join, wide form: %u pairs on %u slabs of %zu bytes\n", pairs, G, slab);
	}
	std::vector<uint64_t> rbs(S);
	for (size_t i = 0; i < S; ++i) rbs[i] = c->segments[i].rb;
	hipError_t e = hipMemcpyAsync(d_rb, rbs.data(), S * 8, hipMemcpyHostToDevice, st);
	if (e == hipSuccess) e = hipMemsetAsync(d_rep, 0, S * X * 4, st);
	if (e == hipSuccess) e = allow_lds(k_bip_texts_wide, lds_texts);
	if (e == hipSuccess) e = allow_lds(k_bip_match_wide, lds_match);
	if (e != hipSuccess) return fail(c, FSEQ_E_HIP, "bipartite join preparation", e);
	hipLaunchKernelGGL(k_join_classes_wide, dim3((uint32_t) S), dim3(JW_T), 0, st, c->d_snap_a, c->d_snap_d, d_rb, (uint32_t) m, X, d_of, d_rep, d_size, d_count, d_start);
	hipLaunchKernelGGL(k_bip_minrow_wide, dim3((uint32_t) S), dim3(JBW_T), 0, st, d_of, (uint32_t) m, X, d_min);
	hipLaunchKernelGGL(k_bip_texts_wide, dim3((uint32_t) S), dim3(JBW_T), lds_texts, st, d_count, d_size, d_min, (uint32_t) m, X, d_tpos, d_src, d_reprow);
	if (pairs)
		hipLaunchKernelGGL(k_bip_match_wide, dim3(G), dim3(JBW_T), lds_match, st, d_of, d_count, d_tpos, d_src, (uint32_t) m, X, pairs, d_slabs, d_match);
	hipLaunchKernelGGL(k_bip_chain_wide, dim3((X + JBW_T - 1) / JBW_T), dim3(JBW_T), 0, st, d_match, d_reprow, (uint32_t) S, X, d_perm);
	std::vector<uint32_t> count(S);
	e = hipMemcpyAsync(count.data(), d_count, S * 4, hipMemcpyDeviceToHost, st);
	if (e == hipSuccess) e = hipMemcpyAsync(permutations, d_perm, S * X * 4, hipMemcpyDeviceToHost, st);
	if (e == hipSuccess) e = hipStreamSynchronize(st);
	if (e == hipSuccess) e = hipGetLastError();
	if (e != hipSuccess) return fail(c, FSEQ_E_HIP, "bipartite join", e);
	for (size_t i = 0; i < S; ++i)
		if (count[i] < 1 || count[i] > X) return FSEQ_OK;         // (implausible class tables: the host joiner builds its own)
	double const t1 = now_ms();
	c->jp = fseq_join_profile{0.0, 0.0, 0.0, t1 - t0, t1 - t0, (uint64_t) S * X * 4ull + (uint64_t) S * 4ull};
	*done = true;
	return FSEQ_OK;
}

// lb of a merged segment = rb of the one in front: what k_join_classes(_wide) goes by
static bool segments_tile(fseq_ctx const *c)
{
	for (size_t i = 0; i < c->segments.size(); ++i)
		if (c->segments[i].lb != (i ? c->segments[i - 1].rb : 0u)) return false;
	return true;
}

// The class tables of every merged segment (k_join_classes_wide) for the callers that need nothing else of the boundary
// states: fseq_join_random's device front and fseq_write_segments_device.  Temporaries of one call.
struct ClassTables {
	size_t S = 0, m = 0;
	uint32_t X = 0;
	DevTemp<uint16_t> d_of;
	DevTemp<uint32_t> d_rep, d_size, d_count, d_start;
	DevTemp<uint64_t> d_lb, d_rb;
	explicit ClassTables(fseq_ctx *c) : d_of(c), d_rep(c), d_size(c), d_count(c), d_start(c), d_lb(c), d_rb(c) {}
	int alloc(size_t S_, size_t m_, uint32_t X_)
	{
		S = S_; m = m_; X = X_;
		int rc;
		if ((rc = d_of.alloc(S * m)) || (rc = d_rep.alloc(S * X)) || (rc = d_size.alloc(S * X)) || (rc = d_count.alloc(S)) ||
		    (rc = d_start.alloc(S * ((size_t) X + 1))) || (rc = d_lb.alloc(S)) || (rc = d_rb.alloc(S)))
			return rc;
		return FSEQ_OK;
	}
	// count: the classes of every segment, on the host; *sane: every one of them in [1, X]
	int run(fseq_ctx *c, std::vector<uint32_t> &count, bool *sane)
	{
		hipStream_t st = c->stream;
		std::vector<uint64_t> b(2 * S);
		for (size_t i = 0; i < S; ++i) { b[i] = c->segments[i].lb; b[S + i] = c->segments[i].rb; }
		hipError_t e = hipMemcpyAsync(d_lb, b.data(), S * 8, hipMemcpyHostToDevice, st);
		if (e == hipSuccess) e = hipMemcpyAsync(d_rb, b.data() + S, S * 8, hipMemcpyHostToDevice, st);
		if (e == hipSuccess) e = hipMemsetAsync(d_rep, 0, S * X * 4, st);
		if (e != hipSuccess) return fail(c, FSEQ_E_HIP, "class tables", e);
		hipLaunchKernelGGL(k_join_classes_wide, dim3((uint32_t) S), dim3(JW_T), 0, st, c->d_snap_a, c->d_snap_d, d_rb, (uint32_t) m, X, d_of, d_rep, d_size, d_count, d_start);
		count.resize(S);
		e = hipMemcpyAsync(count.data(), d_count, S * 4, hipMemcpyDeviceToHost, st);
		if (e == hipSuccess) e = hipStreamSynchronize(st);           // (b and count are read and written to here)
		if (e == hipSuccess) e = hipGetLastError();
		if (e != hipSuccess) return fail(c, FSEQ_E_HIP, "class tables", e);
		*sane = true;
		for (size_t i = 0; *sane && i < S; ++i) *sane = count[i] >= 1 && count[i] <= X;
		return FSEQ_OK;
	}
	void release() { d_of.release(d_of.c); d_rep.release(d_rep.c); d_size.release(d_size.c); d_count.release(d_count.c); d_start.release(d_start.c); d_lb.release(d_lb.c); d_rb.release(d_rb.c); }
};

// a junction's record as k_join_score leaves it (JS_FIELDS words)
static JoinScoreJunction junction_from_words(uint32_t const *w)
{
	JoinScoreJunction j;
	j.supported = w[0]; j.unsupported = w[1]; j.gaps = w[2]; j.rows_through = w[3];
	j.weight = (uint64_t) w[5] << 32 | w[4];
	return j;
}

// what the three entries of the join score hand back: the junctions with their borders rb[p], the breaks, the summary
static void join_score_outputs(uint32_t m, uint32_t X, uint64_t S, uint64_t const *rb, std::vector<JoinScoreJunction> const &J, uint32_t const *br,
                               double ms, fseq_join_score_entry *junctions, uint32_t *breaks, fseq_join_score_summary *summary)
{
	uint64_t const pairs = S - 1;
	for (uint64_t p = 0; junctions && p < pairs; ++p)
		junctions[p] = fseq_join_score_entry{rb[p], J[p].weight, J[p].supported, J[p].unsupported, J[p].gaps, J[p].rows_through};
	if (breaks) std::copy(br, br + X, breaks);
	if (summary)
	{
		JoinScoreTotals const t = join_score_totals(m, X, pairs, J.data(), br);
		*summary = fseq_join_score_summary{t.junctions, t.supported, t.unsupported, t.gaps, t.rows_through, t.weight, t.min_junction,
		                                   t.min_rows_through, t.max_breaks, ms};
	}
}

// The device form of fseq_join_score (fseq_joinscore.hpp): J [S - 1], breaks [X], support [(S - 1) x X] or nullptr.
// *done = false with FSEQ_OK: the caller goes on to the host form (a failed device allocation, implausible class counts),
// with the error text cleared.
static int join_score_device(fseq_ctx *c, uint32_t const *permutations, std::vector<JoinScoreJunction> &J, uint32_t *breaks, uint32_t *support, bool *done)
{
	*done = false;
	hipStream_t st = c->stream;
	size_t const m = c->p.m, S = c->segments.size(), pairs = S - 1;
	uint32_t const X = c->res.max_segment_size;
	ClassTables T(c);
	DevTemp<uint32_t> d_perm(c), d_junc(c), d_sup(c), d_breaks(c);
	auto no_room = [&](int rc) { if (rc == FSEQ_E_OOM) { c->err.clear(); return (int) FSEQ_OK; } return rc; };      // (the host form needs no device memory)
	int rc;
	if ((rc = T.alloc(S, m, X)) || (rc = d_perm.alloc(S * X)) || (rc = d_junc.alloc(pairs * JS_FIELDS)) || (rc = d_sup.alloc(pairs * X)) || (rc = d_breaks.alloc(X)))
		return no_room(rc);
	std::vector<uint32_t> count;
	bool sane = false;
	if ((rc = T.run(c, count, &sane))) return rc;
	if (!sane) return FSEQ_OK;                                 // (the host form builds its own classes from the boundary states)
	JoinScoreArgs A{};
	A.of_row = T.d_of; A.perm = d_perm; A.m = (uint32_t) m; A.X = X; A.S = (uint32_t) S; A.junctions = d_junc; A.support = d_sup;
	std::vector<uint32_t> words(pairs * JS_FIELDS);
	hipError_t e = hipMemcpyAsync(d_perm, permutations, S * X * 4, hipMemcpyHostToDevice, st);
	if (e == hipSuccess) e = launch_join_score(st, A, d_breaks);
	if (e == hipSuccess) e = hipMemcpyAsync(words.data(), d_junc, words.size() * 4, hipMemcpyDeviceToHost, st);
	if (e == hipSuccess) e = hipMemcpyAsync(breaks, d_breaks, (size_t) X * 4, hipMemcpyDeviceToHost, st);
	if (e == hipSuccess && support) e = hipMemcpyAsync(support, d_sup, pairs * X * 4, hipMemcpyDeviceToHost, st);
	hipError_t const es = hipStreamSynchronize(st);             // (the host arrays are read and written to here, whatever was queued)
	if (e == hipSuccess) e = es;
	if (e == hipSuccess) e = hipGetLastError();
	if (e != hipSuccess) return fail(c, FSEQ_E_HIP, "join score", e);
	for (size_t p = 0; p < pairs; ++p) J[p] = junction_from_words(words.data() + p * JS_FIELDS);
	*done = true;
	return FSEQ_OK;
}

static char const SEGFILE_HEADER_BIP[] = "SEGMENT\tLB\tRB\tSIZE\tSUBSEQUENCE\tSEQUENCES\tCOPIED_FROM\n";
static char const SEGFILE_HEADER_COPIES[] = "SEGMENT\tLB\tRB\tSIZE\tSUBSEQUENCE_NUMBER\tCOPY_NUMBER\tSUBSEQUENCE\n";
static constexpr uint64_t SEGFILE_BATCH_BYTES = 256ull << 20;      // (what fseq_write_founders_device takes a batch)

// What the restored form of the writer takes on top: the segments in the source's co-ordinates (host, [S] each) and the identity
// state of the context (device).  nullptr: the reduced form.
struct SegFileRestored {
	uint64_t const *src_lb, *src_rb;
	uint32_t const *kept;
	uint8_t const *mask, *ref;
	uint64_t n_src;
};

// The merged segments of an identity-reduced context in the source's co-ordinates (restored_segment_bounds on the kept columns,
// which are copied to the host: 4 bytes a kept column).  Refuses what the pure function refuses.
int fseq::restored_bounds_of(fseq_ctx *c, std::vector<uint64_t> &src_lb, std::vector<uint64_t> &src_rb)
{
	size_t const S = c->segments.size();
	std::vector<uint32_t> kept;
	std::vector<uint64_t> lb, rb;
	try { kept.resize((size_t) c->p.n); lb.resize(S); rb.resize(S); src_lb.resize(S); src_rb.resize(S); }
	catch (std::bad_alloc const &) { return fail(c, FSEQ_E_OOM, "restored segments: the kept columns on the host"); }
	(void) hipSetDevice(c->p.device);
	HIP_TRY(c, hipMemcpy(kept.data(), c->idn.kept, kept.size() * 4, hipMemcpyDeviceToHost));
	for (size_t s = 0; s < S; ++s) { lb[s] = c->segments[s].lb; rb[s] = c->segments[s].rb; }
	if (char const *why = restored_segment_bounds(kept.data(), (uint64_t) kept.size(), c->idn.n_src, lb.data(), rb.data(), (uint64_t) S, src_lb.data(), src_rb.data()))
	{
		std::string const what = std::string("restored segments: ") + why;
		return fail(c, FSEQ_E_UNSUPPORTED, what.c_str());
	}
	return FSEQ_OK;
}

// The lines of the segments file behind its header, from the device (fseq_segfile.hpp).  The file is opened once everything that
// can refuse has passed: the class counts, the allocations of the tables.  R: the bounds a line prints and the identity columns its
// substring gains (fseq_write_segments_restored); nullptr: the context's own co-ordinates.
static int write_segments_device_lines(fseq_ctx *c, bool const bip, char const *path, char const *header, SegFileRestored const *R)
{
	(void) hipSetDevice(c->p.device);
	hipStream_t st = c->stream;
	size_t const m = c->p.m, S = c->segments.size();
	uint32_t const X = c->res.max_segment_size;
	size_t const X1 = (size_t) X + 1;
	ClassTables T(c);
	DevTemp<uint16_t> d_tpos(c), d_src(c);
	DevTemp<uint32_t> d_min(c), d_reprow(c), d_members(c);
	DevTemp<uint2> d_rline(c);
	DevTemp<uint8_t> d_pool(c), d_lut(c), d_out(c);
	DevTemp<uint64_t> d_ppos(c), d_loff(c), d_segoff(c), d_srcb(c);
	int rc;
	if ((rc = T.alloc(S, m, X))) return rc;
	if (R && (rc = d_srcb.alloc(2 * S))) return rc;
	if (bip && ((rc = d_tpos.alloc(S * X)) || (rc = d_src.alloc(S * X)) || (rc = d_min.alloc(S * X)) || (rc = d_reprow.alloc(S * X)))) return rc;
	if ((rc = d_ppos.alloc(S + 1)) || (rc = d_loff.alloc(S * X1)) || (rc = d_segoff.alloc(S + 1)) || (rc = d_lut.alloc(256))) return rc;
	std::vector<uint32_t> count;
	bool sane = false;
	if ((rc = T.run(c, count, &sane))) return rc;
	if (!sane) return fail(c, FSEQ_E_UNSUPPORTED, "the class tables of the device hold a class count outside [1, max_segment_size] (write the segments from host rows: fseq_write_segments)");
	hipError_t e = hipSuccess;
	if (bip)
	{
		size_t const lds_texts = bip_texts_wide_lds_bytes(X);
		e = allow_lds(k_bip_texts_wide, lds_texts);
		if (e != hipSuccess) return fail(c, FSEQ_E_HIP, "segments file preparation", e);
		hipLaunchKernelGGL(k_bip_minrow_wide, dim3((uint32_t) S), dim3(JBW_T), 0, st, T.d_of, (uint32_t) m, X, d_min);
		hipLaunchKernelGGL(k_bip_texts_wide, dim3((uint32_t) S), dim3(JBW_T), lds_texts, st, T.d_count, T.d_size, d_min, (uint32_t) m, X, d_tpos, d_src, d_reprow);
	}
	else
	{
		// the lines of a segment in the order prepare_copy_numbers(..., false) leaves them: the host's own std::sort on the
		// vector the host writer sorts, built from the device's tables
		std::vector<uint32_t> rep(S * X), size(S * X);
		e = hipMemcpyAsync(rep.data(), T.d_rep, S * X * 4, hipMemcpyDeviceToHost, st);
		if (e == hipSuccess) e = hipMemcpyAsync(size.data(), T.d_size, S * X * 4, hipMemcpyDeviceToHost, st);
		if (e == hipSuccess) e = hipStreamSynchronize(st);
		if (e != hipSuccess) return fail(c, FSEQ_E_HIP, "segments file preparation", e);
		release_all(c, T.d_of, T.d_rep, T.d_size, T.d_start);      // (the random file needs the counts only from here on)
		std::vector<uint2> rline(S * X, make_uint2(0u, 0u));
		for (size_t s = 0; s < S; ++s)
		{
			auto const cn = copy_numbers_from_runs(runs_from_classes(count[s], rep.data() + s * X, size.data() + s * X), X, false);
			uint32_t prev = 0;
			for (size_t j = 0; j < cn.size(); ++j) { rline[s * X + j] = make_uint2(cn[j].substring_idx, cn[j].copy_number - prev); prev = cn[j].copy_number; }
		}
		if ((rc = d_rline.alloc(S * X))) return rc;
		HIP_TRY(c, hipMemcpy(d_rline, rline.data(), S * X * sizeof(uint2), hipMemcpyHostToDevice));
	}
	// the prefixes: write_segments_impl's "%zu\t%llu\t%llu\t%u\t" (restored: with the source's bounds)
	std::string pool;
	std::vector<uint64_t> ppos(S + 1);
	for (size_t s = 0; s < S; ++s)
	{
		char buf[96];
		ppos[s] = pool.size();
		uint64_t const plb = R ? R->src_lb[s] : c->segments[s].lb, prb = R ? R->src_rb[s] : c->segments[s].rb;
		int const len = snprintf(buf, sizeof(buf), "%zu\t%llu\t%llu\t%u\t", s, (unsigned long long) plb, (unsigned long long) prb, c->segments[s].segment_size);
		pool.append(buf, (size_t) len);
	}
	ppos[S] = pool.size();
	if ((rc = d_pool.alloc(pool.size()))) return rc;
	e = hipMemcpyAsync(d_pool, pool.data(), pool.size(), hipMemcpyHostToDevice, st);
	if (e == hipSuccess) e = hipMemcpyAsync(d_ppos, ppos.data(), (S + 1) * 8, hipMemcpyHostToDevice, st);
	if (e == hipSuccess) e = hipMemcpyAsync(d_lut, c->code_to_byte, 256, hipMemcpyHostToDevice, st);
	if (e == hipSuccess && R) e = hipMemcpyAsync(d_srcb, R->src_lb, S * 8, hipMemcpyHostToDevice, st);
	if (e == hipSuccess && R) e = hipMemcpyAsync(d_srcb + S, R->src_rb, S * 8, hipMemcpyHostToDevice, st);
	size_t const lds_lines = segfile_lines_lds_bytes(X, bip), lds_members = segfile_members_lds_bytes(X), lds_write = segfile_write_lds_bytes(X, bip);
	if (e == hipSuccess && bip) e = R ? allow_lds(k_segfile_lines<true, true>, lds_lines) : allow_lds(k_segfile_lines<true>, lds_lines);
	if (e == hipSuccess && bip) e = allow_lds(k_segfile_members, lds_members);
	if (e == hipSuccess && bip) e = R ? allow_lds(k_segfile_write<true, true>, lds_write) : allow_lds(k_segfile_write<true>, lds_write);
	if (e != hipSuccess) return fail(c, FSEQ_E_HIP, "segments file preparation", e);
	SegFileArgs A{};
	A.seg_lb = T.d_lb; A.seg_rb = T.d_rb; A.pool = d_pool; A.ppos = d_ppos; A.count = T.d_count;
	A.m = (uint32_t) m; A.X = X; A.S = (uint32_t) S;
	A.of_row = T.d_of; A.tpos = d_tpos; A.src = d_src; A.reprow = d_reprow; A.rline = d_rline;
	if (R) { A.src_lb = d_srcb; A.src_rb = d_srcb + S; A.kept = R->kept; A.mask = R->mask; A.ref = R->ref; A.n_src = R->n_src; }
	// every line's length, scanned: inside the segments, then over them
	if (bip && R) hipLaunchKernelGGL((k_segfile_lines<true, true>), dim3((uint32_t) S), dim3(SF_T), lds_lines, st, A, (uint64_t *) d_loff);
	else if (bip) hipLaunchKernelGGL(k_segfile_lines<true>, dim3((uint32_t) S), dim3(SF_T), lds_lines, st, A, (uint64_t *) d_loff);
	else if (R) hipLaunchKernelGGL((k_segfile_lines<false, true>), dim3((uint32_t) S), dim3(SF_T), 0, st, A, (uint64_t *) d_loff);
	else hipLaunchKernelGGL(k_segfile_lines<false>, dim3((uint32_t) S), dim3(SF_T), 0, st, A, (uint64_t *) d_loff);
	hipLaunchKernelGGL(k_segfile_scan, dim3(1), dim3(SF_T), 0, st, d_loff, (uint32_t) S, X, d_segoff);
	std::vector<uint64_t> loff, segoff(S + 1);
	try { loff.resize(S * X1); } catch (std::bad_alloc const &) { (void) hipStreamSynchronize(st); return fail(c, FSEQ_E_OOM, "segments file: the line offsets on the host"); }
	e = hipMemcpyAsync(loff.data(), d_loff, S * X1 * 8, hipMemcpyDeviceToHost, st);
	if (e == hipSuccess) e = hipMemcpyAsync(segoff.data(), d_segoff, (S + 1) * 8, hipMemcpyDeviceToHost, st);
	if (e == hipSuccess) e = hipStreamSynchronize(st);
	if (e == hipSuccess) e = hipGetLastError();
	if (e != hipSuccess) return fail(c, FSEQ_E_HIP, "segments file: line lengths", e);
	// batches of whole lines in file order, FSEQ_SEGFILE_BATCH bytes at most; a line above the budget is a batch of its own
	uint64_t const budget = c->tune.segfile_batch > 0 ? (uint64_t) c->tune.segfile_batch : SEGFILE_BATCH_BYTES;
	std::vector<SegFileBatch> batches;
	uint64_t longest = 0, lines = 0, most_bytes = 0, most_segs = 0;
	{
		SegFileBatch cur{};
		bool open = false;
		auto close = [&]() {
			batches.push_back(cur);
			most_bytes = std::max(most_bytes, cur.bytes);
			most_segs = std::max<uint64_t>(most_segs, cur.s1 - cur.s0 + 1);
			open = false;
		};
		for (size_t s = 0; s < S; ++s)
		{
			uint64_t const *lo = loff.data() + s * X1;
			uint32_t const nl = bip ? X : count[s];
			for (uint32_t j = 0; j < nl; ++j)
			{
				uint64_t const len = lo[j + 1] - lo[j];
				if (open && cur.bytes + len > budget) close();
				if (!open) { cur = SegFileBatch{(uint32_t) s, (uint32_t) s, j, j, segoff[s] + lo[j], 0}; open = true; }
				cur.s1 = (uint32_t) s; cur.j_hi = j + 1; cur.bytes += len;
				longest = std::max(longest, len);
				++lines;
			}
		}
		if (open) close();
	}
	if ((rc = d_out.alloc((size_t) most_bytes))) return rc;
	if (bip && (rc = d_members.alloc((size_t) most_segs * m))) return rc;
	uint8_t *h_out = nullptr;
	if (hipHostMalloc(reinterpret_cast<void **>(&h_out), std::max<size_t>((size_t) most_bytes, 1), hipHostMallocDefault) != hipSuccess)
	{
		(void) hipGetLastError();
		return fail(c, FSEQ_E_OOM, "segments output buffer");
	}
	FILE *f = (path && strcmp(path, "-") != 0) ? fopen(path, "wb") : stdout;
	if (!f) { (void) hipHostFree(h_out); return fail(c, FSEQ_E_ARG, "cannot open the segments output file"); }
	bool ok = fputs(header, f) >= 0, hip_ok = true;
	for (size_t b = 0; b < batches.size() && ok && hip_ok; ++b)
	{
		SegFileBatch const &B = batches[b];
		uint32_t const nseg = B.s1 - B.s0 + 1;
		if (bip)
		{
			hipLaunchKernelGGL(k_segfile_members, dim3(nseg), dim3(SF_T), lds_members, st, A, (uint32_t const *) T.d_size, B.s0, (uint32_t *) d_members);
			if (R)
				hipLaunchKernelGGL((k_segfile_write<true, true>), dim3(nseg), dim3(SF_T), lds_write, st, A, B, (uint8_t const *) c->d_msa, c->ld, c->bsh, (uint8_t const *) d_lut,
				                   (uint64_t const *) d_loff, (uint64_t const *) d_segoff, (uint32_t const *) d_members, (uint8_t *) d_out);
			else
				hipLaunchKernelGGL(k_segfile_write<true>, dim3(nseg), dim3(SF_T), lds_write, st, A, B, (uint8_t const *) c->d_msa, c->ld, c->bsh, (uint8_t const *) d_lut,
				                   (uint64_t const *) d_loff, (uint64_t const *) d_segoff, (uint32_t const *) d_members, (uint8_t *) d_out);
		}
		else if (R)
			hipLaunchKernelGGL((k_segfile_write<false, true>), dim3(nseg), dim3(SF_T), 0, st, A, B, (uint8_t const *) c->d_msa, c->ld, c->bsh, (uint8_t const *) d_lut,
			                   (uint64_t const *) d_loff, (uint64_t const *) d_segoff, (uint32_t const *) nullptr, (uint8_t *) d_out);
		else
			hipLaunchKernelGGL(k_segfile_write<false>, dim3(nseg), dim3(SF_T), 0, st, A, B, (uint8_t const *) c->d_msa, c->ld, c->bsh, (uint8_t const *) d_lut,
			                   (uint64_t const *) d_loff, (uint64_t const *) d_segoff, (uint32_t const *) nullptr, (uint8_t *) d_out);
		hip_ok = hipMemcpyAsync(h_out, d_out, (size_t) B.bytes, hipMemcpyDeviceToHost, st) == hipSuccess && hipStreamSynchronize(st) == hipSuccess && hipGetLastError() == hipSuccess;
		if (hip_ok) ok = fwrite(h_out, 1, (size_t) B.bytes, f) == (size_t) B.bytes;
	}
	if (fflush(f) != 0) ok = false;
	if (f != stdout) fclose(f);
	(void) hipHostFree(h_out);
	if (!hip_ok) return fail(c, FSEQ_E_HIP, "writing the segments from the device failed");
	if (!ok) return fail(c, FSEQ_E_ARG, "writing the segments output file failed");
	uint64_t const hl = strlen(header);
	c->segfile = fseq_ctx::SegFileStats{true, (uint64_t) batches.size(), hl + segoff[S], std::max(hl, longest), lines + 1};
	return FSEQ_OK;
}

extern "C" {

int fseq_get_join_profile(fseq_ctx const *c, fseq_join_profile *out)
{
	if (!c || !out) return FSEQ_E_ARG;
	*out = c->jp;
	return FSEQ_OK;
}

int fseq_join_greedy(fseq_ctx *c, uint32_t *permutations)
{
	if (!c || !permutations) return FSEQ_E_ARG;
	if (int const rc = need_result(c)) return rc;
	if (c->segments.empty()) return fail(c, FSEQ_E_ARG, "no segments to join (segmentation failed or was not run)");
	if (c->sh.on) return fail(c, FSEQ_E_UNSUPPORTED, "sharded run: collect the boundary states (fseq_boundary_state on their owners) and use fseq_greedy_match_host");
	(void) hipSetDevice(c->p.device);
	size_t const m = c->p.m, S = c->segments.size();
	double const t0 = now_ms();
	uint32_t const X = c->res.max_segment_size;
	// The wide front: forced (FSEQ_JOIN_WIDE) at any X; by itself above the LDS front's limit, from JOIN_WIDE_MIN_BYTES of
	// boundary states on.  Falls through to the all-host joiner as the LDS front does.
	bool const wide = !c->tune.join_host && X >= 1 && X <= 0xFFFFu && m <= 0xFFFFFFFFull && S <= 0x7FFFFFFFull &&
	                  (c->tune.join_wide || (X > JP_MAX_CLASSES && (uint64_t) S * m * 8ull >= JOIN_WIDE_MIN_BYTES));
	if (wide)
	{
		bool done = false;
		if (int const rc = join_greedy_wide(c, permutations, t0, &done)) return rc;
		if (done) { c->join_path = 2; return FSEQ_OK; }
	}
	// class tables and co-occurrence edges where the boundary states are (fseq_joinprep.hpp); the host hands out
	// the copies and draws the edges (the serial part of greedy_matcher.cc).  Falls through to the all-host joiner
	// below when the edge array cannot be allocated or the tables come back implausible.
	while (!wide && X <= JP_MAX_CLASSES && m <= 0xFFFFFFFFull && !c->tune.join_host)
	{
		hipStream_t st = c->stream;
		// (temporaries: released on every way out of the loop's body)
		DevTemp<uint16_t> d_of(c);
		DevTemp<uint32_t> d_rep(c), d_size(c), d_count(c), d_off(c), d_ne(c);
		DevTemp<uint64_t> d_rb(c);
		DevTemp<uint2> d_edges(c);
		DevTemp<unsigned long long> d_cursor(c);
		// (offsets into the edge array are 32-bit words on the way to the host: the capacity stays below 2^32)
		uint64_t const cap_total = std::min<uint64_t>((uint64_t) (S > 1 ? S - 1 : 0) * std::min<uint64_t>(m, (uint64_t) X * X) + 1, 0xFFFFFFFFull);
		int rc;
		if ((rc = d_of.alloc(S * m)) || (rc = d_rep.alloc(S * X)) || (rc = d_size.alloc(S * X)) || (rc = d_count.alloc(S)) ||
		    (rc = d_off.alloc(S)) || (rc = d_ne.alloc(S)) || (rc = d_rb.alloc(S)) || (rc = d_edges.alloc(cap_total)) ||
		    (rc = d_cursor.alloc(1)))
		{
			if (rc == FSEQ_E_OOM) { c->err.clear(); break; }       // no room for the device front: the host joiner needs none
			return rc;
		}
		std::vector<uint64_t> rbs(S);
		for (size_t i = 0; i < S; ++i) rbs[i] = c->segments[i].rb;
		hipError_t e = hipMemcpyAsync(d_rb, rbs.data(), S * 8, hipMemcpyHostToDevice, st);
		if (e == hipSuccess) e = hipMemsetAsync(d_cursor, 0, 8, st);
		if (e == hipSuccess) e = hipMemsetAsync(d_rep, 0, S * X * 4, st);
		size_t const lds = (size_t) X * X * 4;
		if (e == hipSuccess) e = allow_lds(k_join_edges, lds);
		if (e != hipSuccess) return fail(c, FSEQ_E_HIP, "join preparation", e);
		hipLaunchKernelGGL(k_join_classes, dim3((uint32_t) S), dim3(JP_T), 0, st, c->d_snap_a, c->d_snap_d, d_rb, (uint32_t) m, X, d_of, d_rep, d_size, d_count);
		if (S > 1)
			hipLaunchKernelGGL(k_join_edges, dim3((uint32_t) (S - 1)), dim3(JP_T), lds, st, d_of, d_count, (uint32_t) m, X, d_edges, cap_total, d_off, d_ne, d_cursor);
		std::vector<uint32_t> count(S), rep(S * X), size(S * X), off(S), ne(S);
		unsigned long long total = 0;
		e = hipMemcpyAsync(count.data(), d_count, S * 4, hipMemcpyDeviceToHost, st);
		if (e == hipSuccess) e = hipMemcpyAsync(rep.data(), d_rep, S * X * 4, hipMemcpyDeviceToHost, st);
		if (e == hipSuccess) e = hipMemcpyAsync(size.data(), d_size, S * X * 4, hipMemcpyDeviceToHost, st);
		if (e == hipSuccess && S > 1) e = hipMemcpyAsync(off.data(), d_off, (S - 1) * 4, hipMemcpyDeviceToHost, st);
		if (e == hipSuccess && S > 1) e = hipMemcpyAsync(ne.data(), d_ne, (S - 1) * 4, hipMemcpyDeviceToHost, st);
		if (e == hipSuccess) e = hipMemcpyAsync(&total, d_cursor, 8, hipMemcpyDeviceToHost, st);
		if (e == hipSuccess) e = hipStreamSynchronize(st);
		if (e == hipSuccess) e = hipGetLastError();
		bool sane = e == hipSuccess && total < cap_total && total <= 0xFFFFFFFFull;
		for (size_t i = 0; sane && i < S; ++i) sane = count[i] >= 1 && count[i] <= X;
		std::vector<uint32_t> edge_words(sane ? 2 * (size_t) total + 2 : 2);
		if (sane && total) e = hipMemcpy(edge_words.data(), d_edges, (size_t) total * 8, hipMemcpyDeviceToHost);
		release_all(c, d_of, d_rep, d_size, d_count, d_off, d_ne, d_rb, d_edges, d_cursor);      // (not held through the host's part)
		if (e != hipSuccess) return fail(c, FSEQ_E_HIP, "join preparation", e);
		if (!sane) break;                                         // (the host joiner builds its own tables from the boundary states)
		double const t1 = now_ms();
		JoinProfile prof;
		greedy_match_prepared(c->p.m, X, S, count.data(), rep.data(), size.data(), edge_words.data(), off.data(), ne.data(), permutations, &prof);
		c->jp = fseq_join_profile{t1 - t0, prof.ms_classes, prof.ms_edges, prof.ms_draw, now_ms() - t0,
		                          (uint64_t) S * (2ull * X + 3) * 4 + (uint64_t) total * 8};
		c->join_path = 1;
		return FSEQ_OK;
	}
	std::vector<uint32_t> A(S * m), D(S * m);
	HIP_TRY(c, hipMemcpy(A.data(), c->d_snap_a, S * m * 4, hipMemcpyDeviceToHost));
	HIP_TRY(c, hipMemcpy(D.data(), c->d_snap_d, S * m * 4, hipMemcpyDeviceToHost));
	double const t1 = now_ms();
	std::vector<JoinSegment> segs(S);
	for (size_t i = 0; i < S; ++i) { segs[i].lb = c->segments[i].lb; segs[i].rb = c->segments[i].rb; }
	JoinProfile prof;
	greedy_match(c->p.m, c->res.max_segment_size, segs, A.data(), D.data(), permutations, &prof);
	c->jp = fseq_join_profile{t1 - t0, prof.ms_classes, prof.ms_edges, prof.ms_draw, now_ms() - t0, (uint64_t) S * m * 8ull};
	c->join_path = 0;
	return FSEQ_OK;
}

int fseq_debug_join_path(fseq_ctx *c, int *path)
{
	if (!c || !path) return FSEQ_E_ARG;
	if (c->join_path < 0) return fail(c, FSEQ_E_ARG, "no fseq_join_greedy has finished on this context");
	*path = c->join_path;
	return FSEQ_OK;
}

// boundary states of all merged segments on the host (what join_context reads from the pbwt samples)
static int fetch_boundary_states(fseq_ctx *c, std::vector<uint32_t> &A, std::vector<uint32_t> &D, std::vector<JoinSegment> &segs)
{
	if (int const rc = need_result(c)) return rc;
	if (c->segments.empty()) return fail(c, FSEQ_E_ARG, "no segments to join (segmentation failed or was not run)");
	if (c->sh.on) return fail(c, FSEQ_E_UNSUPPORTED, "sharded run: collect the boundary states (fseq_boundary_state on their owners) and use the *_match_host entry points");
	(void) hipSetDevice(c->p.device);
	size_t const m = c->p.m, S = c->segments.size();
	double const t0 = now_ms();
	A.resize(S * m); D.resize(S * m);
	HIP_TRY(c, hipMemcpy(A.data(), c->d_snap_a, S * m * 4, hipMemcpyDeviceToHost));
	HIP_TRY(c, hipMemcpy(D.data(), c->d_snap_d, S * m * 4, hipMemcpyDeviceToHost));
	c->jp = fseq_join_profile{now_ms() - t0, 0, 0, 0, 0, (uint64_t) S * m * 8ull};
	segs.resize(S);
	for (size_t i = 0; i < S; ++i) { segs[i].lb = c->segments[i].lb; segs[i].rb = c->segments[i].rb; }
	return FSEQ_OK;
}

int fseq_debug_bipartite_path(fseq_ctx *c, int *path)
{
	if (!c || !path) return FSEQ_E_ARG;
	if (c->bip_path < 0) return fail(c, FSEQ_E_ARG, "no fseq_join_bipartite has finished on this context since its input was set");
	*path = c->bip_path;
	return FSEQ_OK;
}

int fseq_join_bipartite(fseq_ctx *c, uint32_t *permutations)
{
	if (!c || !permutations) return FSEQ_E_ARG;
	if (int const rc = need_result(c)) return rc;
	if (c->segments.empty()) return fail(c, FSEQ_E_ARG, "no segments to join (segmentation failed or was not run)");
	size_t const m = c->p.m, S = c->segments.size();
	uint32_t const X = c->res.max_segment_size;
	// [r5] texts, intersection weights, the matchings and their chaining where the boundary states are (fseq_joinbip.hpp);
	// falls through to the host joiner when the tables do not fit a workgroup's LDS or cannot be allocated
	bool tiled = true;                                           // (lb of a segment = rb of the one in front: what k_join_classes goes by)
	for (size_t i = 0; tiled && i < S; ++i) tiled = c->segments[i].lb == (i ? c->segments[i - 1].rb : 0u);
	bool const device = tiled && !c->sh.on && X >= 1 && m <= 0xFFFFFFFFull && S <= 0xFFFFFFFFull && !c->tune.join_host;
	// The wide form (fseq_joinbipw.hpp): forced (FSEQ_JOIN_BIP_WIDE) at any X up to its cap; by itself above the LDS form's
	// limit, from JOIN_BIP_WIDE_MIN_BYTES of boundary states on.  Falls through to the host joiner as the LDS form does.
	bool const wide = device && X <= JBW_MAX_TEXTS &&
	                  (c->tune.join_bip_wide || (X > JP_MAX_CLASSES && (uint64_t) S * m * 8ull >= JOIN_BIP_WIDE_MIN_BYTES));
	if (wide)
	{
		bool done = false;
		if (int const rc = join_bipartite_wide(c, permutations, &done)) return rc;
		if (done) { c->bip_path = 2; return FSEQ_OK; }
	}
	while (device && !wide && X <= JP_MAX_CLASSES)
	{
		(void) hipSetDevice(c->p.device);
		double const t0 = now_ms();
		hipStream_t st = c->stream;
		DevTemp<uint16_t> d_of(c), d_tpos(c), d_src(c), d_match(c);
		DevTemp<uint32_t> d_rep(c), d_size(c), d_count(c), d_min(c), d_reprow(c), d_perm(c);
		DevTemp<uint64_t> d_rb(c);
		int rc;
		if ((rc = d_of.alloc(S * m)) || (rc = d_tpos.alloc(S * X)) || (rc = d_src.alloc(S * X)) || (rc = d_match.alloc(S * X)) ||
		    (rc = d_rep.alloc(S * X)) || (rc = d_size.alloc(S * X)) || (rc = d_count.alloc(S)) || (rc = d_min.alloc(S * X)) ||
		    (rc = d_reprow.alloc(S * X)) || (rc = d_perm.alloc(S * X)) || (rc = d_rb.alloc(S)))
		{
			if (rc == FSEQ_E_OOM) { c->err.clear(); break; }
			return rc;
		}
		std::vector<uint64_t> rbs(S);
		for (size_t i = 0; i < S; ++i) rbs[i] = c->segments[i].rb;
		hipError_t e = hipMemcpyAsync(d_rb, rbs.data(), S * 8, hipMemcpyHostToDevice, st);
		size_t const lds_match = bip_match_lds_bytes(X), lds_chain = bip_chain_lds_bytes(X);
		if (e == hipSuccess) e = allow_lds(k_bip_match, lds_match);
		if (e == hipSuccess) e = allow_lds(k_bip_chain, lds_chain);
		if (e != hipSuccess) return fail(c, FSEQ_E_HIP, "bipartite join preparation", e);
		// (a segment's classes: the rows that agree on [lb, rb), lb = the segment in front's rb -- the merged segments tile the columns)
		hipLaunchKernelGGL(k_join_classes, dim3((uint32_t) S), dim3(JP_T), 0, st, c->d_snap_a, c->d_snap_d, d_rb, (uint32_t) m, X, d_of, d_rep, d_size, d_count);
		hipLaunchKernelGGL(k_bip_minrow, dim3((uint32_t) S), dim3(JP_T), 0, st, d_of, (uint32_t) m, X, d_min);
		hipLaunchKernelGGL(k_bip_texts, dim3((uint32_t) S), dim3(64), 0, st, d_count, d_size, d_min, (uint32_t) m, X, d_tpos, d_src, d_reprow);
		if (S > 1)
			hipLaunchKernelGGL(k_bip_match, dim3((uint32_t) (S - 1)), dim3(64), lds_match, st, d_of, d_count, d_tpos, d_src, (uint32_t) m, X, d_match, (long long *) nullptr);
		hipLaunchKernelGGL(k_bip_chain, dim3(1), dim3(JB_CHAIN_T), lds_chain, st, d_match, d_reprow, (uint32_t) S, X, d_perm);
		std::vector<uint32_t> count(S);
		e = hipMemcpyAsync(count.data(), d_count, S * 4, hipMemcpyDeviceToHost, st);
		if (e == hipSuccess) e = hipMemcpyAsync(permutations, d_perm, S * X * 4, hipMemcpyDeviceToHost, st);
		if (e == hipSuccess) e = hipStreamSynchronize(st);
		if (e == hipSuccess) e = hipGetLastError();
		if (e != hipSuccess) return fail(c, FSEQ_E_HIP, "bipartite join", e);
		bool sane = true;
		for (size_t i = 0; sane && i < S; ++i) sane = count[i] >= 1 && count[i] <= X;
		if (!sane) break;                                         // (implausible class tables: the host joiner builds its own)
		double const t1 = now_ms();
		c->jp = fseq_join_profile{0.0, 0.0, 0.0, t1 - t0, t1 - t0, (uint64_t) S * X * 4ull + (uint64_t) S * 4ull};
		c->bip_path = 1;
		return FSEQ_OK;
	}
	std::vector<uint32_t> A, D;
	std::vector<JoinSegment> segs;
	int const rc = fetch_boundary_states(c, A, D, segs);
	if (rc) return rc;
	double const t0 = now_ms();
	bipartite_match(c->p.m, c->res.max_segment_size, segs, A.data(), D.data(), permutations);
	c->jp.ms_draw = now_ms() - t0; c->jp.ms_total = c->jp.ms_d2h + c->jp.ms_draw;
	c->bip_path = 0;
	return FSEQ_OK;
}

int fseq_debug_random_path(fseq_ctx *c, int *path)
{
	if (!c || !path) return FSEQ_E_ARG;
	if (c->rand_path < 0) return fail(c, FSEQ_E_ARG, "no fseq_join_random has finished on this context since its input was set");
	*path = c->rand_path;
	return FSEQ_OK;
}

int fseq_join_random(fseq_ctx *c, uint32_t seed, uint32_t *permutations)
{
	if (!c || !permutations) return FSEQ_E_ARG;
	if (int const rc = need_result(c)) return rc;
	if (c->segments.empty()) return fail(c, FSEQ_E_ARG, "no segments to join (segmentation failed or was not run)");
	// the class tables where the boundary states are (k_join_classes_wide): the joiner reads nothing of a boundary state but
	// the classes' first rows and sizes, S x X x 8 + S x 4 bytes against S x m x 8.  No size threshold: the front moves at
	// most X / m of the bytes and runs one kernel.  Falls through to the host joiner as the other device fronts do.
	uint32_t const X = c->res.max_segment_size;
	if (segments_tile(c) && !c->sh.on && X >= 1 && X <= 0xFFFFu && c->p.m <= 0x7FFFFFFFull && c->segments.size() <= 0x7FFFFFFFull && !c->tune.join_host)
	{
		(void) hipSetDevice(c->p.device);
		double const t0 = now_ms();
		size_t const S = c->segments.size();
		ClassTables T(c);
		std::vector<uint32_t> count;
		bool sane = false;
		int rc = T.alloc(S, c->p.m, X);
		if (FSEQ_OK == rc) rc = T.run(c, count, &sane);
		if (rc && rc != FSEQ_E_OOM) return rc;
		if (FSEQ_E_OOM == rc) c->err.clear();                      // (the host joiner needs no device memory)
		else if (sane)
		{
			std::vector<uint32_t> rep(S * X), size(S * X);
			hipError_t e = hipMemcpyAsync(rep.data(), T.d_rep, S * X * 4, hipMemcpyDeviceToHost, c->stream);
			if (e == hipSuccess) e = hipMemcpyAsync(size.data(), T.d_size, S * X * 4, hipMemcpyDeviceToHost, c->stream);
			if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
			T.release();                                           // (not held through the host's part)
			if (e != hipSuccess) return fail(c, FSEQ_E_HIP, "random join preparation", e);
			double const t1 = now_ms();
			random_join_classes(X, S, count.data(), rep.data(), size.data(), seed, permutations);
			double const t2 = now_ms();
			c->jp = fseq_join_profile{t1 - t0, 0.0, 0.0, t2 - t1, t2 - t0, (uint64_t) S * X * 8ull + (uint64_t) S * 4ull};
			c->rand_path = 1;
			return FSEQ_OK;
		}
	}
	std::vector<uint32_t> A, D;
	std::vector<JoinSegment> segs;
	int const rc = fetch_boundary_states(c, A, D, segs);
	if (rc) return rc;
	double const t0 = now_ms();
	random_join(c->p.m, c->res.max_segment_size, segs, A.data(), D.data(), seed, permutations);
	c->jp.ms_draw = now_ms() - t0; c->jp.ms_total = c->jp.ms_d2h + c->jp.ms_draw;
	c->rand_path = 0;
	return FSEQ_OK;
}

int fseq_random_join_classes_host(uint32_t m, uint32_t max_segment_size, uint64_t n_segments, uint32_t const *count, uint32_t const *rep,
                                  uint32_t const *size, uint32_t seed, uint32_t *permutations)
{
	if (!m || !max_segment_size || !count || !rep || !size || !permutations) return FSEQ_E_ARG;
	for (uint64_t s = 0; s < n_segments; ++s)
		if (count[s] < 1 || count[s] > max_segment_size) return FSEQ_E_ARG;      // (the slots are filled class by class: a table that does not fit them is no table)
	random_join_classes(max_segment_size, n_segments, count, rep, size, seed, permutations);
	return FSEQ_OK;
}

int fseq_debug_join_score_path(fseq_ctx *c, int *path)
{
	if (!c || !path) return FSEQ_E_ARG;
	if (c->score_path < 0) return fail(c, FSEQ_E_ARG, "no fseq_join_score has finished on this context since its input was set");
	*path = c->score_path;
	return FSEQ_OK;
}

// The score of caller-supplied permutations (fseq_joinscore.hpp on the device, fseq_joinscore_host.hpp on the host).  Touches
// nothing a joiner or a writer left on the context: the temporaries are this call's, the join profile stays the last joiner's.
int fseq_join_score(fseq_ctx *c, uint32_t const *permutations, fseq_join_score_entry *junctions, uint32_t *breaks, uint32_t *support,
                    fseq_join_score_summary *summary)
{
	if (!c || !permutations) return FSEQ_E_ARG;
	if (int const rc = need_result(c)) return rc;
	if (c->segments.empty()) return fail(c, FSEQ_E_ARG, "no segments to score (segmentation failed or was not run)");
	if (c->sh.on) return fail(c, FSEQ_E_UNSUPPORTED, "sharded run: collect the boundary states (fseq_boundary_state on their owners) and use fseq_join_score_host");
	(void) hipSetDevice(c->p.device);
	double const t0 = now_ms();
	size_t const m = c->p.m, S = c->segments.size();
	uint32_t const X = c->res.max_segment_size;
	if (X < 1) return fail(c, FSEQ_E_ARG, "no segments to score");
	std::vector<JoinScoreJunction> J;
	std::vector<uint32_t> br;
	try { J.resize(S - 1); br.resize(X); }
	catch (std::bad_alloc const &) { return fail(c, FSEQ_E_OOM, "join score: the junctions on the host"); }
	// the device form: what ClassTables serves (tiling segments, 2^31 rows and segments at most) and a table of 64 KiB
	bool const device = segments_tile(c) && X <= JS_MAX_SLOTS && m <= 0x7FFFFFFFull && S <= 0x7FFFFFFFull && !c->tune.join_host;
	bool done = device && S < 2;                                 // (one segment: no junction, nothing to launch)
	if (device && !done)
		if (int const rc = join_score_device(c, permutations, J, br.data(), support, &done)) return rc;
	if (!done)
	{
		std::vector<uint32_t> A, D;
		std::vector<uint64_t> lb;
		try { A.resize(S * m); D.resize(S * m); lb.resize(S); }
		catch (std::bad_alloc const &) { return fail(c, FSEQ_E_OOM, "join score: the boundary states on the host"); }
		HIP_TRY(c, hipMemcpy(A.data(), c->d_snap_a, S * m * 4, hipMemcpyDeviceToHost));
		HIP_TRY(c, hipMemcpy(D.data(), c->d_snap_d, S * m * 4, hipMemcpyDeviceToHost));
		for (size_t s = 0; s < S; ++s) lb[s] = c->segments[s].lb;
		if (!join_score_host((uint32_t) m, X, S, lb.data(), A.data(), D.data(), permutations, J.data(), br.data(), support))
			return fail(c, FSEQ_E_HIP, "join score: a boundary state names a row that is none");
	}
	std::vector<uint64_t> rb(S);
	for (size_t s = 0; s < S; ++s) rb[s] = c->segments[s].rb;
	join_score_outputs((uint32_t) m, X, S, rb.data(), J, br.data(), now_ms() - t0, junctions, breaks, summary);
	c->score_path = done ? 1 : 0;
	return FSEQ_OK;
}

int fseq_join_score_host(uint32_t m, uint32_t max_segment_size, uint64_t n_segments, uint64_t const *lb, uint64_t const *rb,
                         uint32_t const *a, uint32_t const *d, uint32_t const *permutations, fseq_join_score_entry *junctions,
                         uint32_t *breaks, uint32_t *support, fseq_join_score_summary *summary)
{
	if (!m || !max_segment_size || !n_segments || !lb || !rb || !a || !d || !permutations) return FSEQ_E_ARG;
	double const t0 = now_ms();
	std::vector<JoinScoreJunction> J(n_segments - 1);
	std::vector<uint32_t> br(max_segment_size);
	if (!join_score_host(m, max_segment_size, n_segments, lb, a, d, permutations, J.data(), br.data(), support)) return FSEQ_E_ARG;
	join_score_outputs(m, max_segment_size, n_segments, rb, J, br.data(), now_ms() - t0, junctions, breaks, summary);
	return FSEQ_OK;
}

int fseq_debug_join_score(int device, uint32_t m, uint32_t X, uint32_t S, uint16_t const *of, uint16_t const *perm_cls_left,
                          uint16_t const *perm_cls_right, fseq_join_score_entry *junctions, uint32_t *breaks, uint32_t *support,
                          fseq_join_score_summary *summary)
{
	// ---- everything an index or a key is formed from, before the first HIP call
	if (!of || !perm_cls_left || !perm_cls_right) return FSEQ_E_ARG;
	if (!m || m > 0x7FFFFFFFu || !X || X > JS_MAX_SLOTS || S < 2u || S > 65536u) return FSEQ_E_ARG;
	for (size_t i = 0; i < (size_t) S * m; ++i)
		if (of[i] >= JS_GAP) return FSEQ_E_ARG;
	double const t0 = now_ms();
	size_t const pairs = S - 1u, slots = pairs * X;
	if (hipSetDevice(device) != hipSuccess) return FSEQ_E_HIP;
	struct Held {
		std::vector<void *> held;
		~Held() { for (void *p : held) (void) hipFree(p); }
		void *get(size_t bytes, void const *from)
		{
			void *p = nullptr;
			if (hipMalloc(&p, std::max<size_t>(bytes, 4)) != hipSuccess) { (void) hipGetLastError(); return nullptr; }
			held.push_back(p);
			if (from && hipMemcpy(p, from, bytes, hipMemcpyHostToDevice) != hipSuccess) return nullptr;
			return p;
		}
	} B;
	JoinScoreArgs A{};
	A.of_row = static_cast<uint16_t const *>(B.get((size_t) S * m * 2, of));
	A.cls_left = static_cast<uint16_t const *>(B.get(slots * 2, perm_cls_left));
	A.cls_right = static_cast<uint16_t const *>(B.get(slots * 2, perm_cls_right));
	A.m = m; A.X = X; A.S = S;
	A.junctions = static_cast<uint32_t *>(B.get(pairs * JS_FIELDS * 4, nullptr));
	A.support = static_cast<uint32_t *>(B.get(slots * 4, nullptr));
	uint32_t *d_breaks = static_cast<uint32_t *>(B.get((size_t) X * 4, nullptr));
	if (!A.of_row || !A.cls_left || !A.cls_right || !A.junctions || !A.support || !d_breaks) return FSEQ_E_OOM;
	if (launch_join_score(0, A, d_breaks) != hipSuccess || hipDeviceSynchronize() != hipSuccess) return FSEQ_E_HIP;
	std::vector<uint32_t> words(pairs * JS_FIELDS), br(X);
	if (hipMemcpy(words.data(), A.junctions, words.size() * 4, hipMemcpyDeviceToHost) != hipSuccess ||
	    hipMemcpy(br.data(), d_breaks, (size_t) X * 4, hipMemcpyDeviceToHost) != hipSuccess ||
	    (support && hipMemcpy(support, A.support, slots * 4, hipMemcpyDeviceToHost) != hipSuccess))
		return FSEQ_E_HIP;
	std::vector<JoinScoreJunction> J(pairs);
	for (size_t p = 0; p < pairs; ++p) J[p] = junction_from_words(words.data() + p * JS_FIELDS);
	std::vector<uint64_t> rb(S, 0);
	join_score_outputs(m, X, S, rb.data(), J, br.data(), now_ms() - t0, junctions, breaks, summary);
	return FSEQ_OK;
}

int fseq_bipartite_match_host(uint32_t m, uint32_t max_segment_size, uint64_t n_segments, uint64_t const *lb, uint64_t const *rb,
                              uint32_t const *a, uint32_t const *d, uint32_t *permutations, int64_t *weights)
{
	if (!m || !max_segment_size || !lb || !rb || !a || !d || !permutations) return FSEQ_E_ARG;
	std::vector<JoinSegment> segs(n_segments);
	for (uint64_t i = 0; i < n_segments; ++i) { segs[i].lb = lb[i]; segs[i].rb = rb[i]; }
	std::vector<int64_t> w;
	bipartite_match(m, max_segment_size, segs, a, d, permutations, nullptr, &w);
	if (weights) std::copy(w.begin(), w.end(), weights);
	return FSEQ_OK;
}

int fseq_random_join_host(uint32_t m, uint32_t max_segment_size, uint64_t n_segments, uint64_t const *lb, uint64_t const *rb,
                          uint32_t const *a, uint32_t const *d, uint32_t seed, uint32_t *permutations)
{
	if (!m || !max_segment_size || !lb || !rb || !a || !d || !permutations) return FSEQ_E_ARG;
	std::vector<JoinSegment> segs(n_segments);
	for (uint64_t i = 0; i < n_segments; ++i) { segs[i].lb = lb[i]; segs[i].rb = rb[i]; }
	random_join(m, max_segment_size, segs, a, d, seed, permutations);
	return FSEQ_OK;
}

static int write_segments_impl(fseq_ctx *c, uint8_t const *const *rows, int joining, uint32_t const *A_, uint32_t const *D_,
                               std::vector<JoinSegment> const &segs, char const *path);

int fseq_write_segments(fseq_ctx *c, uint8_t const *const *rows, int joining, char const *path)
{
	if (!c) return FSEQ_E_ARG;
	if (int const rc = need_result(c)) return rc;
	if (joining != FSEQ_JOIN_GREEDY && !rows) return FSEQ_E_ARG;
	std::vector<uint32_t> A, D;
	std::vector<JoinSegment> segs;
	if (joining != FSEQ_JOIN_GREEDY)
	{
		int const rc = fetch_boundary_states(c, A, D, segs);
		if (rc) return rc;
	}
	return write_segments_impl(c, rows, joining, A.data(), D.data(), segs, path);
}

// the same with the boundary states supplied by the caller (a sharded run: collected from their owners)
int fseq_write_segments_host(fseq_ctx *c, uint8_t const *const *rows, int joining, uint32_t const *a, uint32_t const *d, char const *path)
{
	if (!c) return FSEQ_E_ARG;
	if (int const rc = need_result(c)) return rc;
	if (joining != FSEQ_JOIN_GREEDY && (!rows || !a || !d)) return FSEQ_E_ARG;
	std::vector<JoinSegment> segs;
	if (joining != FSEQ_JOIN_GREEDY)
	{
		segs.resize(c->segments.size());
		for (size_t i = 0; i < segs.size(); ++i) { segs[i].lb = c->segments[i].lb; segs[i].rb = c->segments[i].rb; }
	}
	return write_segments_impl(c, rows, joining, a, d, segs, path);
}

// --output-segments from the alignment and the boundary states the device holds (fseq_segfile.hpp): no host rows, no copy of
// the boundary states.  The bytes are write_segments_impl's.
int fseq_write_segments_device(fseq_ctx *c, int joining, char const *path)
{
	if (!c) return FSEQ_E_ARG;
	if (int const rc = need_result(c)) return rc;
	if (joining != FSEQ_JOIN_GREEDY && joining != FSEQ_JOIN_BIPARTITE && joining != FSEQ_JOIN_RANDOM)
		return fail(c, FSEQ_E_ARG, "unknown joining method (FSEQ_JOIN_GREEDY, FSEQ_JOIN_BIPARTITE or FSEQ_JOIN_RANDOM)");
	if (FSEQ_JOIN_GREEDY == joining)
	{
		// (the copy-number matrix of greedy joining is empty: the header alone)
		FILE *f = (path && strcmp(path, "-") != 0) ? fopen(path, "wb") : stdout;
		if (!f) return fail(c, FSEQ_E_ARG, "cannot open the segments output file");
		bool ok = fputs(SEGFILE_HEADER_COPIES, f) >= 0;
		if (fflush(f) != 0) ok = false;
		if (f != stdout) fclose(f);
		if (!ok) return fail(c, FSEQ_E_ARG, "writing the segments output file failed");
		uint64_t const hl = strlen(SEGFILE_HEADER_COPIES);
		c->segfile = fseq_ctx::SegFileStats{true, 0, hl, hl, 1};
		return FSEQ_OK;
	}
	if (c->segments.empty()) return fail(c, FSEQ_E_ARG, "no segments to write (segmentation failed or was not run)");
	if (!c->have_input || !c->d_msa) return fail(c, FSEQ_E_ARG, "no alignment resident on the device");
	if (c->sh.on) return fail(c, FSEQ_E_UNSUPPORTED, "sharded run: a rank holds its own columns and boundary states only (collect them and use fseq_write_segments_host)");
	if (!segments_tile(c)) return fail(c, FSEQ_E_UNSUPPORTED, "the merged segments do not tile the columns (write the segments from host rows: fseq_write_segments)");
	bool const bip = FSEQ_JOIN_BIPARTITE == joining;
	uint32_t const X = c->res.max_segment_size;
	if (X < 1) return fail(c, FSEQ_E_ARG, "no segments to write");
	if (bip && X > JBW_MAX_TEXTS) return fail(c, FSEQ_E_UNSUPPORTED, "bipartite-matching segments file from the device: more than 4,096 texts a segment (write it from host rows: fseq_write_segments)");
	if (!bip && X > 0xFFFFu) return fail(c, FSEQ_E_UNSUPPORTED, "random-joining segments file from the device: more than 65,535 classes a segment (write it from host rows: fseq_write_segments)");
	if (c->p.m > 0x7FFFFFFFull || c->segments.size() > 0x7FFFFFFFull) return fail(c, FSEQ_E_UNSUPPORTED, "segments file from the device: 2^31 rows or segments or more");
	return write_segments_device_lines(c, bip, path, bip ? SEGFILE_HEADER_BIP : SEGFILE_HEADER_COPIES, nullptr);
}

// what the restored entries refuse of a context, in the order of the other restored entries (csrc/fseq_api_identity.hip)
static int need_restored_result(fseq_ctx *c)
{
	if (!c->idn.have) return fail(c, FSEQ_E_ARG, "not a context made by fseq_create_without_identity_columns");
	if (int const rc = need_result(c)) return rc;
	if (c->segments.empty()) return fail(c, FSEQ_E_ARG, "no segments to write (segmentation failed or was not run)");
	return FSEQ_OK;
}

// fseq_get_segments with lb / rb in the source's co-ordinates (restored_segment_bounds, csrc/fseq_restored_bounds.hpp)
int fseq_get_segments_restored(fseq_ctx *c, fseq_segment *out)
{
	if (!c || !out) return FSEQ_E_ARG;
	if (int const rc = need_restored_result(c)) return rc;
	std::vector<uint64_t> src_lb, src_rb;
	if (int const rc = restored_bounds_of(c, src_lb, src_rb)) return rc;
	for (size_t s = 0; s < c->segments.size(); ++s)
	{
		out[s] = c->segments[s];
		out[s].lb = src_lb[s];
		out[s].rb = src_rb[s];
	}
	return FSEQ_OK;
}

// fseq_write_segments_device in the source's co-ordinates: the bounds of restored_segment_bounds, and substrings of the source's
// length with row 0's byte at every identity column (k_segfile_write<., true>, csrc/fseq_segfile.hpp).  Everything else is the
// reduced writer's, byte for byte.
int fseq_write_segments_restored(fseq_ctx *c, int joining, char const *path)
{
	if (!c) return FSEQ_E_ARG;
	if (int const rc = need_restored_result(c)) return rc;
	if (joining != FSEQ_JOIN_GREEDY && joining != FSEQ_JOIN_BIPARTITE && joining != FSEQ_JOIN_RANDOM)
		return fail(c, FSEQ_E_ARG, "unknown joining method (FSEQ_JOIN_GREEDY, FSEQ_JOIN_BIPARTITE or FSEQ_JOIN_RANDOM)");
	if (FSEQ_JOIN_GREEDY == joining) return fseq_write_segments_device(c, joining, path);      // (the header alone: no co-ordinates in it)
	if (!c->have_input || !c->d_msa) return fail(c, FSEQ_E_ARG, "no alignment resident on the device");
	if (c->sh.on) return fail(c, FSEQ_E_UNSUPPORTED, "sharded run: a rank holds its own columns and boundary states only");
	if (!segments_tile(c)) return fail(c, FSEQ_E_UNSUPPORTED, "the merged segments do not tile the columns");
	bool const bip = FSEQ_JOIN_BIPARTITE == joining;
	uint32_t const X = c->res.max_segment_size;
	if (X < 1) return fail(c, FSEQ_E_ARG, "no segments to write");
	if (bip && X > JBW_MAX_TEXTS) return fail(c, FSEQ_E_UNSUPPORTED, "restored bipartite-matching segments file: more than 4,096 texts a segment");
	if (!bip && X > 0xFFFFu) return fail(c, FSEQ_E_UNSUPPORTED, "restored random-joining segments file: more than 65,535 classes a segment");
	if (c->p.m > 0x7FFFFFFFull || c->segments.size() > 0x7FFFFFFFull) return fail(c, FSEQ_E_UNSUPPORTED, "restored segments file: 2^31 rows or segments or more");
	if (c->idn.n_src >= 0xFFFFFFFFull) return fail(c, FSEQ_E_UNSUPPORTED, "restored segments file: the kept columns' source positions are 32 bits wide (source n < 2^32 - 1)");
	std::vector<uint64_t> src_lb, src_rb;
	if (int const rc = restored_bounds_of(c, src_lb, src_rb)) return rc;
	SegFileRestored const R{src_lb.data(), src_rb.data(), (uint32_t const *) c->idn.kept, (uint8_t const *) c->idn.mask, (uint8_t const *) c->idn.ref, c->idn.n_src};
	return write_segments_device_lines(c, bip, path, bip ? SEGFILE_HEADER_BIP : SEGFILE_HEADER_COPIES, &R);
}

// fseq_debug_restored_bounds: restored_segment_bounds on caller-supplied columns and segments.  No device, no context.
int fseq_debug_restored_bounds(uint64_t const *kept, uint64_t n, uint64_t n_src, uint64_t const *lb, uint64_t const *rb, uint64_t n_segments,
                               uint64_t *src_lb, uint64_t *src_rb)
{
	if (!src_lb || !src_rb) return FSEQ_E_ARG;
	return restored_segment_bounds(kept, n, n_src, lb, rb, n_segments, src_lb, src_rb) ? FSEQ_E_ARG : FSEQ_OK;
}

int fseq_debug_segments_file(fseq_ctx *c, uint64_t *batches, uint64_t *bytes, uint64_t *longest_line, uint64_t *lines)
{
	if (!c) return FSEQ_E_ARG;
	if (!c->segfile.have) return fail(c, FSEQ_E_ARG, "no fseq_write_segments_device or fseq_write_segments_restored has finished on this context");
	if (batches) *batches = c->segfile.batches;
	if (bytes) *bytes = c->segfile.bytes;
	if (longest_line) *longest_line = c->segfile.longest_line;
	if (lines) *lines = c->segfile.lines;
	return FSEQ_OK;
}

static int write_segments_impl(fseq_ctx *c, uint8_t const *const *rows, int joining, uint32_t const *A_, uint32_t const *D_,
                               std::vector<JoinSegment> const &segs, char const *path)
{
	FILE *f = (path && strcmp(path, "-") != 0) ? fopen(path, "wb") : stdout;
	if (!f) return fail(c, FSEQ_E_ARG, "cannot open the segments output file");
	size_t const m = c->p.m, S = segs.size();
	uint32_t const X = c->res.max_segment_size;
	if (FSEQ_JOIN_BIPARTITE == joining)
	{
		// segmentation_dp_arg.cc:59-104
		fputs("SEGMENT\tLB\tRB\tSIZE\tSUBSEQUENCE\tSEQUENCES\tCOPIED_FROM\n", f);
		for (size_t s = 0; s < S; ++s)
		{
			uint32_t const *a = A_ + s * m, *d = D_ + s * m;
			auto const texts = create_segment_texts((uint32_t) m, X, a, prepare_copy_numbers((uint32_t) m, X, segs[s].lb, a, d, true));
			for (size_t i = 0; i < texts.size(); ++i)
			{
				SegmentText const &tx = texts[i];
				fprintf(f, "%zu\t%llu\t%llu\t%u\t", s, (unsigned long long) segs[s].lb, (unsigned long long) segs[s].rb, c->segments[s].segment_size);
				uint32_t const rep = texts[tx.row_number(i)].sequence_indices.front();    // segment_text::write_text
				fwrite(rows[rep] + segs[s].lb, 1, segs[s].rb - segs[s].lb, f);
				fputc('\t', f);
				for (size_t k = 0; k < tx.sequence_indices.size(); ++k) fprintf(f, k ? ",%u" : "%u", tx.sequence_indices[k]);
				if (tx.is_copied()) fprintf(f, "\t%zu\n", tx.copied_from); else fputs("\t-\n", f);
			}
		}
	}
	else
	{
		// segmentation_dp_arg.cc:13-56; with greedy joining the copy-number matrix is empty
		fputs("SEGMENT\tLB\tRB\tSIZE\tSUBSEQUENCE_NUMBER\tCOPY_NUMBER\tSUBSEQUENCE\n", f);
		for (size_t s = 0; FSEQ_JOIN_RANDOM == joining && s < S; ++s)
		{
			uint32_t const *a = A_ + s * m, *d = D_ + s * m;
			auto const cn = prepare_copy_numbers((uint32_t) m, X, segs[s].lb, a, d, false);
			uint32_t prev = 0;
			for (auto const &x : cn)
			{
				fprintf(f, "%zu\t%llu\t%llu\t%u\t%u\t%u\t", s, (unsigned long long) segs[s].lb, (unsigned long long) segs[s].rb, c->segments[s].segment_size,
				        x.substring_idx, x.copy_number - prev);
				prev = x.copy_number;
				fwrite(rows[x.substring_idx] + segs[s].lb, 1, segs[s].rb - segs[s].lb, f);
				fputc('\n', f);
			}
		}
	}
	fflush(f);
	if (f != stdout) fclose(f);
	return FSEQ_OK;
}

int fseq_greedy_match_host(uint32_t m, uint32_t max_segment_size, uint64_t n_segments, uint64_t const *lb, uint64_t const *rb,
                           uint32_t const *a, uint32_t const *d, uint32_t *permutations)
{
	if (!m || !max_segment_size || !lb || !rb || !a || !d || !permutations) return FSEQ_E_ARG;
	std::vector<JoinSegment> segs(n_segments);
	for (uint64_t i = 0; i < n_segments; ++i) { segs[i].lb = lb[i]; segs[i].rb = rb[i]; }
	greedy_match(m, max_segment_size, segs, a, d, permutations);
	return FSEQ_OK;
}

int fseq_write_founders(fseq_ctx *c, uint8_t const *const *rows, uint32_t const *permutations, char const *path)
{
	if (!c || !rows || !permutations) return FSEQ_E_ARG;
	if (int const rc = need_result(c)) return rc;
	FILE *f = (path && strcmp(path, "-") != 0) ? fopen(path, "wb") : stdout;
	if (!f) return fail(c, FSEQ_E_ARG, "cannot open the founders output file");
	size_t const X = c->res.max_segment_size, S = c->segments.size();
	// join_context.cc:341-356: line r = the segments' substrings of the rows permutations[s][r], one after the other.
	// The lines are put together in memory -- a batch of them at a time, on a few host threads: a line is S pieces of a
	// few hundred bytes from S different input rows -- and go out in one write per batch (one fwrite per piece was 41 of a
	// drop-in BASELINE C3 run's ~150 ms, profiles/r03_e2e_C3_greedy.json).
	size_t const line = (size_t) c->p.n + 1;
	size_t const batch = std::max<size_t>(1, std::min<size_t>(X, (size_t) (256u << 20) / line));
	std::vector<char> buf;
	try { buf.resize(batch * line); } catch (std::bad_alloc const &) { if (f != stdout) fclose(f); return fail(c, FSEQ_E_OOM, "founders output buffer"); }
	bool ok = true;
	for (size_t r0 = 0; r0 < X && ok; r0 += batch)
	{
		size_t const r1 = std::min(X, r0 + batch);
		unsigned const nth = (unsigned) std::max<size_t>(1, std::min<size_t>({(size_t) std::thread::hardware_concurrency(), (size_t) 8, r1 - r0}));
		auto work = [&](unsigned t) {
			for (size_t row = r0 + t; row < r1; row += nth)
			{
				char *out = buf.data() + (row - r0) * line;
				for (size_t s = 0; s < S; ++s)
				{
					fseq_segment const &sg = c->segments[s];
					memcpy(out + sg.lb, rows[permutations[s * X + row]] + sg.lb, sg.rb - sg.lb);
				}
				out[line - 1] = '\n';
			}
		};
		std::vector<std::thread> ths;
		for (unsigned t = 1; t < nth; ++t) ths.emplace_back(work, t);
		work(0);
		for (auto &th : ths) th.join();
		ok = fwrite(buf.data(), 1, (r1 - r0) * line, f) == (r1 - r0) * line;
	}
	fflush(f);
	if (f != stdout) fclose(f);
	if (!ok) return fail(c, FSEQ_E_ARG, "writing the founders output file failed");
	return FSEQ_OK;
}


// [r5] --output-founders straight from the alignment the device holds (k_founders, fseq_joinprep.hpp): no host rows needed.
// The lines are put together on the device, a batch of rows (<= 256 MB) at a time, and leave in one copy and one write per batch.
int fseq_write_founders_device(fseq_ctx *c, uint32_t const *permutations, char const *path)
{
	if (!c || !permutations) return FSEQ_E_ARG;
	if (int const rc = need_result(c)) return rc;
	if (!c->have_input || !c->d_msa) return fail(c, FSEQ_E_ARG, "no alignment resident on the device");
	if (c->sh.on) return fail(c, FSEQ_E_UNSUPPORTED, "sharded run: a rank holds its own columns only (write the founders from host rows: fseq_write_founders)");
	(void) hipSetDevice(c->p.device);
	size_t const X = c->res.max_segment_size, S = c->segments.size();
	if (!X || !S) return fail(c, FSEQ_E_ARG, "no segments to write");
	FILE *f = (path && strcmp(path, "-") != 0) ? fopen(path, "wb") : stdout;
	if (!f) return fail(c, FSEQ_E_ARG, "cannot open the founders output file");
	hipStream_t st = c->stream;
	size_t const line = (size_t) c->p.n + 1;
	size_t const batch = std::max<size_t>(1, std::min<size_t>(X, (size_t) (256u << 20) / line));
	DevTemp<uint32_t> d_perm(c);
	DevTemp<uint64_t> d_seg(c);
	DevTemp<uint8_t> d_lut(c), d_out(c);
	uint8_t *h_out = nullptr;
	int rc = FSEQ_OK;
	auto cleanup = [&]() {
		if (h_out) (void) hipHostFree(h_out);
		if (f != stdout) fclose(f);
	};
	if ((rc = d_perm.alloc(S * X)) || (rc = d_seg.alloc(2 * S)) || (rc = d_lut.alloc(256)) || (rc = d_out.alloc(batch * line))) { cleanup(); return rc; }
	if (hipHostMalloc(reinterpret_cast<void **>(&h_out), batch * line, hipHostMallocDefault) != hipSuccess) { h_out = nullptr; cleanup(); return fail(c, FSEQ_E_OOM, "founders output buffer"); }
	std::vector<uint64_t> seg(2 * S);
	for (size_t s = 0; s < S; ++s) { seg[s] = c->segments[s].lb; seg[S + s] = c->segments[s].rb; }
	bool ok = true;
	do {
		if (hipMemcpyAsync(d_perm, permutations, S * X * 4, hipMemcpyHostToDevice, st) != hipSuccess) { ok = false; break; }
		if (hipMemcpyAsync(d_seg, seg.data(), 2 * S * 8, hipMemcpyHostToDevice, st) != hipSuccess) { ok = false; break; }
		if (hipMemcpyAsync(d_lut, c->code_to_byte, 256, hipMemcpyHostToDevice, st) != hipSuccess) { ok = false; break; }
		for (size_t r0 = 0; r0 < X && ok; r0 += batch)
		{
			size_t const nr = std::min(batch, X - r0);
			uint32_t const rows_per_wg = 16;
			hipLaunchKernelGGL(k_founders, dim3((uint32_t) S, (uint32_t) ((nr + rows_per_wg - 1) / rows_per_wg)), dim3(256), 0, st, c->d_msa, c->ld, c->p.m, (uint64_t) c->p.n, c->bsh,
			                   d_perm, (uint32_t) X, d_seg, d_seg + S, (uint32_t) S, (uint32_t) r0, (uint32_t) nr, rows_per_wg, d_lut, d_out);
			if (hipMemcpyAsync(h_out, d_out, nr * line, hipMemcpyDeviceToHost, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess) { ok = false; break; }
			ok = fwrite(h_out, 1, nr * line, f) == nr * line;
		}
	} while (false);
	if (ok && hipGetLastError() != hipSuccess) ok = false;
	fflush(f);
	cleanup();
	if (!ok) return fail(c, FSEQ_E_HIP, "writing the founders from the device failed");
	return FSEQ_OK;
}

} // extern "C"
