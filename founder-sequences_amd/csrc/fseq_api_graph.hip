// fseq_api_graph.hip -- the part of the C ABI (include/fseq.h) behind the founder block graph: fseq_block_graph (the graph as
// arrays), fseq_write_block_graph (the GFA 1.0 file from the device, csrc/fseq_graph.hpp) and fseq_debug_graph_file; and
// fseq_graph_thread_rows / fseq_graph_thread_held_out (rows that are not the graph's own threaded through it,
// csrc/fseq_graphthread.hpp) with fseq_debug_graph_thread; and the three in the SOURCE's co-ordinates on an identity-reduced
// context: fseq_write_block_graph_restored, fseq_graph_thread_rows_restored, fseq_graph_thread_held_out_restored; and
// fseq_graph_nearest_rows / fseq_graph_nearest_held_out (the nearest node of every segment and its distance,
// csrc/fseq_graphnearest.hpp) with fseq_debug_graph_nearest, fseq_debug_graph_nearest_info and fseq_debug_graph_nearest_plan.
//
// No counterpart in the reference.  Both entries build on the device front of fseq_join_greedy (fseq_joinprep.hpp, unchanged):
// k_join_classes_wide numbers the classes of every merged segment, k_join_edges_wide<false> / k_join_scan / <true> leave the
// weighted edges of every adjacent pair in ascending (l, r) order.  Everything here is a temporary of one call: nothing a run, a
// joiner, a writer or a match left on the context is touched, and nothing is allocated or launched unless one of the entries is
// called.  There is no host form: what the device form does not serve is refused.
#include "fseq_ctx.hpp"
#include "fseq_joinprep.hpp"
#include "fseq_graph.hpp"
#include "fseq_graphthread.hpp"
#include "fseq_graphnearest.hpp"

using namespace fseq;

static constexpr uint64_t GRAPH_BATCH_BYTES = 256ull << 20;      // (what fseq_write_segments_device takes a batch)
static char const GRAPH_HEADER[] = "H\tVN:Z:1.0\n";

// The class tables of every merged segment and the edges of every adjacent pair, on the device, with the counts on the host.
struct GraphTables {
	fseq_ctx *c;
	size_t S = 0, m = 0;
	uint32_t X = 0, pairs = 0;
	DevTemp<uint16_t> d_of;
	DevTemp<uint32_t> d_rep, d_size, d_count, d_start, d_off, d_ne, d_noff;
	DevTemp<uint64_t> d_lb, d_rb;
	DevTemp<unsigned long long> d_total;
	DevTemp<uint2> d_edges;
	std::vector<uint32_t> count, noff;       // [S], [S + 1]
	uint64_t nodes = 0, edges = 0;
	explicit GraphTables(fseq_ctx *c_) : c(c_), d_of(c_), d_rep(c_), d_size(c_), d_count(c_), d_start(c_), d_off(c_), d_ne(c_), d_noff(c_), d_lb(c_), d_rb(c_), d_total(c_), d_edges(c_) {}

	// write_edges: the edges themselves (else their number only)
	int build(bool write_edges)
	{
		S = c->segments.size(); m = c->p.m; X = c->res.max_segment_size; pairs = (uint32_t) (S - 1);
		hipStream_t st = c->stream;
		int rc;
		if ((rc = d_of.alloc(S * m)) || (rc = d_rep.alloc(S * X)) || (rc = d_size.alloc(S * X)) || (rc = d_count.alloc(S)) ||
		    (rc = d_start.alloc(S * ((size_t) X + 1))) || (rc = d_off.alloc(S)) || (rc = d_ne.alloc(S)) || (rc = d_noff.alloc(S + 1)) ||
		    (rc = d_lb.alloc(S)) || (rc = d_rb.alloc(S)) || (rc = d_total.alloc(1)))
			return rc;
		std::vector<uint64_t> b;
		try { b.resize(2 * S); count.resize(S); noff.resize(S + 1); }
		catch (std::bad_alloc const &) { return fail(c, FSEQ_E_OOM, "block graph: the segments on the host"); }
		for (size_t i = 0; i < S; ++i) { b[i] = c->segments[i].lb; b[S + i] = c->segments[i].rb; }
		size_t const lds = (size_t) JW_CELLS * 4;
		hipError_t e = hipMemcpyAsync(d_lb, b.data(), S * 8, hipMemcpyHostToDevice, st);
		if (e == hipSuccess) e = hipMemcpyAsync(d_rb, b.data() + S, S * 8, hipMemcpyHostToDevice, st);
		if (e == hipSuccess) e = hipMemsetAsync(d_rep, 0, S * X * 4, st);
		if (e == hipSuccess) e = allow_lds(k_join_edges_wide<false>, lds);
		if (e == hipSuccess) e = allow_lds(k_join_edges_wide<true>, lds);
		if (e != hipSuccess) { (void) hipStreamSynchronize(st); return fail(c, FSEQ_E_HIP, "block graph: class tables", e); }
		hipLaunchKernelGGL(k_join_classes_wide, dim3((uint32_t) S), dim3(JW_T), 0, st, c->d_snap_a, c->d_snap_d, d_rb, (uint32_t) m, X, d_of, d_rep, d_size, d_count, d_start);
		if (pairs)
			hipLaunchKernelGGL(k_join_edges_wide<false>, dim3(pairs), dim3(JW_T), lds, st, c->d_snap_a, d_of, d_count, d_start, (uint32_t) m, X, d_ne, d_off, (uint2 *) nullptr, (uint64_t) 0);
		hipLaunchKernelGGL(k_join_scan, dim3(1), dim3(JW_T), 0, st, d_ne, pairs, d_off, d_total);
		unsigned long long total = 0;
		e = hipMemcpyAsync(count.data(), d_count, S * 4, hipMemcpyDeviceToHost, st);
		if (e == hipSuccess) e = hipMemcpyAsync(&total, d_total, 8, hipMemcpyDeviceToHost, st);
		hipError_t const es = hipStreamSynchronize(st);              // (b, count and total are read and written to here, whatever was queued)
		if (e == hipSuccess) e = es;
		if (e == hipSuccess) e = hipGetLastError();
		if (e != hipSuccess) return fail(c, FSEQ_E_HIP, "block graph: class tables", e);
		nodes = 0;
		for (size_t i = 0; i < S; ++i)
		{
			if (count[i] < 1 || count[i] > X) return fail(c, FSEQ_E_UNSUPPORTED, "block graph: the class tables of the device hold a class count outside [1, max_segment_size]");
			if (i && count[i] > JW_CELLS) return fail(c, FSEQ_E_UNSUPPORTED, "block graph: a right segment of more than 32,768 classes (the edge kernel reports no edges for it)");
			noff[i] = (uint32_t) nodes;
			nodes += count[i];
			if (nodes > 0xFFFFFFFFull) return fail(c, FSEQ_E_UNSUPPORTED, "block graph: 2^32 nodes or more");
		}
		noff[S] = (uint32_t) nodes;
		edges = total;
		if (edges > 0xFFFFFFFFull) return fail(c, FSEQ_E_UNSUPPORTED, "block graph: 2^32 edges or more");
		HIP_TRY(c, hipMemcpyAsync(d_noff, noff.data(), (S + 1) * 4, hipMemcpyHostToDevice, st));      // (noff lives as long as the tables: every caller synchronises before it lets go of them)
		if (write_edges && pairs && edges)
		{
			if ((rc = d_edges.alloc((size_t) edges))) { (void) hipStreamSynchronize(st); return rc; }
			hipLaunchKernelGGL(k_join_edges_wide<true>, dim3(pairs), dim3(JW_T), lds, st, c->d_snap_a, d_of, d_count, d_start, (uint32_t) m, X, d_ne, d_off, (uint2 *) d_edges, (uint64_t) edges);
		}
		return FSEQ_OK;
	}

	GraphArgs args(int gap) const
	{
		GraphArgs A{};
		A.seg_lb = d_lb; A.seg_rb = d_rb; A.count = d_count; A.rep = d_rep; A.size = d_size; A.noff = d_noff; A.of_row = d_of;
		A.m = (uint32_t) m; A.X = X; A.S = (uint32_t) S; A.gap = gap < 0 ? -1 : gap;
		A.msa = c->d_msa; A.ld = c->ld; A.bsh = c->bsh;
		A.edges = d_edges; A.offset = d_off; A.pairs = pairs; A.n_edges = d_edges.base ? edges : 0u;
		return A;
	}
};

// what both entries refuse of a context before a device is touched
static int graph_refusals(fseq_ctx *c)
{
	if (int const rc = need_result(c)) return rc;
	if (c->segments.empty()) return fail(c, FSEQ_E_ARG, "no segments to build the block graph from (segmentation failed or was not run)");
	if (c->sh.on) return fail(c, FSEQ_E_UNSUPPORTED, "sharded run: a rank holds its own columns and boundary states only (the block graph needs them all on one device)");
	for (size_t i = 0; i < c->segments.size(); ++i)
		if (c->segments[i].lb != (i ? c->segments[i - 1].rb : 0u)) return fail(c, FSEQ_E_UNSUPPORTED, "block graph: the merged segments do not tile the columns");
	uint32_t const X = c->res.max_segment_size;
	if (X < 1) return fail(c, FSEQ_E_ARG, "no segments to build the block graph from");
	if (X > 0xFFFFu) return fail(c, FSEQ_E_UNSUPPORTED, "block graph: more than 65,535 classes a segment");
	if (c->p.m > 0x7FFFFFFFull || c->segments.size() > 0x7FFFFFFFull) return fail(c, FSEQ_E_UNSUPPORTED, "block graph: 2^31 rows or segments or more");
	return FSEQ_OK;
}

// what the threading refuses beyond the block graph's refusals; restored: the entries that take an identity-reduced context
static int graph_thread_refusals(fseq_ctx *c, bool restored = false)
{
	if (int const rc = graph_refusals(c)) return rc;
	if (c->idn.have && !restored) return fail(c, FSEQ_E_UNSUPPORTED, "graph threading: a context made by fseq_create_without_identity_columns (queries in source co-ordinates, with their exception cells, are not served)");
	if (c->res.max_segment_size > GT_MAX_CLASSES) return fail(c, FSEQ_E_UNSUPPORTED, "graph threading: more than 4,096 classes in a segment (there is no host form)");
	if (!c->have_input || !c->d_msa) return fail(c, FSEQ_E_ARG, "no alignment resident on the device");
	return FSEQ_OK;
}

// The segments' source ranges of an identity-reduced context on the device, for the restored entries (restored_bounds_of: the
// bounds fseq_get_segments_restored reports).  Refuses what that entry refuses, before a device buffer exists.
struct RestoredBounds {
	std::vector<uint64_t> src_lb, src_rb;
	DevTemp<uint64_t> d_lb, d_rb;
	explicit RestoredBounds(fseq_ctx *c) : d_lb(c), d_rb(c) {}
	int build(fseq_ctx *c, char const *what)
	{
		if (c->idn.n_src >= 0xFFFFFFFFull)
		{
			std::string const why = std::string(what) + ": the kept columns' source positions are 32 bits wide (source n < 2^32 - 1)";
			return fail(c, FSEQ_E_UNSUPPORTED, why.c_str());
		}
		if (int const rc = restored_bounds_of(c, src_lb, src_rb)) return rc;
		size_t const S = src_lb.size();
		int rc;
		if ((rc = d_lb.alloc(S)) || (rc = d_rb.alloc(S))) return rc;
		// (blocking copies: the vectors may go before the stream gets to them)
		HIP_TRY(c, hipMemcpy(d_lb, src_lb.data(), S * 8, hipMemcpyHostToDevice));
		HIP_TRY(c, hipMemcpy(d_rb, src_rb.data(), S * 8, hipMemcpyHostToDevice));
		return FSEQ_OK;
	}
};

// the exception cells of the queries of a restored threading, on the device
struct ThreadExceptions {
	uint64_t const *off;
	uint32_t const *cols;
	uint64_t total;
};

// both entries behind their refusals: the Q queries at q (column-major, packed at qbsh, qld bytes a column) through the graph
// (R / E: the restored form -- the queries are the kept columns of rows of the source's length, E their exception cells)
static int graph_thread(fseq_ctx *c, uint8_t const *q, size_t qld, uint32_t qbsh, uint32_t Q, uint32_t *nodes, uint32_t *steps,
                        fseq_graph_thread_row *per_row, fseq_graph_thread_segment *per_segment, fseq_graph_thread_summary *summary,
                        RestoredBounds const *R = nullptr, ThreadExceptions const *E = nullptr)
{
	double const t0 = now_ms();
	hipStream_t st = c->stream;
	GraphTables T(c);
	if (int const rc = T.build(true)) return rc;
	size_t const S = T.S;
	uint32_t const X = T.X;
	uint32_t slots = GT_MIN_SLOTS;
	while (slots < 2u * X) slots *= 2u;
	size_t const lds = (size_t) slots * (sizeof(uint64_t) + sizeof(uint32_t));
	uint32_t const key_bits = c->tune.graph_thread_key_bits > 0 ? (uint32_t) std::min(c->tune.graph_thread_key_bits, 64) : 64u;
	DevTemp<uint64_t> d_keys(c);
	DevTemp<uint32_t> d_nodes(c), d_steps(c);
	DevTemp<fseq_graph_thread_row> d_rows(c);
	DevTemp<fseq_graph_thread_segment> d_segs(c);
	DevTemp<unsigned long long> d_stats(c);
	int rc;
	if ((rc = d_keys.alloc(S * X)) || (rc = d_nodes.alloc(S * Q)) || (rc = d_steps.alloc(std::max<size_t>(T.pairs, 1) * Q)) ||
	    (rc = d_rows.alloc(Q)) || (rc = d_segs.alloc(S)) || (rc = d_stats.alloc(3)))
	{ (void) hipStreamSynchronize(st); return rc; }
	std::vector<fseq_graph_thread_row> rows;
	try { rows.resize(Q); }
	catch (std::bad_alloc const &) { (void) hipStreamSynchronize(st); return fail(c, FSEQ_E_OOM, "graph threading: the rows' statistics on the host"); }
	GraphThreadArgs A{};
	A.seg_lb = T.d_lb; A.seg_rb = T.d_rb; A.count = T.d_count; A.rep = T.d_rep; A.noff = T.d_noff;
	A.m = (uint32_t) T.m; A.X = X; A.S = (uint32_t) S; A.n = c->p.n;
	A.msa = c->d_msa; A.ld = c->ld; A.bsh = c->bsh;
	A.q = q; A.qld = qld; A.qbsh = qbsh; A.Q = Q; A.sigma = c->sigma;
	A.key_bits = key_bits; A.slots = slots;
	A.keys = d_keys; A.nodes = d_nodes; A.steps = d_steps;
	A.edges = T.d_edges; A.offset = T.d_off; A.nedges = T.d_ne; A.pairs = T.pairs; A.n_edges = T.d_edges.base ? T.edges : 0u;
	A.stats = d_stats;
	bool const restored = R && E;
	if (restored)
	{
		A.src_lb = R->d_lb; A.src_rb = R->d_rb; A.n_src = c->idn.n_src;
		A.exc_off = E->off; A.exc_cols = E->cols; A.n_exc = E->total;
	}
	hipError_t e = hipMemsetAsync(d_stats, 0, 3 * sizeof(unsigned long long), st);
	if (e == hipSuccess) e = allow_lds(k_gt_thread, lds);
	if (e != hipSuccess) { (void) hipStreamSynchronize(st); return fail(c, FSEQ_E_HIP, "graph threading: preparation", e); }
	uint32_t const tiles = (uint32_t) std::min<size_t>(((size_t) Q + GT_T - 1) / GT_T, 1024);
	hipLaunchKernelGGL(k_gt_keys, dim3((uint32_t) S, (X + GT_T - 1u) / GT_T), dim3(GT_T), 0, st, A);
	hipLaunchKernelGGL(k_gt_thread, dim3((uint32_t) S, tiles), dim3(GT_T), lds, st, A);
	if (restored && E->total) hipLaunchKernelGGL(k_gt_exceptions, dim3((Q + GT_T - 1u) / GT_T), dim3(GT_T), 0, st, A);
	if (T.pairs) hipLaunchKernelGGL(k_gt_steps, dim3(T.pairs, tiles), dim3(GT_T), 0, st, A);
	if (restored) hipLaunchKernelGGL(k_gt_rows<true>, dim3((Q + GT_T - 1u) / GT_T), dim3(GT_T), 0, st, A, (fseq_graph_thread_row *) d_rows);
	else hipLaunchKernelGGL(k_gt_rows<false>, dim3((Q + GT_T - 1u) / GT_T), dim3(GT_T), 0, st, A, (fseq_graph_thread_row *) d_rows);
	if (per_segment) hipLaunchKernelGGL(k_gt_segments, dim3((uint32_t) S), dim3(GT_T), 0, st, A, (fseq_graph_thread_segment *) d_segs);
	unsigned long long stats[3] = {0, 0, 0};
	e = hipMemcpyAsync(rows.data(), d_rows, (size_t) Q * sizeof(fseq_graph_thread_row), hipMemcpyDeviceToHost, st);
	if (e == hipSuccess) e = hipMemcpyAsync(stats, d_stats, sizeof(stats), hipMemcpyDeviceToHost, st);
	if (e == hipSuccess && nodes) e = hipMemcpyAsync(nodes, d_nodes, S * Q * 4, hipMemcpyDeviceToHost, st);
	if (e == hipSuccess && steps && T.pairs) e = hipMemcpyAsync(steps, d_steps, (size_t) T.pairs * Q * 4, hipMemcpyDeviceToHost, st);
	if (e == hipSuccess && per_segment) e = hipMemcpyAsync(per_segment, d_segs, S * sizeof(fseq_graph_thread_segment), hipMemcpyDeviceToHost, st);
	hipError_t const es = hipStreamSynchronize(st);                  // (the host arrays are written to here, whatever was queued)
	if (e == hipSuccess) e = es;
	if (e == hipSuccess) e = hipGetLastError();
	if (e != hipSuccess) return fail(c, FSEQ_E_HIP, "graph threading", e);
	fseq_graph_thread_summary sm{};
	sm.rows = Q; sm.segments = S;
	for (fseq_graph_thread_row const &r : rows)
	{
		sm.segments_matched += r.segments_matched; sm.junctions_linked += r.junctions_linked; sm.junctions_novel += r.junctions_novel; sm.walks += r.walks;
		sm.rows_on_graph += r.walks == 1u && r.longest_walk_segments == S;
	}
	if (per_row) memcpy(per_row, rows.data(), (size_t) Q * sizeof(fseq_graph_thread_row));
	sm.ms_device = now_ms() - t0;
	if (summary) *summary = sm;
	c->graphthread.have = true;
	c->graphthread.info = fseq_graph_thread_info{key_bits, slots, stats[0], stats[1], stats[2]};
	return FSEQ_OK;
}

extern "C" {

int fseq_graph_thread_rows(fseq_ctx *c, uint8_t const *const *rows, uint32_t n_rows, uint32_t *nodes, uint32_t *steps,
                           fseq_graph_thread_row *per_row, fseq_graph_thread_segment *per_segment, fseq_graph_thread_summary *summary)
{
	if (!c) return FSEQ_E_ARG;
	if (!rows || 0 == n_rows) return fail(c, FSEQ_E_ARG, "graph threading: no query rows");
	for (uint32_t i = 0; i < n_rows; ++i)
		if (!rows[i]) return fail(c, FSEQ_E_ARG, "graph threading: null query row");
	if (int const rc = graph_thread_refusals(c)) return rc;
	(void) hipSetDevice(c->p.device);
	// the queries' packing: the narrowest that leaves the code `sigma` free for a byte outside the alphabet (as fseq_match_rows)
	uint32_t const sigma = c->sigma, bsh = sigma + 1u <= 4u ? 2u : sigma + 1u <= 16u ? 1u : 0u;
	size_t const ld = ((((size_t) n_rows + (1u << bsh) - 1u) >> bsh) + 15) & ~size_t(15);
	DevTemp<uint8_t> d_q(c);                                         // (the call's own: the last match keeps its queries)
	if (int const rc = upload_queries(c, rows, n_rows, bsh, ld, d_q)) return rc;
	return graph_thread(c, d_q, ld, bsh, n_rows, nodes, steps, per_row, per_segment, summary);
}

// the held-out rows (fseq_create_without_rows, csrc/fseq_api_rowsplit.hip) are on the device already, column-major and packed
// at the alignment's width: nothing is uploaded or packed
int fseq_graph_thread_held_out(fseq_ctx *c, uint32_t *nodes, uint32_t *steps, fseq_graph_thread_row *per_row, fseq_graph_thread_segment *per_segment,
                               fseq_graph_thread_summary *summary)
{
	if (!c) return FSEQ_E_ARG;
	if (!c->hold.have && !c->idn.have) return fail(c, FSEQ_E_ARG, "not a context made by fseq_create_without_rows");
	if (int const rc = graph_thread_refusals(c)) return rc;
	if (!c->hold.have || !c->hold.n_held || !c->hold.cols) return fail(c, FSEQ_E_ARG, "not a context made by fseq_create_without_rows");
	(void) hipSetDevice(c->p.device);
	return graph_thread(c, c->hold.cols, c->hold.ld, c->bsh, c->hold.n_held, nodes, steps, per_row, per_segment, summary);
}

// fseq_graph_thread_rows on an identity-reduced context with queries of the source's length: their kept columns and their
// exception cells go into temporaries of the call (the last match keeps its queries and its exception lists)
int fseq_graph_thread_rows_restored(fseq_ctx *c, uint8_t const *const *rows, uint32_t n_rows, uint32_t *nodes, uint32_t *steps,
                                    fseq_graph_thread_row *per_row, fseq_graph_thread_segment *per_segment, fseq_graph_thread_summary *summary)
{
	if (!c) return FSEQ_E_ARG;
	if (!rows || 0 == n_rows) return fail(c, FSEQ_E_ARG, "graph threading: no query rows");
	for (uint32_t i = 0; i < n_rows; ++i)
		if (!rows[i]) return fail(c, FSEQ_E_ARG, "graph threading: null query row");
	if (!c->idn.have) return fail(c, FSEQ_E_ARG, "not a context made by fseq_create_without_identity_columns");
	if (int const rc = graph_thread_refusals(c, true)) return rc;
	(void) hipSetDevice(c->p.device);
	RestoredBounds R(c);
	if (int const rc = R.build(c, "restored graph threading")) return rc;
	uint32_t const sigma = c->sigma, bsh = sigma + 1u <= 4u ? 2u : sigma + 1u <= 16u ? 1u : 0u;
	size_t const ld = ((((size_t) n_rows + (1u << bsh) - 1u) >> bsh) + 15) & ~size_t(15);
	DevTemp<uint8_t> d_q(c);
	DevTemp<uint64_t> d_off(c);
	DevTemp<uint32_t> d_cols(c);
	uint64_t total = 0;
	if (int const rc = upload_queries_restored(c, rows, n_rows, bsh, ld, d_q, d_off, d_cols, &total)) return rc;
	ThreadExceptions const E{d_off, d_cols, total};
	return graph_thread(c, d_q, ld, bsh, n_rows, nodes, steps, per_row, per_segment, summary, &R, &E);
}

// the held-out rows of a context made by fseq_create_without_identity_columns_held: their kept columns and their exception cells
// are on the device already
int fseq_graph_thread_held_out_restored(fseq_ctx *c, uint32_t *nodes, uint32_t *steps, fseq_graph_thread_row *per_row, fseq_graph_thread_segment *per_segment,
                                        fseq_graph_thread_summary *summary)
{
	if (!c) return FSEQ_E_ARG;
	if (!c->idn.have) return fail(c, FSEQ_E_ARG, "not a context made by fseq_create_without_identity_columns");
	if (!c->hold.have_exc) return fail(c, FSEQ_E_ARG, "not a context made by fseq_create_without_identity_columns_held");
	if (int const rc = graph_thread_refusals(c, true)) return rc;
	if (!c->hold.have || !c->hold.n_held || !c->hold.cols) return fail(c, FSEQ_E_ARG, "not a context made by fseq_create_without_identity_columns_held");
	(void) hipSetDevice(c->p.device);
	RestoredBounds R(c);
	if (int const rc = R.build(c, "restored graph threading")) return rc;
	ThreadExceptions const E{c->hold.exc_off, c->hold.exc_cols, c->hold.exc_total};
	return graph_thread(c, c->hold.cols, c->hold.ld, c->bsh, c->hold.n_held, nodes, steps, per_row, per_segment, summary, &R, &E);
}

int fseq_debug_graph_thread(fseq_ctx *c, fseq_graph_thread_info *out)
{
	if (!c || !out) return FSEQ_E_ARG;
	if (!c->graphthread.have) return fail(c, FSEQ_E_ARG, "no fseq_graph_thread_rows / fseq_graph_thread_held_out has finished on this context");
	*out = c->graphthread.info;
	return FSEQ_OK;
}

} // extern "C"

// ---- the nearest node of every segment (csrc/fseq_graphnearest.hpp)

// The layout of the packed words and the batches, on the host (csrc/fseq_graphnearest_plan.hpp), and what the largest batch takes.
struct GraphNearestPlan {
	std::vector<uint64_t> qoff, roff, first;             // [S + 1], [S + 1], [batches + 1]
	uint64_t batches = 0, most_rw = 0, most_qw = 0;      // the largest batch: representatives' words, words of one query
	// nullptr, or why not (what: FSEQ_E_ARG or FSEQ_E_UNSUPPORTED)
	char const *build(uint64_t const *lb, uint64_t const *rb, uint32_t const *count, uint64_t S, uint32_t bits, uint64_t budget, int *what)
	{
		*what = FSEQ_E_ARG;
		try { qoff.assign(S + 1, 0); roff.assign(S + 1, 0); first.assign(S + 1, 0); }
		catch (std::bad_alloc const &) { *what = FSEQ_E_OOM; return "the plan on the host"; }
		for (uint64_t s = 0; lb && rb && s < S; ++s)
			if (rb[s] > lb[s] && rb[s] - lb[s] >= 0xFFFFFFFFull) { *what = FSEQ_E_UNSUPPORTED; return "a segment of 2^32 - 1 columns or more (distances are 32-bit)"; }
		if (char const *why = graph_nearest_words(lb, rb, count, S, bits, qoff.data(), roff.data())) return why;
		if (char const *why = graph_nearest_plan(roff.data(), S, budget, first.data(), &batches)) return why;
		for (uint64_t b = 0; b < batches; ++b)
		{
			most_rw = std::max(most_rw, roff[first[b + 1]] - roff[first[b]]);
			most_qw = std::max(most_qw, qoff[first[b + 1]] - qoff[first[b]]);
		}
		return nullptr;
	}
};

// The production launcher, for the entries and for fseq_debug_graph_nearest alike: batch by batch the two pack kernels and the
// distance kernel.  A holds everything but the batch; A.rw / A.qw have room for the plan's largest batch.
static void graph_nearest_launch(hipStream_t st, GraphNearestArgs A, GraphNearestPlan const &P)
{
	uint32_t const Q = A.G.Q, X = A.G.X;
	uint32_t const tiles = (uint32_t) std::min<size_t>(((size_t) Q + GT_T - 1) / GT_T, 1024);
	uint32_t const ctiles = (uint32_t) std::min<size_t>(((size_t) X + GT_T - 1) / GT_T, 1024);
	uint32_t const w = 8u >> A.G.qbsh;
	for (uint64_t b = 0; b < P.batches; ++b)
	{
		A.s0 = (uint32_t) P.first[b]; A.s1 = (uint32_t) P.first[b + 1];
		uint32_t const ns = A.s1 - A.s0;
		hipLaunchKernelGGL(k_gn_pack<false>, dim3(ns, ctiles), dim3(GT_T), 0, st, A);
		hipLaunchKernelGGL(k_gn_pack<true>, dim3(ns, tiles), dim3(GT_T), 0, st, A);
		if (w == 2u) hipLaunchKernelGGL(k_gn_distance<2>, dim3(ns, tiles), dim3(GT_T), 0, st, A, (uint32_t const *) A.rw, (uint32_t const *) A.qw);
		else if (w == 4u) hipLaunchKernelGGL(k_gn_distance<4>, dim3(ns, tiles), dim3(GT_T), 0, st, A, (uint32_t const *) A.rw, (uint32_t const *) A.qw);
		else hipLaunchKernelGGL(k_gn_distance<8>, dim3(ns, tiles), dim3(GT_T), 0, st, A, (uint32_t const *) A.rw, (uint32_t const *) A.qw);
	}
}

// both entries behind their refusals: the Q queries at q (column-major, packed at qbsh, qld bytes a column)
static int graph_nearest(fseq_ctx *c, uint8_t const *q, size_t qld, uint32_t qbsh, uint32_t Q, uint32_t max_distance, uint32_t *nodes, uint32_t *distances,
                         uint32_t *ties, uint32_t *steps, fseq_graph_nearest_row *per_row, fseq_graph_nearest_segment *per_segment, fseq_graph_nearest_summary *summary)
{
	double const t0 = now_ms();
	hipStream_t st = c->stream;
	if (qbsh > c->bsh) return fail(c, FSEQ_E_ARG, "nearest nodes: queries packed narrower than the alignment");
	GraphTables T(c);
	if (int const rc = T.build(true)) return rc;
	size_t const S = T.S;
	std::vector<uint64_t> lb, rb;
	try { lb.resize(S); rb.resize(S); }
	catch (std::bad_alloc const &) { (void) hipStreamSynchronize(st); return fail(c, FSEQ_E_OOM, "nearest nodes: the segments on the host"); }
	for (size_t i = 0; i < S; ++i) { lb[i] = c->segments[i].lb; rb[i] = c->segments[i].rb; }
	GraphNearestPlan P;
	uint64_t const budget = c->tune.graph_nearest_batch > 0 ? (uint64_t) c->tune.graph_nearest_batch : GN_BATCH_BYTES;
	int what = FSEQ_E_ARG;
	if (char const *why = P.build(lb.data(), rb.data(), T.count.data(), S, 8u >> qbsh, budget, &what))
	{
		(void) hipStreamSynchronize(st);
		std::string const msg = std::string("nearest nodes: ") + why;
		return fail(c, what, msg.c_str());
	}
	DevTemp<uint64_t> d_qoff(c), d_roff(c);
	DevTemp<uint32_t> d_rw(c), d_qw(c), d_nodes(c), d_dist(c), d_ties(c), d_adm(c), d_steps(c);
	DevTemp<fseq_graph_nearest_row> d_rows(c);
	DevTemp<fseq_graph_nearest_segment> d_segs(c);
	int rc;
	if ((rc = d_qoff.alloc(S + 1)) || (rc = d_roff.alloc(S + 1)) || (rc = d_rw.alloc((size_t) P.most_rw)) || (rc = d_qw.alloc((size_t) P.most_qw * Q)) ||
	    (rc = d_nodes.alloc(S * Q)) || (rc = d_dist.alloc(S * Q)) || (rc = d_ties.alloc(S * Q)) || (rc = d_adm.alloc(S * Q)) ||
	    (rc = d_steps.alloc(std::max<size_t>(T.pairs, 1) * Q)) || (rc = d_rows.alloc(Q)) || (rc = d_segs.alloc(S)))
	{ (void) hipStreamSynchronize(st); return rc; }
	std::vector<fseq_graph_nearest_row> rows;
	try { rows.resize(Q); }
	catch (std::bad_alloc const &) { (void) hipStreamSynchronize(st); return fail(c, FSEQ_E_OOM, "nearest nodes: the rows' statistics on the host"); }
	GraphNearestArgs A{};
	GraphThreadArgs &G = A.G;
	G.seg_lb = T.d_lb; G.seg_rb = T.d_rb; G.count = T.d_count; G.rep = T.d_rep; G.noff = T.d_noff;
	G.m = (uint32_t) T.m; G.X = T.X; G.S = (uint32_t) S; G.n = c->p.n;
	G.msa = c->d_msa; G.ld = c->ld; G.bsh = c->bsh;
	G.q = q; G.qld = qld; G.qbsh = qbsh; G.Q = Q; G.sigma = c->sigma;
	G.nodes = d_adm; G.steps = d_steps;
	G.edges = T.d_edges; G.offset = T.d_off; G.nedges = T.d_ne; G.pairs = T.pairs; G.n_edges = T.d_edges.base ? T.edges : 0u;
	A.qoff = d_qoff; A.roff = d_roff; A.rw = d_rw; A.qw = d_qw; A.rw_cap = P.most_rw; A.qw_cap = P.most_qw * Q;
	A.max_distance = max_distance; A.nodes = d_nodes; A.distances = d_dist; A.ties = d_ties;
	hipError_t e = hipMemcpyAsync(d_qoff, P.qoff.data(), (S + 1) * 8, hipMemcpyHostToDevice, st);      // (P lives until the synchronisation below)
	if (e == hipSuccess) e = hipMemcpyAsync(d_roff, P.roff.data(), (S + 1) * 8, hipMemcpyHostToDevice, st);
	if (e == hipSuccess) e = hipMemsetAsync(d_adm, 0xFF, S * Q * 4, st);
	if (e == hipSuccess) e = hipMemsetAsync(d_nodes, 0, S * Q * 4, st);
	if (e == hipSuccess) e = hipMemsetAsync(d_dist, 0, S * Q * 4, st);
	if (e == hipSuccess) e = hipMemsetAsync(d_ties, 0, S * Q * 4, st);
	if (e != hipSuccess) { (void) hipStreamSynchronize(st); return fail(c, FSEQ_E_HIP, "nearest nodes: preparation", e); }
	graph_nearest_launch(st, A, P);
	uint32_t const tiles = (uint32_t) std::min<size_t>(((size_t) Q + GT_T - 1) / GT_T, 1024);
	if (T.pairs) hipLaunchKernelGGL(k_gt_steps, dim3(T.pairs, tiles), dim3(GT_T), 0, st, G);
	hipLaunchKernelGGL(k_gn_rows, dim3((Q + GT_T - 1u) / GT_T), dim3(GT_T), 0, st, A, (fseq_graph_nearest_row *) d_rows);
	if (per_segment) hipLaunchKernelGGL(k_gn_segments, dim3((uint32_t) S), dim3(GT_T), 0, st, A, (fseq_graph_nearest_segment *) d_segs);
	e = hipMemcpyAsync(rows.data(), d_rows, (size_t) Q * sizeof(fseq_graph_nearest_row), hipMemcpyDeviceToHost, st);
	if (e == hipSuccess && nodes) e = hipMemcpyAsync(nodes, d_nodes, S * Q * 4, hipMemcpyDeviceToHost, st);
	if (e == hipSuccess && distances) e = hipMemcpyAsync(distances, d_dist, S * Q * 4, hipMemcpyDeviceToHost, st);
	if (e == hipSuccess && ties) e = hipMemcpyAsync(ties, d_ties, S * Q * 4, hipMemcpyDeviceToHost, st);
	if (e == hipSuccess && steps && T.pairs) e = hipMemcpyAsync(steps, d_steps, (size_t) T.pairs * Q * 4, hipMemcpyDeviceToHost, st);
	if (e == hipSuccess && per_segment) e = hipMemcpyAsync(per_segment, d_segs, S * sizeof(fseq_graph_nearest_segment), hipMemcpyDeviceToHost, st);
	hipError_t const es = hipStreamSynchronize(st);                  // (the host arrays are written to here, whatever was queued)
	if (e == hipSuccess) e = es;
	if (e == hipSuccess) e = hipGetLastError();
	if (e != hipSuccess) return fail(c, FSEQ_E_HIP, "nearest nodes", e);
	fseq_graph_nearest_summary sm{};
	sm.rows = Q; sm.segments = S;
	for (fseq_graph_nearest_row const &r : rows)
	{
		sm.segments_admitted += r.segments_admitted; sm.segments_exact += r.segments_exact; sm.junctions_linked += r.junctions_linked;
		sm.junctions_novel += r.junctions_novel; sm.walks += r.walks; sm.mismatches += r.mismatches;
		sm.rows_on_graph += r.walks == 1u && r.longest_walk_segments == S;
	}
	if (per_row) memcpy(per_row, rows.data(), (size_t) Q * sizeof(fseq_graph_nearest_row));
	sm.ms_device = now_ms() - t0;
	if (summary) *summary = sm;
	c->graphnearest.have = true;
	c->graphnearest.info = fseq_graph_nearest_info{P.batches, P.roff[S], P.qoff[S], 8u >> qbsh, 0u};
	return FSEQ_OK;
}

// what the nearest-node entries refuse: the threading's refusals but for its cap of 4,096 classes a segment
static int graph_nearest_refusals(fseq_ctx *c)
{
	if (int const rc = graph_refusals(c)) return rc;
	if (c->idn.have) return fail(c, FSEQ_E_UNSUPPORTED, "nearest nodes: a context made by fseq_create_without_identity_columns (queries in source co-ordinates, with their exception cells, are not served)");
	if (!c->have_input || !c->d_msa) return fail(c, FSEQ_E_ARG, "no alignment resident on the device");
	for (size_t i = 0; i < c->segments.size(); ++i)
		if (c->segments[i].rb - c->segments[i].lb >= 0xFFFFFFFFull) return fail(c, FSEQ_E_UNSUPPORTED, "nearest nodes: a segment of 2^32 - 1 columns or more (distances are 32-bit)");
	return FSEQ_OK;
}

extern "C" {

int fseq_graph_nearest_rows(fseq_ctx *c, uint8_t const *const *rows, uint32_t n_rows, uint32_t max_distance, uint32_t *nodes, uint32_t *distances, uint32_t *ties,
                            uint32_t *steps, fseq_graph_nearest_row *per_row, fseq_graph_nearest_segment *per_segment, fseq_graph_nearest_summary *summary)
{
	if (!c) return FSEQ_E_ARG;
	if (!rows || 0 == n_rows) return fail(c, FSEQ_E_ARG, "nearest nodes: no query rows");
	for (uint32_t i = 0; i < n_rows; ++i)
		if (!rows[i]) return fail(c, FSEQ_E_ARG, "nearest nodes: null query row");
	if (int const rc = graph_nearest_refusals(c)) return rc;
	(void) hipSetDevice(c->p.device);
	// the queries' packing: the narrowest that leaves the code `sigma` free for a byte outside the alphabet (as fseq_graph_thread_rows)
	uint32_t const sigma = c->sigma, bsh = sigma + 1u <= 4u ? 2u : sigma + 1u <= 16u ? 1u : 0u;
	size_t const ld = ((((size_t) n_rows + (1u << bsh) - 1u) >> bsh) + 15) & ~size_t(15);
	DevTemp<uint8_t> d_q(c);                                         // (the call's own: the last match keeps its queries)
	if (int const rc = upload_queries(c, rows, n_rows, bsh, ld, d_q)) return rc;
	return graph_nearest(c, d_q, ld, bsh, n_rows, max_distance, nodes, distances, ties, steps, per_row, per_segment, summary);
}

// the held-out rows are on the device already, column-major and packed at the alignment's width: nothing is uploaded
int fseq_graph_nearest_held_out(fseq_ctx *c, uint32_t max_distance, uint32_t *nodes, uint32_t *distances, uint32_t *ties, uint32_t *steps,
                                fseq_graph_nearest_row *per_row, fseq_graph_nearest_segment *per_segment, fseq_graph_nearest_summary *summary)
{
	if (!c) return FSEQ_E_ARG;
	if (!c->hold.have && !c->idn.have) return fail(c, FSEQ_E_ARG, "not a context made by fseq_create_without_rows");
	if (int const rc = graph_nearest_refusals(c)) return rc;
	if (!c->hold.have || !c->hold.n_held || !c->hold.cols) return fail(c, FSEQ_E_ARG, "not a context made by fseq_create_without_rows");
	(void) hipSetDevice(c->p.device);
	return graph_nearest(c, c->hold.cols, c->hold.ld, c->bsh, c->hold.n_held, max_distance, nodes, distances, ties, steps, per_row, per_segment, summary);
}

int fseq_debug_graph_nearest_info(fseq_ctx *c, fseq_graph_nearest_info *out)
{
	if (!c || !out) return FSEQ_E_ARG;
	if (!c->graphnearest.have) return fail(c, FSEQ_E_ARG, "no fseq_graph_nearest_rows / fseq_graph_nearest_held_out has finished on this context");
	*out = c->graphnearest.info;
	return FSEQ_OK;
}

int fseq_debug_graph_nearest_plan(uint64_t const *lb, uint64_t const *rb, uint32_t const *count, uint64_t n_segments, uint32_t bits, uint64_t budget_bytes,
                                  uint64_t *words, uint64_t *first, uint64_t *n_batches)
{
	if (!words || !first || !n_batches || 0 == budget_bytes) return FSEQ_E_ARG;
	GraphNearestPlan P;
	int what = FSEQ_E_ARG;
	if (P.build(lb, rb, count, n_segments, bits, budget_bytes, &what)) return what;
	std::copy(P.roff.begin(), P.roff.end(), words);
	std::copy(P.first.begin(), P.first.begin() + (size_t) P.batches + 1, first);
	*n_batches = P.batches;
	return FSEQ_OK;
}

int fseq_debug_graph_nearest(int device, uint8_t const *cols, uint64_t ld, uint32_t m, uint64_t n, uint32_t bits, uint64_t const *seg_lb, uint64_t const *seg_rb,
                             uint32_t const *count, uint32_t const *rep, uint32_t S, uint32_t X, uint8_t const *qcols, uint64_t qld, uint32_t Q, uint32_t qbits,
                             uint32_t sigma, uint64_t batch_bytes, uint32_t *nodes, uint32_t *distances, uint32_t *ties, fseq_graph_nearest_info *info)
{
	// whatever a kernel could form an index from, before a device is touched
	if (!cols || !seg_lb || !seg_rb || !count || !rep || !qcols || !nodes || !distances || !ties) return FSEQ_E_ARG;
	if (0 == m || 0 == n || 0 == S || 0 == X || 0 == Q || m > 0x7FFFFFFFu || S > 0x7FFFFFFFu || X > 0xFFFFu) return FSEQ_E_ARG;
	if ((bits != 2 && bits != 4 && bits != 8) || (qbits != 2 && qbits != 4 && qbits != 8) || qbits < bits) return FSEQ_E_ARG;
	uint32_t const bsh = bits == 2 ? 2u : bits == 4 ? 1u : 0u, qbsh = qbits == 2 ? 2u : qbits == 4 ? 1u : 0u;
	if (ld < (((uint64_t) m + (1u << bsh) - 1u) >> bsh) || qld < (((uint64_t) Q + (1u << qbsh) - 1u) >> qbsh)) return FSEQ_E_ARG;
	if (n > (1ull << 40) || ld > (1ull << 32) || qld > (1ull << 32) || (uint64_t) S * Q > (1ull << 34) || (uint64_t) S * X > (1ull << 34)) return FSEQ_E_ARG;
	for (uint32_t s = 0; s < S; ++s)
	{
		if (seg_lb[s] >= seg_rb[s] || seg_rb[s] > n || 0 == count[s] || count[s] > X) return FSEQ_E_ARG;
		for (uint32_t j = 0; j < count[s]; ++j)
			if (rep[(size_t) s * X + j] >= m) return FSEQ_E_ARG;
	}
	GraphNearestPlan P;
	int what = FSEQ_E_ARG;
	if (P.build(seg_lb, seg_rb, count, S, qbits, batch_bytes ? batch_bytes : GN_BATCH_BYTES, &what)) return what;
	if (hipSetDevice(device) != hipSuccess) return FSEQ_E_HIP;
	size_t const cells = (size_t) S * Q;
	void *bufs[12] = {};
	size_t const bytes[12] = {(size_t) (n * ld), (size_t) (n * qld), (size_t) S * 8, (size_t) S * 8, (size_t) S * 4, (size_t) S * X * 4, ((size_t) S + 1) * 4,
	                          ((size_t) S + 1) * 8, ((size_t) S + 1) * 8, (size_t) P.most_rw * 4, (size_t) P.most_qw * Q * 4, cells * 16};
	int rc = FSEQ_E_HIP;
	do
	{
		bool ok = true;
		for (int i = 0; i < 12 && ok; ++i) ok = hipMalloc(&bufs[i], bytes[i]) == hipSuccess;
		if (!ok) { rc = FSEQ_E_OOM; break; }
		if (hipMemcpy(bufs[0], cols, bytes[0], hipMemcpyHostToDevice) != hipSuccess || hipMemcpy(bufs[1], qcols, bytes[1], hipMemcpyHostToDevice) != hipSuccess ||
		    hipMemcpy(bufs[2], seg_lb, bytes[2], hipMemcpyHostToDevice) != hipSuccess || hipMemcpy(bufs[3], seg_rb, bytes[3], hipMemcpyHostToDevice) != hipSuccess ||
		    hipMemcpy(bufs[4], count, bytes[4], hipMemcpyHostToDevice) != hipSuccess || hipMemcpy(bufs[5], rep, bytes[5], hipMemcpyHostToDevice) != hipSuccess ||
		    hipMemset(bufs[6], 0, bytes[6]) != hipSuccess ||             // (noff = 0: the nodes come back as class indices)
		    hipMemcpy(bufs[7], P.qoff.data(), bytes[7], hipMemcpyHostToDevice) != hipSuccess || hipMemcpy(bufs[8], P.roff.data(), bytes[8], hipMemcpyHostToDevice) != hipSuccess ||
		    hipMemset(bufs[11], 0, bytes[11]) != hipSuccess)
			break;
		GraphNearestArgs A{};
		GraphThreadArgs &G = A.G;
		G.seg_lb = (uint64_t const *) bufs[2]; G.seg_rb = (uint64_t const *) bufs[3]; G.count = (uint32_t const *) bufs[4]; G.rep = (uint32_t const *) bufs[5];
		G.noff = (uint32_t const *) bufs[6];
		G.m = m; G.X = X; G.S = S; G.n = n;
		G.msa = (uint8_t const *) bufs[0]; G.ld = (size_t) ld; G.bsh = bsh;
		G.q = (uint8_t const *) bufs[1]; G.qld = (size_t) qld; G.qbsh = qbsh; G.Q = Q; G.sigma = sigma;
		uint32_t *const out = (uint32_t *) bufs[11];
		A.nodes = out; A.distances = out + cells; A.ties = out + 2 * cells; G.nodes = out + 3 * cells;
		A.qoff = (uint64_t const *) bufs[7]; A.roff = (uint64_t const *) bufs[8];
		A.rw = (uint32_t *) bufs[9]; A.qw = (uint32_t *) bufs[10]; A.rw_cap = P.most_rw; A.qw_cap = P.most_qw * Q;
		A.max_distance = 0;
		graph_nearest_launch(nullptr, A, P);
		if (hipGetLastError() != hipSuccess || hipDeviceSynchronize() != hipSuccess) break;
		if (hipMemcpy(nodes, A.nodes, cells * 4, hipMemcpyDeviceToHost) != hipSuccess || hipMemcpy(distances, A.distances, cells * 4, hipMemcpyDeviceToHost) != hipSuccess ||
		    hipMemcpy(ties, A.ties, cells * 4, hipMemcpyDeviceToHost) != hipSuccess)
			break;
		if (info) *info = fseq_graph_nearest_info{P.batches, P.roff[S], P.qoff[S], qbits, 0u};
		rc = FSEQ_OK;
	} while (false);
	for (void *p : bufs) (void) hipFree(p);
	return rc;
}

} // extern "C"

extern "C" {

int fseq_block_graph(fseq_ctx *c, fseq_graph_node *nodes, fseq_graph_edge *edges, uint32_t *row_nodes, fseq_graph_summary *summary)
{
	if (!c) return FSEQ_E_ARG;
	if (int const rc = graph_refusals(c)) return rc;
	(void) hipSetDevice(c->p.device);
	double const t0 = now_ms();
	hipStream_t st = c->stream;
	GraphTables T(c);
	if (int const rc = T.build(edges != nullptr)) return rc;
	size_t const S = T.S, m = T.m;
	uint32_t const X = T.X;
	hipError_t e = hipSuccess;
	std::vector<uint32_t> rep, size, off, ne;
	std::vector<uint2> ew;
	try
	{
		if (nodes) { rep.resize(S * X); size.resize(S * X); }
		if (edges) { off.resize(S); ne.resize(S); ew.resize((size_t) T.edges); }
	}
	catch (std::bad_alloc const &) { (void) hipStreamSynchronize(st); return fail(c, FSEQ_E_OOM, "block graph: the tables on the host"); }
	DevTemp<uint32_t> d_rown(c);
	if (row_nodes)
	{
		if (int const rc = d_rown.alloc(S * m)) { (void) hipStreamSynchronize(st); return rc; }
		uint32_t const tiles = (uint32_t) std::min<size_t>((m + GR_T - 1) / GR_T, 1024);
		hipLaunchKernelGGL(k_graph_row_nodes, dim3((uint32_t) S, tiles), dim3(GR_T), 0, st, T.args(-1), (uint32_t *) d_rown);
		e = hipMemcpyAsync(row_nodes, d_rown, S * m * 4, hipMemcpyDeviceToHost, st);
	}
	if (e == hipSuccess && nodes) e = hipMemcpyAsync(rep.data(), T.d_rep, S * X * 4, hipMemcpyDeviceToHost, st);
	if (e == hipSuccess && nodes) e = hipMemcpyAsync(size.data(), T.d_size, S * X * 4, hipMemcpyDeviceToHost, st);
	if (e == hipSuccess && edges && T.pairs) e = hipMemcpyAsync(off.data(), T.d_off, (size_t) T.pairs * 4, hipMemcpyDeviceToHost, st);
	if (e == hipSuccess && edges && T.pairs) e = hipMemcpyAsync(ne.data(), T.d_ne, (size_t) T.pairs * 4, hipMemcpyDeviceToHost, st);
	if (e == hipSuccess && edges && T.edges) e = hipMemcpyAsync(ew.data(), T.d_edges, (size_t) T.edges * 8, hipMemcpyDeviceToHost, st);
	hipError_t const es = hipStreamSynchronize(st);                  // (the host arrays are written to here, whatever was queued)
	if (e == hipSuccess) e = es;
	if (e == hipSuccess) e = hipGetLastError();
	if (e != hipSuccess) return fail(c, FSEQ_E_HIP, "block graph", e);
	if (nodes)
		for (size_t s = 0; s < S; ++s)
			for (uint32_t j = 0; j < T.count[s]; ++j)
				nodes[(size_t) T.noff[s] + j] = fseq_graph_node{c->segments[s].lb, c->segments[s].rb, (uint32_t) s, j, rep[s * X + j], size[s * X + j]};
	if (edges)
		for (size_t p = 0; p < T.pairs; ++p)
		{
			if ((uint64_t) off[p] + ne[p] > T.edges) return fail(c, FSEQ_E_HIP, "block graph: an edge offset past the edges");
			for (uint32_t k = 0; k < ne[p]; ++k)
			{
				uint2 const w = ew[(size_t) off[p] + k];
				edges[(size_t) off[p] + k] = fseq_graph_edge{T.noff[p] + (w.x >> 16), T.noff[p + 1] + (w.x & 0xFFFFu), w.y, (uint32_t) p};
			}
		}
	if (summary) *summary = fseq_graph_summary{(uint64_t) S, T.nodes, T.edges, now_ms() - t0};
	return FSEQ_OK;
}

} // extern "C"

// fseq_write_block_graph and, restored, fseq_write_block_graph_restored: the same file but for the S lines' labels, LN, lb and rb
static int write_block_graph(fseq_ctx *c, uint32_t flags, int gap_byte, char const *path, bool restored)
{
	if (flags & ~(uint32_t) FSEQ_GRAPH_PATHS) return fail(c, FSEQ_E_ARG, "block graph file: unknown flag bits (FSEQ_GRAPH_PATHS)");
	if (gap_byte > 255) return fail(c, FSEQ_E_ARG, "block graph file: the gap byte is a byte (0 .. 255) or negative for none");
	if (restored && !c->idn.have) return fail(c, FSEQ_E_ARG, "not a context made by fseq_create_without_identity_columns");
	if (int const rc = graph_refusals(c)) return rc;
	if (!c->have_input || !c->d_msa) return fail(c, FSEQ_E_ARG, "no alignment resident on the device");
	(void) hipSetDevice(c->p.device);
	hipStream_t st = c->stream;
	bool const paths = (flags & FSEQ_GRAPH_PATHS) != 0;
	RestoredBounds RB(c);
	GraphRestored R{};
	if (restored)
	{
		if (int const rc = RB.build(c, "restored block graph file")) return rc;
		R = GraphRestored{RB.d_lb, RB.d_rb, c->idn.mask, c->idn.ref, c->idn.n_src};
	}
	GraphTables T(c);
	if (int const rc = T.build(true)) return rc;
	T.d_start.release(c);                                            // (the edge kernel's: not needed from here on)
	size_t const S = T.S, m = T.m;
	uint32_t const X = T.X;
	size_t const X1 = (size_t) X + 1;
	uint64_t const E = T.d_edges.base ? T.edges : 0u;
	size_t const nb = (size_t) ((E + GR_T - 1) / GR_T);              // workgroups of the links
	DevTemp<uint8_t> d_lut(c), d_out(c);
	DevTemp<uint32_t> d_lab(c), d_lens(c);
	DevTemp<uint64_t> d_loff(c), d_segoff(c), d_btot(c), d_boff(c), d_plen(c), d_poff(c);
	int rc;
	if ((rc = d_lut.alloc(256)) || (rc = d_lab.alloc(S * X)) || (rc = d_loff.alloc(S * X1)) || (rc = d_segoff.alloc(S + 1)) ||
	    (rc = d_btot.alloc(nb)) || (rc = d_boff.alloc(nb + 1)) || (rc = d_lens.alloc(GR_T)) ||
	    (paths && ((rc = d_plen.alloc(m)) || (rc = d_poff.alloc(m + 1)))))
	{ (void) hipStreamSynchronize(st); return rc; }
	std::vector<uint64_t> loff, segoff, boff, poff;
	try { loff.resize(S * X1); segoff.resize(S + 1); boff.resize(nb + 1); poff.resize(paths ? m + 1 : 1); }
	catch (std::bad_alloc const &) { (void) hipStreamSynchronize(st); return fail(c, FSEQ_E_OOM, "block graph file: the line offsets on the host"); }
	hipError_t e = hipMemcpyAsync(d_lut, c->code_to_byte, 256, hipMemcpyHostToDevice, st);
	if (e != hipSuccess) { (void) hipStreamSynchronize(st); return fail(c, FSEQ_E_HIP, "block graph file preparation", e); }
	GraphArgs A = T.args(gap_byte);
	A.code_to_byte = d_lut;
	// every line's length, scanned: the nodes inside the segments, then over them; the links inside their workgroups, then over
	// them; the paths over the rows
	if (restored) hipLaunchKernelGGL(k_graph_node_lines<true>, dim3((uint32_t) S), dim3(GR_T), 0, st, A, R, (uint32_t *) d_lab, (uint64_t *) d_loff);
	else hipLaunchKernelGGL(k_graph_node_lines<false>, dim3((uint32_t) S), dim3(GR_T), 0, st, A, R, (uint32_t *) d_lab, (uint64_t *) d_loff);
	hipLaunchKernelGGL(k_segfile_scan, dim3(1), dim3(SF_T), 0, st, (uint64_t const *) d_loff, (uint32_t) S, X, (uint64_t *) d_segoff);
	if (nb) hipLaunchKernelGGL(k_graph_link_lines, dim3((uint32_t) nb), dim3(GR_T), 0, st, A, 0u, (uint64_t *) d_btot, (uint32_t *) nullptr);
	hipLaunchKernelGGL(k_segfile_scan, dim3(1), dim3(SF_T), 0, st, (uint64_t const *) d_btot, (uint32_t) nb, 0u, (uint64_t *) d_boff);
	if (paths)
	{
		hipLaunchKernelGGL(k_graph_path_lines, dim3((uint32_t) ((m + GR_T - 1) / GR_T)), dim3(GR_T), 0, st, A, (uint64_t *) d_plen);
		hipLaunchKernelGGL(k_segfile_scan, dim3(1), dim3(SF_T), 0, st, (uint64_t const *) d_plen, (uint32_t) m, 0u, (uint64_t *) d_poff);
	}
	e = hipMemcpyAsync(loff.data(), d_loff, S * X1 * 8, hipMemcpyDeviceToHost, st);
	if (e == hipSuccess) e = hipMemcpyAsync(segoff.data(), d_segoff, (S + 1) * 8, hipMemcpyDeviceToHost, st);
	if (e == hipSuccess) e = hipMemcpyAsync(boff.data(), d_boff, (nb + 1) * 8, hipMemcpyDeviceToHost, st);
	if (e == hipSuccess && paths) e = hipMemcpyAsync(poff.data(), d_poff, (m + 1) * 8, hipMemcpyDeviceToHost, st);
	hipError_t const es = hipStreamSynchronize(st);
	if (e == hipSuccess) e = es;
	if (e == hipSuccess) e = hipGetLastError();
	if (e != hipSuccess) return fail(c, FSEQ_E_HIP, "block graph file: line lengths", e);
	release_all(c, d_btot, d_plen);
	// batches of whole lines in file order, FSEQ_GRAPH_BATCH bytes at most; a line above the budget is a batch of its own.
	// The nodes' and the paths' are cut here from the lines' offsets; the links' while they are written (a cut inside a
	// workgroup's lines asks the device for their lengths)
	uint64_t const budget = c->tune.graph_batch > 0 ? (uint64_t) c->tune.graph_batch : GRAPH_BATCH_BYTES;
	fseq_ctx::GraphFileStats stats;
	stats.have = true;
	std::vector<SegFileBatch> nbatches;
	std::vector<GraphBatch> pbatches;
	uint64_t most_bytes = 1;
	try
	{
		SegFileBatch cur{};
		bool open = false;
		auto close = [&]() { nbatches.push_back(cur); most_bytes = std::max(most_bytes, cur.bytes); open = false; };
		for (size_t s = 0; s < S; ++s)
		{
			uint64_t const *lo = loff.data() + s * X1;
			for (uint32_t j = 0; j < T.count[s]; ++j)
			{
				uint64_t const len = lo[j + 1] - lo[j];
				if (open && cur.bytes + len > budget) close();
				if (!open) { cur = SegFileBatch{(uint32_t) s, (uint32_t) s, j, j, segoff[s] + lo[j], 0}; open = true; }
				cur.s1 = (uint32_t) s; cur.j_hi = j + 1; cur.bytes += len;
				++stats.lines[0];
			}
		}
		if (open) close();
		for (uint64_t row = 0; paths && row < m;)
		{
			GraphBatch B{row, row, poff[row], 0};
			while (B.last < m && (B.last == B.first || poff[B.last + 1] - B.begin <= budget)) ++B.last;
			B.bytes = poff[B.last] - B.begin;
			most_bytes = std::max(most_bytes, B.bytes);
			pbatches.push_back(B);
			row = B.last;
		}
	}
	catch (std::bad_alloc const &) { return fail(c, FSEQ_E_OOM, "block graph file: the batches on the host"); }
	stats.bytes[0] = segoff[S]; stats.bytes[1] = boff[nb]; stats.bytes[2] = paths ? poff[m] : 0u; stats.lines[1] = E; stats.lines[2] = paths ? m : 0u;
	if (E) most_bytes = std::max<uint64_t>(most_bytes, std::max<uint64_t>(std::min(budget, boff[nb]), GR_LINK_MAX));
	if ((rc = d_out.alloc((size_t) most_bytes))) return rc;
	uint8_t *h_out = nullptr;
	if (hipHostMalloc(reinterpret_cast<void **>(&h_out), (size_t) most_bytes, hipHostMallocDefault) != hipSuccess)
	{
		(void) hipGetLastError();
		return fail(c, FSEQ_E_OOM, "block graph output buffer");
	}
	FILE *f = (path && strcmp(path, "-") != 0) ? fopen(path, "wb") : stdout;
	if (!f) { (void) hipHostFree(h_out); return fail(c, FSEQ_E_ARG, "cannot open the block graph output file"); }
	bool ok = fputs(GRAPH_HEADER, f) >= 0, hip_ok = true;
	// one copy and one write a batch
	auto leave = [&](uint64_t bytes, int section) {
		hip_ok = hipMemcpyAsync(h_out, d_out, (size_t) bytes, hipMemcpyDeviceToHost, st) == hipSuccess && hipStreamSynchronize(st) == hipSuccess && hipGetLastError() == hipSuccess;
		if (hip_ok) ok = fwrite(h_out, 1, (size_t) bytes, f) == (size_t) bytes;
		++stats.batches[section];
	};
	for (size_t b = 0; b < nbatches.size() && ok && hip_ok; ++b)
	{
		SegFileBatch const &B = nbatches[b];
		if (restored) hipLaunchKernelGGL(k_graph_write_nodes<true>, dim3(B.s1 - B.s0 + 1), dim3(GR_T), 0, st, A, R, B, (uint32_t const *) d_lab, (uint64_t const *) d_loff, (uint64_t const *) d_segoff, (uint8_t *) d_out);
		else hipLaunchKernelGGL(k_graph_write_nodes<false>, dim3(B.s1 - B.s0 + 1), dim3(GR_T), 0, st, A, R, B, (uint32_t const *) d_lab, (uint64_t const *) d_loff, (uint64_t const *) d_segoff, (uint8_t *) d_out);
		leave(B.bytes, 0);
	}
	uint32_t lens[GR_T];
	for (uint64_t first = 0, pos = 0; first < E && ok && hip_ok;)
	{
		// the workgroup whose lines the budget ends in: whole workgroups in front of it, its lines one by one
		uint64_t const target = pos + budget;
		size_t const bb = (size_t) (std::upper_bound(boff.begin(), boff.end(), target) - boff.begin()) - 1;      // boff[bb] <= target (boff[block of first] <= pos)
		GraphBatch B{first, E, pos, boff[nb] - pos};
		if (bb < nb)
		{
			hipLaunchKernelGGL(k_graph_link_lines, dim3(1), dim3(GR_T), 0, st, A, (uint32_t) bb, (uint64_t *) nullptr, (uint32_t *) d_lens);
			hip_ok = hipMemcpyAsync(lens, d_lens, sizeof(lens), hipMemcpyDeviceToHost, st) == hipSuccess && hipStreamSynchronize(st) == hipSuccess && hipGetLastError() == hipSuccess;
			if (!hip_ok) break;
			uint64_t i = std::max<uint64_t>(first, (uint64_t) bb * GR_T), p = i == first ? pos : boff[bb];
			uint64_t const i_end = std::min<uint64_t>(E, ((uint64_t) bb + 1) * GR_T);
			while (i < i_end && p + lens[i - (uint64_t) bb * GR_T] <= target) p += lens[i++ - (uint64_t) bb * GR_T];
			if (i == first) p += lens[i++ - (uint64_t) bb * GR_T];      // (a line above the budget: a batch of its own)
			B.last = i; B.bytes = p - pos;
		}
		if (B.bytes > most_bytes || B.last <= B.first) { hip_ok = false; break; }      // (never: a line has at most GR_LINK_MAX bytes)
		uint32_t const g = (uint32_t) ((B.last - 1) / GR_T - B.first / GR_T + 1);
		hipLaunchKernelGGL(k_graph_write_links, dim3(g), dim3(GR_T), 0, st, A, B, (uint64_t const *) d_boff, (uint8_t *) d_out);
		leave(B.bytes, 1);
		first = B.last; pos += B.bytes;
	}
	for (size_t b = 0; b < pbatches.size() && ok && hip_ok; ++b)
	{
		GraphBatch const &B = pbatches[b];
		uint32_t const g = (uint32_t) ((B.last - B.first + GR_TILE - 1) / GR_TILE);
		hipLaunchKernelGGL(k_graph_write_paths, dim3(g), dim3(GR_T), 0, st, A, B, (uint64_t const *) d_poff, (uint8_t *) d_out);
		leave(B.bytes, 2);
	}
	if (fflush(f) != 0) ok = false;
	if (f != stdout) fclose(f);
	(void) hipHostFree(h_out);
	if (!hip_ok) return fail(c, FSEQ_E_HIP, "writing the block graph from the device failed");
	if (!ok) return fail(c, FSEQ_E_ARG, "writing the block graph output file failed");
	c->graphfile = stats;
	return FSEQ_OK;
}

extern "C" {

int fseq_write_block_graph(fseq_ctx *c, uint32_t flags, int gap_byte, char const *path)
{
	if (!c) return FSEQ_E_ARG;
	return write_block_graph(c, flags, gap_byte, path, false);
}

// the S lines in the source's co-ordinates (k_graph_node_lines<true> / k_graph_write_nodes<true>, csrc/fseq_graph.hpp): the
// classes, ids, L and P lines are the reduced graph's -- rows that agree on a segment's kept columns agree on its source range
int fseq_write_block_graph_restored(fseq_ctx *c, uint32_t flags, int gap_byte, char const *path)
{
	if (!c) return FSEQ_E_ARG;
	return write_block_graph(c, flags, gap_byte, path, true);
}

int fseq_debug_graph_file(fseq_ctx *c, fseq_graph_file_stats *out)
{
	if (!c || !out) return FSEQ_E_ARG;
	if (!c->graphfile.have) return fail(c, FSEQ_E_ARG, "no fseq_write_block_graph has finished on this context");
	for (int k = 0; k < 3; ++k) { out->batches[k] = c->graphfile.batches[k]; out->lines[k] = c->graphfile.lines[k]; out->bytes[k] = c->graphfile.bytes[k]; }
	return FSEQ_OK;
}

} // extern "C"
