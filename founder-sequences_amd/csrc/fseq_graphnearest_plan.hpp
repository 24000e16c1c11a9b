// fseq_graphnearest_plan.hpp -- how fseq_graph_nearest_rows / _held_out (csrc/fseq_graphnearest.hpp, csrc/fseq_api_graph.hip) lay
// out their packed words and cut the segments into batches.  Host only and pure: no device, no context, nothing but <cstdint>, so
// that it is tested on its own (fseq_debug_graph_nearest_plan, tests/test_graph_nearest_abi.py) and under the host sanitizers
// (tests/graph_nearest_plan_sanitized.cpp), as restored_segment_bounds is (fseq_restored_bounds.hpp).
//
// Segment s of [lb[s], rb[s]) columns takes nw(s) = ceil((rb[s] - lb[s]) / (32 / bits)) words a row at `bits` bits a code: every
// segment starts on a word boundary.  qoff[s] is the sum of nw over the segments in front of s (the queries' words, a query),
// roff[s] the sum of count[s'] * nw(s') (the class representatives' words).  A batch is a run of whole segments whose
// representatives' words take at most budget_bytes; a segment above the budget is a batch of its own.
#pragma once

#include <cstdint>

namespace fseq {

constexpr uint64_t GN_BATCH_BYTES = 256ull << 20;        // the budget by itself (FSEQ_GRAPH_NEAREST_BATCH)

// qoff and roff have S + 1 entries each.  nullptr, or why the input is refused -- with nothing written: no segments, a NULL array,
// bits not 2, 4 or 8, a segment that is empty or runs backwards, a segment of 2^32 - 1 columns or more (distances are 32-bit), a
// segment without a class, a sum that leaves 64 bits.
inline char const *graph_nearest_words(uint64_t const *lb, uint64_t const *rb, uint32_t const *count, uint64_t S, uint32_t bits, uint64_t *qoff, uint64_t *roff)
{
	if (!lb || !rb || !count || !qoff || !roff) return "a NULL array";
	if (0 == S) return "no segments";
	if (bits != 2 && bits != 4 && bits != 8) return "codes of 2, 4 or 8 bits";
	uint64_t const cpw = 32u / bits, limit = ~0ull / 8u;             // (sums stay below 2^61: their byte counts fit 64 bits)
	uint64_t q = 0, r = 0;
	for (uint64_t s = 0; s < S; ++s)
	{
		if (lb[s] >= rb[s]) return "a segment that is empty or runs backwards";
		uint64_t const len = rb[s] - lb[s];
		if (len >= 0xFFFFFFFFull) return "a segment of 2^32 - 1 columns or more";
		if (0 == count[s]) return "a segment without a class";
		uint64_t const nw = (len + cpw - 1) / cpw;                   // (< 2^30)
		if (nw * count[s] > limit - r || nw > limit - q) return "more packed words than 64 bits count";
		q += nw; r += nw * count[s];
	}
	q = r = 0;
	for (uint64_t s = 0; s < S; ++s)
	{
		uint64_t const nw = (rb[s] - lb[s] + cpw - 1) / cpw;
		qoff[s] = q; roff[s] = r;
		q += nw; r += nw * count[s];
	}
	qoff[S] = q; roff[S] = r;
	return nullptr;
}

// The batches from roff (ascending, roff[0] = 0): batch b is the segments [first[b], first[b + 1]), first has S + 1 entries of
// which *n_batches + 1 are written (first[0] = 0, first[*n_batches] = S).  nullptr, or why the input is refused with nothing
// written: a NULL array, no segments, a budget of 0 bytes, offsets that do not ascend or do not start at 0.
inline char const *graph_nearest_plan(uint64_t const *roff, uint64_t S, uint64_t budget_bytes, uint64_t *first, uint64_t *n_batches)
{
	if (!roff || !first || !n_batches) return "a NULL array";
	if (0 == S) return "no segments";
	if (0 == budget_bytes) return "a budget of 0 bytes";
	if (roff[0] != 0) return "offsets that do not start at 0";
	for (uint64_t s = 0; s < S; ++s)
		if (roff[s + 1] < roff[s]) return "offsets that do not ascend";
	uint64_t const budget = budget_bytes / 4u;                       // words
	uint64_t nb = 0;
	for (uint64_t s = 0; s < S;)
	{
		uint64_t e = s + 1;                                          // (a segment above the budget: a batch of its own)
		while (e < S && roff[e + 1] - roff[s] <= budget) ++e;
		first[nb++] = s;
		s = e;
	}
	first[nb] = S;
	*n_batches = nb;
	return nullptr;
}

} // namespace fseq
