// fseq_joinscore_host.hpp -- junction support of a join on the host, from boundary states.  Host-only: no
// device, no context (tests/join_score_sanitized.cpp includes it alone).  What k_join_score computes (fseq_joinscore.hpp), for
// any max_segment_size: the fallback of fseq_join_score, the way of sharded runs (fseq_join_score_host on collected states) and
// the CPU tests' subject.
#pragma once

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

namespace fseq {

struct JoinScoreJunction {
	uint64_t weight = 0;
	uint32_t supported = 0, unsupported = 0, gaps = 0, rows_through = 0;
};

struct JoinScoreTotals {
	uint64_t junctions = 0, supported = 0, unsupported = 0, gaps = 0, rows_through = 0, weight = 0, min_junction = 0;
	uint32_t min_rows_through = 0, max_breaks = 0;
};

// the summary of per-junction records and per-slot breaks: the totals, the smallest rows_through and the first junction it is
// at (m and junction 0 where there is no junction), the largest breaks
inline JoinScoreTotals join_score_totals(uint32_t m, uint32_t X, uint64_t pairs, JoinScoreJunction const *junctions, uint32_t const *breaks)
{
	JoinScoreTotals t;
	t.junctions = pairs;
	t.min_rows_through = m;
	for (uint64_t p = 0; p < pairs; ++p)
	{
		JoinScoreJunction const &j = junctions[p];
		t.supported += j.supported; t.unsupported += j.unsupported; t.gaps += j.gaps; t.rows_through += j.rows_through; t.weight += j.weight;
		if (0 == p || j.rows_through < t.min_rows_through) { t.min_rows_through = j.rows_through; t.min_junction = p; }
	}
	for (uint32_t r = 0; r < X; ++r) t.max_breaks = std::max(t.max_breaks, breaks[r]);
	return t;
}

// A, D: S x m boundary states at every segment's rb; lb: the segments' left bounds; perm: S x X, an entry >= m a gap.
// The classes of a segment by the rule of unique_substring_runs (fseq_join.hpp): pBWT position i starts a class iff i == 0 or
// d[i] > lb.  Out: junctions [S - 1] and support [(S - 1) x X] (either may be nullptr), breaks [X] (never nullptr).
// false, with nothing written: a row of a boundary state that is no row (>= m).
inline bool join_score_host(uint32_t m, uint32_t X, uint64_t S, uint64_t const *lb, uint32_t const *A, uint32_t const *D, uint32_t const *perm,
                            JoinScoreJunction *junctions, uint32_t *breaks, uint32_t *support)
{
	for (uint64_t i = 0; i < S * (uint64_t) m; ++i)
		if (A[i] >= m) return false;
	std::fill(breaks, breaks + X, 0u);
	if (S < 2) return true;
	std::vector<uint32_t> cl(m), cr(m);
	std::vector<uint64_t> keys(m);
	auto classes = [&](uint64_t s, std::vector<uint32_t> &of) {
		uint32_t const *a = A + s * (size_t) m, *d = D + s * (size_t) m;
		uint32_t c = 0;
		for (uint32_t i = 0; i < m; ++i)
		{
			if (i && (uint64_t) d[i] > lb[s]) ++c;
			of[a[i]] = c;
		}
	};
	classes(0, cl);
	for (uint64_t p = 0; p + 1 < S; ++p)
	{
		classes(p + 1, cr);
		// the rows' pairs of classes, sorted: a pair's rows are one run
		for (uint32_t i = 0; i < m; ++i) keys[i] = (uint64_t) cl[i] << 32 | cr[i];
		std::sort(keys.begin(), keys.end());
		JoinScoreJunction j;
		uint32_t const *L = perm + p * (size_t) X, *R = L + X;
		std::vector<uint64_t> used;
		for (uint32_t r = 0; r < X; ++r)
		{
			uint32_t sup = 0;
			if (L[r] >= m || R[r] >= m) ++j.gaps;
			else
			{
				uint64_t const key = (uint64_t) cl[L[r]] << 32 | cr[R[r]];
				auto const range = std::equal_range(keys.begin(), keys.end(), key);
				sup = (uint32_t) (range.second - range.first);
				if (sup) { ++j.supported; used.push_back(key); } else { ++j.unsupported; ++breaks[r]; }
				j.weight += sup;
			}
			if (support) support[p * (size_t) X + r] = sup;
		}
		// rows_through: a pair of classes that several slots share counts once
		std::sort(used.begin(), used.end());
		used.erase(std::unique(used.begin(), used.end()), used.end());
		for (uint64_t const key : used)
		{
			auto const range = std::equal_range(keys.begin(), keys.end(), key);
			j.rows_through += (uint32_t) (range.second - range.first);
		}
		if (junctions) junctions[p] = j;
		cl.swap(cr);
	}
	return true;
}

} // namespace fseq
