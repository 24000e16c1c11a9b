// fseq_restored_bounds.hpp -- the merged segments of an identity-reduced context (fseq_create_without_identity_columns,
// csrc/fseq_api_identity.hip) in the SOURCE's co-ordinates, made by one pure function: what fseq_get_segments_restored reports
// and fseq_write_segments_restored prints and fills (csrc/fseq_api_join.hip, csrc/fseq_segfile.hpp).
// Host only: no HIP header, no context -- plain C++17, so that the arithmetic is tested without a device
// (fseq_debug_restored_bounds, tests/test_segments_restored_cases.py) and under the host sanitizers
// (tests/restored_bounds_sanitized.cpp), as row_split_plan is (fseq_rowsplit_plan.hpp).
//
// kept[0 .. n) are the source columns of the context's columns, strictly ascending and below n_src.  The merged segments
// [lb_s, rb_s), s < S, tile [0, n).  Segment s owns the source positions from its first kept column up to the next segment's
// first kept column -- the rule of the restored split walk (csrc/fseq_api_match.hip) --, segment 0 those in front of kept[0] as
// well, the last one those behind kept[n - 1]:
//   src_lb_0 = 0,          src_lb_s = kept[lb_s]  (s > 0)
//   src_rb_{S-1} = n_src,  src_rb_s = kept[rb_s]  (s < S - 1)
// So the identity columns behind a segment's last kept column are that segment's, and the ranges tile [0, n_src).
#pragma once

#include <cstddef>
#include <cstdint>

namespace fseq {

// what restored_segment_bounds refuses, before it forms an index: nullptr where the input is in order
template <typename K>
inline char const *restored_bounds_refuse(K const *kept, uint64_t n, uint64_t n_src, uint64_t const *lb, uint64_t const *rb, uint64_t S)
{
	if (!kept || !lb || !rb) return "no kept columns or no segments";
	if (0 == S) return "no segments";
	if (0 == n) return "no kept columns";
	if (n > n_src) return "more kept columns than source columns";
	for (uint64_t j = 0; j < n; ++j)
	{
		if ((uint64_t) kept[j] >= n_src) return "a kept column is not below the source's column count";
		if (j && kept[j] <= kept[j - 1]) return "the kept columns do not ascend strictly";
	}
	for (uint64_t s = 0; s < S; ++s)
	{
		if (lb[s] != (s ? rb[s - 1] : 0u)) return "the segments do not tile the kept columns (a segment does not begin where the one in front ends)";
		if (rb[s] <= lb[s]) return "the segments do not tile the kept columns (an empty segment)";
		if (rb[s] > n) return "the segments do not tile the kept columns (a segment ends behind the last kept column)";
	}
	if (rb[S - 1] != n) return "the segments do not tile the kept columns (the last one does not end at the last kept column)";
	return nullptr;
}

// src_lb[s], src_rb[s], s < S; nullptr, or why nothing was written
template <typename K>
inline char const *restored_segment_bounds(K const *kept, uint64_t n, uint64_t n_src, uint64_t const *lb, uint64_t const *rb, uint64_t S,
                                           uint64_t *src_lb, uint64_t *src_rb)
{
	if (!src_lb || !src_rb) return "no room for the bounds";
	if (char const *why = restored_bounds_refuse(kept, n, n_src, lb, rb, S)) return why;
	for (uint64_t s = 0; s < S; ++s)
	{
		src_lb[s] = s ? (uint64_t) kept[lb[s]] : 0u;                 // (0 < lb[s] < n: the segments tile and none is empty)
		src_rb[s] = s + 1 < S ? (uint64_t) kept[rb[s]] : n_src;      // (rb[s] = lb[s + 1] < n)
	}
	return nullptr;
}

} // namespace fseq
