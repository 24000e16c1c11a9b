// fseq_input_kept_range.hpp -- which entries of the kept-column list fall inside a chunk of source columns: what the second pass
// of the reduced chunked input (fseq_input_columns_kept, csrc/fseq_api_input.hip) encodes of a chunk and what
// fseq_input_kept_columns answers, made by one pure function.
// Host only: no HIP header, no context -- plain C++17, so that the arithmetic is tested without a device
// (fseq_debug_input_kept_range, tests/test_input_reduced_abi.py) and under the host sanitizers
// (tests/input_kept_range_sanitized.cpp), as restored_segment_bounds is (fseq_restored_bounds.hpp).
//
// kept[0 .. n_kept) are source columns, strictly ascending.  The chunk is [c0, c0 + ncols), cut off at 2^64 - 1 where the sum
// would wrap.  [*k0, *k1) are the entries with c0 <= kept[k] < c0 + ncols: *k0 the first entry not below c0, *k1 the first not
// below the chunk's end, each found by a binary search that reads kept[] at indices below n_kept only.  No kept column in
// the chunk: *k0 == *k1 (the place in the list where one would stand).
#pragma once

#include <cstddef>
#include <cstdint>

namespace fseq {

// the first k in [lo, n_kept) with kept[k] >= col (n_kept: none)
template <typename K>
inline uint64_t input_kept_lower_bound(K const *kept, uint64_t lo, uint64_t n_kept, uint64_t col)
{
	uint64_t hi = n_kept;
	while (lo < hi)
	{
		uint64_t const mid = lo + (hi - lo) / 2;                     // (lo <= mid < hi <= n_kept)
		if ((uint64_t) kept[mid] < col) lo = mid + 1;
		else hi = mid;
	}
	return lo;
}

// nullptr, or why nothing was written
template <typename K>
inline char const *input_kept_range(K const *kept, uint64_t n_kept, uint64_t c0, uint64_t ncols, uint64_t *k0, uint64_t *k1)
{
	if (!k0 || !k1) return "no room for the range";
	if (!kept && n_kept) return "no kept columns";
	uint64_t const end = ncols > ~0ull - c0 ? ~0ull : c0 + ncols;
	uint64_t const a = input_kept_lower_bound(kept, 0, n_kept, c0);
	*k0 = a;
	*k1 = input_kept_lower_bound(kept, a, n_kept, end);          // (end >= c0: the second search starts where the first ended)
	return nullptr;
}

} // namespace fseq
