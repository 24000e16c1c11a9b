// fseq_tbcheck.hpp -- whether the traceback kernels may follow a caller-supplied lb array (fseq_debug_merge_on_lists,
// csrc/fseq_api_debug.hip; fseq_debug_traceback_parts, csrc/fseq_path_dp.hip), decided by one pure function before a
// runtime call is made.
// Host only: no HIP header, no context -- plain C++17, so that the walk is tested without a device and under the host
// sanitizers (tests/tb_chain_sanitized.cpp), as restored_segment_bounds (fseq_restored_bounds.hpp) and input_kept_range
// (fseq_input_kept_range.hpp) are.
//
// lb[0 .. n - L] is the DP's lb array for n columns at segment length L, n >= 2L.  Only the chain from entry n - L is held
// to anything: an entry t on it has lb == 0 (the chain ends there) or L <= lb <= t (its successor lb - L lies at least L
// entries below it), and the chain ends within n / L + 2 entries -- the room the traceback's output has.  What stands in
// the entries off the chain is the caller's: the kernels take any word there (tb_next, fseq_kernels.hpp).
#pragma once

#include <cstddef>
#include <cstdint>

namespace fseq {

enum { TB_CHAIN_OK = 0, TB_CHAIN_SHAPE = 1, TB_CHAIN_LB = 2, TB_CHAIN_LONG = 3 };

// TB_CHAIN_OK and *entries = the chain's length, or what is wrong: TB_CHAIN_SHAPE (no array, L == 0, n < 2L, n beyond what
// 32-bit entries index), TB_CHAIN_LB (*bad_entry's lb is neither 0 nor in L .. *bad_entry), TB_CHAIN_LONG (*bad_entry is
// the entry the chain stood at when its room ran out).  bad_entry / entries may be nullptr.
inline int tb_chain_check(uint32_t const *lb, uint64_t n, uint64_t L, uint64_t *bad_entry, uint64_t *entries)
{
	if (bad_entry) *bad_entry = ~0ull;
	if (entries) *entries = 0;
	if (!lb || 0 == L || L > n / 2 || n >= 0xFFFFFFF0ull) return TB_CHAIN_SHAPE;      // (n / 2: 2 L may wrap)
	uint64_t const room = n / L + 2;
	uint64_t t = n - L;
	for (uint64_t count = 1; count <= room; ++count)
	{
		uint64_t const v = lb[t];
		if (0 == v)
		{
			if (entries) *entries = count;
			return TB_CHAIN_OK;
		}
		if (v < L || v > t)
		{
			if (bad_entry) *bad_entry = t;
			return TB_CHAIN_LB;
		}
		t = v - L;                                              // (<= t - L: the chain descends)
	}
	if (bad_entry) *bad_entry = t;
	return TB_CHAIN_LONG;
}

} // namespace fseq
