// fseq_scanplan.hpp -- the order of work of a scan over segment lengths (fseq_scan_segment_lengths, csrc/fseq_lengthscan.hip) as a
// value, made by a pure function: which of the caller's lengths take the long path, in which order the distinct ones are worked
// through, and which entry is filled from which.  Host only: no HIP header, no context -- plain C++17, so that the arithmetic is
// tested without a device (fseq_debug_scan_plan, tests/test_length_scan_abi.py), as plan_reduced is (fseq_redplan.hpp).
#pragma once

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

namespace fseq {

struct ScanPlan {
	std::vector<uint64_t> long_lengths;      // the distinct lengths with n >= 2L, ascending: the lists are folded from each to the next
	std::vector<int32_t> slot;               // [entry] its place in long_lengths; -1: the short path (n < 2L)
	uint32_t n_short = 0;                    // entries on the short path: one sweep serves them all
};

// n < 2L without forming 2L (a length may be any 64-bit number)
inline bool scan_short_path(uint64_t n, uint64_t L) { return L > n / 2u; }

inline ScanPlan plan_length_scan(uint64_t n, uint64_t const *lengths, size_t count)
{
	ScanPlan P;
	for (size_t i = 0; i < count; ++i)
		if (!scan_short_path(n, lengths[i])) P.long_lengths.push_back(lengths[i]);
	std::sort(P.long_lengths.begin(), P.long_lengths.end());
	P.long_lengths.erase(std::unique(P.long_lengths.begin(), P.long_lengths.end()), P.long_lengths.end());
	P.slot.assign(count, -1);
	for (size_t i = 0; i < count; ++i)
	{
		if (scan_short_path(n, lengths[i])) { ++P.n_short; continue; }
		P.slot[i] = (int32_t) (std::lower_bound(P.long_lengths.begin(), P.long_lengths.end(), lengths[i]) - P.long_lengths.begin());
	}
	return P;
}

} // namespace fseq
