// fseq_lengthscan.hpp -- k_relump_lists: the per-column lists of phase C, built at one segment length, folded in place to what
// the DP reads at a larger one (the scan over segment lengths, csrc/fseq_lengthscan.hip).
//
// A column's list depends on the segment length L only through its first entry, the lump: columns_body (fseq_kernels.hpp, "emit
// the top of the histogram") puts every divergence value >= thr = k + 2 - L there and takes the distinct values below thr,
// descending, behind it.  For L' > L the threshold only moves down: the list for L' is the list for L with the leading entries
// whose value is >= k + 2 - L' joined to the lump.  The DP clips every value to the same bound anyway (dp_strip / dp_cell_pair), so
// the folded list is exactly what k_dp expects, and its cell-pair path, which looks at 32 entries, keeps holding.  The header's
// cumulative count, `complete` and the count of value 0 are those of the whole list and do not change.  A folded list reaches
// less far below its threshold than one built at L' with the same capacity; the DP tells where that is not enough
// (PathWords::dp[0] bit 0, DpSpecArgs::ovf), so exactness never rests on the folding.  One corner is not a prefix of the list
// built at L': where the capacity cut the list short and every entry it holds joins the lump, further values >= the new
// threshold may lie behind the cut, and the lone lump holds a lower bound of its count.  Such a list is incomplete and offers
// the DP no candidate, so the cell is flagged unproven and the lists are built at that length (tests/test_proto_length_scan.py).
//
// One wave per column, RELUMP_WAVES columns per workgroup; plain vector loads and stores, no atomics, no LDS.  The entries are 8
// bytes and a list starts at an even entry (the stride is even), so entry 1, where the strips start, is 8-byte aligned and no
// more: a lane loads one entry (8 bytes), a wave 512 contiguous bytes per strip of 64 entries.
#pragma once

#include "fseq_core.hpp"
#include "fseq_types.hpp"

namespace fseq {

constexpr int RELUMP_WAVES = 4;

static __global__ __launch_bounds__(64 * RELUMP_WAVES) void k_relump_lists(uint2 *ent, uint4 *hdr, uint32_t stride, uint32_t L_to, uint64_t k0, uint64_t ncols)
{
	uint64_t const j = (uint64_t) blockIdx.x * RELUMP_WAVES + wave_id();
	if (j >= ncols) return;                                       // (wave-uniform)
	uint64_t const k = k0 + j;
	uint32_t const lane = lane_id();
	uint32_t const nent = hdr[k].x;
	// (a header phase C has not written -- FSEQ_POISON_LISTS, a column outside a window -- forms no index)
	if (nent < 2u || nent > stride) return;
	uint32_t const thr = (k + 2 > (uint64_t) L_to) ? (uint32_t) (k + 2 - L_to) : 0u;
	uint2 *const out = ent + k * (size_t) stride;
	// E: the entries from index 1 on whose value is >= thr -- a prefix, the values descend (the entry of value 0 is among them
	// only where thr == 0, as the writer's `if (thr == 0u) R += cnt0`); moved: their counts
	uint32_t E = 0, moved = 0;
	for (uint32_t base = 1u; base < nent; base += 64u)
	{
		uint32_t const i = base + lane;
		bool const in = i < nent;
		uint2 const e = in ? out[i] : make_uint2(0u, 0u);
		bool const mv = in && e.x >= thr;
		unsigned long long const b = __ballot(mv);
		E += (uint32_t) __popcll(b);
		moved += readlane_u32(wave_incl_add(mv ? e.y : 0u), 63);
		if (b != __ballot(in)) break;                             // the prefix ends inside this strip
	}
	if (E == 0u) return;                                          // nothing is written: the column cost its header and one strip
	// the rest moves down by E: strips ascending, a strip's entries in registers before any of them is stored (a lane's store
	// takes the lane's own load, so the wave's loads of a strip have all returned when its stores are issued; a later strip
	// reads behind everything written so far)
	uint32_t const keep = nent - 1u - E;
	for (uint32_t base = 0u; base < keep; base += 64u)
	{
		uint32_t const i = base + lane;
		if (i < keep)
		{
			uint2 const e = out[1u + E + i];
			out[1u + i] = e;
		}
	}
	if (lane == 0u)
	{
		uint2 lump = out[0];
		lump.y += moved;
		out[0] = lump;
		reinterpret_cast<uint32_t *>(hdr + k)[0] = nent - E;      // (the other header words stay; so do the entries behind the new end:
		                                                          // the DP masks by the entry count, its strip loads read into the padding as before)
	}
}

} // namespace fseq
