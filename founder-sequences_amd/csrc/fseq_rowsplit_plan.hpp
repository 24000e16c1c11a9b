// fseq_rowsplit_plan.hpp -- the plan of a split of a resident alignment along its rows (fseq_create_without_rows,
// csrc/fseq_api_rowsplit.hip) as a value, made by pure functions: which rows are kept, from which source fields every 32-bit word
// of a kept column is put together, and in which strips of output words a column too long for the kernel's LDS is taken.
// Host only: no HIP header, no context -- plain C++17, so that the arithmetic is tested without a device
// (fseq_debug_row_split_plan, tests/test_hold_out_abi.py) and under the host sanitizers, as plan_length_scan is (fseq_scanplan.hpp).
//
// A column is packed at `bits` = 2, 4 or 8 bits a row, per = 32 / bits rows a word.  Output word w of a kept column holds the kept
// rows w per .. w per + per - 1; their source rows ascend.  base[w] is the first of them; the word's WINDOW is the 2 per source
// fields from base[w] on (64 bits); keep[w] has bit i set iff source row base[w] + i is one of the word's rows, so the word is
// the window's fields compressed by keep.  The last word may hold fewer than per rows: fewer bits are set and its upper fields
// come out as zeros.  A word whose rows span more than 2 per source rows (more than per rows in a row are held out inside its
// span) has keep = 0 -- impossible otherwise, bit 0 is always set -- and is built field by field from kept[]: a SLOW word.
#pragma once

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

namespace fseq {

constexpr uint32_t RS_STAGE_CHUNKS = 512;            // 16-byte chunks of source a workgroup of k_rows_split stages at a time (8 KiB)
constexpr uint32_t RS_STRIP_CHUNKS = 512;            // most 16-byte chunks of output a strip writes per column (2,048 descriptors in LDS)
constexpr uint32_t RS_PAD_WORD = 0xFFFFFFFFu;        // base of a descriptor behind the last word of a column: the word is zero

struct RowSplitPlan {
	std::vector<uint32_t> kept;              // the rows that stay, ascending
	std::vector<uint32_t> base, keep;        // [n_words] the descriptors
	uint32_t n_words = 0, n_slow = 0;
};

// what fseq_create_without_rows refuses of a held list, before anything is allocated: nullptr where the list is in order
inline char const *row_split_refuse(uint32_t m, uint32_t bits, uint32_t const *held, uint64_t n_held)
{
	if (bits != 2u && bits != 4u && bits != 8u) return "the code width must be 2, 4 or 8 bits";
	if (!held) return "no list of held-out rows";
	if (0 == n_held) return "no row is held out";
	if (n_held >= m) return "the held-out rows leave no row to segment (n_held must be between 1 and m - 1)";
	std::vector<bool> seen(m, false);
	for (uint64_t q = 0; q < n_held; ++q)
	{
		if (held[q] >= m) return "a held-out row index is not below m";
		if (seen[held[q]]) return "a row is held out twice";
		seen[held[q]] = true;
	}
	return nullptr;
}

// (the list has passed row_split_refuse)
inline RowSplitPlan row_split_plan(uint32_t m, uint32_t bits, uint32_t const *held, uint32_t n_held)
{
	RowSplitPlan P;
	uint32_t const per = 32u / bits;
	std::vector<bool> out(m, false);
	for (uint32_t q = 0; q < n_held; ++q) out[held[q]] = true;
	P.kept.reserve(m - n_held);
	for (uint32_t r = 0; r < m; ++r)
		if (!out[r]) P.kept.push_back(r);
	size_t const nk = P.kept.size();
	P.n_words = (uint32_t) ((nk + per - 1u) / per);
	P.base.resize(P.n_words);
	P.keep.resize(P.n_words);
	for (uint32_t w = 0; w < P.n_words; ++w)
	{
		size_t const q0 = (size_t) w * per, q1 = std::min(nk, q0 + per);
		uint32_t const b = P.kept[q0];
		P.base[w] = b;
		if (P.kept[q1 - 1] - b >= 2u * per) { P.keep[w] = 0; ++P.n_slow; continue; }
		uint32_t k = 0;
		for (size_t q = q0; q < q1; ++q) k |= 1u << (P.kept[q] - b);
		P.keep[w] = k;
	}
	return P;
}

// The strips: a workgroup of k_rows_split takes the output chunks [c0, c1) (16 bytes = 4 words each) of its columns and stages
// the source chunks [src0, src0 + src_chunks) of them, which hold every field the windows of its fast words select.  Output
// words map to ascending source ranges, so the strips' source ranges ascend too and overlap by a chunk at most.
struct RowSplitStrip { uint32_t c0, c1, src0, src_chunks; };
struct RowSplitStrips {
	std::vector<RowSplitStrip> strips;
	bool whole = false;                      // one strip that stages the whole column: the held-out rows are gathered from the staged bytes too
	uint32_t out_chunks = 0;                 // 16-byte chunks of a kept column (its ld / 16)
	uint32_t demoted = 0;                    // fast words made slow because the four words of their chunk alone span more than a stage
	uint32_t tile_cols = 1;                  // columns a workgroup takes at a time
};

// (P.keep may change: words are demoted where a chunk of four spans more than RS_STAGE_CHUNKS of source, which takes a run of
// more than 8 KiB of held-out rows inside the chunk)
inline RowSplitStrips row_split_strips(uint32_t m, uint32_t bits, RowSplitPlan &P)
{
	RowSplitStrips S;
	uint32_t const rpb_sh = bits == 2u ? 2u : bits == 4u ? 1u : 0u;      // rows a byte, as a shift
	uint32_t const src_bytes = (m + (1u << rpb_sh) - 1u) >> rpb_sh, src_chunks = (src_bytes + 15u) / 16u;
	S.out_chunks = (P.n_words + 3u) / 4u;
	auto finish = [&]() {
		uint32_t sc = 0, oc = 0;
		for (auto const &s : S.strips) { sc = std::max(sc, s.src_chunks); oc = std::max(oc, s.c1 - s.c0); }
		S.tile_cols = std::max(1u, std::min(RS_STAGE_CHUNKS / (sc + 1u), RS_STAGE_CHUNKS / std::max(oc, 1u)));
	};
	if (src_chunks <= RS_STAGE_CHUNKS)
	{
		S.whole = true;
		S.strips.push_back(RowSplitStrip{0u, S.out_chunks, 0u, src_chunks});
		finish();
		return S;
	}
	RowSplitStrip cur{0u, 0u, 0u, 0u};
	bool have = false;                       // the strip under way has a source range
	uint32_t lo = 0, hi = 0;
	auto close = [&](uint32_t c1) {
		cur.c1 = c1;
		cur.src0 = have ? lo : 0u;
		cur.src_chunks = have ? hi - lo + 1u : 0u;
		S.strips.push_back(cur);
		cur = RowSplitStrip{c1, c1, 0u, 0u};
		have = false;
	};
	for (uint32_t c = 0; c < S.out_chunks; ++c)
	{
		// the source chunks the fast words of this output chunk select fields from
		bool any = false;
		uint32_t glo = 0, ghi = 0;
		uint32_t const w1 = std::min(P.n_words, 4u * c + 4u);
		for (uint32_t w = 4u * c; w < w1; ++w)
		{
			if (!P.keep[w]) continue;
			uint32_t const last = P.base[w] + (31u - (uint32_t) __builtin_clz(P.keep[w]));
			uint32_t const a = (P.base[w] >> rpb_sh) / 16u, b = (last >> rpb_sh) / 16u;
			glo = any ? std::min(glo, a) : a;
			ghi = any ? std::max(ghi, b) : b;
			any = true;
		}
		if (any && ghi - glo + 1u > RS_STAGE_CHUNKS)
		{
			for (uint32_t w = 4u * c; w < w1; ++w)
				if (P.keep[w]) { P.keep[w] = 0; ++P.n_slow; ++S.demoted; }
			any = false;
		}
		bool const full = c - cur.c0 >= RS_STRIP_CHUNKS;
		bool const wide = any && have && std::max(hi, ghi) - std::min(lo, glo) + 1u > RS_STAGE_CHUNKS;
		if (c > cur.c0 && (full || wide)) close(c);
		if (any)
		{
			lo = have ? std::min(lo, glo) : glo;
			hi = have ? std::max(hi, ghi) : ghi;
			have = true;
		}
	}
	close(S.out_chunks);
	finish();
	return S;
}

} // namespace fseq
