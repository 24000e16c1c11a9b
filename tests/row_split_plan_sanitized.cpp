// The plan of a split along the rows (csrc/fseq_rowsplit_plan.hpp) as a program of its own, for AddressSanitizer and
// UndefinedBehaviorSanitizer (tests/test_hold_out_abi.py builds and runs it; nothing here is loaded into Python).  It walks the row
// counts and held patterns of that test, applies every descriptor to a column of known fields and compares with the kept rows, and
// lays the strips of a column too long for one stage, long runs of held-out rows included.
#include "fseq_rowsplit_plan.hpp"

#include <cstdio>
#include <cstdlib>

using namespace fseq;

namespace {

int failures = 0;

void expect(bool ok, char const *what, uint32_t m, uint32_t bits, size_t pattern)
{
	if (ok) return;
	std::fprintf(stderr, "FAILED: %s (m %u, bits %u, pattern %zu)\n", what, m, bits, pattern);
	++failures;
}

// field r of the source column carries r itself (mod 2^bits would lose the row: the check is on row numbers)
void check(uint32_t m, uint32_t bits, std::vector<uint32_t> const &held, size_t pattern)
{
	if (held.empty() || held.size() >= m) return;
	expect(nullptr == row_split_refuse(m, bits, held.data(), held.size()), "the list is in order", m, bits, pattern);
	RowSplitPlan P = row_split_plan(m, bits, held.data(), (uint32_t) held.size());
	uint32_t const per = 32u / bits;
	expect(P.kept.size() + held.size() == m, "kept + held = m", m, bits, pattern);
	expect(P.n_words == (P.kept.size() + per - 1u) / per, "words", m, bits, pattern);
	uint32_t slow = 0;
	for (uint32_t w = 0; w < P.n_words; ++w)
	{
		size_t const q0 = (size_t) w * per, q1 = std::min(P.kept.size(), q0 + per);
		if (!P.keep[w]) { ++slow; expect(P.kept[q1 - 1] - P.kept[q0] >= 2u * per, "a slow word spans more than its window", m, bits, pattern); continue; }
		size_t q = q0;
		for (uint32_t i = 0; i < 2u * per; ++i)
			if (P.keep[w] >> i & 1u) { expect(q < q1 && P.kept[q] == P.base[w] + i, "keep selects the word's rows in order", m, bits, pattern); ++q; }
		expect(q == q1 && (P.keep[w] & 1u), "keep selects all of them, the first at bit 0", m, bits, pattern);
	}
	expect(slow == P.n_slow, "n_slow", m, bits, pattern);
	RowSplitStrips const S = row_split_strips(m, bits, P);
	expect(!S.strips.empty() && S.strips.front().c0 == 0 && S.strips.back().c1 == S.out_chunks && S.tile_cols >= 1, "the strips tile the output chunks", m, bits, pattern);
	uint32_t const rpb = 8u / bits, src_chunks = ((m + rpb - 1u) / rpb + 15u) / 16u;
	for (size_t s = 0; s < S.strips.size(); ++s)
	{
		RowSplitStrip const &t = S.strips[s];
		expect(t.c1 > t.c0 && t.c1 - t.c0 <= RS_STRIP_CHUNKS && (0 == s || t.c0 == S.strips[s - 1].c1), "a strip's chunks", m, bits, pattern);
		expect(t.src_chunks <= RS_STAGE_CHUNKS && t.src0 + t.src_chunks <= src_chunks, "a strip's stage stays inside the column", m, bits, pattern);
		expect(S.tile_cols * (t.src_chunks + 1u) <= RS_STAGE_CHUNKS + 1u && S.tile_cols * (t.c1 - t.c0) <= RS_STAGE_CHUNKS, "a tile fits the LDS arrays", m, bits, pattern);
		for (uint32_t w = 4u * t.c0; w < std::min(P.n_words, 4u * t.c1); ++w)
		{
			if (!P.keep[w]) continue;
			uint32_t const last = P.base[w] + (31u - (uint32_t) __builtin_clz(P.keep[w]));
			expect(P.base[w] / rpb / 16u >= t.src0 && last / rpb / 16u < t.src0 + t.src_chunks, "a fast word's fields are staged", m, bits, pattern);
		}
	}
}

} // namespace

int main()
{
	uint32_t const bits_of[3] = {2, 4, 8};
	std::vector<uint32_t> ms;
	for (uint32_t m = 1; m <= 70; ++m) ms.push_back(m);
	for (uint32_t m : {255u, 256u, 257u, 4097u, 40000u, 300001u}) ms.push_back(m);      // (the last two: columns in several strips)
	for (uint32_t bits : bits_of)
		for (uint32_t m : ms)
		{
			uint32_t const per = 32u / bits, rpb = 8u / bits;
			std::vector<std::vector<uint32_t>> pats;
			pats.push_back({0u});
			pats.push_back({m - 1u});
			pats.push_back({rpb - 1u, rpb, per - 1u, per, 16u * rpb - 1u, 16u * rpb});
			{ std::vector<uint32_t> v; for (uint32_t r = 0; r < m; r += 2) v.push_back(r); pats.push_back(v); }
			{ std::vector<uint32_t> v; for (uint32_t r = 0; r < m; ++r) if (r != m / 2) v.push_back(r); pats.push_back(v); }
			for (uint32_t run : {per, per + 1u, 2u * per + 1u, 70000u})                  // (70,000: more than a stage of source inside one chunk)
				for (uint32_t start : {3u, per})
				{ std::vector<uint32_t> v; for (uint32_t r = start; r < start + run; ++r) v.push_back(r); pats.push_back(v); }
			pats.push_back({m - 1u, 0u, m / 2u});
			for (size_t i = 0; i < pats.size(); ++i)
			{
				// (as the test: what does not exist at this m is dropped)
				std::vector<uint32_t> v;
				std::vector<bool> seen(m, false);
				for (uint32_t r : pats[i])
					if (r < m && !seen[r]) { seen[r] = true; v.push_back(r); }
				check(m, bits, v, i);
			}
		}
	// the refusals
	uint32_t const dup[2] = {1, 1}, big[1] = {5}, ok[1] = {1};
	if (!row_split_refuse(5, 2, dup, 2) || !row_split_refuse(5, 2, big, 1) || !row_split_refuse(5, 2, ok, 0) || !row_split_refuse(1, 2, ok, 1) ||
	    !row_split_refuse(5, 3, ok, 1) || !row_split_refuse(5, 2, nullptr, 1) || row_split_refuse(5, 2, ok, 1))
	{ std::fprintf(stderr, "FAILED: refusals\n"); ++failures; }
	std::printf("%s\n", failures ? "failed" : "ok");
	return failures ? EXIT_FAILURE : EXIT_SUCCESS;
}
