// The bounds of merged segments in the source's co-ordinates (csrc/fseq_restored_bounds.hpp) as a program of its own, for
// AddressSanitizer and UndefinedBehaviorSanitizer (tests/test_segments_restored_cases.py builds and runs it; nothing here is loaded
// into Python).  Every array has exactly the length the function may read or write, so an index formed wrongly leaves it.  Random
// kept columns and tilings are checked against the ownership rule spelled out position by position; then every malformed input
// the function must refuse, each of which would otherwise take kept[] out of bounds or leave a hole in the source.
#include "fseq_restored_bounds.hpp"

#include <cstdio>
#include <cstdlib>
#include <vector>

using namespace fseq;

namespace {

int failures = 0;
uint64_t state = 0x9E3779B97F4A7C15ull;

uint64_t next()
{
	state ^= state << 13; state ^= state >> 7; state ^= state << 17;
	return state;
}

void expect(bool ok, char const *what, uint64_t a, uint64_t b)
{
	if (ok) return;
	std::fprintf(stderr, "FAILED: %s (%llu, %llu)\n", what, (unsigned long long) a, (unsigned long long) b);
	++failures;
}

template <typename K>
void check(uint64_t n_src, uint64_t n, uint64_t S, uint64_t trial)
{
	// n of n_src columns kept (selection sampling), cut into S non-empty segments
	std::vector<K> kept;
	for (uint64_t p = 0, need = n; p < n_src; ++p)
		if (next() % (n_src - p) < need) { kept.push_back((K) p); --need; }
	std::vector<bool> cut(n + 1, false);
	for (uint64_t left = S - 1; left;)
	{
		uint64_t const at = 1 + next() % (n - 1);
		if (!cut[at]) { cut[at] = true; --left; }
	}
	std::vector<uint64_t> lb, rb;
	for (uint64_t c = 0, from = 0; c < n; ++c)
		if (c + 1 == n || cut[c + 1]) { lb.push_back(from); rb.push_back(c + 1); from = c + 1; }
	expect(kept.size() == n && lb.size() == S, "the case itself", n, S);
	std::vector<uint64_t> slb(S, ~0ull), srb(S, ~0ull);
	char const *why = restored_segment_bounds(kept.data(), n, n_src, lb.data(), rb.data(), S, slb.data(), srb.data());
	expect(nullptr == why, "a well-formed input is taken", n_src, trial);
	if (why) return;
	// the owner of every source position: the segment of the last kept column at or in front of it, segment 0 in front of the first
	std::vector<uint64_t> seg_of(n);
	for (uint64_t s = 0; s < S; ++s)
		for (uint64_t c = lb[s]; c < rb[s]; ++c) seg_of[c] = s;
	uint64_t c = 0;
	for (uint64_t p = 0; p < n_src; ++p)
	{
		while (c + 1 < n && (uint64_t) kept[c + 1] <= p) ++c;
		uint64_t const owner = (uint64_t) kept[c] <= p ? seg_of[c] : 0u;
		expect(slb[owner] <= p && p < srb[owner], "a source position lies in its owner's range", p, owner);
	}
	expect(0 == slb[0] && srb[S - 1] == n_src, "the ranges begin at 0 and end at n_src", n_src, trial);
	for (uint64_t s = 1; s < S; ++s) expect(slb[s] == srb[s - 1] && slb[s] < srb[s], "the ranges tile the source", s, trial);
}

bool refused(std::vector<uint64_t> const &kept, uint64_t n_src, std::vector<uint64_t> const &lb, std::vector<uint64_t> const &rb)
{
	std::vector<uint64_t> slb(lb.size() ? lb.size() : 1, 7), srb(slb.size(), 7);
	bool const no = nullptr != restored_segment_bounds(kept.data(), (uint64_t) kept.size(), n_src, lb.data(), rb.data(), (uint64_t) lb.size(), slb.data(), srb.data());
	for (size_t s = 0; s < slb.size(); ++s)
		if (no && (slb[s] != 7 || srb[s] != 7)) return false;       // (a refusal writes nothing)
	return no;
}

} // namespace

int main()
{
	uint64_t trial = 0;
	for (uint64_t n_src : {2ull, 3ull, 64ull, 65ull, 1000ull})
		for (uint64_t n : {2ull, 3ull, 63ull, 64ull, 999ull, 1000ull})
			for (uint64_t S : {1ull, 2ull, 3ull, 17ull})
				if (n <= n_src && S <= n && !(S > 1 && n < 2))
					for (int rep = 0; rep < 8; ++rep)
					{
						check<uint64_t>(n_src, n, S, trial++);
						check<uint32_t>(n_src, n, S, trial++);
					}
	// one kept column, one segment: the whole source
	{
		std::vector<uint32_t> kept{5};
		uint64_t const lb = 0, rb = 1;
		uint64_t slb = 9, srb = 9;
		expect(nullptr == restored_segment_bounds(kept.data(), 1, 9, &lb, &rb, 1, &slb, &srb) && 0 == slb && 9 == srb, "one column", 0, 0);
	}
	std::vector<uint64_t> const kept{1, 4, 5, 9}, lb{0, 2}, rb{2, 4};
	expect(!refused(kept, 10, lb, rb), "the base case of the refusals is in order", 0, 0);
	expect(refused({1, 4, 4, 9}, 10, lb, rb), "kept with an entry twice", 0, 0);
	expect(refused({1, 5, 4, 9}, 10, lb, rb), "kept descending", 0, 0);
	expect(refused({1, 4, 5, 10}, 10, lb, rb), "a kept column at n_src", 0, 0);
	expect(refused({1, 4, 5, ~0ull}, 10, lb, rb), "a kept column far behind n_src", 0, 0);
	expect(refused(kept, 10, {}, {}), "no segments", 0, 0);
	expect(refused(kept, 10, {1, 2}, {2, 4}), "the first segment does not begin at 0", 0, 0);
	expect(refused(kept, 10, {0, 3}, {2, 4}), "a hole between two segments", 0, 0);
	expect(refused(kept, 10, {0, 1}, {2, 4}), "two segments overlap", 0, 0);
	expect(refused(kept, 10, {0, 2}, {2, 3}), "the last segment ends in front of n", 0, 0);
	expect(refused(kept, 10, {0, 2}, {2, 5}), "the last segment ends behind n", 0, 0);
	expect(refused(kept, 10, {0, 5}, {5, 4}), "a border behind n", 0, 0);
	expect(refused(kept, 10, {0, 2, 2}, {2, 2, 4}), "an empty segment", 0, 0);
	expect(refused(kept, 10, {0, ~0ull}, {~0ull, 4}), "a border that wraps", 0, 0);
	expect(refused({}, 10, {0}, {0}), "no kept column", 0, 0);
	{
		uint64_t const l = 0, r = 4;
		uint64_t a = 7, b = 7;
		expect(nullptr != restored_segment_bounds((uint64_t const *) nullptr, 4, 10, &l, &r, 1, &a, &b) &&
		       nullptr != restored_segment_bounds(kept.data(), 4, 10, (uint64_t const *) nullptr, &r, 1, &a, &b) &&
		       nullptr != restored_segment_bounds(kept.data(), 4, 10, &l, &r, 1, (uint64_t *) nullptr, &b) && 7 == a && 7 == b, "NULL arrays", 0, 0);
	}
	std::printf("%s\n", failures ? "failed" : "ok");
	return failures ? EXIT_FAILURE : EXIT_SUCCESS;
}
