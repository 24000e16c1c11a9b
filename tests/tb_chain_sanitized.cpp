// The host's check of a caller-supplied lb chain (csrc/fseq_tbcheck.hpp) as a program of its own, for AddressSanitizer and
// UndefinedBehaviorSanitizer (tests/test_merge_list_cases.py builds and runs it; nothing here is loaded into Python).  Every lb
// array has exactly n - L + 1 words, so an index formed wrongly leaves it.  Random good chains are taken with their length, whatever
// stands off the chain; then every way an entry on the chain can be wrong, each of which would send a kernel out of the array or
// round in circles.
#include "fseq_tbcheck.hpp"

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

// a chain from entry n - L with hops of at least L, garbage everywhere else; returns its entries, the last segment first
std::vector<uint64_t> make_chain(uint64_t n, uint64_t L, std::vector<uint32_t> &lb)
{
	lb.assign(n - L + 1, 0);
	for (uint32_t &w : lb)
		switch (next() % 5)
		{
		case 0: w = 0; break;
		case 1: w = 0xFFFFFFFFu; break;
		case 2: w = (uint32_t) (next() % (L ? L : 1)); break;
		case 3: w = (uint32_t) (n + next() % 1000); break;
		default: w = (uint32_t) next(); break;
		}
	std::vector<uint64_t> chain{n - L};
	while (true)
	{
		uint64_t const t = chain.back();
		if (t < L || next() % 7 == 0) { lb[t] = 0; break; }
		uint64_t const v = L + next() % (t - L + 1);                // L <= v <= t
		lb[t] = (uint32_t) v;
		chain.push_back(v - L);
	}
	return chain;
}

void good(uint64_t n, uint64_t L)
{
	std::vector<uint32_t> lb;
	std::vector<uint64_t> const chain = make_chain(n, L, lb);
	uint64_t bad = 7, entries = 7;
	expect(TB_CHAIN_OK == tb_chain_check(lb.data(), n, L, &bad, &entries), "a good chain is taken", n, L);
	expect(entries == chain.size() && bad == ~0ull, "its length is the chain's, and no entry is named", entries, chain.size());
	expect(entries <= n / L + 2, "a chain fits the traceback's room", entries, n / L + 2);
	expect(TB_CHAIN_OK == tb_chain_check(lb.data(), n, L, nullptr, nullptr), "the outputs may be NULL", n, L);
	// break every entry of the chain in turn, every way: the check names that entry
	for (uint64_t t : chain)
	{
		uint32_t const keep = lb[t];
		std::vector<uint32_t> wrong{(uint32_t) (t + 1), (uint32_t) (t + L), 0xFFFFFFFFu, (uint32_t) (n - L + 1), (uint32_t) (n + L)};
		if (L > 1) { wrong.push_back(1); wrong.push_back((uint32_t) (L - 1)); }
		for (uint32_t v : wrong)
		{
			if (v >= L && v <= t) continue;                        // (a valid word after all)
			lb[t] = v;
			uint64_t b = 7, e = 7;
			expect(TB_CHAIN_LB == tb_chain_check(lb.data(), n, L, &b, &e), "a chain entry out of range is refused", t, v);
			expect(b == t && e == 0, "... by its entry, with no length", b, t);
		}
		lb[t] = keep;
	}
	expect(TB_CHAIN_OK == tb_chain_check(lb.data(), n, L, nullptr, nullptr), "the chain restored is good again", n, L);
}

} // namespace

int main()
{
	for (uint64_t L : {1ull, 2ull, 3ull, 7ull, 64ull, 500ull})
	{
		uint64_t const widths[] = {2 * L, 2 * L + 1, 3 * L, 10 * L + 3, 2000 + L};
		for (uint64_t n : widths)
			for (int rep = 0; rep < 6; ++rep)
				good(n, L);
	}
	// every entry, L = 1: the longest chain there is, n entries of n + 2
	{
		uint64_t const n = 5000;
		std::vector<uint32_t> lb(n);
		for (uint64_t t = 0; t < n; ++t) lb[t] = (uint32_t) t;          // lb = t: successor t - 1; lb[0] = 0 ends it
		uint64_t entries = 0;
		expect(TB_CHAIN_OK == tb_chain_check(lb.data(), n, 1, nullptr, &entries) && entries == n, "every entry on the chain", entries, n);
	}
	// the shapes: nothing is read
	{
		std::vector<uint32_t> lb(4, 0);
		uint64_t b = 7, e = 7;
		expect(TB_CHAIN_SHAPE == tb_chain_check(nullptr, 8, 2, &b, &e) && b == ~0ull && e == 0, "no array", 0, 0);
		expect(TB_CHAIN_SHAPE == tb_chain_check(lb.data(), 8, 0, &b, &e), "L == 0", 0, 0);
		expect(TB_CHAIN_SHAPE == tb_chain_check(lb.data(), 7, 4, &b, &e), "n < 2L", 0, 0);
		expect(TB_CHAIN_SHAPE == tb_chain_check(lb.data(), 0xFFFFFFF0ull, 4, &b, &e), "n beyond 32-bit entries", 0, 0);
		expect(TB_CHAIN_SHAPE == tb_chain_check(lb.data(), 8, (1ull << 63) + 1, &b, &e), "an L whose double wraps to 2", 0, 0);
	}
	std::printf("%s\n", failures ? "failed" : "ok");
	return failures ? EXIT_FAILURE : EXIT_SUCCESS;
}
