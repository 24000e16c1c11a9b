// The range of a kept-column list inside a chunk (csrc/fseq_input_kept_range.hpp) as a program of its own, for AddressSanitizer
// and UndefinedBehaviorSanitizer (tests/test_input_reduced_abi.py builds and runs it; nothing here is loaded into Python).  Every
// list has exactly the length the function may read, so an index formed wrongly leaves it.  Random lists and chunks are checked
// against a count made entry by entry; then the corners: an empty list, chunks in front of, behind and around the whole list,
// a chunk of no columns, a chunk whose end would wrap, and the NULL arguments.
#include "fseq_input_kept_range.hpp"

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
void check_one(std::vector<K> const &kept, uint64_t c0, uint64_t ncols)
{
	uint64_t k0 = ~0ull, k1 = ~0ull;
	char const *why = input_kept_range(kept.data(), (uint64_t) kept.size(), c0, ncols, &k0, &k1);
	expect(nullptr == why, "a well-formed input is taken", c0, ncols);
	if (why) return;
	uint64_t const end = ncols > ~0ull - c0 ? ~0ull : c0 + ncols;
	uint64_t below = 0, inside = 0;
	for (K v : kept)
	{
		if ((uint64_t) v < c0) ++below;
		else if ((uint64_t) v < end) ++inside;
	}
	expect(k0 == below, "k0 is the number of kept columns in front of the chunk", c0, ncols);
	expect(k1 == below + inside, "k1 - k0 is the number of kept columns inside the chunk", c0, ncols);
	expect(k0 <= k1 && k1 <= kept.size(), "the range lies inside the list", k0, k1);
}

template <typename K>
void check(uint64_t n_src, uint64_t n)
{
	std::vector<K> kept;
	for (uint64_t p = 0, need = n; p < n_src; ++p)
		if (next() % (n_src - p) < need) { kept.push_back((K) p); --need; }
	expect(kept.size() == n, "the case itself", n_src, n);
	// every tiling the second pass makes, at a few widths, and random chunks that reach behind the source
	for (uint64_t width : {1ull, 7ull, 16ull, 64ull, 1000ull})
		for (uint64_t c0 = 0; c0 < n_src; c0 += width) check_one(kept, c0, width < n_src - c0 ? width : n_src - c0);
	for (int rep = 0; rep < 64; ++rep) check_one(kept, next() % (n_src + 3), next() % (n_src + 3));
	check_one(kept, 0, n_src);
	check_one(kept, 0, 0);
	check_one(kept, n_src, 5);
	check_one(kept, n_src / 2, ~0ull);                              // (the end is cut off at 2^64 - 1)
	check_one(kept, ~0ull, ~0ull);
}

} // namespace

int main()
{
	for (uint64_t n_src : {1ull, 2ull, 3ull, 64ull, 65ull, 1000ull, 4097ull})
		for (uint64_t n : {0ull, 1ull, 2ull, 63ull, 64ull, 999ull, 1000ull, 4097ull})
			if (n <= n_src)
				for (int rep = 0; rep < 4; ++rep)
				{
					check<uint64_t>(n_src, n);
					check<uint32_t>(n_src, n);
				}
	// the largest 32-bit columns: no arithmetic on a kept column wraps
	check_one(std::vector<uint32_t>{0u, 0xFFFFFFFDu, 0xFFFFFFFEu}, 0xFFFFFFFDull, 2);
	check_one(std::vector<uint32_t>{0u, 0xFFFFFFFDu, 0xFFFFFFFEu}, 1, 0xFFFFFFFFull);
	{
		std::vector<uint32_t> const kept{3, 5};
		uint64_t a = 7, b = 7;
		expect(nullptr != input_kept_range(kept.data(), 2, 0, 9, (uint64_t *) nullptr, &b) && nullptr != input_kept_range(kept.data(), 2, 0, 9, &a, (uint64_t *) nullptr) &&
		       nullptr != input_kept_range((uint32_t const *) nullptr, 2, 0, 9, &a, &b) && 7 == a && 7 == b, "NULL arguments are refused and nothing is written", a, b);
		expect(nullptr == input_kept_range((uint32_t const *) nullptr, 0, 0, 9, &a, &b) && 0 == a && 0 == b, "an empty list needs no array", a, b);
	}
	std::printf("%s\n", failures ? "failed" : "ok");
	return failures ? EXIT_FAILURE : EXIT_SUCCESS;
}
