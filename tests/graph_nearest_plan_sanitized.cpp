// The packed-word layout and the batch cut of fseq_graph_nearest_rows (csrc/fseq_graphnearest_plan.hpp) as a program of its own,
// for AddressSanitizer and UndefinedBehaviorSanitizer (tests/test_graph_nearest_abi.py builds and runs it; nothing here is loaded
// into Python).  Every array has exactly the length the functions may read or write, so an index formed wrongly leaves it.  Random
// segments are checked against the rules spelled out segment by segment; then every malformed input the functions must refuse.
#include "fseq_graphnearest_plan.hpp"

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

void check(uint64_t S, uint32_t bits, uint64_t budget, uint64_t widest, uint64_t trial)
{
	std::vector<uint64_t> lb(S), rb(S);
	std::vector<uint32_t> count(S);
	uint64_t at = next() % 5;
	for (uint64_t s = 0; s < S; ++s)
	{
		lb[s] = at; at += 1 + next() % widest; rb[s] = at;
		count[s] = 1 + (uint32_t) (next() % 9);
	}
	std::vector<uint64_t> qoff(S + 1, ~0ull), roff(S + 1, ~0ull), first(S + 1, ~0ull);
	uint64_t nb = ~0ull;
	char const *why = graph_nearest_words(lb.data(), rb.data(), count.data(), S, bits, qoff.data(), roff.data());
	expect(nullptr == why, "a well-formed input is taken", S, trial);
	if (why) return;
	uint64_t const cpw = 32u / bits;
	expect(0 == qoff[0] && 0 == roff[0], "the offsets start at 0", S, trial);
	for (uint64_t s = 0; s < S; ++s)
	{
		uint64_t const nw = qoff[s + 1] - qoff[s];
		expect(nw * cpw >= rb[s] - lb[s] && (nw - 1) * cpw < rb[s] - lb[s], "a segment's words hold its columns and no word more", s, trial);
		expect(roff[s + 1] - roff[s] == nw * count[s], "a class takes the segment's words", s, trial);
	}
	why = graph_nearest_plan(roff.data(), S, budget, first.data(), &nb);
	expect(nullptr == why && nb >= 1 && nb <= S, "the plan is taken", S, trial);
	if (why) return;
	expect(0 == first[0] && S == first[nb], "the batches begin at 0 and end at S", S, trial);
	for (uint64_t b = 0; b < nb; ++b)
	{
		expect(first[b] < first[b + 1], "a batch holds a segment", b, trial);
		uint64_t const bytes = (roff[first[b + 1]] - roff[first[b]]) * 4u;
		expect(bytes <= budget || first[b + 1] - first[b] == 1, "a batch is inside the budget or one segment", b, trial);
		// greedy: the next segment would not have fitted
		if (b + 1 < nb) expect((roff[first[b + 1] + 1] - roff[first[b]]) * 4u > budget / 4u * 4u, "a batch is full", b, trial);
	}
	for (uint64_t s = nb + 1; s <= S; ++s) expect(~0ull == first[s], "nothing is written behind the last batch", s, trial);
}

bool refused_words(std::vector<uint64_t> const &lb, std::vector<uint64_t> const &rb, std::vector<uint32_t> const &count, uint32_t bits)
{
	std::vector<uint64_t> qoff(lb.size() + 1, 7), roff(lb.size() + 1, 7);
	bool const no = nullptr != graph_nearest_words(lb.data(), rb.data(), count.data(), (uint64_t) lb.size(), bits, qoff.data(), roff.data());
	for (size_t s = 0; s < qoff.size(); ++s)
		if (no && (qoff[s] != 7 || roff[s] != 7)) return false;       // (a refusal writes nothing)
	return no;
}

bool refused_plan(std::vector<uint64_t> const &roff, uint64_t S, uint64_t budget)
{
	std::vector<uint64_t> first(S + 1, 7);
	uint64_t nb = 7;
	bool const no = nullptr != graph_nearest_plan(roff.data(), S, budget, first.data(), &nb);
	for (uint64_t f : first)
		if (no && f != 7) return false;
	return no && 7 == nb;
}

} // namespace

int main()
{
	uint64_t trial = 0;
	for (uint64_t S : {1ull, 2ull, 3ull, 17ull, 100ull})
		for (uint32_t bits : {2u, 4u, 8u})
			for (uint64_t budget : {1ull, 3ull, 4ull, 64ull, 1000ull, 1ull << 28})
				for (uint64_t widest : {1ull, 17ull, 200ull})
					for (int rep = 0; rep < 4; ++rep) check(S, bits, budget, widest, trial++);
	// widths on both sides of a word
	{
		std::vector<uint64_t> const lb{0, 15, 31, 48}, rb{15, 31, 48, 49};
		std::vector<uint32_t> const count{2, 1, 3, 5};
		std::vector<uint64_t> qoff(5), roff(5), first(5);
		uint64_t nb = 0;
		expect(nullptr == graph_nearest_words(lb.data(), rb.data(), count.data(), 4, 2, qoff.data(), roff.data()), "15, 16, 17 and 1 columns", 0, 0);
		expect(qoff == std::vector<uint64_t>{0, 1, 2, 4, 5} && roff == std::vector<uint64_t>{0, 2, 3, 9, 14}, "their words at 2 bits", qoff[4], roff[4]);
		expect(nullptr == graph_nearest_plan(roff.data(), 4, 12, first.data(), &nb) && 3 == nb && 0 == first[0] && 2 == first[1] && 3 == first[2] && 4 == first[3],
		       "12 bytes: {0, 1}, {2} above the budget, {3}", nb, first[1]);
		expect(nullptr == graph_nearest_plan(roff.data(), 4, 56, first.data(), &nb) && 1 == nb && 4 == first[1], "56 bytes hold all", nb, 0);
		expect(nullptr == graph_nearest_plan(roff.data(), 4, 55, first.data(), &nb) && 2 == nb && 3 == first[1], "55 bytes do not", nb, 0);
	}
	std::vector<uint64_t> const lb{0, 4}, rb{4, 9};
	std::vector<uint32_t> const count{1, 2};
	expect(!refused_words(lb, rb, count, 2), "the base case of the refusals is in order", 0, 0);
	expect(refused_words({}, {}, {}, 2), "no segments", 0, 0);
	expect(refused_words(lb, rb, count, 3) && refused_words(lb, rb, count, 0) && refused_words(lb, rb, count, 16), "bits not 2, 4 or 8", 0, 0);
	expect(refused_words({0, 4}, {4, 4}, count, 2), "an empty segment", 0, 0);
	expect(refused_words({0, 9}, {4, 4}, count, 2), "a backward segment", 0, 0);
	expect(refused_words({0, 4}, {4, 4 + 0xFFFFFFFFull}, count, 2), "a segment of 2^32 - 1 columns", 0, 0);
	expect(!refused_words({0, 4}, {4, 4 + 0xFFFFFFFEull}, count, 8), "a segment of 2^32 - 2 columns is taken", 0, 0);
	expect(refused_words(lb, rb, {1, 0}, 2), "a segment without a class", 0, 0);
	{
		// 2^30 segments' worth of words cannot be made here; two segments whose representatives' words pass 2^61 can
		std::vector<uint64_t> const l{0, 0}, r{0xFFFFFFFEull, 0xFFFFFFFEull};
		expect(refused_words(l, r, {0xFFFFFFFFu, 0xFFFFFFFFu}, 8), "more words than 64 bits count bytes for", 0, 0);
	}
	{
		uint64_t q[3] = {7, 7, 7}, r[3] = {7, 7, 7};
		expect(nullptr != graph_nearest_words(nullptr, rb.data(), count.data(), 2, 2, q, r) && nullptr != graph_nearest_words(lb.data(), nullptr, count.data(), 2, 2, q, r) &&
		       nullptr != graph_nearest_words(lb.data(), rb.data(), nullptr, 2, 2, q, r) && nullptr != graph_nearest_words(lb.data(), rb.data(), count.data(), 2, 2, nullptr, r) &&
		       nullptr != graph_nearest_words(lb.data(), rb.data(), count.data(), 2, 2, q, nullptr) && 7 == q[0] && 7 == r[2], "NULL arrays", 0, 0);
	}
	std::vector<uint64_t> const roff{0, 1, 5};
	expect(!refused_plan(roff, 2, 8), "the base case of the plan's refusals is in order", 0, 0);
	expect(refused_plan(roff, 0, 8), "no segments", 0, 0);
	expect(refused_plan(roff, 2, 0), "a budget of 0 bytes", 0, 0);
	expect(refused_plan({1, 2, 5}, 2, 8), "offsets that do not start at 0", 0, 0);
	expect(refused_plan({0, 6, 5}, 2, 8), "offsets that descend", 0, 0);
	{
		uint64_t f[3] = {7, 7, 7}, nb = 7;
		expect(nullptr != graph_nearest_plan(nullptr, 2, 8, f, &nb) && nullptr != graph_nearest_plan(roff.data(), 2, 8, nullptr, &nb) &&
		       nullptr != graph_nearest_plan(roff.data(), 2, 8, f, nullptr) && 7 == f[0] && 7 == nb, "NULL arrays of the plan", 0, 0);
	}
	std::printf("%s\n", failures ? "failed" : "ok");
	return failures ? EXIT_FAILURE : EXIT_SUCCESS;
}
