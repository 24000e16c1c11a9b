// The host form of the join score (csrc/fseq_joinscore_host.hpp) as a program of its own, for AddressSanitizer and
// UndefinedBehaviorSanitizer (tests/test_join_score_abi.py builds and runs it; nothing here is loaded into Python).  Every array has
// exactly the length the function may read or write, so an index formed wrongly leaves it.  Random classes, boundary states made
// from them and random permutations with gaps are checked against counting spelled out row by row; then the corners: one
// segment, one row, one slot, optional outputs left out, and the input the function must refuse.
#include "fseq_joinscore_host.hpp"

#include <cstdio>
#include <cstdlib>
#include <numeric>
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

// boundary states of S segments of `width` columns each in which row i has class cls[s][i]: the rows in class order (a stable
// sort: pBWT order inside a class is any), d = the segment's rb at a class's first row -- above lb -- and a column at or in front
// of lb behind it
void states_from_classes(uint32_t m, uint64_t S, uint64_t width, std::vector<uint32_t> const &cls, std::vector<uint64_t> &lb,
                         std::vector<uint32_t> &A, std::vector<uint32_t> &D)
{
	lb.resize(S); A.resize(S * m); D.resize(S * m);
	for (uint64_t s = 0; s < S; ++s)
	{
		lb[s] = s * width;
		uint32_t *a = A.data() + s * m, *d = D.data() + s * m;
		std::iota(a, a + m, 0u);
		std::stable_sort(a, a + m, [&](uint32_t x, uint32_t y) { return cls[s * m + x] < cls[s * m + y]; });
		for (uint32_t i = 0; i < m; ++i)
		{
			bool const first = 0 == i || cls[s * m + a[i]] != cls[s * m + a[i - 1]];
			d[i] = (uint32_t) (first ? (s + 1) * width : (s ? next() % (lb[s] + 1) : 0u));
		}
	}
}

void check(uint32_t m, uint32_t X, uint64_t S, uint32_t classes, uint64_t trial)
{
	std::vector<uint32_t> cls(S * m), perm(S * X);
	for (auto &c : cls) c = (uint32_t) (next() % classes);
	for (auto &r : perm) { uint64_t const v = next(); r = v % 7 == 0 ? (v % 14 == 0 ? m : 0xFFFFFFFFu) : (uint32_t) ((v >> 8) % m); }
	std::vector<uint64_t> lb;
	std::vector<uint32_t> A, D;
	states_from_classes(m, S, 5, cls, lb, A, D);
	std::vector<JoinScoreJunction> J(S - 1);
	std::vector<uint32_t> breaks(X, 77u), support((S - 1) * X, 77u);
	expect(join_score_host(m, X, S, lb.data(), A.data(), D.data(), perm.data(), J.data(), breaks.data(), support.data()), "a well-formed input is taken", trial, 0);
	std::vector<uint32_t> want_breaks(X, 0u);
	for (uint64_t p = 0; p + 1 < S; ++p)
	{
		JoinScoreJunction w;
		std::vector<uint8_t> through(m, 0);
		for (uint32_t r = 0; r < X; ++r)
		{
			uint32_t const L = perm[p * X + r], R = perm[(p + 1) * X + r];
			uint32_t sup = 0;
			if (L >= m || R >= m) ++w.gaps;
			else
			{
				for (uint32_t i = 0; i < m; ++i)
					if (cls[p * m + i] == cls[p * m + L] && cls[(p + 1) * m + i] == cls[(p + 1) * m + R]) { ++sup; through[i] = 1; }
				if (sup) ++w.supported; else { ++w.unsupported; ++want_breaks[r]; }
				w.weight += sup;
			}
			expect(support[p * X + r] == sup, "a slot's support", p, r);
		}
		for (uint32_t i = 0; i < m; ++i) w.rows_through += through[i];
		expect(J[p].supported == w.supported && J[p].unsupported == w.unsupported && J[p].gaps == w.gaps, "a junction's slot counts", p, trial);
		expect(J[p].weight == w.weight && J[p].rows_through == w.rows_through, "a junction's weight and rows_through", p, trial);
		expect(w.supported + w.unsupported + w.gaps == X && w.rows_through <= m, "the definitions' bounds", p, trial);
	}
	expect(breaks == want_breaks, "the breaks", trial, 0);
	// the optional outputs left out: the breaks alone, the same
	std::vector<uint32_t> alone(X, 77u);
	expect(join_score_host(m, X, S, lb.data(), A.data(), D.data(), perm.data(), nullptr, alone.data(), nullptr) && alone == want_breaks, "without junctions and support", trial, 0);
	JoinScoreTotals const t = join_score_totals(m, X, S - 1, J.data(), breaks.data());
	uint64_t weight = 0;
	uint32_t least = m, most = 0;
	for (auto const &j : J) { weight += j.weight; least = std::min(least, j.rows_through); }
	for (uint32_t b : breaks) most = std::max(most, b);
	expect(t.junctions == S - 1 && t.weight == weight && t.max_breaks == most, "the totals", trial, 0);
	expect(S < 2 ? (t.min_rows_through == m && 0 == t.min_junction) : (t.min_rows_through == least && J[t.min_junction].rows_through == least), "the smallest rows_through", trial, 0);
}

} // namespace

int main()
{
	uint64_t trial = 0;
	for (uint32_t m : {1u, 2u, 63u, 64u, 65u, 300u})
		for (uint32_t X : {1u, 2u, 17u, 64u})
			for (uint64_t S : {1ull, 2ull, 3ull, 9ull})
				for (uint32_t classes : {1u, 3u, 40u})
					check(m, X, S, classes, trial++);
	// more slots than rows, and as many classes as rows
	check(5, 40, 4, 5, trial++);
	check(200, 4100, 3, 200, trial++);
	// a boundary state that names a row that is none: refused, nothing written
	{
		std::vector<uint64_t> lb{0, 5};
		std::vector<uint32_t> A{0, 1, 2, 0, 3, 1}, D{5, 0, 0, 10, 0, 0}, perm{0, 1, 1, 2}, breaks{7, 7}, support{7, 7};
		JoinScoreJunction j;
		j.gaps = 7;
		expect(!join_score_host(3, 2, 2, lb.data(), A.data(), D.data(), perm.data(), &j, breaks.data(), support.data()), "a row >= m in a boundary state", 0, 0);
		expect(7 == j.gaps && 7 == breaks[0] && 7 == breaks[1] && 7 == support[0] && 7 == support[1], "a refusal writes nothing", 0, 0);
	}
	std::printf("%s\n", failures ? "failed" : "ok");
	return failures ? EXIT_FAILURE : EXIT_SUCCESS;
}
