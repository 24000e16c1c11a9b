// The packed local pass of a partition step (csrc/fseq_localpass.hpp, the host side of the text the device runs) against the
// plain pass restated here, for E = 11, 12 and 15.  Built and run by tests/test_local_pass_packed.py; exit status 0 and a
// last line "ok <cases>" when every case of the E given as the argument agrees, the first disagreeing case on stderr otherwise.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include "fseq_localpass.hpp"

using namespace fseq;

// the plain pass of partition_step (csrc/fseq_core.hpp): four running maxima; a row takes the one of its symbol and resets it
template <int E>
static void plain(uint32_t const (&d)[E], uint32_t const (&s)[E], uint32_t (&dnew)[E], uint32_t (&run)[4])
{
	for (int x = 0; x < 4; ++x) run[x] = 0;
	for (int e = 0; e < E; ++e)
	{
		uint32_t o = 0;
		for (uint32_t x = 0; x < 4; ++x)
		{
			uint32_t const r = run[x] > d[e] ? run[x] : d[e];
			bool const is = s[e] == x;
			o = is ? r : o;
			run[x] = is ? 0u : r;
		}
		dnew[e] = o;
	}
}

static unsigned long long n_cases = 0;

template <int E>
static void check(uint32_t const (&d)[E], uint32_t const (&s)[E], char const *what)
{
	uint32_t want[E], wrun[4], got[E], grun[4];
	plain<E>(d, s, want, wrun);
	local_pass_packed<E>(d, s, got, grun);
	bool ok = true;
	for (int e = 0; e < E; ++e) ok = ok && want[e] == got[e];
	for (int x = 0; x < 4; ++x) ok = ok && wrun[x] == grun[x];
	++n_cases;
	if (ok) return;
	fprintf(stderr, "E = %d, %s:\n  s    ", E, what);
	for (int e = 0; e < E; ++e) fprintf(stderr, " %5u", s[e]);
	fprintf(stderr, "\n  d    ");
	for (int e = 0; e < E; ++e) fprintf(stderr, " %5u", d[e]);
	fprintf(stderr, "\n  plain");
	for (int e = 0; e < E; ++e) fprintf(stderr, " %5u", want[e]);
	fprintf(stderr, " | %u %u %u %u\n  packd", wrun[0], wrun[1], wrun[2], wrun[3]);
	for (int e = 0; e < E; ++e) fprintf(stderr, " %5u", got[e]);
	fprintf(stderr, " | %u %u %u %u\n", grun[0], grun[1], grun[2], grun[3]);
	exit(1);
}

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint32_t rnd()
{
	rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17;       // xorshift64
	return (uint32_t) (rng_state >> 32);
}

static uint32_t const EDGE[6] = {0u, 1u, 0x7FFFu, 0x8000u, 0xFFFEu, 0xFFFFu};

// every symbol pattern of five rows (symbols 0 .. 4; an unused position holds the value 0, as the kernels guarantee) with every
// choice of the six edge values, in the thread's first five positions; the others are unused
template <int E>
static void exhaustive_five()
{
	for (uint32_t sp = 0; sp < 3125u; ++sp)
		for (uint32_t vp = 0; vp < 7776u; ++vp)
		{
			uint32_t d[E], s[E];
			for (int e = 0; e < E; ++e) { d[e] = 0; s[e] = 4; }
			uint32_t a = sp, b = vp;
			bool twice = false;                                      // (an unused position has one value: its other five digits repeat a case)
			for (int i = 0; i < 5; ++i)
			{
				s[i] = a % 5u; a /= 5u;
				twice = twice || (s[i] == 4u && b % 6u != 0u);
				d[i] = s[i] == 4u ? 0u : EDGE[b % 6u];
				b /= 6u;
			}
			if (twice) continue;
			check<E>(d, s, "five rows, exhaustive");
		}
}

template <int E>
static void random_threads(int n)
{
	for (int t = 0; t < n; ++t)
	{
		uint32_t d[E], s[E];
		// a third of the threads with values from the edges, a third small ones (many ties), a third anything below 2^16
		uint32_t const kind = rnd() % 3u;
		for (int e = 0; e < E; ++e)
		{
			s[e] = rnd() & 3u;
			d[e] = kind == 0 ? EDGE[rnd() % 6u] : kind == 1 ? rnd() % 5u : rnd() & 0xFFFFu;
		}
		// (fifteen rows where E allows: the unused positions of a shorter thread are the named cases' business)
		check<E>(d, s, "random thread");
	}
}

template <int E>
static void named()
{
	uint32_t d[E], s[E];
	auto values = [&](int kind) {
		for (int e = 0; e < E; ++e)
			d[e] = kind == 0 ? 0xFFFFu - 97u * (uint32_t) e          // strictly falling from the top
			     : kind == 1 ? 0x7FF8u + (uint32_t) e                // strictly rising through bit 15
			     : kind == 2 ? 0x8000u                               // all equal
			     : rnd() & 0xFFFFu;
	};
	for (int kind = 0; kind < 4; ++kind)
	{
		for (uint32_t x = 0; x < 4; ++x)                            // one symbol only
		{
			values(kind);
			for (int e = 0; e < E; ++e) s[e] = x;
			check<E>(d, s, "one symbol only");
		}
		for (uint32_t x = 0; x < 4; ++x)                            // each symbol absent in turn
		{
			values(kind);
			for (int e = 0; e < E; ++e) { s[e] = (uint32_t) e % 3u; s[e] += s[e] >= x ? 1u : 0u; }
			check<E>(d, s, "one symbol absent");
		}
		for (uint32_t x = 0; x < 4; ++x)                            // alternating symbols
			for (uint32_t y = 0; y < 4; ++y)
			{
				if (x == y) continue;
				values(kind);
				for (int e = 0; e < E; ++e) s[e] = (e & 1) ? y : x;
				check<E>(d, s, "alternating symbols");
			}
		for (int tail = 1; tail <= 14 && tail < E; ++tail)          // one to fourteen trailing unused positions
		{
			values(kind);
			for (int e = 0; e < E; ++e) s[e] = rnd() & 3u;
			for (int e = E - tail; e < E; ++e) { s[e] = 4u; d[e] = 0u; }
			check<E>(d, s, "trailing unused positions");
		}
		values(kind);                                               // all four, in turn
		for (int e = 0; e < E; ++e) s[e] = (uint32_t) e & 3u;
		check<E>(d, s, "symbols in turn");
	}
	for (int e = 0; e < E; ++e) { s[e] = 4u; d[e] = 0u; }           // no row at all
	check<E>(d, s, "no row");
}

template <int E>
static void all_of()
{
	exhaustive_five<E>();
	named<E>();
	random_threads<E>(100000);
}

// argument: the rows of a thread, 11, 12 or 15 (the test runs the three side by side)
int main(int argc, char **argv)
{
	int const E = argc > 1 ? atoi(argv[1]) : 0;
	if (E == 11) all_of<11>();
	else if (E == 12) all_of<12>();
	else if (E == 15) all_of<15>();
	else { fprintf(stderr, "usage: %s 11|12|15\n", argv[0]); return 2; }
	printf("ok %llu\n", n_cases);
	return 0;
}
