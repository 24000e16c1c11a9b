// The planner of phase C on representative rows (plan_reduced, csrc/fseq_redplan.hpp) in a program of its own: the header is
// host-only, so tests/test_red_plan.py builds this with g++ -fsanitize=address,undefined and runs it -- the decline rule on
// both sides of its thresholds, a rank's range, and the layout of the block list, with every index the planner forms under
// the sanitizers.  Exit status 0: every check held.
#include "fseq_redplan.hpp"

#include <cstdio>

using namespace fseq;

static int failures = 0;
#define CHECK(cond) do { if (!(cond)) { fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond); ++failures; } } while (0)

// three configurations: one wave of 192 rows, 512 x 5 with a list wave (2,240 rows) and beside it the one without (2,560), slim 512 x 15
static std::vector<RedConfig> configs()
{
	return {RedConfig{192, 192, 64, 3, false, true}, RedConfig{2240, 2560, 512, 5, true, true}, RedConfig{2560, 2560, 512, 5, false, true},
	        RedConfig{6720, 4096, 512, 15, true, true}, RedConfig{6720, 7168, 1024, 7, true, true}, RedConfig{7168, 7168, 1024, 7, false, false}};
}

static RedPlanInput input(uint32_t m, std::vector<uint32_t> cnt)
{
	RedPlanInput in;
	in.m = m; in.nblocks = (uint32_t) cnt.size(); in.b_lo = 0; in.b_hi = in.nblocks;
	in.force.assign(cnt.size(), 0);
	in.cnt = std::move(cnt);
	in.configs = configs();
	return in;
}

int main()
{
	// the rows clause: 20 blocks of 1,000 rows, 4,000 representatives in all | 4,001
	{
		RedPlanInput in = input(1000, std::vector<uint32_t>(20, 200));
		CHECK(plan_reduced(in).verdict == RedVerdict::Use);
		in.cnt[7] = 201;
		CHECK(plan_reduced(in).verdict == RedVerdict::Declined);
		in.reduced_always = true;
		CHECK(plan_reduced(in).verdict == RedVerdict::Use);
	}
	// blocks on all rows count one and a half: two of 20 | three; none reduced: declined whatever the knob says
	{
		RedPlanInput in = input(1000, std::vector<uint32_t>(20, 10));
		in.cnt[0] = in.cnt[19] = RED_NONE;
		CHECK(plan_reduced(in).verdict == RedVerdict::Use);
		in.no_block_list = true;
		CHECK(plan_reduced(in).verdict == RedVerdict::NoBlockList);
		in.no_block_list = false;
		in.cnt[5] = RED_NONE;
		CHECK(plan_reduced(in).verdict == RedVerdict::Declined);
		in.reduced_always = true;
		CHECK(plan_reduced(in).verdict == RedVerdict::Use);
		in.cnt.assign(20, RED_NONE);
		RedPlan const P = plan_reduced(in);
		CHECK(P.verdict == RedVerdict::Declined && P.nfull == 20 && P.listed == 0 && P.bins.empty() && P.blocks.size() == 20);
	}
	// the layout, on a rank's range [1, 11) of 12 blocks
	{
		//                                     0     1    2     3         4     5    6     7     8    9     10    11
		RedPlanInput in = input(100000, {5000, 100, 2000, RED_NONE, 5000, 100, 5000, 2000, 100, 7000, 5000, 100});
		in.b_lo = 1; in.b_hi = 11;
		in.force[6] = RED_FORCE_WIDE; in.force[8] = RED_FORCE_FULL;
		in.reduced_always = true;                              // (three of ten blocks on all rows: declined by itself)
		RedPlan const P = plan_reduced(in);
		CHECK(P.verdict == RedVerdict::Use);
		// (7,000 rows: the one configuration that holds them does not fit -- all rows, though pass 2 has none either)
		std::vector<uint32_t> const want = {1, 2, 4, 5, 6, 7, 8, 9, 10, /* 192 */ 1, 5, /* 512 x 5 */ 2, 7, /* slim */ 4, 10, /* 1024 x 7 */ 6, /* all rows */ 3, 8, 9};
		CHECK(P.blocks == want);
		CHECK(P.listed == 9 && P.full_at == 16 && P.nfull == 3 && P.max_rows == 7000 && P.reduced_blocks == 7);
		CHECK(P.rows_mean == (100 + 100 + 2000 + 2000 + 5000 + 5000 + 5000) / 7);
		CHECK(P.bins.size() == 4);
		int const cf[4] = {0, 1, 3, 4};
		uint32_t const first[4] = {9, 11, 13, 15}, count[4] = {2, 2, 2, 1};
		for (size_t i = 0; i < P.bins.size() && i < 4; ++i)
			CHECK(P.bins[i].config == cf[i] && P.bins[i].first == first[i] && P.bins[i].count == count[i]);
		CHECK(P.config_of[0] == -1 && P.config_of[11] == -1 && !P.full[0] && !P.full[11] && P.cnt[0] == RED_NONE && P.cnt[11] == RED_NONE);
		CHECK(P.config_snap_of[2] == 2 && P.config_snap_of[8] == 0 && P.full[8] && P.config_snap_of[9] == -1 && P.config_of[9] == -1);
	}
	if (failures) fprintf(stderr, "%d checks failed\n", failures);
	return failures ? 1 : 0;
}
