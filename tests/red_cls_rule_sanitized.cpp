// [r10] The direct-or-gather rule of the reduced column kernel's configurations (red_cls_direct) and what plan_reduced makes of it per
// block (RedPlan::from_cls, gathered; csrc/fseq_redplan.hpp) in a program of its own: the header is host-only, so
// tests/test_red_cls_rule.py builds this with g++ -fsanitize=address,undefined and runs it.  Exit status 0: every check held.
#include "fseq_redplan.hpp"

#include <cstdio>

using namespace fseq;

static int failures = 0;
#define CHECK(cond) do { if (!(cond)) { fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond); ++failures; } } while (0)

// one wave of 192 rows (gathers), 512 x 5 with a list wave (gathers) and without (stages), the slim 512 x 15 (stages), 1024 x 7 with a list
// wave (stages) and without (gathers)
static std::vector<RedConfig> configs()
{
	return {RedConfig{192, 192, 64, 3, false, true, false}, RedConfig{2240, 2560, 512, 5, true, true, false}, RedConfig{2560, 2560, 512, 5, false, true, true},
	        RedConfig{6720, 4096, 512, 15, true, true, true}, RedConfig{6720, 7168, 1024, 7, true, true, true}, RedConfig{7168, 7168, 1024, 7, false, true, false}};
}

int main()
{
	constexpr size_t LIMIT = 160 * 1024;
	// the rule: the class width fits, and as many workgroups stay resident
	CHECK(red_cls_direct(73920, LIMIT, 2, 2));               // the slim configuration at blocks of 814 columns: 71,872 + 2 KB
	CHECK(!red_cls_direct(58368, LIMIT, 3, 2));              // 512 x 5: 54,272 bytes three times in 160 KB, 58,368 twice
	CHECK(!red_cls_direct(LIMIT + 1, LIMIT, 1, 1));
	CHECK(red_cls_direct(LIMIT, LIMIT, 1, 1));
	CHECK(!red_cls_direct(1024, LIMIT, 0, 0));               // (no answer from the device is no licence)
	CHECK(red_cls_direct(30000, LIMIT, 4, 5));

	RedPlanInput in;
	in.m = 20000; in.nblocks = 9; in.b_lo = 1; in.b_hi = 9;
	//          not mine, one wave, ew 512x5 / 512x5, slim / 1024x7, slim / 1024x7 plain (the sweep gathers), none holds it, wide: 1024x7 / plain, full by force
	in.cnt = {100, 150, 2000, 2500, 6000, 6800, RED_NONE, 3000, 3000};
	in.force = {0, 0, 0, 0, 0, 0, 0, RED_FORCE_WIDE, RED_FORCE_FULL};
	in.configs = configs();
	in.reduced_always = true;
	RedPlan const P = plan_reduced(in);
	CHECK(P.verdict == RedVerdict::Use);
	CHECK(P.from_cls.size() == 9);
	CHECK(P.from_cls[0] == 0);                               // not a block of mine
	CHECK(P.config_of[1] == 0 && P.from_cls[1] == 0);        // the one-wave configuration gathers
	CHECK(P.config_of[2] == 1 && P.config_snap_of[2] == 2 && P.from_cls[2] == 0);      // phase C's configuration gathers, the sweep's would stage: one source for both
	CHECK(P.config_of[3] == 3 && P.config_snap_of[3] == 2 && P.from_cls[3] == 1);      // slim and 512 x 5 plain: both stage
	CHECK(P.config_of[4] == 3 && P.config_snap_of[4] == 5 && P.from_cls[4] == 0);      // the sweep's configuration gathers
	CHECK(P.full[5] && P.config_snap_of[5] == 5 && P.from_cls[5] == 0);                // 6,800 rows: no list-wave configuration; swept on 1024 x 7 plain, which gathers
	CHECK(P.full[6] && P.from_cls[6] == 0);                  // not listed
	CHECK(P.config_of[7] == 4 && P.config_snap_of[7] == 5 && P.from_cls[7] == 0);
	CHECK(P.full[8] && P.config_snap_of[8] == 5 && P.from_cls[8] == 0);
	CHECK(P.gathered == 6);                                  // blocks 1, 2, 4, 5, 7, 8
	// every configuration stages: every listed block does, and nothing is gathered
	for (RedConfig &f : in.configs) f.cls = true;
	RedPlan const Q = plan_reduced(in);
	CHECK(Q.gathered == 0);
	for (uint32_t b = 1; b < 9; ++b) CHECK(Q.from_cls[b] == (b == 6 ? 0 : 1));
	// ... none does (a run without class columns): the plan is the one before, every listed block is gathered
	for (RedConfig &f : in.configs) f.cls = false;
	RedPlan const R = plan_reduced(in);
	CHECK(R.gathered == 7 && R.blocks == Q.blocks && R.config_of == Q.config_of && R.full == Q.full);
	if (failures) { fprintf(stderr, "%d checks failed\n", failures); return 1; }
	printf("red_cls_rule_sanitized: ok\n");
	return 0;
}
