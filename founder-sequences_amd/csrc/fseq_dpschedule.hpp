// fseq_dpschedule.hpp -- the round schedule of phase D (fseq_dp.hpp) and the modes of k_dp: what the host needs of the DP to plan
// launches, list windows and chunks.  No kernel and no device-only code: a unit that only plans includes this, not fseq_dp.hpp.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace fseq {

constexpr uint32_t DP_RL = 56;            // cells per round (<= L)

struct DpRound {
	uint32_t e0, len, t0, t1;
	bool final_round;
};

// Round schedule.  nreg regular rounds of <= RL cells (end = L + r*RL + i), then -- pipelined mode
// only -- one empty drain round (the update of the last regular round), then the final cell at
// rb = n (lp.cc:165-183).
struct DpSchedule {
	uint32_t L, n, RL, nreg, nrounds;
	bool pipe;
};

__host__ __device__ inline DpRound dp_round(DpSchedule const &S, uint32_t r)
{
	DpRound R;
	uint32_t const last_end = S.n - S.L;
	R.final_round = (r + 1u == S.nrounds);
	bool const regular = r < S.nreg;
	R.e0 = R.final_round ? S.n : (regular ? S.L + r * S.RL : last_end + 1u);
	uint32_t const rest = last_end - R.e0 + 1u;
	R.len = R.final_round ? 1u : (regular ? (S.RL < rest ? S.RL : rest) : 0u);
	R.t0 = R.e0 - S.L;
	R.t1 = R.t0 + R.len;
	return R;
}

// Two schedules.  Classic: rounds of <= min(L, DP_RL) cells, the rmq.update of a round between two
// barriers.  Pipelined (L >= 96): rounds of 48 cells -- a round then never reads what the previous
// round wrote (a cell reads entries <= end - 2L), so two dedicated waves do the update of round r-1
// while the compute waves are already in round r: one barrier a round.
__host__ __device__ inline DpSchedule dp_schedule(uint32_t L, uint32_t n)
{
	DpSchedule S;
	S.L = L; S.n = n;
#ifndef FSEQ_DP_PIPE_MIN_L
#define FSEQ_DP_PIPE_MIN_L 96u
#endif
	S.pipe = L >= FSEQ_DP_PIPE_MIN_L;                         // measured: pays only with 4 cells per compute wave
	uint32_t const half = L / 2u < 48u ? L / 2u : 48u;
	S.RL = S.pipe ? (half / 12u) * 12u : (L < DP_RL ? L : DP_RL);   // pipelined: whole cells per compute wave
	S.nreg = ((n - L) - L) / S.RL + 1u;
	S.nrounds = S.nreg + (S.pipe ? 2u : 1u);
	return S;
}

// Rounds of the schedule whose cells only need the lists of columns < col_hi (a cell `end` reads the list
// of column end - 1): the DP of a column prefix can run while later columns are still being produced.
__host__ __device__ inline uint32_t dp_rounds_within(DpSchedule const &S, uint64_t col_hi)
{
	if (col_hi >= S.n) return S.nrounds;
	// the regular rounds need ascending columns (the drain round needs none, the final cell needs column n - 1):
	// first regular round that needs a column >= col_hi
	uint32_t lo = 0, hi = S.nreg;
	while (lo < hi)
	{
		uint32_t const mid = (lo + hi) / 2u;
		DpRound const R = dp_round(S, mid);
		bool const needs = (uint64_t) R.e0 + R.len - 2u >= col_hi;
		if (needs) hi = mid; else lo = mid + 1u;
	}
	return lo < S.nreg ? lo : S.nrounds - 1u;                  // all regular rounds (and the drain): everything but the final cell
}

// MODE 0: the whole schedule in one launch (r_begin_arg / r_end_arg ignored: the common case keeps its registers).
// MODE 1: rounds [r_begin_arg, r_end_arg).  MODE 2: workgroup = chunk of the speculative iteration.
enum { DP_WHOLE = 0, DP_PARTIAL = 1, DP_SPEC = 2 };

} // namespace fseq
