// fseq_joinscore.hpp -- what a join is worth: junction support per adjacent segment pair and founder slot.
//
// A join places, for every merged segment s and founder slot r, the substring of input row perm[s][r] (an entry >= m is a gap,
// as k_founders prints it).  At the junction p = (s, s + 1) slot r carries the classes (cls_s(L), cls_{s+1}(R)) of its two rows
// L = perm[s][r], R = perm[s + 1][r]; its support is the number of input rows that are in both classes, i.e. that carry the
// founder's substring on both sides of the border.  The classes are the of_row arrays k_join_classes_wide leaves on the device
// (fseq_joinprep.hpp); nothing else of a boundary state is read.
//   k_join_score           one workgroup per junction.  The X slot keys l << 16 | r go into an open-addressing table in LDS
//                          (a key word and a counter word an entry, the power of two >= 2 X entries: never more than half
//                          full, so every probe sequence ends at an empty entry), equal keys on one entry.  The m rows are
//                          streamed once -- two coalesced 16-bit loads a row --, each looked up, the counter of its entry
//                          incremented.  Every result is a sum of such counters: the order in which the atomics land changes
//                          nothing, and none of them decides an order.
//   k_join_score_founders  breaks[r] = the junctions at which slot r is unsupported: a thread per slot down the columns of
//                          the support matrix, no atomics.
// A class is at most 0xFFFE wherever a key is formed (the launcher's callers see to it: X <= JS_MAX_SLOTS in the library,
// checked arrays in the debug entry), so no key equals JS_EMPTY; a row whose two classes are both 0xFFFF -- class tables the
// host rejects afterwards -- is skipped all the same.
#pragma once

#include "fseq_core.hpp"

namespace fseq {

constexpr uint32_t JS_T = 1024;
constexpr uint32_t JS_MAX_SLOTS = 4096;                  // 8,192 entries of 8 bytes: 64 KiB of table
constexpr uint32_t JS_EMPTY = 0xFFFFFFFFu;
constexpr uint32_t JS_GAP = 0xFFFFu;                     // a slot's class where its row is a gap
constexpr uint32_t JS_FIELDS = 6;                        // words of a junction's record: supported, unsupported, gaps, rows_through, weight (low, high)

// log2 of the table's capacity: the power of two >= 2 X
inline uint32_t join_score_cap_log2(uint32_t X)
{
	uint32_t lg = 1;
	while ((1u << lg) < 2u * X) ++lg;
	return lg;
}
// the table and, behind it, the workgroup's five accumulators (16 words kept for them)
inline size_t join_score_lds_bytes(uint32_t X) { return ((size_t) 2 << join_score_cap_log2(X)) * 4 + 64; }

// Fibonacci hashing on the top bits: the home entry of a key in a table of 2^lg entries (tests/join_score_model.py restates it
// to build colliding keys)
__host__ __device__ __forceinline__ uint32_t join_score_home(uint32_t key, uint32_t lg) { return (key * 0x9E3779B1u) >> (32u - lg); }

// perm != nullptr: the slots' rows, [S][X]; else cls_left / cls_right [S - 1][X]: the slots' classes as the caller built them
// (JS_GAP: a gap).  of_row [S][m].  Out: junctions [S - 1][JS_FIELDS], support [S - 1][X].
struct JoinScoreArgs {
	uint16_t const *of_row;
	uint32_t const *perm;
	uint16_t const *cls_left, *cls_right;
	uint32_t m, X, S;
	uint32_t *junctions, *support;
};

// the classes (l, r) of slot r at junction p, JS_GAP where the slot has no row on that side
template <bool FROM_PERM>
__device__ __forceinline__ void join_score_slot(JoinScoreArgs const &A, uint32_t p, uint32_t r, uint32_t *l, uint32_t *rr)
{
	if (FROM_PERM)
	{
		uint32_t const L = A.perm[(size_t) p * A.X + r], R = A.perm[(size_t) (p + 1) * A.X + r];
		*l = L < A.m ? A.of_row[(size_t) p * A.m + L] : JS_GAP;
		*rr = R < A.m ? A.of_row[(size_t) (p + 1) * A.m + R] : JS_GAP;
	}
	else
	{
		*l = A.cls_left[(size_t) p * A.X + r];
		*rr = A.cls_right[(size_t) p * A.X + r];
	}
}

template <bool FROM_PERM>
__global__ __launch_bounds__(JS_T) void k_join_score(JoinScoreArgs const A, uint32_t lg)
{
	extern __shared__ __attribute__((aligned(16))) uint32_t js_lds[];
	uint32_t const cap = 1u << lg, mask = cap - 1u;
	uint32_t *const keys = js_lds, *const cnt = js_lds + cap, *const acc = js_lds + 2 * (size_t) cap;
	uint32_t const p = blockIdx.x, tid = threadIdx.x, m = A.m, X = A.X;
	for (uint32_t i = tid; i < cap; i += JS_T) { keys[i] = JS_EMPTY; cnt[i] = 0u; }
	if (tid < 16u) acc[tid] = 0u;
	__syncthreads();
	// the slots' keys: equal keys fall on one entry
	for (uint32_t r = tid; r < X; r += JS_T)
	{
		uint32_t l, rr;
		join_score_slot<FROM_PERM>(A, p, r, &l, &rr);
		if (l >= JS_GAP || rr >= JS_GAP) continue;
		uint32_t const key = l << 16 | rr;
		for (uint32_t h = join_score_home(key, lg);; h = (h + 1u) & mask)
		{
			uint32_t const was = atomicCAS(&keys[h], JS_EMPTY, key);
			if (was == JS_EMPTY || was == key) break;
		}
	}
	__syncthreads();
	// the rows, once
	uint16_t const *const ofl = A.of_row + (size_t) p * m, *const ofr = ofl + m;
	for (uint32_t i = tid; i < m; i += JS_T)
	{
		uint32_t const key = (uint32_t) ofl[i] << 16 | ofr[i];
		if (key == JS_EMPTY) continue;
		for (uint32_t h = join_score_home(key, lg);; h = (h + 1u) & mask)
		{
			uint32_t const at = keys[h];
			if (at == key) { atomicAdd(&cnt[h], 1u); break; }
			if (at == JS_EMPTY) break;
		}
	}
	__syncthreads();
	// every slot reads its entry's counter
	uint32_t supported = 0, unsupported = 0, gaps = 0;
	unsigned long long weight = 0;
	for (uint32_t r = tid; r < X; r += JS_T)
	{
		uint32_t l, rr, sup = 0;
		join_score_slot<FROM_PERM>(A, p, r, &l, &rr);
		if (l >= JS_GAP || rr >= JS_GAP) ++gaps;
		else
		{
			uint32_t const key = l << 16 | rr;
			uint32_t h = join_score_home(key, lg);
			while (keys[h] != key) h = (h + 1u) & mask;          // (inserted above)
			sup = cnt[h];
			if (sup) ++supported; else ++unsupported;
			weight += sup;
		}
		A.support[(size_t) p * X + r] = sup;
	}
	// rows_through: over the entries, so a pair of classes that several slots share counts once
	uint32_t through = 0;
	for (uint32_t i = tid; i < cap; i += JS_T) through += cnt[i];
	if (supported) atomicAdd(&acc[0], supported);
	if (unsupported) atomicAdd(&acc[1], unsupported);
	if (gaps) atomicAdd(&acc[2], gaps);
	if (through) atomicAdd(&acc[3], through);
	if (weight) atomicAdd(reinterpret_cast<unsigned long long *>(acc + 4), weight);
	__syncthreads();
	if (tid < JS_FIELDS) A.junctions[(size_t) p * JS_FIELDS + tid] = acc[tid];
}

// breaks[r] = junctions p with support[p][r] = 0 whose slot r is no gap
template <bool FROM_PERM>
__global__ __launch_bounds__(256) void k_join_score_founders(JoinScoreArgs const A, uint32_t *__restrict__ breaks)
{
	uint32_t const r = blockIdx.x * 256u + threadIdx.x;
	if (r >= A.X) return;
	uint32_t n = 0;
	for (uint32_t p = 0; p + 1u < A.S; ++p)
	{
		if (A.support[(size_t) p * A.X + r]) continue;
		uint32_t l, rr;
		join_score_slot<FROM_PERM>(A, p, r, &l, &rr);
		n += (l < JS_GAP && rr < JS_GAP) ? 1u : 0u;
	}
	breaks[r] = n;
}

// both kernels behind one launch: the library's entry and the debug entry go through here
inline hipError_t launch_join_score(hipStream_t st, JoinScoreArgs const &A, uint32_t *breaks)
{
	uint32_t const lg = join_score_cap_log2(A.X);
	size_t const lds = join_score_lds_bytes(A.X);
	uint32_t const pairs = A.S - 1u;
	hipError_t e = hipSuccess;
	if (lds > 64 * 1024)
		e = A.perm ? hipFuncSetAttribute(reinterpret_cast<void const *>(k_join_score<true>), hipFuncAttributeMaxDynamicSharedMemorySize, (int) lds)
		           : hipFuncSetAttribute(reinterpret_cast<void const *>(k_join_score<false>), hipFuncAttributeMaxDynamicSharedMemorySize, (int) lds);
	if (e != hipSuccess) return e;
	if (A.perm)
	{
		hipLaunchKernelGGL(k_join_score<true>, dim3(pairs), dim3(JS_T), lds, st, A, lg);
		hipLaunchKernelGGL(k_join_score_founders<true>, dim3((A.X + 255u) / 256u), dim3(256), 0, st, A, breaks);
	}
	else
	{
		hipLaunchKernelGGL(k_join_score<false>, dim3(pairs), dim3(JS_T), lds, st, A, lg);
		hipLaunchKernelGGL(k_join_score_founders<false>, dim3((A.X + 255u) / 256u), dim3(256), 0, st, A, breaks);
	}
	return hipGetLastError();
}

} // namespace fseq
