// fseq_joinbipw.hpp -- the wide form of the bipartite-matching joiner on the device: 181 < max_segment_size <= JBW_MAX_TEXTS.
//
// fseq_joinbip.hpp solves a pair of segments in one workgroup's LDS, which holds the X x X intersection weights up to
// X = 181 (JP_MAX_CLASSES).  The weight matrix is the only structure that outgrows LDS: the potentials, the matching, the
// `way` array and the per-column state are X + 1 entries each.  So here the weights of the real texts live in a slab of
// X x X words of device memory that a workgroup owns for the whole launch, and everything else stays in LDS:
//   k_join_classes_wide  (fseq_joinprep.hpp, unchanged) of_row, start, size, rep, count per merged segment
//   k_bip_minrow_wide    one workgroup per segment: the smallest row of every class (the texts' first_sequence_index)
//   k_bip_texts_wide     one workgroup per segment: k_bip_texts for up to JBW_MAX_TEXTS classes
//   k_bip_match_wide     G persistent workgroups, workgroup g solves the pairs g, g + G, ... one after the other on its slab.
//                        No workgroup waits on another: no spin loop, no look-back, no cooperative launch.
//   k_bip_chain_wide     one thread per slot: the permutations chained through the matchings
// The order of the arithmetic is max_weight_perfect_matching's (fseq_join.hpp): rows i = 1 .. X, the columns' minima taken
// with strict <, the lowest column among equal minima; potentials, minima and delta are 64-bit as there.  The permutations
// are therefore the host joiner's, entry for entry (tests/test_gpu_join_bip_wide.py).
#pragma once

#include "fseq_joinbip.hpp"

namespace fseq {

// The cap: the solver's LDS is 33 bytes a column -- u, v, minv (8 each), p, way, srcl, sr (2 each: every value is at most
// X < 2^16), used (1) -- so X = 4,096 needs 4,097 x 33 = 135,201 bytes = 132.1 KiB of the 160 KiB a CU has, one workgroup a
// CU.  (8,192 columns would need 264 KiB; 4-byte indices at 4,096 columns 164 KiB.)  A slab at the cap is 64 MiB.
constexpr uint32_t JBW_MAX_TEXTS = 4096;
constexpr uint32_t JBW_T = 256;                          // threads of every kernel here
constexpr uint32_t JBW_NW = JBW_T / WAVE;
constexpr size_t JBW_LDS_CU = 160u * 1024u;              // LDS of a CU
static_assert(JBW_MAX_TEXTS < 0xFFFFu, "texts, rows and columns of a pair are 16-bit words in LDS and in tpos / src / matching");

// smallest row of every class.  A class is the run of pBWT positions [start[c], start[c + 1]) and of_row[row] is the class
// whose run holds row's position, so the minimum of snap_a over the run is the minimum of the rows with of_row[row] = c.
static __global__ __launch_bounds__(JBW_T) void k_bip_minrow_wide(
	uint16_t const *__restrict__ of_row, uint32_t m, uint32_t X, uint32_t *__restrict__ minrow)
{
	__shared__ uint32_t mn[JBW_MAX_TEXTS];
	uint32_t const s = blockIdx.x, tid = threadIdx.x;
	for (uint32_t c = tid; c < X; c += JBW_T) mn[c] = 0xFFFFFFFFu;
	__syncthreads();
	uint16_t const *of = of_row + (size_t) s * m;
	for (uint32_t row = tid; row < m; row += JBW_T)
	{
		uint32_t const c = of[row];
		if (c < X) atomicMin(&mn[c], row);               // (a class count above X -- which the host rejects afterwards -- has classes no table holds)
	}
	__syncthreads();
	for (uint32_t c = tid; c < X; c += JBW_T) minrow[(size_t) s * X + c] = mn[c];
}

__host__ __device__ inline size_t bip_texts_wide_lds_bytes(uint32_t X) { return (size_t) X * 14u; }

// k_bip_texts for up to JBW_MAX_TEXTS classes: tpos[s][class], src[s][text], reprow[s][text] (fseq_joinbip.hpp)
static __global__ __launch_bounds__(JBW_T) void k_bip_texts_wide(
	uint32_t const *__restrict__ count, uint32_t const *__restrict__ size, uint32_t const *__restrict__ minrow, uint32_t m, uint32_t X,
	uint16_t *__restrict__ tpos, uint16_t *__restrict__ src, uint32_t *__restrict__ reprow)
{
	extern __shared__ __attribute__((aligned(16))) uint32_t jt_lds[];
	uint32_t *const c_size = jt_lds;                             // [X] sizes by class
	uint32_t *const t_size = c_size + X;                         // [X] sizes by text
	uint32_t *const t_min = t_size + X;                          // [X] first rows by text
	uint16_t *const t_src = reinterpret_cast<uint16_t *>(t_min + X);      // [X]
	uint32_t const s = blockIdx.x, tid = threadIdx.x;
	uint32_t const nc = min(count[s], X);
	for (uint32_t c = tid; c < nc; c += JBW_T) c_size[c] = size[(size_t) s * X + c];
	__syncthreads();
	// fewer classes than slots: the texts in descending order of their sizes, equal sizes in the classes' order (the stable
	// rank k_bip_texts computes), else the classes' own order
	bool const sorted = nc < X;
	for (uint32_t c = tid; c < nc; c += JBW_T)
	{
		uint32_t const mine = c_size[c];
		uint32_t pos = c;
		if (sorted)
		{
			pos = 0;
			for (uint32_t c2 = 0; c2 < nc; ++c2)
			{
				uint32_t const other = c_size[c2];
				pos += (other > mine || (other == mine && c2 < c)) ? 1u : 0u;
			}
		}
		tpos[(size_t) s * X + c] = (uint16_t) pos;
		t_size[pos] = mine;
		t_min[pos] = minrow[(size_t) s * X + c];
		t_src[pos] = (uint16_t) pos;
	}
	__syncthreads();
	if (tid == 0 && sorted && nc)
	{
		// the placeholders: copies in proportion to the texts' sizes, then one each in turn -- the host's expression in double
		uint32_t remaining = X - nc, it = nc;
		for (uint32_t i = 0; i < nc && remaining; ++i)
		{
			double const share = ceil(1.0 * (double) t_size[i] / (double) m * (double) remaining);
			uint32_t const cn = share < (double) remaining ? (uint32_t) share : remaining;
			for (uint32_t k = 0; k < cn; ++k) t_src[it++] = (uint16_t) i;
			remaining -= cn;
		}
		while (remaining)
			for (uint32_t i = 0; i < nc && remaining; ++i) { t_src[it++] = (uint16_t) i; --remaining; }
	}
	__syncthreads();
	for (uint32_t i = tid; i < X; i += JBW_T)
	{
		uint32_t const r = nc ? t_src[i] : 0u;
		src[(size_t) s * X + i] = (uint16_t) r;
		reprow[(size_t) s * X + i] = nc ? t_min[r] : 0xFFFFFFFFu;
	}
}

__host__ __device__ inline size_t bip_match_wide_lds_bytes(uint32_t X) { return (((size_t) X + 1u) * 33u + 15u) & ~(size_t) 15u; }

// Workgroup g, pairs g, g + gridDim.x, ...: matching[p][l] = r of a maximum-weight perfect matching of pair p = (segment p,
// segment p + 1).  slabs: gridDim.x x X x X words; a workgroup zeroes the nl x nr cells a pair uses, counts the rows into
// them and reads them back itself (its own stores and atomics, ordered by the workgroup's barriers; the reads are served by L2).
static __global__ __launch_bounds__(JBW_T) void k_bip_match_wide(
	uint16_t const *__restrict__ of_row, uint32_t const *__restrict__ count, uint16_t const *__restrict__ tpos, uint16_t const *__restrict__ src,
	uint32_t m, uint32_t X, uint32_t pairs, uint32_t *slabs, uint16_t *__restrict__ matching)
{
	extern __shared__ __attribute__((aligned(16))) unsigned char jbw_lds[];
	__shared__ long long r_best[JBW_NW];
	__shared__ uint32_t r_j[JBW_NW];
	size_t const X1 = (size_t) X + 1u;
	long long *const u_l = reinterpret_cast<long long *>(jbw_lds);           // [X + 1] potentials of the rows
	long long *const v_l = u_l + X1;                             // [X + 1] ... of the columns
	long long *const minv = v_l + X1;                            // [X + 1]
	uint16_t *const p_l = reinterpret_cast<uint16_t *>(minv + X1);           // [X + 1] row matched to column j (0: none)
	uint16_t *const way_l = p_l + X1;                            // [X + 1]
	uint16_t *const srcl = way_l + X1;                           // [X + 1] the real text of the left segment behind row i (at i - 1)
	uint16_t *const sr = srcl + X1;                              // [X + 1] the real text of the right segment behind column j (at j)
	uint8_t *const used = reinterpret_cast<uint8_t *>(sr + X1);  // [X + 1]
	uint32_t const tid = threadIdx.x, lane = lane_id();
	uint32_t const wv = (uint32_t) __builtin_amdgcn_readfirstlane((int) wave_id());
	uint32_t *const wreal = slabs + (size_t) blockIdx.x * X * X; // [nl][nr]: rows in real text l of the left and r of the right segment
	long long const INF = 0x1FFFFFFFFFFFFFFFll;                  // (the host's numeric_limits<int64_t>::max() / 4)
	for (uint32_t p = blockIdx.x; p < pairs; p += gridDim.x)
	{
		uint32_t const nl = min(count[p], X), nr = min(count[p + 1], X);
		uint16_t const *ofl = of_row + (size_t) p * m, *ofr = of_row + (size_t) (p + 1) * m;
		uint16_t const *tl = tpos + (size_t) p * X, *tr = tpos + (size_t) (p + 1) * X;
		__syncthreads();                                         // (the pair before this one is read to its end)
		for (uint32_t i = tid; i < nl * nr; i += JBW_T) wreal[i] = 0;
		for (uint32_t j = tid; j <= X; j += JBW_T) { u_l[j] = 0; v_l[j] = 0; p_l[j] = 0; way_l[j] = 0; }
		for (uint32_t j = tid; j < X; j += JBW_T)
		{
			srcl[j] = src[(size_t) p * X + j];
			sr[j + 1u] = src[(size_t) (p + 1) * X + j];
		}
		__syncthreads();
		for (uint32_t row = tid; row < m; row += JBW_T)
		{
			uint32_t const cl = ofl[row], cr = ofr[row];
			if (cl < nl && cr < nr) atomicAdd(&wreal[(uint32_t) tl[cl] * nr + tr[cr]], 1u);
		}
		__syncthreads();
		for (uint32_t i = 1; i <= X; ++i)
		{
			if (tid == 0) p_l[0] = (uint16_t) i;
			for (uint32_t j = tid + 1u; j <= X; j += JBW_T) { minv[j] = INF; used[j] = 0; }
			__syncthreads();
			uint32_t j0 = 0;
			do
			{
				uint32_t const i0 = p_l[j0];
				long long const ui0 = u_l[i0];
				uint32_t const *const wrow = wreal + (size_t) srcl[i0 - 1u] * nr;
				long long best = INF;
				uint32_t bestj = 0xFFFFFFFFu;
				// (column j belongs to thread (j - 1) % JBW_T alone: used, v, minv and way of a column have one writer)
				for (uint32_t j = tid + 1u; j <= X; j += JBW_T)
				{
					if (j == j0) used[j] = 1;
					else if (!used[j])
					{
						// (the counters were made by atomics, which run in L2: the load goes there too, past this CU's L1,
						// which may hold the line from the pair before)
						uint32_t const w = __hip_atomic_load(wrow + sr[j], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
						long long const cur = -(long long) w - ui0 - v_l[j];
						long long mv = minv[j];
						if (cur < mv) { mv = cur; minv[j] = cur; way_l[j] = (uint16_t) j0; }
						if (mv < best) { best = mv; bestj = j; }         // (the lowest column among equal ones: ascending j)
					}
				}
#pragma unroll
				for (int off = 32; off >= 1; off >>= 1)
				{
					long long const ob = __shfl_xor(best, off, WAVE);
					uint32_t const oj = (uint32_t) __shfl_xor((int) bestj, off, WAVE);
					if (ob < best || (ob == best && oj < bestj)) { best = ob; bestj = oj; }
				}
				if (lane == 0) { r_best[wv] = best; r_j[wv] = bestj; }
				__syncthreads();                                 // (and u_l[i0] has been read by everybody)
				best = r_best[0]; bestj = r_j[0];
#pragma unroll
				for (uint32_t k = 1; k < JBW_NW; ++k)
				{
					long long const ob = r_best[k];
					uint32_t const oj = r_j[k];
					if (ob < best || (ob == best && oj < bestj)) { best = ob; bestj = oj; }
				}
				long long const delta = best;
				for (uint32_t j = tid + 1u; j <= X; j += JBW_T)
				{
					if (used[j]) { u_l[p_l[j]] += delta; v_l[j] -= delta; }      // (matched columns have distinct rows)
					else minv[j] -= delta;
				}
				if (tid == 0) u_l[p_l[0]] += delta;
				__syncthreads();
				j0 = bestj;
			} while (p_l[j0] != 0u);
			__syncthreads();                                     // (every wave has left the loop before p_l changes)
			if (tid == 0)
			{
				do
				{
					uint32_t const j1 = way_l[j0];
					p_l[j0] = p_l[j1];
					j0 = j1;
				} while (j0);
			}
			__syncthreads();
		}
		for (uint32_t j = tid + 1u; j <= X; j += JBW_T) matching[(size_t) p * X + p_l[j] - 1u] = (uint16_t) (j - 1u);
	}
}

// slot i's chain through the matchings depends on no other slot: one thread per slot, perm[s][i] = the first row of the
// text that slot i's text of segment s - 1 is matched to (k_bip_chain, from memory)
static __global__ __launch_bounds__(JBW_T) void k_bip_chain_wide(
	uint16_t const *__restrict__ matching, uint32_t const *__restrict__ reprow, uint32_t S, uint32_t X, uint32_t *__restrict__ perm)
{
	uint32_t const i = blockIdx.x * JBW_T + threadIdx.x;
	if (i >= X) return;
	uint32_t order = i;
	perm[i] = reprow[i];
	for (uint32_t s = 1; s < S; ++s)
	{
		uint32_t const matched = min((uint32_t) matching[(size_t) (s - 1u) * X + order], X - 1u);
		perm[(size_t) s * X + i] = reprow[(size_t) s * X + matched];
		order = matched;
	}
}

} // namespace fseq
