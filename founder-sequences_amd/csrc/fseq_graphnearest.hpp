// fseq_graphnearest.hpp -- for rows threaded through the founder block graph, the NEAREST node of every segment and how far it is
// (fseq_graph_nearest_rows, fseq_graph_nearest_held_out, fseq_debug_graph_nearest; csrc/fseq_api_graph.hip, beside the threading
// of csrc/fseq_graphthread.hpp, whose k_gt_steps runs here unchanged).
//
// For every (query q, segment s): the Hamming distance, in CODES, to the representative row of every class of s, its minimum, the
// smallest class that attains it and the number of classes that do.  The alignment and the queries lie column-major and packed,
// possibly at different widths, so comparing them where they lie is a byte gather a code.  Instead:
//   k_gn_pack<false> the class representatives of a batch of whole segments as row-major words at the queries' width w (never
//                    below the rows'): lanes along the classes, a wave reads within one packed column of ld bytes at rep >> bsh,
//                    as k_gt_keys does, never at stride ld; a lane builds a word in a register from 32 / w consecutive columns.
//                    Class j of segment s lies at roff[s] - roff[s0] + j nw(s), its words contiguous.
//   k_gn_pack<true>  the queries of the same segments: lanes along the queries (contiguous bytes of a query column), word k of
//                    segment s at [qoff[s] - qoff[s0] + k][Q], so that a wave's loads in the distance kernel are contiguous.
//                    Every segment starts on a word boundary, and the codes behind a segment's last column are 0 on both sides:
//                    padding is never a mismatch.
//   k_gn_distance<W> one workgroup per (segment, tiles of 256 queries), lanes along the queries, the loop over the classes
//                    wave-uniform: x = a ^ b, the W bits of a code folded into one, __popc -- 32 / W codes an operation.  The
//                    class words are the same for every lane: their address is made of launch arguments, the block index and
//                    the loop counters alone (uniform loads).  A lane keeps the segment's query words in registers up to
//                    GN_REG_WORDS; above that it reads them again for every class, contiguous along the wave.  The running
//                    minimum, the smallest class and the tie count are a lane's own.  There is no early exit: every class is
//                    looked at, so `ties` is what the definition says.  It also writes the temporary k_gt_steps reads: the node
//                    where the distance is at most max_distance, FSEQ_GRAPH_NONE elsewhere.
//   k_gn_rows        one lane per query walks the S segments (k_gt_rows' shape); k_gn_segments one workgroup per segment
//                    (k_gt_segments' shape): integer sums and maxima, which do not depend on the order of their atomics.
// As in fseq_graphthread.hpp: no atomic decides an order, no kernel waits on another workgroup, every table value is clipped
// before it indexes (class < count <= X, row < m, a column < n, a word offset against its array's size), every store is bounded by
// its array's size.  There is no table in LDS, so the threading's cap of 4,096 classes a segment is not this feature's.
#pragma once

#include "fseq_graphthread.hpp"
#include "fseq_graphnearest_plan.hpp"

namespace fseq {

constexpr uint32_t GN_REG_WORDS = 16;                    // query words of a segment a lane keeps in registers

struct GraphNearestArgs {
	GraphThreadArgs G;                       // the threading's: G.nodes is the temporary of admitted nodes, G.steps the steps
	uint32_t s0, s1;                         // the batch: segments [s0, s1)
	uint64_t const *qoff, *roff;             // [S + 1] (graph_nearest_words)
	uint32_t *rw, *qw;                       // the batch's packed representatives and queries
	uint64_t rw_cap, qw_cap;                 // ... and their sizes in words
	uint32_t max_distance;
	uint32_t *nodes, *distances, *ties;      // [S][Q]
};

// the words of segment s, as both the pack kernels and the distance kernel count them (0: the tables contradict each other)
__device__ __forceinline__ uint32_t gn_segment_words(GraphNearestArgs const &A, uint32_t s, uint64_t lb, uint64_t rb)
{
	uint64_t const cpw = 4u << A.G.qbsh, want = (rb - lb + cpw - 1u) / cpw, have = A.qoff[s + 1u] - A.qoff[s];
	return want == have && want <= 0x3FFFFFFFull ? (uint32_t) want : 0u;
}

// workgroup (x, y): segment s0 + x; QUERIES: the query tiles y, y + gridDim.y, ..., else the class tiles
template <bool QUERIES>
static __global__ __launch_bounds__(GT_T) void k_gn_pack(GraphNearestArgs A)
{
	GraphThreadArgs const &G = A.G;
	uint32_t const s = A.s0 + blockIdx.x;
	if (s >= A.s1 || s >= G.S) return;
	uint64_t lb, rb;
	gt_columns(G, s, lb, rb);
	uint32_t const w = 8u >> G.qbsh, cpw = 32u / w, nw = gn_segment_words(A, s, lb, rb);
	uint32_t const items = QUERIES ? G.Q : min(G.count[s], G.X);
	uint64_t const base = QUERIES ? A.qoff[s] - A.qoff[A.s0] : A.roff[s] - A.roff[A.s0];
	for (uint64_t i64 = (uint64_t) blockIdx.y * GT_T + threadIdx.x; i64 < items; i64 += (uint64_t) gridDim.y * GT_T)
	{
		uint32_t const i = (uint32_t) i64;
		uint32_t const row = QUERIES ? i : G.rep[(size_t) s * G.X + i];
		bool const have = QUERIES || row < G.m;
		for (uint32_t k = 0; k < nw; ++k)
		{
			uint32_t word = 0;
			uint64_t const c0 = lb + (uint64_t) k * cpw;
			if (have)
				for (uint32_t e = 0; e < cpw && c0 + e < rb; ++e)
					word |= (QUERIES ? gt_code(G.q + (c0 + e) * G.qld, row, G.qbsh) : gt_code(G.msa + (c0 + e) * G.ld, row, G.bsh)) << (e * w);
			if constexpr (QUERIES)
			{
				uint64_t const at = (base + k) * G.Q + i;
				if (at < A.qw_cap) A.qw[at] = word;
			}
			else
			{
				uint64_t const at = base + (uint64_t) i * nw + k;
				if (at < A.rw_cap) A.rw[at] = word;
			}
		}
	}
}

// the codes in which two words of W-bit codes differ
template <uint32_t W>
__device__ __forceinline__ uint32_t gn_differ(uint32_t a, uint32_t b)
{
	uint32_t x = a ^ b;
	if constexpr (W == 2) x = (x | x >> 1) & 0x55555555u;
	else if constexpr (W == 4) { x |= x >> 1; x = (x | x >> 2) & 0x11111111u; }
	else { x |= x >> 1; x |= x >> 2; x = (x | x >> 4) & 0x01010101u; }
	return (uint32_t) __popc(x);
}

// workgroup (x, y): segment s0 + x, the query tiles y, y + gridDim.y, ...; rw_all = A.rw, qw_all = A.qw
template <uint32_t W>
static __global__ __launch_bounds__(GT_T) void k_gn_distance(GraphNearestArgs A, uint32_t const *__restrict__ rw_all, uint32_t const *__restrict__ qw_all)
{
	GraphThreadArgs const &G = A.G;
	uint32_t const s = A.s0 + blockIdx.x, Q = G.Q;
	if (s >= A.s1 || s >= G.S) return;
	uint64_t lb, rb;
	gt_columns(G, s, lb, rb);
	uint32_t const nw = (uint32_t) __builtin_amdgcn_readfirstlane((int) gn_segment_words(A, s, lb, rb));
	uint32_t const nc = (uint32_t) __builtin_amdgcn_readfirstlane((int) min(G.count[s], G.X));
	uint64_t const rbase = A.roff[s] - A.roff[A.s0], qbase = A.qoff[s] - A.qoff[A.s0];
	// (what the pack kernels wrote lies inside the two arrays: else the plan and the tables disagree, and nothing is read)
	if (0 == nw || rbase + (uint64_t) nc * nw > A.rw_cap || (qbase + nw) * Q > A.qw_cap) return;
	// (A.rw and A.qw once more, as parameters of their own that nothing else aliases: the class words become scalar loads)
	uint32_t const *__restrict__ const rw = rw_all + rbase;
	uint32_t const *__restrict__ const qw = qw_all + qbase * Q;
	uint32_t const id0 = G.noff[s];
	for (uint64_t q0 = (uint64_t) blockIdx.y * GT_T; q0 < Q; q0 += (uint64_t) gridDim.y * GT_T)
	{
		uint64_t const q64 = q0 + threadIdx.x;
		bool const live = q64 < Q;
		uint32_t const q = live ? (uint32_t) q64 : Q - 1u;           // (a lane behind the last query reads the last one's words and stores nothing)
		uint32_t best = 0xFFFFFFFFu, arg = 0, ties = 0;
		if (nw <= GN_REG_WORDS)
		{
			uint32_t mine[GN_REG_WORDS];
#pragma unroll
			for (uint32_t k = 0; k < GN_REG_WORDS; ++k) mine[k] = k < nw ? qw[(size_t) k * Q + q] : 0u;
			for (uint32_t j = 0; j < nc; ++j)
			{
				uint32_t const *__restrict__ const theirs = rw + (size_t) j * nw;
				uint32_t d = 0;
#pragma unroll
				for (uint32_t k = 0; k < GN_REG_WORDS; ++k)
					if (k < nw) d += gn_differ<W>(mine[k], theirs[k]);
				if (d < best) { best = d; arg = j; ties = 1; }
				else ties += d == best;
			}
		}
		else
			for (uint32_t j = 0; j < nc; ++j)
			{
				uint32_t const *__restrict__ const theirs = rw + (size_t) j * nw;
				uint32_t d = 0;
				for (uint32_t k = 0; k < nw; ++k) d += gn_differ<W>(qw[(size_t) k * Q + q], theirs[k]);
				if (d < best) { best = d; arg = j; ties = 1; }
				else ties += d == best;
			}
		if (!live || 0 == nc) continue;
		size_t const at = (size_t) s * Q + q;
		uint32_t const node = id0 + arg;
		A.nodes[at] = node;
		A.distances[at] = best;
		A.ties[at] = ties;
		G.nodes[at] = best <= A.max_distance ? node : GT_NONE;
	}
}

// per_row[q]: one lane per query (k_gt_rows with "matched" read as "admitted", and the distances)
static __global__ __launch_bounds__(GT_T) void k_gn_rows(GraphNearestArgs A, fseq_graph_nearest_row *__restrict__ per_row)
{
	GraphThreadArgs const &G = A.G;
	uint64_t const q = (uint64_t) blockIdx.x * GT_T + threadIdx.x;
	uint32_t const Q = G.Q;
	if (q >= Q) return;
	fseq_graph_nearest_row R{};
	uint32_t run_segments = 0;               // the walk under way (0: none)
	uint64_t run_columns = 0;
	bool linked = false;                     // the junction in front of segment s
	for (uint32_t s = 0; s < G.S; ++s)
	{
		bool const admitted = G.nodes[(size_t) s * Q + q] != GT_NONE;
		uint32_t const d = A.distances[(size_t) s * Q + q];
		uint64_t lb, rb;
		gt_columns(G, s, lb, rb);
		R.mismatches += d;
		R.max_distance = max(R.max_distance, d);
		if (admitted)
		{
			++R.segments_admitted;
			R.segments_exact += 0 == d;
			R.columns_admitted += rb - lb;
			R.mismatches_admitted += d;
			if (run_segments && linked) { ++run_segments; run_columns += rb - lb; }
			else
			{
				if (run_segments) ++R.junctions_novel;           // (both sides admitted, no edge)
				++R.walks; run_segments = 1; run_columns = rb - lb;
			}
			R.longest_walk_segments = max(R.longest_walk_segments, run_segments);
			R.longest_walk_columns = max(R.longest_walk_columns, run_columns);
		}
		else run_segments = 0;
		linked = s + 1u < G.S && G.steps[(size_t) s * Q + q] != GT_NONE;
		if (linked) ++R.junctions_linked;
	}
	per_row[q] = R;
}

// per_segment[s]: one workgroup per segment
static __global__ __launch_bounds__(GT_T) void k_gn_segments(GraphNearestArgs A, fseq_graph_nearest_segment *__restrict__ per_segment)
{
	GraphThreadArgs const &G = A.G;
	__shared__ uint32_t sums[5];
	__shared__ unsigned long long total;
	uint32_t const s = blockIdx.x, tid = threadIdx.x, Q = G.Q;
	if (tid < 5u) sums[tid] = 0;
	if (tid == 5u) total = 0;
	__syncthreads();
	bool const junction = s + 1u < G.S;
	uint32_t admitted = 0, exact = 0, linked = 0, novel = 0, most = 0;
	unsigned long long mismatches = 0;
	for (uint64_t q = tid; q < Q; q += GT_T)
	{
		bool const here = G.nodes[(size_t) s * Q + q] != GT_NONE;
		uint32_t const d = A.distances[(size_t) s * Q + q];
		admitted += here;
		exact += here && 0 == d;
		mismatches += d;
		most = max(most, d);
		if (junction)
		{
			bool const step = G.steps[(size_t) s * Q + q] != GT_NONE;
			linked += step;
			novel += !step && here && G.nodes[(size_t) (s + 1u) * Q + q] != GT_NONE;
		}
	}
	if (admitted) atomicAdd(&sums[0], admitted);
	if (exact) atomicAdd(&sums[1], exact);
	if (linked) atomicAdd(&sums[2], linked);
	if (novel) atomicAdd(&sums[3], novel);
	if (most) atomicMax(&sums[4], most);
	if (mismatches) atomicAdd(&total, mismatches);
	__syncthreads();
	if (tid == 0) per_segment[s] = fseq_graph_nearest_segment{total, sums[0], sums[1], sums[2], sums[3], sums[4], 0u};
}

} // namespace fseq
