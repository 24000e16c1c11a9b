// fseq_graphthread.hpp -- rows that are not the graph's own threaded through the founder block graph of a finished run
// (fseq_graph_thread_rows, fseq_graph_thread_held_out; csrc/fseq_api_graph.hip, beside GraphTables, which is built with its edges).
//
// For every (query row, segment) the node whose substring the query carries, for every (query row, junction) the edge between
// the two nodes, and the statistics of both.  The queries lie column-major and packed like the alignment, possibly at another
// width (sigma = 4: 2-bit rows, 4-bit queries, whose code 4 is a byte outside the alphabet), so everything here compares CODES.
//   k_gt_keys       a 64-bit key of every class of every segment: lanes along the classes, a loop over the segment's columns; a
//                   wave reads within one packed column of ld bytes at rep >> bsh, never at stride ld; the key stays in
//                   registers: key = key * GT_MUL + code + 1 a column, a mixing step at the end, then the truncation to
//                   key_bits (FSEQ_GRAPH_THREAD_KEY_BITS) -- after the mixing, so that few bits still spread.  A segment is not
//                   cut into column chunks: the polynomial form would allow it, nothing measured asks for it.
//   k_gt_thread     one workgroup per (segment, tiles of 256 queries): the segment's keys and classes go into an LDS table with
//                   open addressing and linear probing, `slots` = the power of two from twice max_segment_size on (at most half
//                   full: 8,192 slots for 4,096 classes, 96 KiB).  Two arrays, not one of pairs: the classes are 32-bit words
//                   (the empty test of a probe is one ds_read_b32, and the insert's compare-and-swap has its word), the keys
//                   64-bit words read only in occupied slots; the slots of a wave's probes are spread by the keys, so no layout
//                   orders them on the banks.  Then every query's key, lanes along the queries (contiguous bytes of a query
//                   column); a query that meets a code >= sigma is unmatched.  The probe runs from the key's slot to the empty
//                   slot that ends the chain, and EVERY entry with the query's key on the way is a candidate that is compared
//                   code by code with the class's representative row: the result is exact whatever the keys do, two classes
//                   with one key are both looked at, and at most one candidate can pass (the classes of a segment are distinct
//                   substrings).  The insert's compare-and-swap decides where an entry lies in its chain and nothing else:
//                   the set of occupied slots of linear probing does not depend on the order of the inserts, every entry
//                   with key K lies between K's slot and the chain's end, and a probe visits them all -- neither the nodes
//                   nor the counts of candidates depend on it.
//   k_gt_steps      one lane per (junction, query): l << 16 | r is searched in the junction's slice of k_join_edges_wide<true>'s
//                   output, ascending by construction; the step is offset[p] + k, the index of the edge in fseq_block_graph's
//                   edges.
//   k_gt_exceptions the restored form alone (a context over the kept columns of a longer source, queries of the source's length):
//                   k_gt_keys / k_gt_thread run on the kept columns as they are, then one lane per query walks the query's
//                   exception cells -- the identity columns in which it differs from row 0 -- and unmatches the segment
//                   whose source range holds one, before k_gt_steps looks for the edges
//   k_gt_rows       one lane per query walks the S segments: the loads of a wave are contiguous in [S][Q]
//   k_gt_segments   one workgroup per segment counts along the queries; integer sums, which do not depend on the order of
//                   their atomics
// No atomic decides an order, no kernel waits on another workgroup, every table value is clipped before it indexes (class <
// count <= X, row < m, query < Q, a slot by the table's mask, a column < n), every store is bounded by its array's size.
#pragma once

#include "fseq_graph.hpp"

namespace fseq {

constexpr uint32_t GT_T = 256;                           // threads of every kernel here = queries of a tile
constexpr uint32_t GT_MAX_CLASSES = 4096;                // the cap of the device join score and the bipartite joiner
constexpr uint32_t GT_MIN_SLOTS = 64;
constexpr uint32_t GT_NONE = 0xFFFFFFFFu;                // FSEQ_GRAPH_NONE; an empty slot of the table
constexpr uint64_t GT_MUL = 0x9E3779B97F4A7C15ull;
static_assert(GT_NONE == (uint32_t) FSEQ_GRAPH_NONE, "the kernels' mark of no node is the ABI's");

struct GraphThreadArgs {
	uint64_t const *seg_lb, *seg_rb;         // [S]
	uint32_t const *count, *rep, *noff;      // [S], [S][X], [S + 1]
	uint32_t m, X, S;
	uint64_t n;
	uint8_t const *msa;                      // the alignment: packed, column-major
	size_t ld;
	uint32_t bsh;
	uint8_t const *q;                        // the queries, the same way at their own width
	size_t qld;
	uint32_t qbsh, Q, sigma;
	uint32_t key_bits, slots;
	uint64_t *keys;                          // [S][X]
	uint32_t *nodes, *steps;                 // [S][Q], [S - 1][Q]
	uint2 const *edges;
	uint32_t const *offset, *nedges;         // [pairs]
	uint32_t pairs;
	uint64_t n_edges;
	unsigned long long *stats;               // candidates verified, candidates rejected, cells with a byte outside the alphabet
	// the restored form alone (fseq_graph_thread_rows_restored / _held_out_restored): the segments' source ranges, and the
	// queries' exception cells (csrc/fseq_exceptions.hpp): query q's are exc_cols[exc_off[q] .. exc_off[q + 1]), ascending
	uint64_t const *src_lb, *src_rb;         // [S]
	uint64_t n_src;
	uint64_t const *exc_off;                 // [Q + 1]
	uint32_t const *exc_cols;                // [n_exc]
	uint64_t n_exc;
};

// the code of `row` in a packed column
__device__ __forceinline__ uint32_t gt_code(uint8_t const *__restrict__ col, uint32_t row, uint32_t bsh)
{
	uint32_t const bits = 8u >> bsh;
	return ((uint32_t) col[row >> bsh] >> ((row & ((1u << bsh) - 1u)) * bits)) & ((1u << bits) - 1u);
}

__device__ __forceinline__ uint64_t gt_key_step(uint64_t key, uint32_t code) { return key * GT_MUL + code + 1u; }

__device__ __forceinline__ uint64_t gt_key_end(uint64_t key, uint32_t key_bits)
{
	key ^= key >> 30; key *= 0xBF58476D1CE4E5B9ull;
	key ^= key >> 27; key *= 0x94D049BB133111EBull;
	key ^= key >> 31;
	return key_bits >= 64u ? key : key & ((1ull << key_bits) - 1ull);
}

__device__ __forceinline__ uint32_t gt_slot(uint64_t key, uint32_t slots) { return ((uint32_t) key ^ (uint32_t) (key >> 32)) & (slots - 1u); }

// the columns of segment s, inside the alignment
__device__ __forceinline__ void gt_columns(GraphThreadArgs const &A, uint32_t s, uint64_t &lb, uint64_t &rb)
{
	rb = min(A.seg_rb[s], A.n);
	lb = min(A.seg_lb[s], rb);
}

// workgroup (s, y): the classes [y GT_T, (y + 1) GT_T) of segment s
static __global__ __launch_bounds__(GT_T) void k_gt_keys(GraphThreadArgs A)
{
	uint32_t const s = blockIdx.x, j = blockIdx.y * GT_T + threadIdx.x;
	if (j >= min(A.count[s], A.X)) return;
	uint32_t const row = A.rep[(size_t) s * A.X + j];
	uint64_t lb, rb, key = 0;
	gt_columns(A, s, lb, rb);
	if (row < A.m)
		for (uint64_t k = lb; k < rb; ++k) key = gt_key_step(key, gt_code(A.msa + k * A.ld, row, A.bsh));
	A.keys[(size_t) s * A.X + j] = gt_key_end(key, A.key_bits);
}

// workgroup (s, y): segment s, the query tiles y, y + gridDim.y, ...; dynamic LDS: slots x (8 + 4) bytes
static __global__ __launch_bounds__(GT_T) void k_gt_thread(GraphThreadArgs A)
{
	extern __shared__ __attribute__((aligned(16))) uint64_t gt_table[];
	__shared__ uint32_t sums[3];
	uint32_t const s = blockIdx.x, tid = threadIdx.x, slots = A.slots, Q = A.Q;
	uint64_t *const tkey = gt_table;
	uint32_t *const tcls = reinterpret_cast<uint32_t *>(gt_table + slots);
	uint32_t const nc = min(min(A.count[s], A.X), slots / 2u);
	for (uint32_t i = tid; i < slots; i += GT_T) tcls[i] = GT_NONE;
	if (tid < 3u) sums[tid] = 0;
	__syncthreads();
	for (uint32_t j = tid; j < nc; j += GT_T)
	{
		uint64_t const key = A.keys[(size_t) s * A.X + j];
		uint32_t h = gt_slot(key, slots);
		for (uint32_t probe = 0; probe < slots; ++probe, h = (h + 1u) & (slots - 1u))
			if (atomicCAS(&tcls[h], GT_NONE, j) == GT_NONE) { tkey[h] = key; break; }
	}
	__syncthreads();                       // (the table is this workgroup's own stores)
	uint64_t lb, rb;
	gt_columns(A, s, lb, rb);
	uint32_t verified = 0, rejected = 0, outside = 0;
	for (uint64_t q0 = (uint64_t) blockIdx.y * GT_T; q0 < Q; q0 += (uint64_t) gridDim.y * GT_T)
	{
		uint64_t const q64 = q0 + tid;
		if (q64 >= Q) continue;
		uint32_t const q = (uint32_t) q64;
		uint64_t key = 0;
		bool bad = false;
		for (uint64_t k = lb; k < rb; ++k)
		{
			uint32_t const code = gt_code(A.q + k * A.qld, q, A.qbsh);
			bad |= code >= A.sigma;
			key = gt_key_step(key, code);
		}
		key = gt_key_end(key, A.key_bits);
		uint32_t found = GT_NONE;
		if (bad) ++outside;
		else
		{
			uint32_t h = gt_slot(key, slots);
			for (uint32_t probe = 0; probe < slots; ++probe, h = (h + 1u) & (slots - 1u))
			{
				uint32_t const cls = tcls[h];
				if (cls == GT_NONE) break;
				if (tkey[h] != key) continue;
				++verified;
				uint32_t const row = cls < nc ? A.rep[(size_t) s * A.X + cls] : A.m;
				bool same = row < A.m;
				for (uint64_t k = lb; same && k < rb; ++k)
					same = gt_code(A.q + k * A.qld, q, A.qbsh) == gt_code(A.msa + k * A.ld, row, A.bsh);
				if (same) found = cls;
				else ++rejected;
			}
		}
		A.nodes[(size_t) s * Q + q] = found == GT_NONE ? GT_NONE : A.noff[s] + found;
	}
	if (verified) atomicAdd(&sums[0], verified);
	if (rejected) atomicAdd(&sums[1], rejected);
	if (outside) atomicAdd(&sums[2], outside);
	__syncthreads();
	if (tid < 3u && sums[tid]) atomicAdd(&A.stats[tid], (unsigned long long) sums[tid]);
}

// The restored form, between k_gt_thread and k_gt_steps: a query with an exception cell in a segment's source range carries no
// node of it.  One lane per query walks the query's ascending cells; the segment of a cell is the last s with src_lb[s] <= cell
// (the ranges tile [0, n_src)), and the cells up to that segment's src_rb are skipped.  A lane stores into its own query's
// column of nodes[][] only, so nothing races.
static __global__ __launch_bounds__(GT_T) void k_gt_exceptions(GraphThreadArgs A)
{
	uint64_t const q = (uint64_t) blockIdx.x * GT_T + threadIdx.x;
	uint32_t const Q = A.Q, S = A.S;
	if (q >= Q || 0 == S) return;
	uint64_t at = A.exc_off[q];
	uint64_t const end = min(A.exc_off[q + 1u], A.n_exc);
	uint64_t done = 0;                       // the source positions below this are dealt with
	while (at < end)
	{
		uint64_t const cell = A.exc_cols[at++];
		if (cell < done || cell >= A.n_src) continue;
		uint32_t lo = 0, hi = S;             // src_lb[lo] <= cell (src_lb[0] = 0)
		while (hi - lo > 1u)
		{
			uint32_t const mid = lo + (hi - lo) / 2u;
			if (A.src_lb[mid] <= cell) lo = mid;
			else hi = mid;
		}
		A.nodes[(size_t) lo * Q + q] = GT_NONE;
		done = max(A.src_rb[lo], cell + 1u);
	}
}

// workgroup (p, y): junction p, the query tiles y, y + gridDim.y, ...
static __global__ __launch_bounds__(GT_T) void k_gt_steps(GraphThreadArgs A)
{
	uint32_t const p = blockIdx.x, Q = A.Q;
	if (p >= A.pairs) return;
	uint64_t const base = min((uint64_t) A.offset[p], A.n_edges);
	uint32_t const ne = (uint32_t) min((uint64_t) A.nedges[p], A.n_edges - base);
	uint32_t const id_l = A.noff[p], id_r = A.noff[p + 1u];
	for (uint64_t q = (uint64_t) blockIdx.y * GT_T + threadIdx.x; q < Q; q += (uint64_t) gridDim.y * GT_T)
	{
		uint32_t const l = A.nodes[(size_t) p * Q + q], r = A.nodes[(size_t) (p + 1u) * Q + q];
		uint32_t step = GT_NONE;
		if (l != GT_NONE && r != GT_NONE)
		{
			uint32_t const w = ((l - id_l) << 16) | ((r - id_r) & 0xFFFFu);
			uint32_t lo = 0, hi = ne;
			while (lo < hi)
			{
				uint32_t const mid = lo + (hi - lo) / 2u;
				if (A.edges[base + mid].x < w) lo = mid + 1u;
				else hi = mid;
			}
			if (lo < ne && A.edges[base + lo].x == w) step = (uint32_t) (base + lo);
		}
		A.steps[(size_t) p * Q + q] = step;
	}
}

// the columns the statistics count for segment s: SRC: its source range, inside the source
template <bool SRC>
__device__ __forceinline__ void gt_counted_columns(GraphThreadArgs const &A, uint32_t s, uint64_t &lb, uint64_t &rb)
{
	if constexpr (SRC)
	{
		rb = min(A.src_rb[s], A.n_src);
		lb = min(A.src_lb[s], rb);
	}
	else gt_columns(A, s, lb, rb);
}

// per_row[q]: one lane per query.  SRC: the column counts are the source's (the restored form)
template <bool SRC>
static __global__ __launch_bounds__(GT_T) void k_gt_rows(GraphThreadArgs A, fseq_graph_thread_row *__restrict__ per_row)
{
	uint64_t const q = (uint64_t) blockIdx.x * GT_T + threadIdx.x;
	uint32_t const Q = A.Q;
	if (q >= Q) return;
	fseq_graph_thread_row R{};
	uint32_t run_segments = 0;               // the walk under way (0: none)
	uint64_t run_columns = 0;
	bool linked = false;                     // the junction in front of segment s
	for (uint32_t s = 0; s < A.S; ++s)
	{
		bool const matched = A.nodes[(size_t) s * Q + q] != GT_NONE;
		uint64_t lb, rb;
		gt_counted_columns<SRC>(A, s, lb, rb);
		if (matched)
		{
			++R.segments_matched;
			R.columns_matched += rb - lb;
			if (run_segments && linked) { ++run_segments; run_columns += rb - lb; }
			else
			{
				if (run_segments) ++R.junctions_novel;           // (both sides matched, no edge)
				++R.walks; run_segments = 1; run_columns = rb - lb;
			}
			R.longest_walk_segments = max(R.longest_walk_segments, run_segments);
			R.longest_walk_columns = max(R.longest_walk_columns, run_columns);
		}
		else run_segments = 0;
		linked = s + 1u < A.S && A.steps[(size_t) s * Q + q] != GT_NONE;
		if (linked) ++R.junctions_linked;
	}
	per_row[q] = R;
}

// per_segment[s]: one workgroup per segment
static __global__ __launch_bounds__(GT_T) void k_gt_segments(GraphThreadArgs A, fseq_graph_thread_segment *__restrict__ per_segment)
{
	__shared__ uint32_t sums[3];
	uint32_t const s = blockIdx.x, tid = threadIdx.x, Q = A.Q;
	if (tid < 3u) sums[tid] = 0;
	__syncthreads();
	bool const junction = s + 1u < A.S;
	uint32_t matched = 0, linked = 0, novel = 0;
	for (uint64_t q = tid; q < Q; q += GT_T)
	{
		bool const here = A.nodes[(size_t) s * Q + q] != GT_NONE;
		matched += here;
		if (junction)
		{
			bool const step = A.steps[(size_t) s * Q + q] != GT_NONE;
			linked += step;
			novel += !step && here && A.nodes[(size_t) (s + 1u) * Q + q] != GT_NONE;
		}
	}
	if (matched) atomicAdd(&sums[0], matched);
	if (linked) atomicAdd(&sums[1], linked);
	if (novel) atomicAdd(&sums[2], novel);
	__syncthreads();
	if (tid == 0) per_segment[s] = fseq_graph_thread_segment{sums[0], sums[1], sums[2], 0u};
}

} // namespace fseq
