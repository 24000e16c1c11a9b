// fseq_graph.hpp -- the founder block graph of a finished run as a GFA 1.0 file, from what the device holds
// (fseq_write_block_graph, csrc/fseq_api_graph.hip).
//
// The graph: a node is a class of a merged segment (k_join_classes_wide's numbering, fseq_joinprep.hpp), node id = the classes
// of the segments in front + the class; an edge joins class l of segment p to class r of segment p + 1 with the rows that carry
// both as its weight (k_join_edges_wide's {l << 16 | r, rows}, ascending (l, r) per junction); every input row is a path.
// The file has three sections of lines, each in the count / scan / write pattern of fseq_segfile.hpp -- a line's length, a 64-bit
// exclusive scan, then every line written at its offset; no atomic decides an order and no kernel waits on another workgroup:
//   S  k_graph_node_lines   one workgroup per merged segment, a wave per node: the label is the representative row's bytes over
//                           [lb, rb) without the gap byte, so its length is counted -- lanes along the segment's columns of the
//                           packed alignment (2, 4 or 8 bits a code), a ballot of the lanes that keep their byte per strip of 64
//                           columns, the popcounts summed; the line's length from sf_digits; the scan inside the segment as
//                           k_segfile_lines does it (loff[s][j], stride X + 1), over the segments by k_segfile_scan itself
//      k_graph_write_nodes  one workgroup per segment a batch touches, a wave per line: the prefix, then the label compacted in
//                           order -- in a strip a lane's place is the running offset plus mbcnt of the ballot below it, the
//                           running offset moves on by the popcount, so the stores of a strip are contiguous -- then the tags,
//                           one lane a tag
//   L  k_graph_link_lines   one lane per edge, 256 edges a workgroup: the junction of an edge by a binary search in k_join_scan's
//                           offset[], the length from the three numbers' digits, the workgroup's bytes into btot[b]; k_segfile_scan
//                           over btot (64-bit); with `lens` the lengths of one workgroup's lines (where the host cuts a batch
//                           inside a workgroup's lines)
//      k_graph_write_links  the same lanes: the scan inside the workgroup again, then the line, a lane a line (17 to 47 bytes;
//                           the lanes of a wave cover one contiguous stretch)
//   P  k_graph_path_lines   one lane per input row, the segments one after the other: of_row is [S][m], so the loads of a wave
//                           are 128 contiguous bytes of one segment's classes; row i's line is S steps of digits(id + 1) + 2
//                           bytes; k_segfile_scan over the rows
//      k_graph_write_paths  the loads stay along the rows, the stores go along the line: a workgroup takes 64 rows and the
//                           segments 64 at a time through an LDS tile -- every wave loads 16 segments' classes of the 64 rows
//                           (lanes along the rows), then writes 16 rows' steps (lanes along the segments: a wave scan of the
//                           steps' lengths gives each its place, the 64 steps are one contiguous stretch of the line).  The
//                           other choice, a lane a row in the write as well, stores single bytes S x 6 bytes apart.
// The S section in the SOURCE's co-ordinates on an identity-reduced context (fseq_write_block_graph_restored): the two S kernels
// with RESTORED set.  The layout stays -- a workgroup a segment, a wave a node --, the lanes go along the source positions of
// the segment's range [src_lb, src_rb) (fseq_restored_bounds.hpp) in strips of 64, and a strip has two running cursors: the kept
// column (the segment's lb + the positions in front that are no identity columns: mbcnt / popcount of the ballot of !mask[p]) and
// the label (mbcnt / popcount of the ballot of "not the gap", as in the reduced form).  A lane at an identity column takes row 0's
// byte (ref[p]), a lane at a kept column the representative row's code at its column; a strip may hold no kept column, or 64.
// The lines' lb / rb are the source range.  The L and P sections are the reduced graph's: nothing of them has a restored form.
// Every store is checked against the batch buffer's size; every table value is clipped before it indexes (class < count <= X,
// row < m), as in the segfile kernels.  The bytes of a label are the alignment's, decoded through the context's code table.
#pragma once

#include "fseq_segfile.hpp"

namespace fseq {

constexpr uint32_t GR_T = SF_T;                          // threads of every kernel here
constexpr uint32_t GR_NW = GR_T / WAVE;
constexpr uint32_t GR_TILE = 64;                         // rows of a workgroup and segments of a pass of k_graph_write_paths
constexpr uint32_t GR_LINK_MAX = 17u + 3u * 10u;         // the longest L line
static_assert(GR_TILE == WAVE && GR_TILE % GR_NW == 0, "k_graph_write_paths: a wave's lanes are a tile's rows, then its segments");

__host__ __device__ inline uint32_t gr_digits64(uint64_t v)
{
	uint32_t d = 1;
	while (v >= 10u) { v /= 10u; ++d; }
	return d;
}

__device__ __forceinline__ void gr_put(uint8_t *out, uint64_t at, uint64_t cap, uint8_t b)
{
	if (at < cap) out[at] = b;
}

__device__ __forceinline__ void gr_put_dec64(uint8_t *out, uint64_t at, uint64_t cap, uint64_t v, uint32_t nd)
{
	for (uint32_t k = nd; k-- > 0;)
	{
		if (at + k < cap) out[at + k] = (uint8_t) ('0' + (uint32_t) (v % 10u));
		v /= 10u;
	}
}

// "\tab:i:" and the nd digits of v
__device__ __forceinline__ void gr_put_tag(uint8_t *out, uint64_t at, uint64_t cap, char a, char b, uint64_t v, uint32_t nd)
{
	gr_put(out, at, cap, (uint8_t) '\t'); gr_put(out, at + 1u, cap, (uint8_t) a); gr_put(out, at + 2u, cap, (uint8_t) b);
	gr_put(out, at + 3u, cap, (uint8_t) ':'); gr_put(out, at + 4u, cap, (uint8_t) 'i'); gr_put(out, at + 5u, cap, (uint8_t) ':');
	gr_put_dec64(out, at + 6u, cap, v, nd);
}

// what the kernels share of a call: the segments, the class tables, the first node of every segment, the alignment
struct GraphArgs {
	uint64_t const *seg_lb, *seg_rb;         // [S]
	uint32_t const *count, *rep, *size;      // [S], [S][X], [S][X]
	uint32_t const *noff;                    // [S + 1] nodes in front of a segment
	uint16_t const *of_row;                  // [S][m]
	uint32_t m, X, S;
	int32_t gap;                             // the byte a label leaves out; below 0: none
	uint8_t const *msa;                      // packed, column-major
	size_t ld;
	uint32_t bsh;
	uint8_t const *code_to_byte;             // [256]
	// the links: k_join_edges_wide's edges and k_join_scan's offsets
	uint2 const *edges;
	uint32_t const *offset;                  // [pairs]
	uint32_t pairs;
	uint64_t n_edges;
};

// the restored form of the S section (fseq_write_block_graph_restored): the segments' ranges in the SOURCE's co-ordinates
// (restored_segment_bounds, fseq_restored_bounds.hpp) and the identity columns of the context (fseq_identity.hpp).  Unread by
// the reduced form
struct GraphRestored {
	uint64_t const *src_lb, *src_rb;         // [S]
	uint8_t const *mask, *ref;               // [n_src]: 1 = identity column; row 0 of the source as raw bytes
	uint64_t n_src;
};

// a batch of the links or the paths: the lines [first, last) in file order, which begin `begin` bytes into their section;
// out holds `bytes` of them
struct GraphBatch {
	uint64_t first, last, begin, bytes;
};

// the classes of a segment, never 0 and never above X (the host refuses other counts before anything is written)
__device__ __forceinline__ uint32_t gr_count(GraphArgs const &A, uint32_t s) { return max(min(A.count[s], A.X), 1u); }

__device__ __forceinline__ uint64_t gr_node_tags_len(uint32_t lab, uint32_t rows, uint32_t s, uint64_t lb, uint64_t rb)
{
	return 6u + sf_digits(lab) + 6u + sf_digits(rows) + 6u + sf_digits(s) + 6u + gr_digits64(lb) + 6u + gr_digits64(rb) + 1u;
}

// One strip of 64 SOURCE positions of a restored label, [base, base + 64) inside [base, srb): a lane at an identity column takes
// row 0's byte, a lane at a kept column the representative row's code at column kc + (kept columns of the strip below the
// lane) -- the kept columns of a segment's source range are its [lb, rb) in order, so two cursors run along the strips: kc, which
// moves on by the strip's kept columns here, and the caller's label cursor.  A strip may hold no kept column, or 64.
// Returns whether the lane has a byte (b) at all; a column past rb (never: mask and kept are one context's) has none.
__device__ __forceinline__ bool gr_restored_byte(GraphArgs const &A, GraphRestored const &R, uint8_t const *lut, uint64_t base, uint64_t srb, uint64_t &kc, uint64_t rb,
                                                 uint32_t off, uint32_t sh, uint32_t cmask, uint32_t lane, uint8_t &b)
{
	uint64_t const p = base + lane;
	bool const in = p < srb && p < R.n_src;
	bool const ident = in && R.mask[p] != 0;
	uint64_t const kmask = __ballot(in && !ident);
	uint64_t const col = kc + __builtin_amdgcn_mbcnt_hi((uint32_t) (kmask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t) kmask, 0u));
	kc += (uint32_t) __popcll(kmask);
	bool have = ident;
	b = 0;
	if (ident) b = R.ref[p];
	else if (in && col < rb)
	{
		b = lut[(A.msa[col * A.ld + off] >> sh) & cmask];
		have = true;
	}
	return have;
}

// lab[s][j] (stride X): the bytes of node j's label; loff[s][j], j <= X (stride X + 1): bytes of the segment's lines in front of line j
// RESTORED: the label over the segment's source range (gr_restored_byte), the line's lb / rb the source's
template <bool RESTORED>
static __global__ __launch_bounds__(GR_T) void k_graph_node_lines(GraphArgs A, GraphRestored R, uint32_t *__restrict__ lab, uint64_t *__restrict__ loff)
{
	__shared__ uint8_t lut[256];
	__shared__ uint64_t scratch[GR_NW];
	uint32_t const s = blockIdx.x, tid = threadIdx.x, X = A.X, m = A.m, lane = lane_id();
	uint32_t const wv = (uint32_t) __builtin_amdgcn_readfirstlane((int) wave_id());
	lut[tid] = A.code_to_byte[tid];
	__syncthreads();
	uint32_t const nc = min(A.count[s], X);
	uint64_t const lb = A.seg_lb[s], rb = A.seg_rb[s], W = rb > lb ? rb - lb : 0u;
	uint64_t const plb = RESTORED ? R.src_lb[s] : lb, prb = RESTORED ? R.src_rb[s] : rb;      // what the line prints
	uint32_t const bits = 8u >> A.bsh, cmask = (1u << bits) - 1u;
	for (uint32_t j = wv; j < nc; j += GR_NW)
	{
		uint32_t const row = A.rep[(size_t) s * X + j];
		uint32_t n = 0;
		if (row < m)
		{
			uint32_t const off = row >> A.bsh, sh = (row & ((1u << A.bsh) - 1u)) * bits;
			if constexpr (RESTORED)
			{
				uint64_t kc = lb;
				for (uint64_t base = plb; base < prb; base += WAVE)
				{
					uint8_t b;
					bool const have = gr_restored_byte(A, R, lut, base, prb, kc, rb, off, sh, cmask, lane, b);
					n += (uint32_t) __popcll(__ballot(have && (A.gap < 0 || (int32_t) b != A.gap)));
				}
			}
			else
			for (uint64_t base = 0; base < W; base += WAVE)
			{
				uint64_t const k = base + lane;
				bool keep = false;
				if (k < W)
				{
					uint8_t const b = lut[(A.msa[(lb + k) * A.ld + off] >> sh) & cmask];
					keep = A.gap < 0 || (int32_t) b != A.gap;
				}
				n += (uint32_t) __popcll(__ballot(keep));
			}
		}
		if (lane == 0) lab[(size_t) s * X + j] = n;
	}
	__syncthreads();                       // (the labels' lengths are this workgroup's own stores)
	uint64_t *lo = loff + (size_t) s * ((size_t) X + 1u);
	uint32_t const id0 = A.noff[s];
	uint64_t running = 0;
	for (uint32_t base = 0; base < X; base += GR_T)
	{
		uint32_t const j = base + tid;
		uint64_t len = 0;
		if (j < nc)
		{
			uint32_t const n = lab[(size_t) s * X + j];
			len = 2u + sf_digits(id0 + j + 1u) + 1u + max(n, 1u) + gr_node_tags_len(n, A.size[(size_t) s * X + j], s, plb, prb);
		}
		uint64_t total;
		uint64_t const before = sf_block_excl_add64(len, scratch, &total);
		if (j < X) lo[j] = running + before;
		running += total;
	}
	if (tid == 0) lo[X] = running;
}

// the S lines of a batch (SegFileBatch: from line j_lo of segment s0 to line j_hi - 1 of segment s1)
template <bool RESTORED>
static __global__ __launch_bounds__(GR_T) void k_graph_write_nodes(
	GraphArgs A, GraphRestored R, SegFileBatch B, uint32_t const *__restrict__ lab, uint64_t const *__restrict__ loff, uint64_t const *__restrict__ seg_off, uint8_t *__restrict__ out)
{
	__shared__ uint8_t lut[256];
	uint32_t const s = B.s0 + blockIdx.x, tid = threadIdx.x, X = A.X, m = A.m, lane = lane_id();
	uint32_t const wv = (uint32_t) __builtin_amdgcn_readfirstlane((int) wave_id());
	lut[tid] = A.code_to_byte[tid];
	__syncthreads();
	uint32_t const nc = min(A.count[s], X);
	uint32_t const j_lo = s == B.s0 ? min(B.j_lo, nc) : 0u, j_hi = s == B.s1 ? min(B.j_hi, nc) : nc;
	uint64_t const lb = A.seg_lb[s], rb = A.seg_rb[s], W = rb > lb ? rb - lb : 0u;
	uint64_t const *lo = loff + (size_t) s * ((size_t) X + 1u);
	uint64_t const seg_at = seg_off[s] - B.begin;                    // (mod 2^64 where the segment begins in front of the batch: only its lines inside are addressed)
	uint64_t const plb = RESTORED ? R.src_lb[s] : lb, prb = RESTORED ? R.src_rb[s] : rb;      // what the lines print
	uint32_t const bits = 8u >> A.bsh, cmask = (1u << bits) - 1u, id0 = A.noff[s];
	uint32_t const dsg = sf_digits(s), dlb = gr_digits64(plb), drb = gr_digits64(prb);
	for (uint32_t j = j_lo + wv; j < j_hi; j += GR_NW)
	{
		uint64_t const at = seg_at + lo[j], end = seg_at + lo[j + 1u];
		if (end > B.bytes || at > end) continue;                     // (never: the batch was cut from these offsets)
		uint32_t const id1 = id0 + j + 1u, n = lab[(size_t) s * X + j], rows = A.size[(size_t) s * X + j], row = A.rep[(size_t) s * X + j];
		uint32_t const did = sf_digits(id1), dn = sf_digits(n), drw = sf_digits(rows);
		uint64_t const sub = at + 2u + did + 1u, tag = sub + max(n, 1u);
		if (tag + gr_node_tags_len(n, rows, s, plb, prb) != end) continue;      // (never: the lengths are k_graph_node_lines')
		if (lane == 0)
		{
			gr_put(out, at, B.bytes, (uint8_t) 'S'); gr_put(out, at + 1u, B.bytes, (uint8_t) '\t');
			sf_put_dec(out, at + 2u, B.bytes, id1, did);
			gr_put(out, at + 2u + did, B.bytes, (uint8_t) '\t');
			if (0 == n) gr_put(out, sub, B.bytes, (uint8_t) '*');
		}
		else if (lane == 1) gr_put_tag(out, tag, B.bytes, 'L', 'N', n, dn);
		else if (lane == 2) gr_put_tag(out, tag + 6u + dn, B.bytes, 'R', 'C', rows, drw);
		else if (lane == 3) gr_put_tag(out, tag + 12u + dn + drw, B.bytes, 's', 'g', s, dsg);
		else if (lane == 4) gr_put_tag(out, tag + 18u + dn + drw + dsg, B.bytes, 'l', 'b', plb, dlb);
		else if (lane == 5)
		{
			gr_put_tag(out, tag + 24u + dn + drw + dsg + dlb, B.bytes, 'r', 'b', prb, drb);
			gr_put(out, end - 1u, B.bytes, (uint8_t) '\n');
		}
		if (row >= m || 0 == n) continue;
		uint32_t const off = row >> A.bsh, sh = (row & ((1u << A.bsh) - 1u)) * bits;
		uint32_t run = 0;                                            // bytes of the label in front of this strip
		if constexpr (RESTORED)
		{
			uint64_t kc = lb;
			for (uint64_t base = plb; base < prb; base += WAVE)
			{
				uint8_t b;
				bool const have = gr_restored_byte(A, R, lut, base, prb, kc, rb, off, sh, cmask, lane, b);
				bool const keep = have && (A.gap < 0 || (int32_t) b != A.gap);
				uint64_t const mask = __ballot(keep);
				uint32_t const pos = run + __builtin_amdgcn_mbcnt_hi((uint32_t) (mask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t) mask, 0u));
				if (keep && pos < n) gr_put(out, sub + pos, B.bytes, b);
				run += (uint32_t) __popcll(mask);
			}
		}
		else
		for (uint64_t base = 0; base < W; base += WAVE)
		{
			uint64_t const k = base + lane;
			bool keep = false;
			uint8_t b = 0;
			if (k < W)
			{
				b = lut[(A.msa[(lb + k) * A.ld + off] >> sh) & cmask];
				keep = A.gap < 0 || (int32_t) b != A.gap;
			}
			uint64_t const mask = __ballot(keep);
			uint32_t const pos = run + __builtin_amdgcn_mbcnt_hi((uint32_t) (mask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t) mask, 0u));
			if (keep && pos < n) gr_put(out, sub + pos, B.bytes, b);       // (pos < n: the label never reaches the tags)
			run += (uint32_t) __popcll(mask);
		}
	}
}

// the junction of edge e: the last p with offset[p] <= e (offset[0] = 0; a junction without edges shares its offset with the next)
__device__ __forceinline__ uint32_t gr_junction(uint32_t const *__restrict__ offset, uint32_t pairs, uint32_t e)
{
	uint32_t lo = 0, hi = pairs;
	while (hi - lo > 1u)
	{
		uint32_t const mid = lo + (hi - lo) / 2u;
		if (offset[mid] <= e) lo = mid;
		else hi = mid;
	}
	return lo;
}

// edge e as the file prints it: the two node ids + 1 and the rows
__device__ __forceinline__ uint3 gr_link(GraphArgs const &A, uint64_t e)
{
	uint32_t const p = gr_junction(A.offset, A.pairs, (uint32_t) e);
	uint2 const w = A.edges[e];
	uint32_t const l = min(w.x >> 16, gr_count(A, p) - 1u), r = min(w.x & 0xFFFFu, gr_count(A, p + 1u) - 1u);
	return make_uint3(A.noff[p] + l + 1u, A.noff[p + 1u] + r + 1u, w.y);
}

__device__ __forceinline__ uint32_t gr_link_len(uint3 k) { return 17u + sf_digits(k.x) + sf_digits(k.y) + sf_digits(k.z); }

// workgroup b0 + blockIdx.x takes the edges [b GR_T, (b + 1) GR_T): btot[b] their lines' bytes (or nullptr);
// lens[blockIdx.x GR_T + tid] every line's (or nullptr)
static __global__ __launch_bounds__(GR_T) void k_graph_link_lines(GraphArgs A, uint32_t b0, uint64_t *__restrict__ btot, uint32_t *__restrict__ lens)
{
	__shared__ uint64_t scratch[GR_NW];
	uint32_t const b = b0 + blockIdx.x, tid = threadIdx.x;
	uint64_t const e = (uint64_t) b * GR_T + tid;
	uint32_t const len = (A.pairs && e < A.n_edges) ? gr_link_len(gr_link(A, e)) : 0u;
	uint64_t total;
	(void) sf_block_excl_add64(len, scratch, &total);
	if (btot && tid == 0) btot[b] = total;
	if (lens) lens[(size_t) blockIdx.x * GR_T + tid] = len;
}

// the L lines [B.first, B.last): boff[b] the bytes of the links' section in front of workgroup b's lines
static __global__ __launch_bounds__(GR_T) void k_graph_write_links(GraphArgs A, GraphBatch B, uint64_t const *__restrict__ boff, uint8_t *__restrict__ out)
{
	__shared__ uint64_t scratch[GR_NW];
	uint32_t const b = (uint32_t) (B.first / GR_T) + blockIdx.x, tid = threadIdx.x;
	uint64_t const e = (uint64_t) b * GR_T + tid;
	bool const have = A.pairs && e < A.n_edges;
	uint3 const k = have ? gr_link(A, e) : make_uint3(0u, 0u, 0u);
	uint32_t const len = have ? gr_link_len(k) : 0u;
	uint64_t total;
	uint64_t const before = sf_block_excl_add64(len, scratch, &total);
	if (!have || e < B.first || e >= B.last) return;
	uint64_t at = boff[b] + before - B.begin;
	if (at > B.bytes || at + len > B.bytes) return;                  // (never: the batch was cut from these offsets)
	uint32_t const d1 = sf_digits(k.x), d2 = sf_digits(k.y), d3 = sf_digits(k.z);
	gr_put(out, at, B.bytes, (uint8_t) 'L'); gr_put(out, at + 1u, B.bytes, (uint8_t) '\t');
	sf_put_dec(out, at + 2u, B.bytes, k.x, d1);
	at += 2u + d1;
	gr_put(out, at, B.bytes, (uint8_t) '\t'); gr_put(out, at + 1u, B.bytes, (uint8_t) '+'); gr_put(out, at + 2u, B.bytes, (uint8_t) '\t');
	sf_put_dec(out, at + 3u, B.bytes, k.y, d2);
	at += 3u + d2;
	gr_put(out, at, B.bytes, (uint8_t) '\t'); gr_put(out, at + 1u, B.bytes, (uint8_t) '+'); gr_put(out, at + 2u, B.bytes, (uint8_t) '\t');
	gr_put(out, at + 3u, B.bytes, (uint8_t) '0'); gr_put(out, at + 4u, B.bytes, (uint8_t) 'M');
	gr_put_tag(out, at + 5u, B.bytes, 'R', 'C', k.z, d3);
	gr_put(out, at + 11u + d3, B.bytes, (uint8_t) '\n');
}

// the node id + 1 of `row` in segment s
__device__ __forceinline__ uint32_t gr_step(GraphArgs const &A, uint32_t s, uint32_t row)
{
	return A.noff[s] + min((uint32_t) A.of_row[(size_t) s * A.m + row], gr_count(A, s) - 1u) + 1u;
}

// plen[row]: the bytes of row's P line -- "P\t", the row, "\t", S steps of digits + 2 with the last step's comma left out, "\t*\n"
static __global__ __launch_bounds__(GR_T) void k_graph_path_lines(GraphArgs A, uint64_t *__restrict__ plen)
{
	uint32_t const row = blockIdx.x * GR_T + threadIdx.x;
	if (row >= A.m) return;
	uint64_t steps = 0;
	for (uint32_t s = 0; s < A.S; ++s) steps += sf_digits(gr_step(A, s, row)) + 2u;
	plen[row] = 2u + sf_digits(row) + 1u + steps - 1u + 3u;
}

// the P lines [B.first, B.last): workgroup x takes the rows B.first + x GR_TILE ...; poff[row] the bytes of the paths' section in front of row's line
static __global__ __launch_bounds__(GR_T) void k_graph_write_paths(GraphArgs A, GraphBatch B, uint64_t const *__restrict__ poff, uint8_t *__restrict__ out)
{
	__shared__ uint32_t tile[GR_TILE][GR_TILE + 1];                  // [segment of the pass][row of the workgroup], padded: the reads go down a column
	constexpr uint32_t PER = GR_TILE / GR_NW;                        // segments a wave loads and rows a wave writes
	uint32_t const lane = lane_id();
	uint32_t const wv = (uint32_t) __builtin_amdgcn_readfirstlane((int) wave_id());
	uint64_t const r0 = B.first + (uint64_t) blockIdx.x * GR_TILE;
	uint64_t const r_end = min(B.last, (uint64_t) A.m);
	// lane i < PER of a wave holds where the next step of row r0 + wv PER + i goes; it writes the line's two ends
	uint64_t cursor = ~0ull;
	{
		uint64_t const row = r0 + (uint64_t) wv * PER + lane;
		if (lane < PER && row < r_end)
		{
			uint64_t const at = poff[row] - B.begin, end = poff[row + 1u] - B.begin;
			uint32_t const dr = sf_digits((uint32_t) row);
			if (at <= end && end <= B.bytes && at + 2u + dr + 1u + 3u <= end)      // (else never: the batch was cut from these offsets; the line is left out)
			{
				gr_put(out, at, B.bytes, (uint8_t) 'P'); gr_put(out, at + 1u, B.bytes, (uint8_t) '\t');
				sf_put_dec(out, at + 2u, B.bytes, (uint32_t) row, dr);
				gr_put(out, at + 2u + dr, B.bytes, (uint8_t) '\t');
				gr_put(out, end - 3u, B.bytes, (uint8_t) '\t'); gr_put(out, end - 2u, B.bytes, (uint8_t) '*'); gr_put(out, end - 1u, B.bytes, (uint8_t) '\n');
				cursor = at + 2u + dr + 1u;
			}
		}
	}
	for (uint32_t s0 = 0; s0 < A.S; s0 += GR_TILE)
	{
		// lanes along the rows: the classes of 64 rows in one segment are 128 contiguous bytes
		for (uint32_t i = 0; i < PER; ++i)
		{
			uint32_t const sg = s0 + wv * PER + i;
			uint64_t const row = r0 + lane;
			tile[wv * PER + i][lane] = (sg < A.S && row < r_end) ? gr_step(A, sg, (uint32_t) row) : 0u;
		}
		__syncthreads();
		// lanes along the segments: the 64 steps of a row are one contiguous stretch of its line
		for (uint32_t i = 0; i < PER; ++i)
		{
			uint64_t const at0 = (uint64_t) __shfl((unsigned long long) cursor, (int) i, WAVE);
			bool const in = s0 + lane < A.S;
			uint32_t const id1 = tile[lane][wv * PER + i];
			uint32_t const nd = sf_digits(id1), len = in ? nd + 2u : 0u;
			uint32_t inc = len;
#pragma unroll
			for (int off = 1; off < (int) WAVE; off <<= 1)
			{
				uint32_t const o = __shfl_up(inc, off, WAVE);
				if ((int) lane >= off) inc += o;
			}
			uint32_t const total = __shfl(inc, (int) WAVE - 1, WAVE);
			if (at0 != ~0ull && in)
			{
				uint64_t const at = at0 + (inc - len);
				sf_put_dec(out, at, B.bytes, id1, nd);
				gr_put(out, at + nd, B.bytes, (uint8_t) '+');
				if (s0 + lane + 1u < A.S) gr_put(out, at + nd + 1u, B.bytes, (uint8_t) ',');      // (the last step's comma is the tail's tab)
			}
			if (lane == i && cursor != ~0ull) cursor += total;
		}
		__syncthreads();                   // (the tile is read to here)
	}
}

// rown[s][row] = the node of row in segment s (fseq_block_graph's row_nodes)
static __global__ __launch_bounds__(GR_T) void k_graph_row_nodes(GraphArgs A, uint32_t *__restrict__ rown)
{
	uint32_t const s = blockIdx.x;
	for (uint64_t row = (uint64_t) blockIdx.y * GR_T + threadIdx.x; row < A.m; row += (uint64_t) gridDim.y * GR_T)
		rown[(size_t) s * A.m + row] = gr_step(A, s, (uint32_t) row) - 1u;
}

} // namespace fseq
