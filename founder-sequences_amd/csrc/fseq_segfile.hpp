// fseq_segfile.hpp -- the --output-segments file from what the device holds (fseq_write_segments_device, csrc/fseq_api_join.hip).
//
// The host writer (write_segments_impl) copies every boundary state to the host (S x m x 8 bytes) and reads the substrings
// from raw rows the caller must hold.  Everything the file needs is on the device already: the packed alignment, the
// boundary states, the class tables of k_join_classes_wide (fseq_joinprep.hpp) and, for bipartite-matching joining, the
// texts of k_bip_minrow_wide / k_bip_texts_wide (fseq_joinbipw.hpp).  What is added here is the file itself, in the
// project's count / scan / write pattern (k_match_walk, k_join_edges_wide):
//   k_segfile_lines<BIP>    one workgroup per merged segment: the length of every line of the segment -- prefix, substring,
//                           the index field (bipartite: the decimal digits and commas of the text's rows, summed per text
//                           in LDS by integer atomics, whose result does not depend on their order), the tail -- and their
//                           exclusive scan inside the segment, 64-bit: loff[s][j], loff[s][X] = the segment's bytes
//   k_segfile_scan          one workgroup: the segments' bytes scanned into seg_off[s] (64-bit), seg_off[S] = the file's lines
//   k_segfile_members       (bipartite) one workgroup per segment a batch touches: the rows 0 .. m - 1 partitioned stably by
//                           their text, tpos[of_row[row]] < X <= 4,096: text 0's rows ascending, then text 1's, ...  The
//                           rows are taken 256 at a time in ascending order; inside a wave the rows of one text are found
//                           with one ballot per key bit (cs_match of fseq_chainsort.hpp, here for 12-bit keys) and ranked by
//                           a popcount below the lane; the waves of a tile take their turns one after the other at the LDS
//                           cursors of the texts.  No atomic hands out a position: the order is exactly ascending whatever
//                           the order in which waves or workgroups run.
//   k_segfile_write<BIP>    one workgroup per segment a batch touches: a wave per line writes prefix, substring (lanes along
//                           the columns, as k_founders) and tail; then (bipartite) the members in order, 256 at a time: a
//                           scan of digits + 1 gives every member's offset in the segment's index bytes, the offset of a
//                           text's first member is the smallest of its members' (an LDS minimum, order-independent), and a
//                           member's digits go to the line's index field at the difference.
// The RESTORED forms (fseq_write_segments_restored, on a context made by fseq_create_without_identity_columns) print a line in the
// SOURCE's co-ordinates: its substring is src_rb - src_lb bytes (restored_segment_bounds, fseq_restored_bounds.hpp), filled in
// two passes over disjoint bytes -- the reference row's byte at every identity column of the range, lanes along the source
// positions, and the row's byte of every kept column c of [lb, rb) at kept[c] - src_lb, lanes along the kept columns.  The class
// tables, the texts and the members stay in reduced co-ordinates, where the boundary states are.
// No kernel waits on another workgroup.  Class counts are clipped to X, texts to X, rows to m, and every store is checked
// against the batch buffer's size: a table value never indexes unchecked.
// The index field is written with byte stores, one member (2 to 11 bytes) a lane: the lanes of a wave cover one contiguous
// stretch of a few hundred bytes, which L2 merges; staging a line's field through LDS for 16-byte stores was not tried.
#pragma once

#include "fseq_core.hpp"

namespace fseq {

constexpr uint32_t SF_T = 256;                           // threads of every kernel here
constexpr uint32_t SF_NW = SF_T / WAVE;
constexpr uint32_t SF_KEY_BITS = 12;                     // texts of a segment: below JBW_MAX_TEXTS = 4,096

__host__ __device__ inline uint32_t sf_digits(uint32_t v)
{
	return 1u + (v >= 10u) + (v >= 100u) + (v >= 1000u) + (v >= 10000u) + (v >= 100000u) + (v >= 1000000u) + (v >= 10000000u) +
	       (v >= 100000000u) + (v >= 1000000000u);
}

// the nd decimal digits of v at p[0 .. nd), each store checked against the buffer's end
__device__ __forceinline__ void sf_put_dec(uint8_t *out, uint64_t at, uint64_t cap, uint32_t v, uint32_t nd)
{
	for (uint32_t k = nd; k-- > 0;)
	{
		if (at + k < cap) out[at + k] = (uint8_t) ('0' + v % 10u);
		v /= 10u;
	}
}

// block-wide exclusive add-scan of one 64-bit value per thread (block_excl_add's shape); scratch: SF_NW words of LDS
__device__ __forceinline__ uint64_t sf_block_excl_add64(uint64_t v, uint64_t *scratch, uint64_t *total)
{
	uint64_t inc = v;
#pragma unroll
	for (int off = 1; off < WAVE; off <<= 1)
	{
		uint64_t const o = (uint64_t) __shfl_up((unsigned long long) inc, off, WAVE);
		if ((int) lane_id() >= off) inc += o;
	}
	__syncthreads();                       // protect scratch against the previous use
	if (lane_id() == 63) scratch[wave_id()] = inc;
	__syncthreads();
	uint64_t pre = 0, tot = 0;
#pragma unroll
	for (uint32_t w = 0; w < SF_NW; ++w)
	{
		uint64_t const x = scratch[w];
		if (w < wave_id()) pre += x;
		tot += x;
	}
	*total = tot;
	return pre + inc - v;
}

// lanes of the wave whose key equals mine (in = this lane holds a row): cs_match for keys of SF_KEY_BITS bits
__device__ __forceinline__ uint64_t sf_match(uint32_t key, bool in)
{
	uint64_t mask = __ballot(in);
#pragma unroll
	for (uint32_t b = 0; b < SF_KEY_BITS; ++b)
	{
		uint64_t const bal = __ballot(in && ((key >> b) & 1u));
		mask &= ((key >> b) & 1u) ? bal : ~bal;
	}
	return mask;
}

// what the kernels share of a call: the segments, their prefixes ("s\tlb\trb\tsize\t", formatted on the host), the tables
struct SegFileArgs {
	uint64_t const *seg_lb, *seg_rb;         // [S]
	uint8_t const *pool;                     // the prefixes one after the other
	uint64_t const *ppos;                    // [S + 1] where each begins
	uint32_t const *count;                   // [S] classes
	uint32_t m, X, S;
	// bipartite: the class of every row, the text of every class, the text a placeholder copies, the texts' first rows
	uint16_t const *of_row, *tpos, *src;
	uint32_t const *reprow;
	// random: {substring_idx, copies} of line j of segment s at [s * X + j], j < count[s], in the file's order
	uint2 const *rline;
	// restored: the segments in the source's co-ordinates, [S] each; the source column of every kept column, [seg_rb[S - 1]];
	// which source columns are identity columns and row 0 of the source as raw bytes, [n_src] each (nullptr / 0 otherwise)
	uint64_t const *src_lb, *src_rb;
	uint32_t const *kept;
	uint8_t const *mask, *ref;
	uint64_t n_src;
};

// bytes of a line's substring: the segment's columns, in the restored form its source positions
template <bool RESTORED>
__device__ __forceinline__ uint64_t sf_width(SegFileArgs const &A, uint32_t s)
{
	if (RESTORED)
	{
		uint64_t const a = A.src_lb[s], b = A.src_rb[s];
		return b > a ? b - a : 0u;
	}
	return A.seg_rb[s] - A.seg_lb[s];
}

__host__ __device__ inline size_t segfile_lines_lds_bytes(uint32_t X, bool bip) { return bip ? (size_t) X * 8u : 0u; }

// loff[s][j], j <= X (stride X + 1): bytes of the segment's lines in front of line j; a segment has X lines (bipartite) or
// count[s] (random: the lines behind them have no bytes)
template <bool BIP, bool RESTORED = false>
static __global__ __launch_bounds__(SF_T) void k_segfile_lines(SegFileArgs A, uint64_t *__restrict__ loff)
{
	extern __shared__ __attribute__((aligned(16))) unsigned long long sf_dig[];      // [X] bipartite: digits + 1 over a text's rows
	__shared__ uint64_t scratch[SF_NW];
	uint32_t const s = blockIdx.x, tid = threadIdx.x, X = A.X, m = A.m;
	uint32_t const nc = min(A.count[s], X);
	uint64_t const fixed = (A.ppos[s + 1] - A.ppos[s]) + sf_width<RESTORED>(A, s) + 1u;      // prefix, substring, one tab or the newline
	if (BIP)
	{
		for (uint32_t t = tid; t < X; t += SF_T) sf_dig[t] = 0;
		__syncthreads();
		uint16_t const *of = A.of_row + (size_t) s * m, *tp = A.tpos + (size_t) s * X;
		for (uint32_t row = tid; row < m; row += SF_T)
		{
			uint32_t const c = of[row];
			if (c < nc)
			{
				uint32_t const t = tp[c];
				if (t < X) atomicAdd(&sf_dig[t], (unsigned long long) (sf_digits(row) + 1u));
			}
		}
		__syncthreads();
	}
	uint64_t *lo = loff + (size_t) s * ((size_t) X + 1u);
	uint64_t running = 0;
	for (uint32_t base = 0; base < X; base += SF_T)
	{
		uint32_t const j = base + tid;
		uint64_t len = 0;
		if (BIP)
		{
			if (j < nc) len = fixed + (sf_dig[j] ? sf_dig[j] - 1u : 0u) + 3u;                  // rows and commas, "\t-\n"
			else if (j < X) len = fixed + 2u + sf_digits(A.src[(size_t) s * X + j]);            // "\t", the text copied, "\n"
		}
		else if (j < nc)
		{
			uint2 const r = A.rline[(size_t) s * X + j];
			len = fixed + sf_digits(r.x) + 1u + sf_digits(r.y) + 1u;
		}
		uint64_t total;
		uint64_t const before = sf_block_excl_add64(len, scratch, &total);
		if (j < X) lo[j] = running + before;
		running += total;
	}
	if (tid == 0) lo[X] = running;
}

// seg_off[s] = bytes of the segments before s, seg_off[S] = all of them
static __global__ __launch_bounds__(SF_T) void k_segfile_scan(uint64_t const *__restrict__ loff, uint32_t S, uint32_t X, uint64_t *__restrict__ seg_off)
{
	__shared__ uint64_t scratch[SF_NW];
	uint64_t running = 0;
	for (uint32_t base = 0; base < S; base += SF_T)
	{
		uint32_t const s = base + threadIdx.x;
		uint64_t const v = s < S ? loff[(size_t) s * ((size_t) X + 1u) + X] : 0u;
		uint64_t total;
		uint64_t const before = sf_block_excl_add64(v, scratch, &total);
		if (s < S) seg_off[s] = running + before;
		running += total;
	}
	if (threadIdx.x == 0) seg_off[S] = running;
}

__host__ __device__ inline size_t segfile_members_lds_bytes(uint32_t X) { return (size_t) X * 4u; }

// members[(s - s0) * m + k]: the rows of segment s by (text, row), for the segments s0 + blockIdx.x
static __global__ __launch_bounds__(SF_T) void k_segfile_members(SegFileArgs A, uint32_t const *__restrict__ size, uint32_t s0, uint32_t *__restrict__ members)
{
	extern __shared__ __attribute__((aligned(16))) uint32_t sf_cur[];      // [X] where the next row of every text goes
	__shared__ uint32_t scratch[SF_NW + 1];
	uint32_t const s = s0 + blockIdx.x, tid = threadIdx.x, X = A.X, m = A.m, lane = lane_id();
	uint32_t const wv = (uint32_t) __builtin_amdgcn_readfirstlane((int) wave_id());
	uint32_t const nc = min(A.count[s], X);
	uint16_t const *of = A.of_row + (size_t) s * m, *tp = A.tpos + (size_t) s * X;
	uint32_t *mem = members + (size_t) blockIdx.x * m;
	for (uint32_t t = tid; t < X; t += SF_T) sf_cur[t] = 0;
	__syncthreads();
	for (uint32_t c = tid; c < nc; c += SF_T)
	{
		uint32_t const t = tp[c];
		if (t < X) sf_cur[t] = size[(size_t) s * X + c];             // (the texts of the classes are distinct)
	}
	__syncthreads();
	uint32_t running = 0;
	for (uint32_t base = 0; base < X; base += SF_T)
	{
		uint32_t const t = base + tid;
		uint32_t const v = t < X ? sf_cur[t] : 0u;
		uint32_t total;
		uint32_t const before = block_excl_add<SF_T>(v, scratch, &total);
		if (t < X) sf_cur[t] = running + before;
		running += total;
	}
	__syncthreads();
	for (uint32_t base = 0; base < m; base += SF_T)
	{
		uint32_t const row = base + tid;
		uint32_t key = X;
		if (row < m)
		{
			uint32_t const c = of[row];
			if (c < nc) key = tp[c];
		}
		bool const in = key < X;
		uint64_t const same = sf_match(key, in);
		uint32_t const below = (uint32_t) __builtin_amdgcn_mbcnt_hi((uint32_t) (same >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t) same, 0u));
		uint32_t at = 0;
		// the waves of the tile one after the other, lower rows first: a text's cursor is read by its rows of this wave and
		// moved on by the lowest of them
		for (uint32_t w = 0; w < SF_NW; ++w)
		{
			if (w == wv)
			{
				if (in) at = sf_cur[key];
				__builtin_amdgcn_wave_barrier();
				if (in && 0 == below) sf_cur[key] = at + (uint32_t) __popcll(same);
			}
			__syncthreads();
		}
		if (in && at + below < m) mem[at + below] = row;
	}
}

__host__ __device__ inline size_t segfile_write_lds_bytes(uint32_t X, bool bip) { return bip ? (size_t) X * 8u : 0u; }

// what a batch is: whole lines in file order, from line j_lo of segment s0 to line j_hi - 1 of segment s1, which begin
// `begin` bytes into the file's lines; out holds `bytes` of them
struct SegFileBatch {
	uint32_t s0, s1, j_lo, j_hi;
	uint64_t begin, bytes;
};

template <bool BIP, bool RESTORED = false>
static __global__ __launch_bounds__(SF_T) void k_segfile_write(
	SegFileArgs A, SegFileBatch B, uint8_t const *__restrict__ msa, size_t ld, uint32_t bsh, uint8_t const *__restrict__ code_to_byte,
	uint64_t const *__restrict__ loff, uint64_t const *__restrict__ seg_off, uint32_t const *__restrict__ members, uint8_t *__restrict__ out)
{
	extern __shared__ __attribute__((aligned(16))) unsigned long long sf_first[];      // [X] bipartite: index bytes in front of a text's first row
	__shared__ uint8_t lut[256];
	__shared__ uint32_t scratch[SF_NW + 1];
	uint32_t const s = B.s0 + blockIdx.x, tid = threadIdx.x, X = A.X, m = A.m, lane = lane_id();
	uint32_t const wv = (uint32_t) __builtin_amdgcn_readfirstlane((int) wave_id());
	lut[tid] = code_to_byte[tid];
	uint32_t const nc = min(A.count[s], X), nl = BIP ? X : nc;
	uint32_t const j_lo = s == B.s0 ? min(B.j_lo, nl) : 0u, j_hi = s == B.s1 ? min(B.j_hi, nl) : nl;
	uint64_t const lb = A.seg_lb[s], rb = A.seg_rb[s], W = sf_width<RESTORED>(A, s);
	uint64_t const slb = RESTORED ? A.src_lb[s] : 0u;
	uint64_t const p0 = A.ppos[s], plen = A.ppos[s + 1] - p0;
	uint64_t const *lo = loff + (size_t) s * ((size_t) X + 1u);
	uint64_t const seg_at = seg_off[s] - B.begin;                    // (mod 2^64 where the segment begins in front of the batch: only its lines inside are addressed)
	uint32_t const bits = 8u >> bsh, cmask = (1u << bits) - 1u;
	if (BIP)
		for (uint32_t t = tid; t < X; t += SF_T) sf_first[t] = ~0ull;
	__syncthreads();
	for (uint32_t j = j_lo + wv; j < j_hi; j += SF_NW)
	{
		uint64_t const at = seg_at + lo[j], end = seg_at + lo[j + 1u];
		if (end > B.bytes || at > end) continue;                     // (never: the batch was cut from these offsets)
		for (uint64_t k = lane; k < plen; k += 64u) out[at + k] = A.pool[p0 + k];
		uint64_t sub = at + plen;
		uint32_t row;
		if (BIP)
		{
			row = A.reprow[(size_t) s * X + j];
			if (lane == 0)
			{
				out[sub + W] = (uint8_t) '\t';
				if (j < nc) { out[end - 3u] = (uint8_t) '\t'; out[end - 2u] = (uint8_t) '-'; }
				else
				{
					uint32_t const from = A.src[(size_t) s * X + j], nd = sf_digits(from);
					out[end - 2u - nd] = (uint8_t) '\t';
					sf_put_dec(out, end - 1u - nd, B.bytes, from, nd);
				}
				out[end - 1u] = (uint8_t) '\n';
			}
		}
		else
		{
			uint2 const r = A.rline[(size_t) s * X + j];
			uint32_t const d1 = sf_digits(r.x), d2 = sf_digits(r.y);
			row = r.x;
			if (lane == 0)
			{
				sf_put_dec(out, sub, B.bytes, r.x, d1);
				out[sub + d1] = (uint8_t) '\t';
				sf_put_dec(out, sub + d1 + 1u, B.bytes, r.y, d2);
				out[sub + d1 + 1u + d2] = (uint8_t) '\t';
				out[end - 1u] = (uint8_t) '\n';
			}
			sub += d1 + d2 + 2u;
		}
		if (sub + W > end) continue;                                 // (never)
		uint32_t const off = row >> bsh, sh = (row & ((1u << bsh) - 1u)) * bits;
		if (RESTORED)
		{
			// the identity columns of [src_lb, src_rb): row 0's byte, lanes along the source positions
			for (uint64_t k = lane; k < W; k += 64u)
			{
				uint64_t const p = slb + k;
				if (p < A.n_src && A.mask[p]) out[sub + k] = A.ref[p];
			}
			// the kept columns of [lb, rb) at their source positions, which the pass above left alone (mask is 0 at a kept
			// column: k_identity_scatter made kept from it); one outside the range stores nothing
			for (uint64_t c = lb + lane; c < rb; c += 64u)
			{
				uint64_t const p = A.kept[c];
				if (p >= slb && p - slb < W)
					out[sub + (p - slb)] = row < m ? lut[(msa[c * ld + off] >> sh) & cmask] : (uint8_t) '-';
			}
		}
		else
			for (uint64_t k = lane; k < W; k += 64u)
				out[sub + k] = row < m ? lut[(msa[(lb + k) * ld + off] >> sh) & cmask] : (uint8_t) '-';
	}
	if (!BIP) return;
	// the index fields: the segment's members in order, digits + 1 each
	uint16_t const *of = A.of_row + (size_t) s * m, *tp = A.tpos + (size_t) s * X;
	uint32_t const *mem = members + (size_t) blockIdx.x * m;
	uint64_t running = 0;
	for (uint32_t base = 0; base < m; base += SF_T)
	{
		uint32_t const k = base + tid;
		uint32_t const row = k < m ? mem[k] : 0xFFFFFFFFu;
		uint32_t t = X;
		if (row < m)
		{
			uint32_t const c = of[row];
			if (c < nc) t = tp[c];
		}
		bool const in = t < nc;                                      // (the texts of the classes are the first count[s])
		uint32_t const nd = in ? sf_digits(row) : 0u;
		uint32_t total;
		uint32_t const before = block_excl_add<SF_T>(in ? nd + 1u : 0u, scratch, &total);
		uint64_t const mine = running + before;
		if (in) atomicMin(&sf_first[t], (unsigned long long) mine);
		__syncthreads();
		if (in && t >= j_lo && t < j_hi)
		{
			uint64_t const end = seg_at + lo[t + 1u];
			uint64_t const at = seg_at + lo[t] + plen + W + 1u + (mine - sf_first[t]);
			if (end <= B.bytes && at + nd + 3u <= end)
			{
				sf_put_dec(out, at, B.bytes, row, nd);
				if (at + nd + 3u < end) out[at + nd] = (uint8_t) ',';   // (the last row of a text stands in front of the tail, "\t-\n")
			}
		}
		running += total;
	}
}

} // namespace fseq
