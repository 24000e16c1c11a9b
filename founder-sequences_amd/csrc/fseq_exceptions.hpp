// fseq_exceptions.hpp -- the exception cells of query rows: where a row that took no part in a reconstruction differs from
// row 0 in an identity column of it (fseq_create_without_identity_columns_held, fseq_match_rows_restored; include/fseq.h).
//
// replaces: nothing of the reference by itself; it is what lets match-sequences-to-founders' loop (match_founder_sequences.cc:
// 166-208) over the full-length queries and the full-length restored founders be walked over the kept columns only.  In an
// identity column every restored founder carries row 0's byte, so the founders that agree with a query there are all of them or
// -- an exception cell -- none.  k_match_walk<.., true, true> (csrc/fseq_match.hpp) reads, per query row, the source positions of
// its exception cells in ascending order:
//     off[rows + 1]   64-bit: row r's cells are cols[off[r] .. off[r + 1])
//     cols[off[rows]] 32-bit source columns, exactly as many entries as there are cells
// No atomic decides an order: the cells are first marked in a transient bit matrix [row][ceil(n_src / 32)] (bit k % 32 of word
// k / 32 = column k), an eighth of the raw query bytes, then
//   k_exc_count   popcount of every row                         \  one workgroup a row
//   k_exc_scan    exclusive scan of the rows' counts             >
//   k_exc_write   the bits of every row extracted in order      /
// and the matrix is released before the walk.  The marks come from
//   k_exc_bits_held   held-out rows, on the device already and packed like the alignment: one lane per identity column and
//                     16-byte chunk of it; a chunk equal to row 0's code broadcast is done after one compare, any other sets
//                     the bits of its rows that differ (atomicOr into a zeroed matrix: the OR of the bits, whatever the order)
//   k_exc_bits_rows   host rows, a staged chunk of raw bytes: one lane per row and word of the matrix, 32 raw bytes against
//                     the 32 reference bytes under the mask; every word of the matrix is written by exactly one lane
//   k_match_pack_rows_kept   k_match_pack_rows (csrc/fseq_match.hpp) for the kept columns of such a chunk, gathered into their
//                     reduced positions
#pragma once

#include "fseq_ctx.hpp"
#include "fseq_identity.hpp"
#include "fseq_match.hpp"

namespace fseq {

constexpr uint32_t EX_T = 256;

// held: column k of the held-out rows at held + k * h_ld (chunks = h_ld / 16, the padding zeroed); msa / ld: the alignment the
// identity columns were found in (its row 0 gives the code every founder carries); bitsm zeroed, nw words a row
static __global__ __launch_bounds__(EX_T) void k_exc_bits_held(
	uint8_t const *__restrict__ held, size_t h_ld, uint32_t n_held, uint32_t chunks, uint8_t const *__restrict__ msa, size_t ld,
	uint8_t const *__restrict__ mask, uint64_t n_src, uint32_t bsh, uint32_t *__restrict__ bitsm, size_t nw)
{
	uint32_t const bits = 8u >> bsh, cmask = (1u << bits) - 1u, per_word = 32u / bits;
	uint32_t const ones = bsh == 2 ? 0x55555555u : bsh == 1 ? 0x11111111u : 0x01010101u;
	uint64_t const work = n_src * chunks;
	for (uint64_t q = (uint64_t) blockIdx.x * EX_T + threadIdx.x; q < work; q += (uint64_t) gridDim.x * EX_T)
	{
		uint64_t const k = q / chunks;
		uint32_t const ch = (uint32_t) (q - k * chunks);
		if (!mask[k]) continue;
		uint32_t const ref = (uint32_t) msa[k * ld] & cmask, pattern = ref * ones;
		uint4 const v = *reinterpret_cast<uint4 const *>(held + k * h_ld + (size_t) ch * 16u);
		if (((v.x ^ pattern) | (v.y ^ pattern) | (v.z ^ pattern) | (v.w ^ pattern)) == 0u) continue;
		uint32_t const w[4] = {v.x, v.y, v.z, v.w};
		uint32_t const row0 = ch * 4u * per_word;                            // (the fields behind row n_held - 1 are padding)
		for (uint32_t f = 0; f < 4u * per_word && row0 + f < n_held; ++f)
			if (((w[f / per_word] >> ((f % per_word) * bits)) & cmask) != ref)
				atomicOr(bitsm + (size_t) (row0 + f) * nw + (size_t) (k >> 5), 1u << (uint32_t) (k & 31u));
	}
}

// raw: a staged chunk, row q's bytes of the source columns [c0, c0 + cw) at raw[q * stride ..] (c0 and stride multiples of 64,
// the base 16-byte aligned); ref / mask: [n_src].  One lane per (row, word): the word of columns [c0 + 32 w, c0 + 32 w + 32)
static __global__ __launch_bounds__(EX_T) void k_exc_bits_rows(
	uint8_t const *__restrict__ raw, size_t stride, uint32_t n_rows, uint64_t c0, uint32_t cw, uint8_t const *__restrict__ ref,
	uint8_t const *__restrict__ mask, uint64_t n_src, uint32_t *__restrict__ bitsm, size_t nw)
{
	uint32_t const words = (cw + 31u) / 32u;
	uint64_t const idx = (uint64_t) blockIdx.x * EX_T + threadIdx.x;
	if (idx >= (uint64_t) n_rows * words) return;
	uint32_t const r = (uint32_t) (idx / words), w = (uint32_t) (idx - (uint64_t) r * words);
	uint64_t const cb = c0 + 32u * (uint64_t) w;
	uint8_t const *const src = raw + (size_t) r * stride + 32u * (size_t) w;
	uint32_t out = 0;
	if (cb + 32u <= n_src)
	{
		uint4 const a0 = *reinterpret_cast<uint4 const *>(src), a1 = *reinterpret_cast<uint4 const *>(src + 16);
		uint4 const b0 = *reinterpret_cast<uint4 const *>(ref + cb), b1 = *reinterpret_cast<uint4 const *>(ref + cb + 16);
		uint32_t const x[8] = {a0.x ^ b0.x, a0.y ^ b0.y, a0.z ^ b0.z, a0.w ^ b0.w, a1.x ^ b1.x, a1.y ^ b1.y, a1.z ^ b1.z, a1.w ^ b1.w};
		if (x[0] | x[1] | x[2] | x[3] | x[4] | x[5] | x[6] | x[7])          // (32 bytes equal to the reference: done)
		{
			uint4 const m0 = *reinterpret_cast<uint4 const *>(mask + cb), m1 = *reinterpret_cast<uint4 const *>(mask + cb + 16);
			uint32_t const mk[8] = {m0.x, m0.y, m0.z, m0.w, m1.x, m1.y, m1.z, m1.w};
#pragma unroll
			for (uint32_t i = 0; i < 32u; ++i)
				if (((x[i >> 2] >> (8u * (i & 3u))) & 0xFFu) && ((mk[i >> 2] >> (8u * (i & 3u))) & 0xFFu)) out |= 1u << i;
		}
	}
	else
		for (uint32_t i = 0; i < 32u && cb + i < n_src; ++i)
			if (mask[cb + i] && src[i] != ref[cb + i]) out |= 1u << i;
	bitsm[(size_t) r * nw + (size_t) (cb >> 5)] = out;
}

// the kept columns [j_lo, j_hi) of the context, whose source positions kept[j] lie in the staged chunk [c0, c0 + cw): as
// k_match_pack_rows, the tile's 64 columns gathered from the rows' bytes at kept[j] - c0
static __global__ __launch_bounds__(MT_T) void k_match_pack_rows_kept(
	uint8_t const *__restrict__ raw, size_t stride, uint32_t n_rows, uint64_t c0, uint64_t j_lo, uint64_t j_hi, uint32_t const *__restrict__ kept,
	uint8_t const *__restrict__ code_of, uint32_t bsh, uint8_t *__restrict__ out, size_t ld)
{
	__shared__ uint8_t lut[256];
	__shared__ uint32_t at_of[MT_PACK_COLS];
	__shared__ __attribute__((aligned(16))) uint8_t tile[MT_PACK_COLS][MT_PACK_LD];
	uint32_t const tid = threadIdx.x;
	uint64_t const j0 = j_lo + (uint64_t) blockIdx.x * MT_PACK_COLS;
	uint32_t const r0 = blockIdx.y * MT_T;
	uint32_t const nc = (uint32_t) mt_min(MT_PACK_COLS, j_hi - j0);
	lut[tid] = code_of[tid];
	if (tid < nc) at_of[tid] = (uint32_t) (kept[j0 + tid] - c0);
	__syncthreads();
	// (a wave: 64 columns of one row, whose bytes lie close together)
	for (uint32_t i = tid; i < MT_T * MT_PACK_COLS; i += MT_T)
	{
		uint32_t const col = i % MT_PACK_COLS, r = i / MT_PACK_COLS;
		tile[col][r] = (col < nc && r0 + r < n_rows) ? lut[raw[(size_t) (r0 + r) * stride + at_of[col]]] : (uint8_t) 0;
	}
	__syncthreads();
	uint32_t const bits = 8u >> bsh, per = 1u << bsh, rowbytes = MT_T >> bsh, cpc = rowbytes / 16u;
	for (uint32_t i = tid; i < MT_PACK_COLS * cpc; i += MT_T)
	{
		uint32_t const col = i / cpc, ch = i - col * cpc;
		size_t const at = (size_t) blockIdx.y * rowbytes + (size_t) ch * 16u;
		if (col >= nc || at >= ld) continue;
		uint8_t const *const src = &tile[col][ch * 16u * per];
		uint32_t w[4] = {0u, 0u, 0u, 0u};
#pragma unroll
		for (uint32_t b = 0; b < 16u; ++b)
		{
			uint32_t byte = 0;
			for (uint32_t e = 0; e < per; ++e) byte |= (uint32_t) src[b * per + e] << (e * bits);
			w[b / 4u] |= byte << (8u * (b % 4u));
		}
		*reinterpret_cast<uint4 *>(out + (j0 + col) * ld + at) = make_uint4(w[0], w[1], w[2], w[3]);
	}
}

// ---- the lists from the bit matrix ----
static __global__ __launch_bounds__(EX_T) void k_exc_count(uint32_t const *__restrict__ bitsm, size_t nw, uint32_t *__restrict__ cnt)
{
	__shared__ uint32_t wsum[4];
	uint32_t const *const row = bitsm + (size_t) blockIdx.x * nw;
	uint32_t mine = 0;
	for (size_t i = threadIdx.x; i < nw; i += EX_T) mine += __popc(row[i]);
	uint32_t total;
	(void) id_block_exscan(mine, wsum, &total);
	if (threadIdx.x == 0) cnt[blockIdx.x] = total;
}

// off[0 .. rows], off[rows] = all cells.  One workgroup; a thread sums a run of rows (k_match_scan's scheme)
static __global__ __launch_bounds__(MT_SCAN_T) void k_exc_scan(uint32_t const *__restrict__ cnt, uint32_t rows, uint64_t *__restrict__ off)
{
	__shared__ uint64_t s_p[MT_SCAN_T];
	uint32_t const t = threadIdx.x, per = (rows + MT_SCAN_T - 1u) / MT_SCAN_T;
	uint32_t const lo = min(rows, t * per), hi = min(rows, lo + per);
	uint64_t p = 0;
	for (uint32_t r = lo; r < hi; ++r) p += cnt[r];
	s_p[t] = p;
	__syncthreads();
	if (t == 0)
	{
		uint64_t run = 0;
		for (uint32_t i = 0; i < MT_SCAN_T; ++i) { uint64_t const v = s_p[i]; s_p[i] = run; run += v; }
		off[rows] = run;
	}
	__syncthreads();
	uint64_t run = s_p[t];
	for (uint32_t r = lo; r < hi; ++r) { off[r] = run; run += cnt[r]; }
}

static __global__ __launch_bounds__(EX_T) void k_exc_write(uint32_t const *__restrict__ bitsm, size_t nw, uint64_t const *__restrict__ off, uint32_t *__restrict__ cols)
{
	__shared__ uint32_t wsum[4];
	uint32_t const *const row = bitsm + (size_t) blockIdx.x * nw;
	uint64_t base = off[blockIdx.x];
	for (size_t t0 = 0; t0 < nw; t0 += EX_T)
	{
		size_t const i = t0 + threadIdx.x;
		uint32_t v = i < nw ? row[i] : 0u;
		uint32_t total;
		uint64_t at = base + id_block_exscan(__popc(v), wsum, &total);
		for (; v; v &= v - 1u) cols[at++] = (uint32_t) (i * 32u + (uint32_t) __builtin_ctz(v));
		base += total;
	}
}

// off and cols (buffers of `owner`, whose error text a failure sets) from a finished bit matrix on stream st
inline int exc_lists_from_bits(fseq_ctx *owner, hipStream_t st, uint32_t const *bitsm, size_t nw, uint32_t rows, DevBuf<uint64_t> &off, DevBuf<uint32_t> &cols,
                               uint64_t *total)
{
	int rc;
	DevTemp<uint32_t> d_cnt(owner);
	if ((rc = d_cnt.alloc(rows)) || (rc = off.alloc(owner, (size_t) rows + 1))) return rc;
	hipLaunchKernelGGL(k_exc_count, dim3(rows), dim3(EX_T), 0, st, bitsm, nw, (uint32_t *) d_cnt);
	hipLaunchKernelGGL(k_exc_scan, dim3(1), dim3(MT_SCAN_T), 0, st, (uint32_t const *) d_cnt, rows, (uint64_t *) off);
	HIP_TRY(owner, hipGetLastError());
	uint64_t all = 0;
	HIP_TRY(owner, hipMemcpyAsync(&all, off + rows, 8, hipMemcpyDeviceToHost, st));
	HIP_TRY(owner, hipStreamSynchronize(st));
	if ((rc = cols.alloc(owner, (size_t) all))) return rc;
	hipLaunchKernelGGL(k_exc_write, dim3(rows), dim3(EX_T), 0, st, bitsm, nw, (uint64_t const *) off, (uint32_t *) cols);
	HIP_TRY(owner, hipGetLastError());
	HIP_TRY(owner, hipStreamSynchronize(st));
	*total = all;
	return FSEQ_OK;
}

} // namespace fseq
