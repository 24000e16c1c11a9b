// fseq_input_reduced.hpp -- kernels of the chunked input path that drops the identity columns on the way (csrc/fseq_api_input.hip;
// include/fseq.h, fseq_input_scan_identity .. fseq_input_end_kept).  The staged chunk is the one of fseq_input.hpp: row r at
// stage + r * rs, rs = the chunk's columns rounded up to 16 bytes, stale bytes behind the chunk's last column.
//
// k_input_identity         the scan pass: the byte values present (k_input_presence's words) and, per 16-column piece, the OR over
//                          the rows of (piece ^ row 0's piece), in one pass of 16-byte loads.  The grid is pieces x row slabs: a
//                          chunk of 1,300 columns of 100,000 rows is 6 workgroups of pieces, and the slabs fill the chip.  The
//                          slabs of a piece meet in acc[] through atomicOr: no order among workgroups, nobody waits
// k_input_identity_finish  behind it on the stream: mask[c0 + j] = (byte j of acc == 0), ref[c0 + j] = row 0's byte, acc cleared
//                          for the next chunk
// k_input_encode_kept      k_input_encode on the kept columns of the chunk: tile column j is column k0 + col0 + j of the NEW
//                          alignment and reads chunk column kept[k0 + col0 + j] - c0.  The kept list (k_identity_count / _offsets /
//                          _scatter of fseq_identity.hpp on the finished mask) is the new context's own
//
// How k_input_encode_kept fetches its bytes: the tile's 128 chunk offsets go to LDS once.  A wave takes a 16-column piece as in
// k_input_encode; where the piece's 16 kept columns are 16 consecutive chunk columns starting at a multiple of 16 (always so
// where no identity column lies in reach: the 0 %-identity case runs k_input_encode's loads) it is one 16-byte load a row,
// otherwise 16 byte loads a row through the offsets (a broadcast LDS read each; the bytes of a row lie within a few cache
// lines, kept ascends).  The choice is per piece, so uniform over the wave.  Register use: profiles/input_reduced_resources.txt.
#pragma once

#include "fseq_input.hpp"

namespace fseq {

constexpr uint32_t INR_PX = 16;                  // k_input_identity: 16-column pieces across a workgroup (256 bytes of a staged row)
constexpr uint32_t INR_RY = IN_T / INR_PX;       // ... rows a workgroup reads at a time
constexpr uint32_t INR_NONE = 0xFFFFFFFFu;       // k_input_encode_kept: no kept column at this place of the tile (a chunk offset is below 2^31)

// acc words the scan of chunks of at most `cols` columns touches: 4 a piece, pieces in whole workgroups
inline size_t input_identity_acc_words(uint64_t cols) { return (size_t) ((((cols + 15) / 16 + INR_PX - 1) / INR_PX) * INR_PX * 4); }

// grid (ceil(pieces / INR_PX), slabs); workgroup (x, y) takes the rows [y * slab_rows, (y + 1) * slab_rows) of its pieces
static __global__ __launch_bounds__(IN_T) void k_input_identity(uint8_t const *__restrict__ stage, size_t rs, uint32_t m, uint32_t ncols, uint32_t slab_rows,
                                                                 uint32_t *__restrict__ present /* 8 words */, uint32_t *__restrict__ acc)
{
	__shared__ uint32_t bm[8];
	__shared__ uint32_t diff[INR_PX * 4];
	uint32_t const tid = threadIdx.x;
	if (tid < 8) bm[tid] = 0;
	if (tid < INR_PX * 4) diff[tid] = 0;
	__syncthreads();
	uint32_t const ppr = (ncols + 15u) >> 4;                       // pieces of a row that hold a column of the chunk
	uint32_t const px = tid & (INR_PX - 1u), p = blockIdx.x * INR_PX + px;
	uint64_t const r_lo = (uint64_t) blockIdx.y * slab_rows, r_hi = min((uint64_t) m, r_lo + slab_rows);
	uint32_t loc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
	uint32_t x[4] = {0, 0, 0, 0};
	if (p < ppr)
	{
		uint32_t const valid = min(16u, ncols - p * 16u);          // (the rest of the piece is the row's padding: stale bytes)
		uint8_t const *const at = stage + (size_t) p * 16u;
		uint4 const ref = *reinterpret_cast<uint4 const *>(at);    // row 0
		uint32_t const f[4] = {ref.x, ref.y, ref.z, ref.w};
		for (uint64_t r = r_lo + tid / INR_PX; r < r_hi; r += INR_RY)
		{
			uint4 const v = *reinterpret_cast<uint4 const *>(at + (size_t) r * rs);
			uint32_t const w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
			for (int q = 0; q < 4; ++q)
			{
				x[q] |= w[q] ^ f[q];
#pragma unroll
				for (int b = 0; b < 4; ++b)
				{
					uint32_t const c = (w[q] >> (8 * b)) & 255u;
					bool const in = (uint32_t) (4 * q + b) < valid;
#pragma unroll
					for (int k = 0; k < 8; ++k) loc[k] |= (in && (c >> 5) == (uint32_t) k) ? (1u << (c & 31u)) : 0u;
				}
			}
		}
#pragma unroll
		for (int q = 0; q < 4; ++q)
		{
			uint32_t const vb = valid > 4u * q ? valid - 4u * q : 0u;      // bytes of word q that are columns of the chunk
			x[q] &= vb >= 4u ? 0xFFFFFFFFu : (1u << (8u * vb)) - 1u;
			if (x[q]) atomicOr(&diff[px * 4u + q], x[q]);
		}
	}
#pragma unroll
	for (int k = 0; k < 8; ++k)
		if (loc[k]) atomicOr(&bm[k], loc[k]);
	__syncthreads();
	if (tid < 8 && bm[tid]) atomicOr(&present[tid], bm[tid]);
	if (tid < INR_PX * 4 && diff[tid]) atomicOr(&acc[(size_t) blockIdx.x * (INR_PX * 4u) + tid], diff[tid]);      // (< gridDim.x * 64 words: input_identity_acc_words)
}

// a thread takes one word of acc, the 4 columns [4 t, 4 t + 4) of the chunk; mask_c0 / ref_c0: column c0 of the two arrays
static __global__ __launch_bounds__(IN_T) void k_input_identity_finish(uint8_t const *__restrict__ stage /* row 0 */, uint32_t ncols, uint32_t *__restrict__ acc,
                                                                        uint8_t *__restrict__ mask_c0, uint8_t *__restrict__ ref_c0)
{
	uint32_t const words = (ncols + 3u) >> 2;
	for (uint32_t t = blockIdx.x * IN_T + threadIdx.x; t < words; t += gridDim.x * IN_T)
	{
		uint32_t const w = acc[t];
		acc[t] = 0;
		uint32_t const row0 = *reinterpret_cast<uint32_t const *>(stage + (size_t) t * 4u);     // (inside the padded row)
#pragma unroll
		for (uint32_t b = 0; b < 4; ++b)
		{
			uint32_t const j = t * 4u + b;
			if (j < ncols)
			{
				mask_c0[j] = ((w >> (8u * b)) & 255u) ? 0 : 1;
				ref_c0[j] = (uint8_t) (row0 >> (8u * b));
			}
		}
	}
}

// k_input_encode's tile (IN_TILE_COLS columns x IN_TILE_BYTES packed bytes, the same LDS transpose and 16-byte stores) over the
// kept columns [k0, k1) of the chunk that begins at source column c0: workgroup blockIdx.x takes row tile blockIdx.x % row_tiles of
// the kept columns k0 + (blockIdx.x / row_tiles) * IN_TILE_COLS on.  msa: column 0 of the new alignment.  Rows >= m give code 0 and
// the bytes up to ld are stored as zeros, as there; `bad` records a byte outside the alphabet in a kept cell only -- no other
// cell is read.
template <int BSH>
static __global__ __launch_bounds__(IN_T) void k_input_encode_kept(uint8_t const *__restrict__ stage, size_t rs, uint32_t m, uint64_t c0,
                                                                    uint32_t const *__restrict__ kept, uint64_t k0, uint64_t k1,
                                                                    uint8_t const *__restrict__ table, uint32_t check, uint8_t *__restrict__ msa, size_t ld,
                                                                    uint32_t row_tiles, uint32_t *__restrict__ bad)
{
	constexpr uint32_t SPB = 1u << BSH, BITS = 8u >> BSH;
	__shared__ __attribute__((aligned(16))) uint8_t out[IN_TILE_COLS * IN_TILE_BYTES];
	__shared__ uint8_t tab[256];
	__shared__ uint32_t badbm[8];
	__shared__ uint32_t offs[IN_TILE_COLS];
	uint32_t const tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
	uint32_t const ty = blockIdx.x % row_tiles, tx = blockIdx.x / row_tiles;
	uint64_t const kc0 = k0 + (uint64_t) tx * IN_TILE_COLS;            // the tile's first kept column
	tab[tid] = table[tid];
	if (tid < 8) badbm[tid] = 0;
	if (tid < IN_TILE_COLS) offs[tid] = kc0 + tid < k1 ? (uint32_t) (kept[kc0 + tid] - c0) : INR_NONE;      // (c0 <= kept[k] < c0 + the chunk's columns for k in [k0, k1))
	__syncthreads();
	size_t const byte0 = (size_t) ty * IN_TILE_BYTES;
	uint64_t const row0 = (uint64_t) (byte0 + lane) << BSH;
	for (uint32_t p = wave; p < IN_TILE_COLS / 16u; p += IN_T / 64u)
	{
		uint32_t const o0 = offs[p * 16u], o15 = offs[p * 16u + 15u];
		uint32_t acc[4] = {0, 0, 0, 0};
		if (o0 != INR_NONE)
		{
			// kept ascends strictly: 15 apart is 16 consecutive chunk columns
			bool const run = o15 != INR_NONE && o15 - o0 == 15u && 0u == (o0 & 15u);
#pragma unroll
			for (uint32_t i = 0; i < SPB; ++i)
			{
				uint64_t const r = row0 + i;
				if (r < m)
				{
					uint8_t const *const row = stage + (size_t) r * rs;
					if (run)
					{
						uint4 const v = *reinterpret_cast<uint4 const *>(row + o0);
						uint32_t const w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
						for (uint32_t q = 0; q < 4; ++q)
#pragma unroll
							for (uint32_t b = 0; b < 4; ++b)
							{
								uint32_t const byte = (w[q] >> (8u * b)) & 255u;
								uint32_t code = tab[byte];
								if (check && code == 0xFFu)
								{
									atomicOr(&badbm[byte >> 5], 1u << (byte & 31u));
									code = 0;
								}
								acc[q] |= code << (8u * b + BITS * i);
							}
					}
					else
					{
#pragma unroll
						for (uint32_t j = 0; j < 16; ++j)
						{
							uint32_t const o = offs[p * 16u + j];
							if (o != INR_NONE)
							{
								uint32_t const byte = row[o];
								uint32_t code = tab[byte];
								if (check && code == 0xFFu)
								{
									atomicOr(&badbm[byte >> 5], 1u << (byte & 31u));
									code = 0;
								}
								acc[j >> 2] |= code << (8u * (j & 3u) + BITS * i);
							}
						}
					}
				}
			}
		}
#pragma unroll
		for (uint32_t j = 0; j < 16; ++j)
			out[(p * 16u + j) * IN_TILE_BYTES + lane] = (uint8_t) (acc[j >> 2] >> (8u * (j & 3u)));
	}
	__syncthreads();
	for (uint32_t u = tid; u < IN_TILE_COLS * (IN_TILE_BYTES / 16u); u += IN_T)
	{
		uint32_t const col = u >> 2, piece = u & 3u;
		size_t const at = byte0 + piece * 16u;
		if (kc0 + col < k1 && at < ld)
			*reinterpret_cast<uint4 *>(msa + (size_t) (kc0 + col) * ld + at) = *reinterpret_cast<uint4 const *>(out + col * IN_TILE_BYTES + piece * 16u);
	}
	if (tid < 8 && badbm[tid]) atomicOr(&bad[tid], badbm[tid]);
}

} // namespace fseq
