// fseq_input.hpp -- kernels of the chunked input path (csrc/fseq_api_input.hip; include/fseq.h, fseq_input_begin .. fseq_input_end).
//
// A chunk of consecutive columns arrives row-major in one half of the staging buffer: row r at stage + r * rs, rs = the chunk's
// columns rounded up to 16 bytes, so every 16-byte piece of a staged row is aligned and lies inside the row.  The bytes of a
// row behind the chunk's last column are whatever the half held before: both kernels mask them.
//
// k_input_presence  which byte values occur in the chunk (the scan pass; dense codes in ascending byte order need the whole
//                   alphabet before the first column is encoded: consecutive_alphabet_as_builder, generate_context.cc:135-147)
// k_input_encode    bytes -> codes -> packed columns [c0, c0 + ncols) of the resident alignment, in their final place: columns
//                   are packed on their own (whole bytes, ld bytes a column), so a chunk touches no other chunk's bytes
// and, for the input that drops its identity columns on the way (fseq_input_scan_identity .. fseq_input_end_kept), in
// fseq_input_reduced.hpp:
// k_input_identity         k_input_presence's words and, per 16-column piece, the OR over the rows of (piece ^ row 0's piece): the
//                          grid is pieces x row slabs, the slabs meet through atomicOr
// k_input_identity_finish  mask[c0 + j], ref[c0 + j] of the chunk from that accumulator, which it clears for the next chunk
// k_input_encode_kept      k_input_encode on the kept columns of the chunk alone, into an alignment of exactly their number
#pragma once

#include <hip/hip_runtime.h>
#include <cstdint>

namespace fseq {

constexpr uint32_t IN_T = 256;               // threads of both kernels
constexpr uint32_t IN_TILE_COLS = 128;       // k_input_encode: columns of a tile = one 128-byte line of every staged row
constexpr uint32_t IN_TILE_BYTES = 64;       // ... packed bytes of each of them = 64 << bsh rows (one byte per lane of a wave)

static __global__ __launch_bounds__(IN_T) void k_input_presence(uint8_t const *__restrict__ stage, size_t rs, uint32_t m, uint32_t ncols,
                                                                 uint32_t *__restrict__ present /* 8 words */)
{
	__shared__ uint32_t bm[8];
	if (threadIdx.x < 8) bm[threadIdx.x] = 0;
	__syncthreads();
	uint32_t loc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
	uint32_t const ppr = (ncols + 15u) >> 4;                       // pieces of a row that hold a column of the chunk
	uint64_t const total = (uint64_t) m * ppr, stride = (uint64_t) gridDim.x * IN_T;
	for (uint64_t i = (uint64_t) blockIdx.x * IN_T + threadIdx.x; i < total; i += stride)
	{
		uint32_t const r = (uint32_t) (i / ppr), p = (uint32_t) (i - (uint64_t) r * ppr);
		uint32_t const valid = min(16u, ncols - p * 16u);          // (the rest of the piece is the row's padding)
		uint4 const v = *reinterpret_cast<uint4 const *>(stage + (size_t) r * rs + (size_t) p * 16u);
		uint32_t const w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
		for (int q = 0; q < 4; ++q)
#pragma unroll
			for (int b = 0; b < 4; ++b)
			{
				uint32_t const c = (w[q] >> (8 * b)) & 255u;
				bool const in = (uint32_t) (4 * q + b) < valid;
#pragma unroll
				for (int k = 0; k < 8; ++k) loc[k] |= (in && (c >> 5) == (uint32_t) k) ? (1u << (c & 31u)) : 0u;
			}
	}
#pragma unroll
	for (int k = 0; k < 8; ++k)
		if (loc[k]) atomicOr(&bm[k], loc[k]);
	__syncthreads();
	if (threadIdx.x < 8 && bm[threadIdx.x]) atomicOr(&present[threadIdx.x], bm[threadIdx.x]);
}

// One tile = IN_TILE_COLS columns x IN_TILE_BYTES packed bytes (256 / 128 / 64 rows at 2 / 4 / 8 bits); workgroup blockIdx.x
// takes row tile blockIdx.x % row_tiles of column tile blockIdx.x / row_tiles (neighbours write one column's neighbouring bytes).
//   in:   a lane owns one packed byte of the column, that is 1 << BSH consecutive rows, and a wave one 16-column piece at a
//         time: 1 << BSH 16-byte loads along the lane's rows (the four waves and their second pieces use up every 128-byte
//         line the first one fetched), 16 look-ups per load in the 256-byte table in LDS, the codes of the rows of a byte
//         OR-ed together in registers: the pack costs no LDS traffic.
//   LDS:  out[column][byte], 64 bytes a column and NO padding.  A wave writes byte `lane` of one column per instruction: 64
//         consecutive bytes, 16 banks, conflict-free.  The stores read it as 16-byte pieces, thread t piece t & 3 of column
//         t >> 2: the 16 lanes of every ds_read_b128 group hold 4 columns x 4 pieces whose 16-byte slots (column * 4 + piece)
//         mod 16 are all different -- the lane groups {0-3, 12-15, 20-27} and {4-11, 16-19, 28-31} are columns {0, 3, 5, 6} and
//         {1, 2, 4, 7}, residues {0, 3, 1, 2} and {1, 2, 0, 3} mod 4 -- so the read is conflict-free where tile[64][65] read
//         bytes at a stride of 65.
//   out:  16-byte stores along a column (64, 32 or 16 rows each); four lanes write 64 consecutive bytes of a column.
// Rows >= m give code 0, so the padding fields behind row m - 1 and the padding bytes up to ld are written as zeros.  check:
// the table holds 0xFF for a byte outside the alphabet (sigma < 256); such a byte in a cell of the chunk is recorded in
// bad[8] (256 bits) and encoded as code 0 -- the host looks once, at the end of the input.
template <int BSH>
static __global__ __launch_bounds__(IN_T) void k_input_encode(uint8_t const *__restrict__ stage, size_t rs, uint32_t m, uint32_t ncols,
                                                               uint8_t const *__restrict__ table, uint32_t check, uint8_t *__restrict__ msa_c0 /* column c0 */,
                                                               size_t ld, uint32_t row_tiles, uint32_t *__restrict__ bad)
{
	constexpr uint32_t SPB = 1u << BSH, BITS = 8u >> BSH;
	__shared__ __attribute__((aligned(16))) uint8_t out[IN_TILE_COLS * IN_TILE_BYTES];
	__shared__ uint8_t tab[256];
	__shared__ uint32_t badbm[8];
	uint32_t const tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
	tab[tid] = table[tid];
	if (tid < 8) badbm[tid] = 0;
	__syncthreads();
	uint32_t const ty = blockIdx.x % row_tiles, tx = blockIdx.x / row_tiles;
	uint32_t const col0 = tx * IN_TILE_COLS;
	size_t const byte0 = (size_t) ty * IN_TILE_BYTES;
	uint64_t const row0 = (uint64_t) (byte0 + lane) << BSH;
	for (uint32_t p = wave; p < IN_TILE_COLS / 16u; p += IN_T / 64u)
	{
		uint32_t const cp = col0 + p * 16u;
		uint32_t acc[4] = {0, 0, 0, 0};
		if (cp < ncols)                                            // (then the whole piece lies inside the padded row)
		{
#pragma unroll
			for (uint32_t i = 0; i < SPB; ++i)
			{
				uint64_t const r = row0 + i;
				if (r < m)
				{
					uint4 const v = *reinterpret_cast<uint4 const *>(stage + (size_t) r * rs + cp);
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
								if (cp + 4u * q + b < ncols) atomicOr(&badbm[byte >> 5], 1u << (byte & 31u));
								code = 0;
							}
							acc[q] |= code << (8u * b + BITS * i);
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
		if (col0 + col < ncols && at < ld)
			*reinterpret_cast<uint4 *>(msa_c0 + (size_t) (col0 + col) * ld + at) = *reinterpret_cast<uint4 const *>(out + col * IN_TILE_BYTES + piece * 16u);
	}
	if (tid < 8 && badbm[tid]) atomicOr(&bad[tid], badbm[tid]);
}

} // namespace fseq
