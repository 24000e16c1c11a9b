// fseq_rowsplit.hpp -- a resident alignment split along its rows on the device: every source column is read once and gives a kept
// column (the rows that stay, compacted) and a held-out column (the rows set aside, in the order of the caller's list).
//
// replaces: nothing of the reference, whose chain holds rows out by removing lines from the list file and reading everything again.
// The alignment is column-major, 8 >> bsh bits a code, column k at src + k * src_ld, ld a multiple of 16 and the base 16-byte
// aligned on every input path.  Dropping rows is a compaction of 2-, 4- or 8-bit fields inside every packed column; the plan of it
// (csrc/fseq_rowsplit_plan.hpp) is made once on the host and is the same for every column: one descriptor {base, keep} per 32-bit
// output word, and the strips of output chunks a long column is taken in.
//
//   k_rows_split<BITS>   grid (column tiles, strips), 256 threads.  A workgroup owns one strip for good and walks over tiles of
//                        consecutive columns.  Once: its strip's descriptors (8 bytes a word, at most 2,048) and, where it fits,
//                        the held list go into LDS and stay there across all its columns.  Per tile, three steps:
//     stage   the strip's source chunks of every column of the tile, 16-byte loads into LDS (a chunk of slack behind every
//             column: a window may reach 8 bytes past the last chunk it selects fields from; what it finds there is deleted)
//     build   a lane a word: the 64-bit window from three LDS words by two funnel shifts, then one delete-a-field step per
//             hole of keep (x = (x & low) | ((x >> bits) & ~low), keep folded the same way); a word without holes is one funnel
//             shift and a mask.  Consecutive lanes read consecutive LDS words.  The words go to an LDS image of the output tile.
//             Slow words (keep = 0) are gathered field by field through kept[] from the source in memory: the plan makes them
//             only where more than `per` held-out rows follow each other, and they are the one place kept[] is read.
//             The held-out words are gathered field by field in the same step: from the staged bytes where the strip stages
//             whole columns, from memory (bytes this pass has in L2) where columns go in strips; the strips share them out.
//     store   16 bytes a lane from the image, contiguous along the column and across the columns of the tile where the
//             strip is the whole column.  Padding words up to ld carry the pad descriptor and come out as zeros.
// No atomics, nothing waits on another workgroup.  Loads stay inside [column, column + ld): the staged chunks are chunks of the
// column's ceil(col_bytes / 16), and a field is only ever taken at a row index the host's checked plan names (< m), so whatever a
// borrowed buffer holds behind row m - 1 reaches no output field.  No index is formed from device data but those of the plan.
#pragma once

#include "fseq_core.hpp"
#include "fseq_rowsplit_plan.hpp"

namespace fseq {

constexpr uint32_t RS_T = 256;
constexpr uint32_t RS_HELD_LDS = 2048;               // held rows up to here: the list in LDS

struct RowSplitArgs {
	uint8_t const *src; size_t src_ld; uint64_t n;
	uint2 const *desc;                       // [4 out_chunks] {base, keep}; behind the last word {RS_PAD_WORD, 0}
	uint32_t const *kept; uint32_t n_kept;   // (slow words only)
	uint32_t const *held; uint32_t n_held;
	RowSplitStrip const *strips; uint32_t whole;
	uint32_t tile_cols;
	uint32_t lds_in, lds_out, lds_desc;      // the LDS layout: 16-byte chunks of the stage and of the output image, descriptors (rs_lds_bytes)
	uint8_t *dst; size_t dst_ld;
	uint8_t *hdst; size_t h_ld;
};

// the 32 bits from bit sh (< 32) of hi:lo on
__device__ __forceinline__ uint32_t rs_funnel(uint32_t lo, uint32_t hi, uint32_t sh) { return (uint32_t) ((((uint64_t) hi << 32) | lo) >> sh); }

// the dynamic LDS of a launch: [lds_in chunks][lds_out chunks][lds_desc descriptors][the held list where it has at most RS_HELD_LDS rows]
inline size_t rs_lds_bytes(RowSplitArgs const &A)
{
	return ((size_t) A.lds_in + A.lds_out) * 16u + (size_t) A.lds_desc * 8u + (A.n_held <= RS_HELD_LDS ? (size_t) A.n_held * 4u : 0u);
}

template <uint32_t BITS>
static __global__ __launch_bounds__(256) void k_rows_split(RowSplitArgs const A)
{
	constexpr uint32_t PER = 32u / BITS, RPB_SH = BITS == 2u ? 2u : BITS == 4u ? 1u : 0u, RPB_M = (1u << RPB_SH) - 1u, CM = (1u << BITS) - 1u;
	// sized by the launcher for the strips of this call (at most 513 + 512 chunks, 2,048 descriptors and 2,048 held rows: 41 KiB):
	// short columns leave room for more workgroups on a CU
	extern __shared__ uint4 rs_lds[];
	uint4 *const s_in = rs_lds, *const s_out = s_in + A.lds_in;
	uint2 *const s_desc = reinterpret_cast<uint2 *>(s_out + A.lds_out);
	uint32_t *const s_held = reinterpret_cast<uint32_t *>(s_desc + A.lds_desc);
	RowSplitStrip const S = A.strips[blockIdx.y];
	uint32_t const oc = S.c1 - S.c0, nw = 4u * oc, sc = S.src_chunks, stride = sc + 1u;      // stride: chunks of s_in a column takes
	uint32_t const hw_n = (uint32_t) (A.h_ld / 4u);                                           // words of a held-out column, padding included
	bool const held_lds = A.n_held <= RS_HELD_LDS;
	for (uint32_t w = threadIdx.x; w < nw; w += RS_T) s_desc[w] = A.desc[(size_t) 4u * S.c0 + w];
	if (held_lds)
		for (uint32_t q = threadIdx.x; q < A.n_held; q += RS_T) s_held[q] = A.held[q];
	uint64_t const tiles = (A.n + A.tile_cols - 1u) / A.tile_cols;
	uint32_t const *const in_w = reinterpret_cast<uint32_t const *>(s_in);
	uint8_t const *const in_b = reinterpret_cast<uint8_t const *>(s_in);
	uint32_t *const out_w = reinterpret_cast<uint32_t *>(s_out);
	for (uint64_t t = blockIdx.x; t < tiles; t += gridDim.x)
	{
		uint64_t const col0 = t * A.tile_cols;
		uint32_t const nc = (uint32_t) min((uint64_t) A.tile_cols, A.n - col0);
		__syncthreads();                                                      // (the descriptors; the stores of the tile before)
		for (uint32_t q = threadIdx.x; q < nc * sc; q += RS_T)
		{
			uint32_t const jl = q / sc, ch = q - jl * sc;
			s_in[jl * stride + ch] = *reinterpret_cast<uint4 const *>(A.src + (col0 + jl) * A.src_ld + ((size_t) S.src0 + ch) * 16u);
		}
		__syncthreads();
		for (uint32_t q = threadIdx.x; q < nc * nw; q += RS_T)
		{
			uint32_t const jl = q / nw, wl = q - jl * nw;
			uint2 const d = s_desc[wl];
			uint32_t word = 0;
			if (d.y)
			{
				uint32_t const rel = (d.x >> RPB_SH) - S.src0 * 16u;             // byte of the window's first field in the staged range
				uint32_t const sh = (rel & 3u) * 8u + (d.x & RPB_M) * BITS;
				uint32_t const *const p = in_w + jl * stride * 4u + (rel >> 2);
				uint32_t const a = p[0], b = p[1];
				uint32_t k = d.y;
				if (0u == (k & (k + 1u)))
					word = rs_funnel(a, b, sh);
				else
				{
					uint32_t const c = p[2];
					uint64_t x = ((uint64_t) rs_funnel(b, c, sh) << 32) | rs_funnel(a, b, sh);
					do {
						uint32_t const z = (uint32_t) __builtin_ctz(~k), lowk = (1u << z) - 1u;
						uint64_t const low = (1ull << (z * BITS)) - 1ull;
						x = (x & low) | ((x >> BITS) & ~low);
						k = (k & lowk) | ((k >> 1) & ~lowk);
					} while (k & (k + 1u));
					word = (uint32_t) x;
				}
				uint32_t const cnt = (uint32_t) __popc(k);
				if (cnt < PER) word &= (1u << (cnt * BITS)) - 1u;
			}
			else if (d.x != RS_PAD_WORD)
			{
				uint8_t const *const col = A.src + (col0 + jl) * A.src_ld;
				uint32_t const q0 = (4u * S.c0 + wl) * PER;
				uint32_t const nf = min(PER, A.n_kept - q0);                     // (q0 < n_kept: the word is one of the plan's)
				for (uint32_t i = 0; i < nf; ++i)
				{
					uint32_t const r = A.kept[q0 + i];
					word |= (((uint32_t) col[r >> RPB_SH] >> ((r & RPB_M) * BITS)) & CM) << (i * BITS);
				}
			}
			out_w[jl * nw + wl] = word;
		}
		// the held-out words: strip s takes the words s, s + strips, ... (a strip that stages whole columns is the only one)
		for (uint32_t q = threadIdx.x; q < nc * hw_n; q += RS_T)
		{
			uint32_t const jl = q / hw_n, hw = q - jl * hw_n;
			if (hw % gridDim.y != blockIdx.y) continue;
			uint8_t const *const col = A.src + (col0 + jl) * A.src_ld;
			uint32_t word = 0;
			uint32_t const nf = hw * PER < A.n_held ? min(PER, A.n_held - hw * PER) : 0u;      // (0: a padding word)
			for (uint32_t i = 0; i < nf; ++i)
			{
				uint32_t const r = held_lds ? s_held[hw * PER + i] : A.held[hw * PER + i];
				uint32_t const byte = A.whole ? (uint32_t) in_b[(size_t) jl * stride * 16u + (r >> RPB_SH)] : (uint32_t) col[r >> RPB_SH];
				word |= ((byte >> ((r & RPB_M) * BITS)) & CM) << (i * BITS);
			}
			*reinterpret_cast<uint32_t *>(A.hdst + (col0 + jl) * A.h_ld + (size_t) hw * 4u) = word;
		}
		__syncthreads();
		for (uint32_t q = threadIdx.x; q < nc * oc; q += RS_T)
		{
			uint32_t const jl = q / oc, ch = q - jl * oc;
			*reinterpret_cast<uint4 *>(A.dst + (col0 + jl) * A.dst_ld + ((size_t) S.c0 + ch) * 16u) = s_out[jl * oc + ch];
		}
	}
}

} // namespace fseq
