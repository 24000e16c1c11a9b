// fseq_identity.hpp -- identity columns (columns in which every row carries the same symbol) found, dropped and put back on
// the device.
//
// replaces: remove-identity-columns (main.cc:105-153 the per-chunk comparison, :157-227 the driver) and
// insert-identity-columns (main.cc:138-195), which stream the rows through 32 KiB host buffers.  Here the alignment is
// already resident: column-major, 8 >> bsh bits per code, column k at msa + k * ld, ld a multiple of 16 and the base
// 16-byte aligned on every input path (alloc_msa, fseq_set_device_columns, fseq_set_device_columns_packed).
//
//   k_identity_mask     one pass of 16-byte loads over every column; mask[k] = 1 iff all rows agree with row 0
//   k_identity_count    kept columns (mask == 0) per tile of ID_TILE columns            \  the exclusive scan of the kept flags
//   k_identity_offsets  exclusive scan of the tile counts (one workgroup) + the total    >  in three launches: no launch waits
//   k_identity_scatter  kept[j] = the j-th kept column, tile by tile                    /   for another workgroup of its own
//   k_identity_gather   column kept[j] of the source -> column j of the new alignment, 16 bytes a lane
//   k_identity_ref      row 0 of every source column as a raw byte
//   k_identity_fill     every line of a batch of founders = the reference bytes + '\n', in aligned 16-byte stores
//   k_founders_restored k_founders (fseq_joinprep.hpp) writing the kept positions: line[kept[k]]
//
// Lanes to columns in k_identity_mask, by the 16-byte chunks C = ceil(col_bytes / 16) of a column:
//   C <= 64   (a column of at most 1 KiB: BASELINE C3's 626 bytes, the 16 bytes of small inputs): a sub-group of
//             G = 2^ceil(log2 C) lanes per column, one load per lane; a wave covers 64 / G consecutive columns, a workgroup
//             256 / G, so the loads of a wave run on through consecutive columns (contiguous where ld == 16 C)
//   C <= 1024 (up to 16 KiB): one wave per column, striding over it 1 KiB at a time
//   beyond    (BASELINE C4's 25,000 bytes) one workgroup per column, 4 KiB at a time, the four waves' words combined through LDS
// In all three the lanes OR together (word ^ first code replicated over the word), with the bytes from col_bytes on and the
// fields behind row m - 1 in the last byte masked off (a borrowed buffer may hold anything there; nothing between the last
// chunk of a column and ld is ever loaded), and the OR is reduced across the lanes of the (sub-)group by DPP as k_max_code does.
#pragma once

#include "fseq_core.hpp"

namespace fseq {

constexpr uint32_t ID_T = 256;                       // threads of every kernel here
constexpr uint32_t ID_WAVE_CHUNKS = 64;              // C up to here: sub-groups of a wave
constexpr uint32_t ID_WG_CHUNKS = 1024;              // C up to here: a wave per column; beyond: a workgroup
constexpr uint32_t ID_TILE = 2048;                   // columns per workgroup of the scan (8 per thread)

struct IdShape {
	uint32_t col_bytes, chunks, tail_rows, G;        // G: lanes per column (1 .. 64), or 256: a workgroup
	uint32_t cols_per_wg;
};

inline IdShape id_shape(uint32_t m, uint32_t bsh)
{
	IdShape s{};
	s.col_bytes = (m + (1u << bsh) - 1u) >> bsh;
	s.chunks = (s.col_bytes + 15u) / 16u;
	s.tail_rows = m & ((1u << bsh) - 1u);
	if (s.chunks > ID_WG_CHUNKS) s.G = ID_T;
	else if (s.chunks > ID_WAVE_CHUNKS) s.G = 64;
	else { s.G = 1; while (s.G < s.chunks) s.G <<= 1; }
	s.cols_per_wg = ID_T / s.G;
	return s;
}

// the bits of word w of chunk `chunk` that hold rows of the column
__device__ __forceinline__ uint32_t id_word_mask(uint32_t chunk, uint32_t w, uint32_t col_bytes, uint32_t tail_rows, uint32_t bits)
{
	uint32_t const b0 = chunk * 16u + 4u * w;
	if (b0 >= col_bytes) return 0u;
	uint32_t const vb = col_bytes - b0;                                  // bytes of the column from b0 on
	uint32_t wm = vb >= 4u ? 0xFFFFFFFFu : (1u << (8u * vb)) - 1u;
	if (tail_rows && vb <= 4u)                                           // the column's last byte is byte vb - 1 of this word
		wm &= ~((0xFFu & ~((1u << (tail_rows * bits)) - 1u)) << (8u * (vb - 1u)));
	return wm;
}

__device__ __forceinline__ uint32_t id_chunk_diff(uint8_t const *__restrict__ col, uint32_t chunk, uint32_t pattern, uint32_t col_bytes,
                                                   uint32_t chunks, uint32_t tail_rows, uint32_t bits)
{
	uint4 const v = *reinterpret_cast<uint4 const *>(col + (size_t) chunk * 16u);
	if (chunk + 1u < chunks) return (v.x ^ pattern) | (v.y ^ pattern) | (v.z ^ pattern) | (v.w ^ pattern);
	return ((v.x ^ pattern) & id_word_mask(chunk, 0, col_bytes, tail_rows, bits)) | ((v.y ^ pattern) & id_word_mask(chunk, 1, col_bytes, tail_rows, bits)) |
	       ((v.z ^ pattern) & id_word_mask(chunk, 2, col_bytes, tail_rows, bits)) | ((v.w ^ pattern) & id_word_mask(chunk, 3, col_bytes, tail_rows, bits));
}

// count: += identity columns, one atomic per workgroup
static __global__ __launch_bounds__(256) void k_identity_mask(uint8_t const *__restrict__ msa, size_t ld, uint64_t n, uint32_t bsh, IdShape const s,
                                                       uint8_t *__restrict__ mask, uint32_t *__restrict__ count)
{
	__shared__ uint32_t part[4];
	__shared__ uint32_t wg_count;
	uint32_t const bits = 8u >> bsh, cmask = (1u << bits) - 1u;
	uint32_t const ones = bsh == 2 ? 0x55555555u : bsh == 1 ? 0x11111111u : 0x01010101u;
	if (threadIdx.x == 0) wg_count = 0;
	__syncthreads();
	uint32_t mine = 0;                                                   // identity columns this thread reported
	uint64_t const groups = (n + s.cols_per_wg - 1u) / s.cols_per_wg;
	for (uint64_t g = blockIdx.x; g < groups; g += gridDim.x)
	{
		if (s.G <= 64u)
		{
			uint32_t const sub = threadIdx.x & (s.G - 1u);
			uint64_t const c = g * s.cols_per_wg + threadIdx.x / s.G;
			uint32_t x = 0;
			if (c < n)
			{
				uint8_t const *const col = msa + c * ld;
				if (s.chunks <= ID_WAVE_CHUNKS)
				{
					// one load per lane; the first code comes from the sub-group's first lane
					uint32_t first = 0;
					uint4 v = make_uint4(0, 0, 0, 0);
					if (sub < s.chunks) v = *reinterpret_cast<uint4 const *>(col + (size_t) sub * 16u);
					first = v.x;
					uint32_t const pattern = ((uint32_t) __shfl((int) first, (int) (lane_id() & ~(s.G - 1u)), WAVE) & cmask) * ones;
					if (sub < s.chunks)
					{
						if (sub + 1u < s.chunks) x = (v.x ^ pattern) | (v.y ^ pattern) | (v.z ^ pattern) | (v.w ^ pattern);
						else
							x = ((v.x ^ pattern) & id_word_mask(sub, 0, s.col_bytes, s.tail_rows, bits)) | ((v.y ^ pattern) & id_word_mask(sub, 1, s.col_bytes, s.tail_rows, bits)) |
							    ((v.z ^ pattern) & id_word_mask(sub, 2, s.col_bytes, s.tail_rows, bits)) | ((v.w ^ pattern) & id_word_mask(sub, 3, s.col_bytes, s.tail_rows, bits));
					}
				}
				else
				{
					uint32_t const pattern = ((uint32_t) col[0] & cmask) * ones;
#pragma unroll 4
					for (uint32_t ch = sub; ch < s.chunks; ch += 64u) x |= id_chunk_diff(col, ch, pattern, s.col_bytes, s.chunks, s.tail_rows, bits);
				}
			}
			// (every lane of the wave takes part: a column past the end contributes 0, and a sub-group's last lane collects its own lanes only)
			if (s.G > 1u) x |= dpp_mov<DPP_ROW_SHR1, 0xF>(0u, x);
			if (s.G > 2u) x |= dpp_mov<DPP_ROW_SHR2, 0xF>(0u, x);
			if (s.G > 4u) x |= dpp_mov<DPP_ROW_SHR4, 0xF>(0u, x);
			if (s.G > 8u) x |= dpp_mov<DPP_ROW_SHR8, 0xF>(0u, x);
			if (s.G > 16u) x |= dpp_mov<DPP_ROW_BCAST15, 0xA>(0u, x);
			if (s.G > 32u) x |= dpp_mov<DPP_ROW_BCAST31, 0xC>(0u, x);
			if (sub == s.G - 1u && c < n)
			{
				mask[c] = x == 0u ? 1 : 0;
				mine += x == 0u ? 1u : 0u;
			}
		}
		else
		{
			uint64_t const c = g;
			uint8_t const *const col = msa + c * ld;
			uint32_t const pattern = ((uint32_t) col[0] & cmask) * ones;
			uint32_t x = 0;
#pragma unroll 4
			for (uint32_t ch = threadIdx.x; ch < s.chunks; ch += ID_T) x |= id_chunk_diff(col, ch, pattern, s.col_bytes, s.chunks, s.tail_rows, bits);
			x |= dpp_mov<DPP_ROW_SHR1, 0xF>(0u, x);
			x |= dpp_mov<DPP_ROW_SHR2, 0xF>(0u, x);
			x |= dpp_mov<DPP_ROW_SHR4, 0xF>(0u, x);
			x |= dpp_mov<DPP_ROW_SHR8, 0xF>(0u, x);
			x |= dpp_mov<DPP_ROW_BCAST15, 0xA>(0u, x);
			x |= dpp_mov<DPP_ROW_BCAST31, 0xC>(0u, x);
			if (lane_id() == 63) part[wave_id()] = x;
			__syncthreads();
			if (threadIdx.x == 0)
			{
				uint32_t const all = part[0] | part[1] | part[2] | part[3];
				mask[c] = all == 0u ? 1 : 0;
				mine += all == 0u ? 1u : 0u;
			}
			__syncthreads();
		}
	}
	if (mine) atomicAdd(&wg_count, mine);
	__syncthreads();
	if (threadIdx.x == 0 && wg_count) atomicAdd(count, wg_count);
}

// ---- the kept-column list: exclusive scan of (mask == 0) over the n columns ----
// a thread's 8 consecutive columns of tile t; returns how many are kept and their flags (bit i: column base + i kept)
__device__ __forceinline__ uint32_t id_kept_flags(uint8_t const *__restrict__ mask, uint64_t n, uint64_t base)
{
	uint32_t f = 0;
	if (base + 8u <= n)
	{
		uint2 const v = *reinterpret_cast<uint2 const *>(mask + base);   // (base is a multiple of 8, the mask 16-byte aligned)
#pragma unroll
		for (uint32_t i = 0; i < 4; ++i)
		{
			f |= ((v.x >> (8u * i)) & 255u) ? 0u : (1u << i);
			f |= ((v.y >> (8u * i)) & 255u) ? 0u : (16u << i);
		}
	}
	else
		for (uint32_t i = 0; i < 8u && base + i < n; ++i) f |= mask[base + i] ? 0u : (1u << i);
	return f;
}

// exclusive scan of v over the 256 threads of the workgroup; *total = the sum
__device__ __forceinline__ uint32_t id_block_exscan(uint32_t v, uint32_t *wsum /* 4 words of LDS */, uint32_t *total)
{
	uint32_t inc = v;
#pragma unroll
	for (int d = 1; d < WAVE; d <<= 1)
	{
		uint32_t const t = shfl_up_u32(inc, d);
		if ((int) lane_id() >= d) inc += t;
	}
	if (lane_id() == 63) wsum[wave_id()] = inc;
	__syncthreads();
	uint32_t before = 0, all = 0;
#pragma unroll
	for (uint32_t w = 0; w < 4; ++w)
	{
		uint32_t const s = wsum[w];
		before += w < wave_id() ? s : 0u;
		all += s;
	}
	__syncthreads();
	*total = all;
	return before + inc - v;
}

static __global__ __launch_bounds__(256) void k_identity_count(uint8_t const *__restrict__ mask, uint64_t n, uint32_t *__restrict__ tile_cnt)
{
	__shared__ uint32_t wsum[4];
	uint64_t const base = (uint64_t) blockIdx.x * ID_TILE + threadIdx.x * 8u;
	uint32_t total;
	(void) id_block_exscan(__popc(id_kept_flags(mask, n, base)), wsum, &total);
	if (threadIdx.x == 0) tile_cnt[blockIdx.x] = total;
}

// one workgroup: tile_cnt[t] becomes the number of kept columns in front of tile t; tile_cnt[ntiles] the total
static __global__ __launch_bounds__(256) void k_identity_offsets(uint32_t *__restrict__ tile_cnt, uint32_t ntiles)
{
	__shared__ uint32_t wsum[4];
	uint32_t carry = 0;
	for (uint32_t t0 = 0; t0 < ntiles; t0 += ID_T)
	{
		uint32_t const t = t0 + threadIdx.x;
		uint32_t const v = t < ntiles ? tile_cnt[t] : 0u;
		uint32_t total;
		uint32_t const ex = id_block_exscan(v, wsum, &total);
		if (t < ntiles) tile_cnt[t] = carry + ex;
		carry += total;
	}
	if (threadIdx.x == 0) tile_cnt[ntiles] = carry;
}

static __global__ __launch_bounds__(256) void k_identity_scatter(uint8_t const *__restrict__ mask, uint64_t n, uint32_t const *__restrict__ tile_off,
                                                          uint32_t *__restrict__ kept)
{
	__shared__ uint32_t wsum[4];
	uint64_t const base = (uint64_t) blockIdx.x * ID_TILE + threadIdx.x * 8u;
	uint32_t const f = id_kept_flags(mask, n, base);
	uint32_t total;
	uint32_t at = tile_off[blockIdx.x] + id_block_exscan(__popc(f), wsum, &total);
	for (uint32_t v = f; v; v &= v - 1u) kept[at++] = (uint32_t) (base + (uint32_t) __builtin_ctz(v));
}

// ---- the reduced alignment: column kept[j] of the source at column j, dst_ld = 16 chunks; the bytes behind the column and
// the fields behind row m - 1 in its last byte are written as zeros.  A workgroup takes cols_per_wg consecutive columns of
// the destination and its lanes run over their chunks in order: the stores are contiguous across columns, the loads within one.
static __global__ __launch_bounds__(256) void k_identity_gather(uint8_t const *__restrict__ src, size_t src_ld, uint32_t const *__restrict__ kept, uint64_t n_kept,
                                                         uint32_t bsh, IdShape const s, uint32_t cols_per_wg, uint8_t *__restrict__ dst)
{
	uint32_t const bits = 8u >> bsh;
	size_t const dst_ld = (size_t) s.chunks * 16u;
	uint64_t const groups = (n_kept + cols_per_wg - 1u) / cols_per_wg;
	for (uint64_t g = blockIdx.x; g < groups; g += gridDim.x)
	{
		uint64_t const j0 = g * cols_per_wg;
		uint32_t const nc = (uint32_t) min((uint64_t) cols_per_wg, n_kept - j0);
		uint32_t const work = nc * s.chunks;                              // (cols_per_wg * chunks < 2^32: the launcher's choice)
		for (uint32_t q = threadIdx.x; q < work; q += ID_T)
		{
			uint32_t const jl = q / s.chunks, ch = q - jl * s.chunks;
			uint4 v = *reinterpret_cast<uint4 const *>(src + (size_t) kept[j0 + jl] * src_ld + (size_t) ch * 16u);
			if (ch + 1u == s.chunks)
			{
				v.x &= id_word_mask(ch, 0, s.col_bytes, s.tail_rows, bits);
				v.y &= id_word_mask(ch, 1, s.col_bytes, s.tail_rows, bits);
				v.z &= id_word_mask(ch, 2, s.col_bytes, s.tail_rows, bits);
				v.w &= id_word_mask(ch, 3, s.col_bytes, s.tail_rows, bits);
			}
			*reinterpret_cast<uint4 *>(dst + (j0 + jl) * dst_ld + (size_t) ch * 16u) = v;
		}
	}
}

// row 0 of every source column as the byte it stands for (insert-identity-columns' --reference = input row 0)
static __global__ __launch_bounds__(256) void k_identity_ref(uint8_t const *__restrict__ msa, size_t ld, uint64_t n, uint32_t bsh,
                                                      uint8_t const *__restrict__ code_to_byte, uint8_t *__restrict__ ref)
{
	__shared__ uint8_t lut[256];
	lut[threadIdx.x] = code_to_byte[threadIdx.x];
	__syncthreads();
	uint32_t const cmask = (1u << (8u >> bsh)) - 1u;
	for (uint64_t k = (uint64_t) blockIdx.x * ID_T + threadIdx.x; k < n; k += (uint64_t) gridDim.x * ID_T)
		ref[k] = lut[msa[k * ld] & cmask];
}

// ---- the restored founders (insert-identity-columns/main.cc:138-195) ----
// out: `lines` lines of n reference bytes + '\n', back to back (total = lines * (n + 1) bytes, the buffer rounded up to 16):
// a lane writes the 16 bytes at a multiple of 16, whatever lines they belong to
static __global__ __launch_bounds__(256) void k_identity_fill(uint8_t const *__restrict__ ref, uint64_t n, uint64_t total, uint8_t *__restrict__ out)
{
	uint64_t const line = n + 1u;
	for (uint64_t o = ((uint64_t) blockIdx.x * ID_T + threadIdx.x) * 16u; o < total; o += (uint64_t) gridDim.x * ID_T * 16u)
	{
		uint64_t p = o % line;
		uint32_t w[4] = {0, 0, 0, 0};
#pragma unroll
		for (uint32_t i = 0; i < 16; ++i)
		{
			uint32_t const b = p == n ? (uint32_t) '\n' : (uint32_t) ref[p];
			w[i >> 2] |= b << (8u * (i & 3u));
			p = p == n ? 0u : p + 1u;
		}
		*reinterpret_cast<uint4 *>(out + o) = make_uint4(w[0], w[1], w[2], w[3]);
	}
}

// k_founders (fseq_joinprep.hpp) on a context over the kept columns: the segment's reduced column k goes to position kept[k]
// of its line (kept ascends, so a wave's stores stay nearly contiguous); the identity positions and the '\n' are k_identity_fill's.
// out: [rows of the batch][n_src + 1] bytes
static __global__ __launch_bounds__(256) void k_founders_restored(
	uint8_t const *__restrict__ msa, size_t ld, uint32_t m, uint64_t n_src, uint32_t bsh, uint32_t const *__restrict__ perm, uint32_t X,
	uint64_t const *__restrict__ seg_lb, uint64_t const *__restrict__ seg_rb, uint32_t row0, uint32_t nrows, uint32_t rows_per_wg,
	uint8_t const *__restrict__ code_to_byte, uint32_t const *__restrict__ kept, uint8_t *__restrict__ out)
{
	__shared__ uint8_t lut[256];
	lut[threadIdx.x] = code_to_byte[threadIdx.x];
	__syncthreads();
	uint32_t const s = blockIdx.x;
	uint64_t const lb = seg_lb[s], rb = seg_rb[s];
	uint32_t const bits = 8u >> bsh, cmask = (1u << bits) - 1u, wv = threadIdx.x >> 6, lane = threadIdx.x & 63u;
	uint32_t const r_lo = blockIdx.y * rows_per_wg, r_hi = min(nrows, r_lo + rows_per_wg);
	for (uint32_t r = r_lo + wv; r < r_hi; r += 4u)
	{
		uint32_t const src = perm[(size_t) s * X + row0 + r];
		uint8_t *const line = out + (size_t) r * (n_src + 1u);
		uint32_t const off = src >> bsh, sh = (src & ((1u << bsh) - 1u)) * bits;
		for (uint64_t k = lb + lane; k < rb; k += 64u)
			line[kept[k]] = src < m ? lut[(msa[k * ld + off] >> sh) & cmask] : (uint8_t) '-';
	}
}

} // namespace fseq
