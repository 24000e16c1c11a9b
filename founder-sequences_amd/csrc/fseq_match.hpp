// fseq_match.hpp -- the input rows matched against founders on the device (include/fseq.h, fseq_match_founders).
//
// replaces: match-sequences-to-founders (match_founder_sequences.cc:108-259): per input row, the loop of
// match_context::match_sequence_and_report (:152-216) with the set of founders that still agree with the row held as a bit
// set instead of an index vector -- one AND per 32 founders and cell instead of one byte compare per live founder.
//
//   k_match_founders_cols / k_match_founder_rows   the K founders as columns of one code per byte: founder f at column k in
//       fcols[k * Kp + f], Kp = K rounded up to 64 (a tile of columns is one contiguous piece of memory).  From the
//       permutations of a finished run and the resident alignment (founder r in segment s is row permutations[s][r]; a slot
//       >= m is the byte '-', as k_founders prints it), or from K raw rows (bytes through the context's alphabet).
//       A founder symbol no row can have is MT_NOCODE.  (One byte per code whatever the alignment's packing: at 2 bits a
//       full alphabet has no code left for "matches nothing", and the walk reads 64 founders of a column as 64 lanes.)
//   k_match_walk<WR, WRITE>   one LANE per input row, the columns in order.  Per tile of columns the workgroup lays out in
//       LDS, for every column and code, the set of founders that carry the code there (64 founders = 64 lanes, one __ballot
//       per code present among them), then every lane walks the tile: live &= set[column][my code], test for zero, on a
//       close restart from set[column][my code].  The tile's founder codes and the workgroup's slice of the tile's alignment
//       columns come in through registers, 16 bytes a lane and load, one tile ahead of the walk.
//       The live set: WR words in registers (WR = 1, 2, 4, 8: up to 256 founders), or -- WR = 0 -- ceil(K / 32) words per lane
//       in LDS, up to MT_MAX_FOUNDERS = 2,048 founders.
//       The walk runs twice: WRITE = false counts the pieces, uncovered cells and short pieces of every row; after
//       k_match_scan's exclusive scan over the rows WRITE = true stores the pieces and their sets where they belong.
//   k_match_walk<WR, WRITE, true>   the restored form (fseq_match_founders_restored): the context holds the kept columns of a
//       longer source (fseq_create_without_identity_columns), and the rows and founders matched are the source-length ones, in
//       which every founder agrees with every row in every identity column.  The walk still visits the kept columns only.  It
//       reads the source position of every column of the tile (idn.kept, 64 words in LDS, staged with the tile), carries lb in
//       source co-ordinates, and runs a gap step before every kept column and once after the last one, for the identity
//       columns [g_lo, g_hi) between two kept columns: an empty live set (the kept cell before was uncovered) closes
//       [lb, g_lo) and starts again from all founders; with min_len != 0 the piece is closed every min_len source columns
//       while lb + min_len < g_hi, the first time with the live set as it is, then with all founders.  The counting pass takes
//       the number of these closes from one division; the writing pass loops over the pieces it stores.  An empty gap costs one
//       uniform compare.  The plain form (RST = false) is a kernel of its own.
//   k_match_walk<WR, WRITE, true, true>   the restored form for QUERY rows (fseq_match_held_out_restored,
//       fseq_match_rows_restored): a row that took no part in the reconstruction may differ from row 0 in an identity column,
//       where every restored founder carries row 0's byte: an EXCEPTION cell, in which no founder agrees with the row.  That is
//       the ordinary column step with the empty set.  Every lane carries a cursor into its row's ascending list of exception
//       columns (csrc/fseq_exceptions.hpp) and, before a kept column k, drains the exceptions below k: the gap step up to the
//       exception, the column step there, then on from the column behind it.  A row without exceptions pays one compare a
//       kept column.
//
//   k_match_pack_rows   rows that are not the alignment's (fseq_match_rows): a staged chunk of raw query bytes, one row after
//       the other, is sent through the context's code table, transposed and packed like the alignment, at the narrowest of
//       2 / 4 / 8 bits that leaves the code `sigma` free for a byte outside the alphabet (the walk sends code >= sigma to the
//       empty set: an uncovered cell).  16-byte loads along the rows, the code table in LDS, 16-byte stores along the columns.
//   k_match_walk_split<WR, WRITE>   the walk split along the columns: workgroup (256 rows, segment g of G) walks
//       [s_g, c_{g+1}) cold from s_g = c_g - overlap and counts / stores only the closes in [c_g, c_{g+1}).  After a close at
//       column k the state is lb = k, live = set[k][code]: a function of k and the row alone (a cold start at s_g is the
//       state of a close at s_g).  Every walk keeps `last`, the column of its latest close; head[g] is `last` on reaching c_g,
//       tail[g] is `last` behind c_{g+1} - 1.  A row STANDS iff head[g] == tail[g - 1] for every g >= 1: then walk g shared a
//       close with walk g - 1 in front of its own range, and by induction from segment 0 (the true walk) every piece stored is
//       the true walk's.  Nothing forces such a close to exist (DESIGN.md section 7 has the periodic counter-example), so
//       k_match_split_check flags every 256-row group with a row that does not stand, and the flagged groups are walked
//       again by the same kernel with one segment (G = 1 of the split kernel IS the unsplit walk) over the list of them; their
//       workgroups in the split writing pass return at once.  The counts are [m x G]; k_match_scan_split gives the offsets
//       per (row, g), so the pieces stay ordered by row, then lb.
//   k_match_walk_split<WR, WRITE, true> / <WR, WRITE, true, true>   the restored forms split the same way, the segments counted
//       in kept columns.  After a close at SOURCE position p the state is lb = p and a live set that is a function of p and the
//       row alone: set[p][code] at a kept column, the empty set at an exception column, all founders at any other identity
//       column (the close in the gap step behind an uncovered cell, every forced min_len close in a gap).  Segment g owns the
//       source positions [kept[c_g], kept[c_{g+1}]) (the first from 0, the last up to n_src), starts cold at kept[s_g] and walks
//       on behind its last kept column up to the next segment's first position; head and tail are source positions, and the
//       check, the fall-back and the scan are the plain form's.
//
// The walk is sequential along the columns: with m rows only ceil(m / 64) waves are in flight, and the time is a chain over n
// columns, not throughput.  fseq_match_founders / fseq_match_founder_rows / fseq_match_founders_restored walk unsplit unless
// FSEQ_MATCH_SPLIT is set; fseq_match_rows, fseq_match_held_out, fseq_match_held_out_restored and fseq_match_rows_restored choose
// the split by themselves (match_split_plan; the restored two over the kept columns).
#pragma once

#include "../../include/fseq.h"

#include <hip/hip_runtime.h>

#include <algorithm>

namespace fseq {

constexpr uint32_t MT_T = 256;                      // threads = rows of a walk workgroup
constexpr uint32_t MT_MAX_FOUNDERS = 2048;          // the LDS variant's live sets: 64 words a lane
constexpr uint32_t MT_TILE_MAX = 64;                // columns of a tile at most
constexpr uint32_t MT_PREFETCH = 4;                 // 16-byte loads per lane and staged array: 16 KB of either a tile
constexpr uint32_t MT_STAGE_BYTES = MT_T * MT_PREFETCH * 16;
constexpr uint32_t MT_SET_BYTES = 64 * 1024;        // the tile's founder sets
constexpr size_t   MT_LDS_BYTES = 152 * 1024;       // what a workgroup may take in all
constexpr uint32_t MT_NOCODE = 0xFF;                // a founder symbol outside the alphabet (sigma < 256; with 256 codes there is none)
constexpr uint32_t MT_SCAN_T = 1024;
constexpr uint32_t MT_NO_EXC = 0xFFFFFFFFu;          // no exception column left (a source has fewer than 2^32 - 1 columns)

__host__ __device__ inline uint64_t mt_min(uint64_t a, uint64_t b) { return a < b ? a : b; }
__host__ __device__ inline uint64_t mt_max(uint64_t a, uint64_t b) { return a > b ? a : b; }

struct MatchShape {
	uint32_t K, Kp, W, WR, Wk, TC;                  // founders, padded to 64, words of a set, register words (0: LDS), words the kernel holds, tile
	size_t lds;
};

inline size_t match_lds_bytes(uint32_t sigma, uint32_t bsh, MatchShape const &s)
{
	return (size_t) s.TC * s.Kp + (size_t) s.TC * (MT_T >> bsh) + ((size_t) s.TC * sigma + 1) * s.Wk * 4 + (s.WR ? 0 : (size_t) s.Wk * MT_T * 4);
}

// the variant and the tile for K founders (K <= MT_MAX_FOUNDERS)
inline MatchShape match_shape(uint32_t K, uint32_t sigma, uint32_t bsh)
{
	MatchShape s{};
	s.K = K; s.Kp = (K + 63u) & ~63u; s.W = (K + 31u) / 32u;
	s.WR = s.W <= 1 ? 1u : s.W <= 2 ? 2u : s.W <= 4 ? 4u : s.W <= 8 ? 8u : 0u;
	s.Wk = s.WR ? s.WR : s.W;
	uint32_t tc = MT_TILE_MAX;
	tc = std::min<uint32_t>(tc, MT_SET_BYTES / (sigma * s.Wk * 4u));
	tc = std::min<uint32_t>(tc, MT_STAGE_BYTES / s.Kp);
	tc = std::min<uint32_t>(tc, MT_STAGE_BYTES / (MT_T >> bsh));
	s.TC = std::max<uint32_t>(tc, 1u);
	while (s.TC > 1 && match_lds_bytes(sigma, bsh, s) > MT_LDS_BYTES) --s.TC;
	s.lds = match_lds_bytes(sigma, bsh, s);
	return s;
}

// ------------------------------------------------------------------------------------------------
// founders as columns, from the permutations of a run.  Workgroup: 64 columns; the segment of every column is found once
// (seg_rb ascending, the segments tile [0, n)), then the lanes run along the founders (coalesced stores; the loads hit the
// column's ld bytes).
// ------------------------------------------------------------------------------------------------
static __global__ __launch_bounds__(256) void k_match_founders_cols(
	uint8_t const *__restrict__ msa, size_t ld, uint32_t m, uint64_t n, uint32_t bsh, uint32_t const *__restrict__ perm, uint32_t X,
	uint64_t const *__restrict__ seg_rb, uint32_t S, uint32_t gap_code, uint32_t Kp, uint8_t *__restrict__ fcols)
{
	__shared__ uint32_t seg_of[64];
	uint64_t const c0 = (uint64_t) blockIdx.x * 64u;
	uint32_t const tc = (uint32_t) mt_min(64u, n - c0);
	if (threadIdx.x < tc)
	{
		uint64_t const k = c0 + threadIdx.x;
		uint32_t lo = 0, hi = S - 1u;                    // first segment whose rb is beyond k
		while (lo < hi) { uint32_t const mid = (lo + hi) / 2u; if (seg_rb[mid] > k) hi = mid; else lo = mid + 1u; }
		seg_of[threadIdx.x] = lo;
	}
	__syncthreads();
	uint32_t const bits = 8u >> bsh, cmask = (1u << bits) - 1u;
	for (uint32_t i = threadIdx.x; i < tc * Kp; i += 256u)
	{
		uint32_t const j = i / Kp, f = i - j * Kp;
		uint64_t const k = c0 + j;
		uint32_t code = MT_NOCODE;
		if (f < X)
		{
			uint32_t const src = perm[(size_t) seg_of[j] * X + f];
			code = src < m ? (msa[k * ld + (src >> bsh)] >> ((src & ((1u << bsh) - 1u)) * bits)) & cmask : gap_code;
		}
		fcols[k * Kp + f] = (uint8_t) code;
	}
}

// ... from K raw rows (raw[f * n + k]): 64 x 64 tiles through LDS, loads along the columns, stores along the founders
static __global__ __launch_bounds__(256) void k_match_founder_rows(
	uint8_t const *__restrict__ raw, uint64_t n, uint32_t K, uint32_t Kp, uint8_t const *__restrict__ code_of, uint8_t *__restrict__ fcols)
{
	__shared__ uint8_t lut[256];
	__shared__ uint8_t tile[64][65];
	lut[threadIdx.x] = code_of[threadIdx.x];
	uint64_t const c0 = (uint64_t) blockIdx.x * 64u;
	uint32_t const x = threadIdx.x & 63u, y = threadIdx.x >> 6;
	for (uint32_t f0 = 0; f0 < Kp; f0 += 64u)
	{
		__syncthreads();
		for (uint32_t fy = y; fy < 64u; fy += 4u)
			tile[fy][x] = (f0 + fy < K && c0 + x < n) ? lut[raw[(size_t) (f0 + fy) * n + c0 + x]] : (uint8_t) MT_NOCODE;
		__syncthreads();
		for (uint32_t cy = y; cy < 64u; cy += 4u)
			if (c0 + cy < n) fcols[(c0 + cy) * Kp + f0 + x] = tile[x][cy];
	}
}

// ------------------------------------------------------------------------------------------------
// the live set of a lane: WR words in registers, or (WR = 0) `words` words in LDS, word i of lane t at p[i * MT_T + t]
// ------------------------------------------------------------------------------------------------
template <uint32_t WR>
struct MatchLive {
	uint32_t w[WR];
	__device__ __forceinline__ MatchLive(uint32_t *, uint32_t) {}
	__device__ __forceinline__ uint32_t words() const { return WR; }
	__device__ __forceinline__ uint32_t get(uint32_t i) const { return w[i]; }
	__device__ __forceinline__ void set(uint32_t i, uint32_t v) { w[i] = v; }
};
template <>
struct MatchLive<0> {
	uint32_t *p;
	uint32_t nw;
	__device__ __forceinline__ MatchLive(uint32_t *p_, uint32_t nw_) : p(p_), nw(nw_) {}
	__device__ __forceinline__ uint32_t words() const { return nw; }
	__device__ __forceinline__ uint32_t get(uint32_t i) const { return p[i * MT_T]; }
	__device__ __forceinline__ void set(uint32_t i, uint32_t v) { p[i * MT_T] = v; }
};

struct MatchWalkArgs {
	uint8_t const *msa; size_t ld; uint32_t m; uint64_t n; uint32_t bsh, sigma;
	uint8_t const *fcols;
	uint32_t K, Kp, W, Wk, TC;
	uint64_t min_len;
	uint32_t *cnt;                                   // WRITE = false: [3][m]
	uint64_t const *off;                             // WRITE = true: first piece of every row
	fseq_match_piece *pieces;
	uint32_t *sets;
	uint32_t const *kept;                            // RST: source position of every column, ascending; n_src source columns
	uint64_t n_src;
	uint64_t const *exc_off;                         // EXC: row r's exception columns are exc_cols[exc_off[r] .. exc_off[r + 1]), source
	uint32_t const *exc_cols;                        //      positions, ascending
};

// LDS: [TC x Kp founder codes][TC x (MT_T >> bsh) bytes of alignment columns][(TC x sigma + 1) sets of Wk words; the last one
// stays empty][WR = 0: Wk x MT_T words of live sets]; RST: the tile's source positions in 64 words of their own
template <uint32_t WR, bool WRITE, bool RST = false, bool EXC = false>
static __global__ __launch_bounds__(MT_T) void k_match_walk(MatchWalkArgs const A)
{
	static_assert(RST || !EXC, "exception columns are identity columns of a restored walk");
	extern __shared__ uint4 mt_smem[];
	__shared__ uint32_t mt_pos[RST ? MT_TILE_MAX : 1];
	uint32_t const tid = threadIdx.x, lane = tid & 63u, wv = tid >> 6;
	uint32_t const bsh = A.bsh, bits = 8u >> bsh, cmask = (1u << bits) - 1u, smask = (1u << bsh) - 1u;
	uint32_t const rowbytes = MT_T >> bsh, cpc = rowbytes / 16u;         // this workgroup's rows in a column: bytes, 16-byte chunks
	uint32_t const Kp = A.Kp, K = A.K, Wk = A.Wk, TC = A.TC, sigma = A.sigma, groups = Kp / 64u;
	uint8_t *const fst = reinterpret_cast<uint8_t *>(mt_smem);
	uint8_t *const syms = fst + (size_t) TC * Kp;
	uint32_t *const sets = reinterpret_cast<uint32_t *>(syms + (size_t) TC * rowbytes);
	uint32_t *const empty_set = sets + (size_t) TC * sigma * Wk;
	uint32_t *const live_lds = empty_set + Wk + tid;
	size_t const slice = (size_t) blockIdx.x * rowbytes;                 // where the workgroup's rows start in a column
	uint32_t const row = blockIdx.x * MT_T + tid;
	bool const active = row < A.m;
	uint64_t const n = A.n, min_len = A.min_len;

	for (uint32_t i = tid; i < Wk; i += MT_T) empty_set[i] = 0u;

	MatchLive<WR> live(live_lds, Wk);
	auto all_founders = [&]() {
		for (uint32_t i = 0; i < live.words(); ++i)
			live.set(i, K >= 32u * (i + 1u) ? ~0u : (K > 32u * i ? (1u << (K - 32u * i)) - 1u : 0u));
	};
	all_founders();
	uint64_t lb = 0;
	uint32_t npieces = 0, nunc = 0, nshort = 0;
	bool alive = true;
	uint64_t src_next = 0;                                               // RST: the source column behind the last column walked
	uint64_t const out0 = (WRITE && active) ? A.off[row] : 0;
	// EXC: the cursor into the row's exception columns and the one it stands at (none left: beyond every source column)
	uint64_t e_at = (EXC && active) ? A.exc_off[row] : 0;
	uint64_t const e_end = (EXC && active) ? A.exc_off[row + 1u] : 0;
	uint32_t e_col = (EXC && e_at < e_end) ? A.exc_cols[e_at] : MT_NO_EXC;

	auto emit = [&](uint64_t rb) {
		if (WRITE)
		{
			uint64_t const at = out0 + npieces;
			uint32_t pc = 0;
			for (uint32_t i = 0; i < live.words(); ++i)
			{
				uint32_t const v = live.get(i);
				pc += __popc(v);
				if (i < A.W) A.sets[at * A.W + i] = v;
			}
			fseq_match_piece *const p = A.pieces + at;
			p->lb = lb; p->rb = rb; p->row = row; p->n_founders = pc;
		}
		++npieces;
	};

	// RST: the identity columns [g_lo, g_hi) in front of a kept column, or behind the last one.  Every founder agrees with the
	// row there, so match_founder_sequences.cc:166-208 over these columns comes to: an empty set closes at g_lo (the tool's
	// "under the given limit" line where it prints one: the cell before was uncovered, so no founder is left at g_lo either),
	// and a piece of min_len columns closes wherever it is reached before g_hi
	auto gap_step = [&](uint64_t g_lo, uint64_t g_hi) {
		if (g_lo >= g_hi) return;
		if (!alive)
		{
			if (min_len != 0 && g_lo - lb < min_len) ++nshort;
			emit(g_lo);
			lb = g_lo;
			all_founders();
			alive = true;
		}
		if (min_len != 0)
		{
			// closes at lb + i * min_len < g_hi, i = 1 ..: (g_hi - lb - 1) / min_len of them (lb < g_hi < 2^32)
			uint32_t const room = (uint32_t) (g_hi - lb - 1u);
			uint32_t const closes = min_len > room ? 0u : room / (uint32_t) min_len;
			if (closes)
			{
				if (WRITE)
				{
					emit(lb + min_len);
					lb += min_len;
					all_founders();
					for (uint32_t i = 1; i < closes; ++i) { emit(lb + min_len); lb += min_len; }
				}
				else
				{
					npieces += closes;
					lb += (uint64_t) closes * min_len;
					all_founders();
				}
			}
		}
	};

	// the step of one column, match_founder_sequences.cc:166-208: k its position, M the founders that carry the row's symbol
	// there.  The AND is made once: kept in registers where the set is (WR words), and for the sets in LDS written over the
	// live set only when the piece goes on (a close prints the set as it was)
	auto col_step = [&](uint64_t k, uint32_t const *const M) {
		bool recheck = false;
		uint32_t any = 0;
		uint32_t nv[WR ? WR : 1];
		if (min_len != 0 && min_len <= k - lb) recheck = true;
		else
		{
			if (WR)
			{
				for (uint32_t i = 0; i < live.words(); ++i) { nv[i] = live.get(i) & M[i]; any |= nv[i]; }
			}
			else
			{
				// (only whether a founder is left: stops at the first word that keeps one)
				for (uint32_t i = 0; i < live.words() && !any; ++i) any = live.get(i) & M[i];
			}
			if (!any) { if (min_len != 0) ++nshort; recheck = true; }
		}
		if (recheck)
		{
			emit(k);
			lb = k;
			any = 0;
			for (uint32_t i = 0; i < live.words(); ++i) { uint32_t const v = M[i]; live.set(i, v); any |= v; }
			if (!any) ++nunc;
		}
		else if (WR)
		{
			for (uint32_t i = 0; i < live.words(); ++i) live.set(i, nv[i]);
		}
		else
		{
			for (uint32_t i = 0; i < live.words(); ++i) live.set(i, live.get(i) & M[i]);
		}
		alive = any != 0;
	};
	// EXC: the row's exception columns below `upto`: each is the column step with no founder, between the gaps around it
	auto drain = [&](uint64_t upto) {
		while (e_col < upto)
		{
			gap_step(src_next, e_col);
			col_step(e_col, empty_set);
			src_next = (uint64_t) e_col + 1u;
			++e_at;
			e_col = e_at < e_end ? A.exc_cols[e_at] : MT_NO_EXC;
		}
	};

	uint4 rf[MT_PREFETCH], rs[MT_PREFETCH];
	uint32_t rp = 0;
	auto prefetch = [&](uint64_t c0, uint32_t tc) {
		if (RST) rp = tid < tc ? A.kept[c0 + tid] : 0u;
		uint32_t const nf = tc * Kp / 16u, ns = tc * cpc;
		uint4 const *const fsrc = reinterpret_cast<uint4 const *>(A.fcols + c0 * Kp);
#pragma unroll
		for (uint32_t j = 0; j < MT_PREFETCH; ++j)
		{
			uint32_t const q = tid + j * MT_T;
			rf[j] = q < nf ? fsrc[q] : make_uint4(0, 0, 0, 0);
			uint32_t const col = q / cpc, ch = q - col * cpc;
			size_t const at = slice + (size_t) ch * 16u;                 // (ld is a multiple of 16: a chunk is inside the column or beyond it)
			rs[j] = (q < ns && at < A.ld) ? *reinterpret_cast<uint4 const *>(A.msa + (c0 + col) * A.ld + at) : make_uint4(0, 0, 0, 0);
		}
	};

	prefetch(0, (uint32_t) mt_min(TC, n));
	for (uint64_t c0 = 0; c0 < n; c0 += TC)
	{
		uint32_t const tc = (uint32_t) mt_min(TC, n - c0);
		// the tile's codes into LDS, its sets cleared
		{
			uint32_t const nf = tc * Kp / 16u, ns = tc * cpc;
#pragma unroll
			for (uint32_t j = 0; j < MT_PREFETCH; ++j)
			{
				uint32_t const q = tid + j * MT_T;
				if (q < nf) reinterpret_cast<uint4 *>(fst)[q] = rf[j];
				if (q < ns) reinterpret_cast<uint4 *>(syms)[q] = rs[j];
			}
			if (RST && tid < MT_TILE_MAX) mt_pos[tid] = rp;
			for (uint32_t i = tid; i < tc * sigma * Wk; i += MT_T) sets[i] = 0u;
		}
		__syncthreads();
		if (c0 + TC < n) prefetch(c0 + TC, (uint32_t) mt_min(TC, n - c0 - TC));
		// set[column][code]: 64 founders of a column are the lanes of a wave; one ballot per code present among them
		for (uint32_t it = wv; it < tc * groups; it += MT_T / 64u)
		{
			uint32_t const j = it / groups, g = it - j * groups, f = g * 64u + lane;
			uint32_t const code = fst[j * Kp + f];
			bool const todo = f < K && code < sigma;
			unsigned long long rem = __ballot(todo);
			while (rem)
			{
				uint32_t const s = (uint32_t) __shfl((int) code, (int) (__ffsll((long long) rem) - 1));
				unsigned long long const b = __ballot(todo && code == s);
				rem &= ~b;
				uint32_t *const dst = sets + ((size_t) j * sigma + s) * Wk;
				if (lane == 0 && 2u * g < Wk) dst[2u * g] = (uint32_t) b;
				if (lane == 1 && 2u * g + 1u < Wk) dst[2u * g + 1u] = (uint32_t) (b >> 32);
			}
		}
		__syncthreads();
		if (active)
			for (uint32_t j = 0; j < tc; ++j)
			{
				uint64_t const k = RST ? (uint64_t) mt_pos[j] : c0 + j;
				if (EXC) drain(k);
				if (RST) { gap_step(src_next, k); src_next = k + 1u; }
				uint32_t const code = (syms[j * rowbytes + (tid >> bsh)] >> ((tid & smask) * bits)) & cmask;
				col_step(k, code < sigma ? sets + ((size_t) j * sigma + code) * Wk : empty_set);
			}
		__syncthreads();
	}
	if (active)
	{
		if (EXC) drain(A.n_src);
		if (RST) gap_step(src_next, A.n_src);
		if (alive) emit(RST ? A.n_src : n);
		if (!WRITE) { A.cnt[row] = npieces; A.cnt[A.m + row] = nunc; A.cnt[2u * (size_t) A.m + row] = nshort; }
	}
}

// ------------------------------------------------------------------------------------------------
// exclusive scan of the rows' piece counts (off[0 .. m], off[m] = all pieces) and the summary's totals:
// tot = {pieces, uncovered cells, short pieces, most pieces in a row}.  One workgroup; a thread sums a run of rows.
// ------------------------------------------------------------------------------------------------
static __global__ __launch_bounds__(MT_SCAN_T) void k_match_scan(uint32_t const *__restrict__ cnt, uint32_t m, uint64_t *__restrict__ off, uint64_t *__restrict__ tot)
{
	__shared__ uint64_t s_p[MT_SCAN_T], s_u[MT_SCAN_T], s_s[MT_SCAN_T], s_x[MT_SCAN_T];
	uint32_t const t = threadIdx.x, per = (m + MT_SCAN_T - 1u) / MT_SCAN_T;
	uint32_t const lo = min(m, t * per), hi = min(m, lo + per);
	uint64_t p = 0, u = 0, s = 0, x = 0;
	for (uint32_t r = lo; r < hi; ++r)
	{
		uint32_t const v = cnt[r];
		p += v; u += cnt[m + r]; s += cnt[2u * (size_t) m + r];
		x = mt_max(x, v);
	}
	s_p[t] = p; s_u[t] = u; s_s[t] = s; s_x[t] = x;
	__syncthreads();
	if (t == 0)
	{
		uint64_t run = 0, su = 0, ss = 0, mx = 0;
		for (uint32_t i = 0; i < MT_SCAN_T; ++i)
		{
			uint64_t const v = s_p[i];
			s_p[i] = run; run += v;
			su += s_u[i]; ss += s_s[i]; mx = mt_max(mx, s_x[i]);
		}
		off[m] = run;
		tot[0] = run; tot[1] = su; tot[2] = ss; tot[3] = mx;
	}
	__syncthreads();
	uint64_t run = s_p[t];
	for (uint32_t r = lo; r < hi; ++r) { off[r] = run; run += cnt[r]; }
}

// ------------------------------------------------------------------------------------------------
// The split of the columns.  G segments with the bounds c_g = floor(g n / G) (G <= n: none is empty); the cold start of
// segment g >= 1 is s_g = c_g - clamp(overlap, 1, c_g - c_{g-1}), s_0 = 0.
// ------------------------------------------------------------------------------------------------
constexpr uint32_t MT_SPLIT_MAX = 4096;             // most segments (FSEQ_MATCH_SPLIT)
// fseq_match_rows by itself: about MT_SPLIT_WG_PER_CU workgroups a CU, segments of at least MT_SPLIT_MIN_OVERLAPS overlaps of
// MT_SPLIT_OVERLAP columns.  From one measurement (profiles/match_split_C3_overlap4096.txt): rows of C3's population held out of the
// reconstruction stand at an overlap of 16,384 columns and none does at 4,096, the value this started from; a segment of one
// overlap (G = 61 on C3's 1,000,000 columns) was the fastest shape measured.  No other input has been measured.
// The restored query entries plan with the same constants over the KEPT columns (profiles/match_restored_split_C3.txt: C3 with
// 400,293 kept columns, held-out rows stand at 16,384 kept columns and 18 of 256 do not at 4,096).
constexpr uint32_t MT_SPLIT_WG_PER_CU = 2;
constexpr uint64_t MT_SPLIT_OVERLAP = 16384;
constexpr uint64_t MT_SPLIT_MIN_OVERLAPS = 1;

__host__ __device__ inline uint64_t mt_seg_bound(uint64_t n, uint32_t G, uint32_t g) { return (uint64_t) g * n / G; }
__host__ __device__ inline uint64_t mt_seg_start(uint64_t n, uint32_t G, uint32_t g, uint64_t overlap)
{
	if (0 == g) return 0;
	uint64_t const c = mt_seg_bound(n, G, g);
	return c - mt_max(1u, mt_min(overlap, c - mt_seg_bound(n, G, g - 1u)));
}

struct MatchSplitPlan { uint32_t G; uint64_t overlap; };

// forced_g / forced_overlap: the knobs (0: not set).  by_itself: fseq_match_rows' own choice where forced_g is 0
inline MatchSplitPlan match_split_plan(uint64_t n, uint32_t rows, uint32_t cus, uint32_t forced_g, uint64_t forced_overlap, bool by_itself)
{
	MatchSplitPlan p{1u, forced_overlap ? forced_overlap : MT_SPLIT_OVERLAP};
	if (forced_g) p.G = forced_g;
	else if (by_itself)
	{
		uint64_t const groups = ((uint64_t) rows + MT_T - 1u) / MT_T;
		uint64_t const want = std::max<uint64_t>(1u, (uint64_t) MT_SPLIT_WG_PER_CU * std::max(cus, 1u) / groups);
		p.G = (uint32_t) std::max<uint64_t>(1u, std::min<uint64_t>(want, n / (MT_SPLIT_MIN_OVERLAPS * p.overlap)));
	}
	p.G = (uint32_t) std::max<uint64_t>(1u, std::min<uint64_t>(std::min<uint32_t>(p.G, MT_SPLIT_MAX), n));
	uint64_t const longest = (n + p.G - 1u) / p.G;
	p.overlap = p.G > 1u ? mt_max(1u, mt_min(p.overlap, longest)) : 0u;
	return p;
}

struct MatchSplitArgs {
	MatchWalkArgs w;                                 // cnt: [3][m x GS]; off: [m x GS]
	uint32_t G, GS;                                  // segments this launch walks; segments of the count arrays (the fall-back: G = 1 into slot 0 of GS)
	uint64_t overlap;
	uint32_t *head, *tail;                           // WRITE = false: [m x GS]
	uint32_t const *flag;                            // the split launch, WRITE = true: groups that fell back return at once (or nullptr)
	uint32_t const *list, *nlist;                    // the fall-back launch: the flagged groups and their number (or nullptr)
};

// LDS as k_match_walk's.  grid: (row groups, G), or -- A.list -- (row groups) of which the first *A.nlist work.
// RST / EXC: the restored forms, as k_match_walk has them.  The segments are counted in KEPT columns (n = n_kept); segment g owns
// the source positions [P_g, P_{g+1}), P_0 = 0, P_g = kept[c_g], P_G = n_src, and a close at source position p is counted and
// stored by the segment that owns p.  Segment g >= 1 starts cold at kept[s_g] (the exception cursor at the row's first exception
// not below it, by binary search); behind its last kept column it drains and gap-steps up to P_{g+1}.  `mine` turns true on
// reaching kept index c_g, after the drain and the gap step in front of it: a gap lies strictly between two kept or exception
// columns, so it never straddles a P_g and the counting pass keeps its closed form.  head and tail are source positions.
template <uint32_t WR, bool WRITE, bool RST = false, bool EXC = false>
static __global__ __launch_bounds__(MT_T) void k_match_walk_split(MatchSplitArgs const S)
{
	static_assert(RST || !EXC, "exception columns are identity columns of a restored walk");
	extern __shared__ uint4 mt_smem[];
	__shared__ uint32_t mt_pos[RST ? MT_TILE_MAX : 1];
	MatchWalkArgs const &A = S.w;
	uint32_t grp = blockIdx.x;
	uint32_t const g = S.list ? 0u : blockIdx.y;
	if (S.list)
	{
		if (blockIdx.x >= *S.nlist) return;
		grp = S.list[blockIdx.x];
	}
	else if (S.flag && S.flag[grp]) return;
	uint32_t const tid = threadIdx.x, lane = tid & 63u, wv = tid >> 6;
	uint32_t const bsh = A.bsh, bits = 8u >> bsh, cmask = (1u << bits) - 1u, smask = (1u << bsh) - 1u;
	uint32_t const rowbytes = MT_T >> bsh, cpc = rowbytes / 16u;
	uint32_t const Kp = A.Kp, K = A.K, Wk = A.Wk, TC = A.TC, sigma = A.sigma, groups = Kp / 64u;
	uint8_t *const fst = reinterpret_cast<uint8_t *>(mt_smem);
	uint8_t *const syms = fst + (size_t) TC * Kp;
	uint32_t *const sets = reinterpret_cast<uint32_t *>(syms + (size_t) TC * rowbytes);
	uint32_t *const empty_set = sets + (size_t) TC * sigma * Wk;
	uint32_t *const live_lds = empty_set + Wk + tid;
	size_t const slice = (size_t) grp * rowbytes;
	uint32_t const row = grp * MT_T + tid;
	bool const active = row < A.m;
	uint64_t const n = A.n, min_len = A.min_len;
	uint64_t const c_lo = mt_seg_bound(n, S.G, g), c_hi = mt_seg_bound(n, S.G, g + 1u), s_lo = mt_seg_start(n, S.G, g, S.overlap);
	size_t const slot = (size_t) row * S.GS + g, total = (size_t) A.m * S.GS;

	for (uint32_t i = tid; i < Wk; i += MT_T) empty_set[i] = 0u;

	MatchLive<WR> live(live_lds, Wk);
	auto all_founders = [&]() {
		for (uint32_t i = 0; i < live.words(); ++i)
			live.set(i, K >= 32u * (i + 1u) ? ~0u : (K > 32u * i ? (1u << (K - 32u * i)) - 1u : 0u));
	};
	all_founders();
	uint64_t lb = s_lo;
	uint32_t last = (uint32_t) s_lo, head = (uint32_t) s_lo;
	uint32_t npieces = 0, nunc = 0, nshort = 0;
	bool alive = true;
	uint64_t const out0 = (WRITE && active) ? A.off[slot] : 0;

	auto emit = [&](uint64_t rb) {
		if (WRITE)
		{
			uint64_t const at = out0 + npieces;
			uint32_t pc = 0;
			for (uint32_t i = 0; i < live.words(); ++i)
			{
				uint32_t const v = live.get(i);
				pc += __popc(v);
				if (i < A.W) A.sets[at * A.W + i] = v;
			}
			fseq_match_piece *const p = A.pieces + at;
			p->lb = lb; p->rb = rb; p->row = row; p->n_founders = pc;
		}
		++npieces;
	};

	// RST: the state and the steps of k_match_walk's restored form, with the owner rule: every close sets `last`, and it is
	// counted and stored only where `mine`
	bool mine = s_lo == c_lo;                                            // (segment 0, and the fall-back's one segment)
	uint64_t src_next = 0, p_hi = 0;
	uint64_t e_at = 0, e_end = 0;
	uint32_t e_col = MT_NO_EXC;
	if (RST)
	{
		if (g) { lb = A.kept[s_lo]; last = head = (uint32_t) lb; }
		src_next = lb;
		p_hi = c_hi == n ? A.n_src : (uint64_t) A.kept[c_hi];
		if (EXC && active)
		{
			e_at = A.exc_off[row];
			e_end = A.exc_off[row + 1u];
			if (g)
			{
				// the row's first exception at or behind the cold start (none is at a kept column)
				uint64_t hi = e_end;
				while (e_at < hi) { uint64_t const mid = e_at + (hi - e_at) / 2u; if (A.exc_cols[mid] < (uint32_t) lb) e_at = mid + 1u; else hi = mid; }
			}
			if (e_at < e_end) e_col = A.exc_cols[e_at];
		}
	}
	auto gap_step = [&](uint64_t g_lo, uint64_t g_hi) {
		if (g_lo >= g_hi) return;
		if (!alive)
		{
			if (mine)
			{
				if (min_len != 0 && g_lo - lb < min_len) ++nshort;
				emit(g_lo);
			}
			lb = g_lo;
			last = (uint32_t) g_lo;
			all_founders();
			alive = true;
		}
		if (min_len != 0)
		{
			// closes at lb + i * min_len < g_hi, i = 1 ..: (g_hi - lb - 1) / min_len of them (lb < g_hi < 2^32)
			uint32_t const room = (uint32_t) (g_hi - lb - 1u);
			uint32_t const closes = min_len > room ? 0u : room / (uint32_t) min_len;
			if (closes)
			{
				if (WRITE && mine)
				{
					emit(lb + min_len);
					lb += min_len;
					all_founders();
					for (uint32_t i = 1; i < closes; ++i) { emit(lb + min_len); lb += min_len; }
				}
				else
				{
					if (mine) npieces += closes;
					lb += (uint64_t) closes * min_len;
					all_founders();
				}
				last = (uint32_t) lb;
			}
		}
	};
	auto col_step = [&](uint64_t k, uint32_t const *const M) {
		bool recheck = false;
		uint32_t any = 0;
		uint32_t nv[WR ? WR : 1];
		if (min_len != 0 && min_len <= k - lb) recheck = true;
		else
		{
			if (WR)
			{
				for (uint32_t i = 0; i < live.words(); ++i) { nv[i] = live.get(i) & M[i]; any |= nv[i]; }
			}
			else
			{
				for (uint32_t i = 0; i < live.words() && !any; ++i) any = live.get(i) & M[i];
			}
			if (!any) { if (min_len != 0 && mine) ++nshort; recheck = true; }
		}
		if (recheck)
		{
			if (mine) emit(k);
			lb = k;
			last = (uint32_t) k;
			any = 0;
			for (uint32_t i = 0; i < live.words(); ++i) { uint32_t const v = M[i]; live.set(i, v); any |= v; }
			if (!any && mine) ++nunc;
		}
		else if (WR)
		{
			for (uint32_t i = 0; i < live.words(); ++i) live.set(i, nv[i]);
		}
		else
		{
			for (uint32_t i = 0; i < live.words(); ++i) live.set(i, live.get(i) & M[i]);
		}
		alive = any != 0;
	};
	auto drain = [&](uint64_t upto) {
		while (e_col < upto)
		{
			gap_step(src_next, e_col);
			col_step(e_col, empty_set);
			src_next = (uint64_t) e_col + 1u;
			++e_at;
			e_col = e_at < e_end ? A.exc_cols[e_at] : MT_NO_EXC;
		}
	};

	uint4 rf[MT_PREFETCH], rs[MT_PREFETCH];
	uint32_t rp = 0;
	auto prefetch = [&](uint64_t c0, uint32_t tc) {
		if (RST) rp = tid < tc ? A.kept[c0 + tid] : 0u;
		uint32_t const nf = tc * Kp / 16u, ns = tc * cpc;
		uint4 const *const fsrc = reinterpret_cast<uint4 const *>(A.fcols + c0 * Kp);
#pragma unroll
		for (uint32_t j = 0; j < MT_PREFETCH; ++j)
		{
			uint32_t const q = tid + j * MT_T;
			rf[j] = q < nf ? fsrc[q] : make_uint4(0, 0, 0, 0);
			uint32_t const col = q / cpc, ch = q - col * cpc;
			size_t const at = slice + (size_t) ch * 16u;
			rs[j] = (q < ns && at < A.ld) ? *reinterpret_cast<uint4 const *>(A.msa + (c0 + col) * A.ld + at) : make_uint4(0, 0, 0, 0);
		}
	};

	prefetch(s_lo, (uint32_t) mt_min(TC, c_hi - s_lo));
	for (uint64_t c0 = s_lo; c0 < c_hi; c0 += TC)
	{
		uint32_t const tc = (uint32_t) mt_min(TC, c_hi - c0);
		{
			uint32_t const nf = tc * Kp / 16u, ns = tc * cpc;
#pragma unroll
			for (uint32_t j = 0; j < MT_PREFETCH; ++j)
			{
				uint32_t const q = tid + j * MT_T;
				if (q < nf) reinterpret_cast<uint4 *>(fst)[q] = rf[j];
				if (q < ns) reinterpret_cast<uint4 *>(syms)[q] = rs[j];
			}
			if (RST && tid < MT_TILE_MAX) mt_pos[tid] = rp;
			for (uint32_t i = tid; i < tc * sigma * Wk; i += MT_T) sets[i] = 0u;
		}
		__syncthreads();
		if (c0 + TC < c_hi) prefetch(c0 + TC, (uint32_t) mt_min(TC, c_hi - c0 - TC));
		for (uint32_t it = wv; it < tc * groups; it += MT_T / 64u)
		{
			uint32_t const j = it / groups, fg = it - j * groups, f = fg * 64u + lane;
			uint32_t const code = fst[j * Kp + f];
			bool const todo = f < K && code < sigma;
			unsigned long long rem = __ballot(todo);
			while (rem)
			{
				uint32_t const s = (uint32_t) __shfl((int) code, (int) (__ffsll((long long) rem) - 1));
				unsigned long long const b = __ballot(todo && code == s);
				rem &= ~b;
				uint32_t *const dst = sets + ((size_t) j * sigma + s) * Wk;
				if (lane == 0 && 2u * fg < Wk) dst[2u * fg] = (uint32_t) b;
				if (lane == 1 && 2u * fg + 1u < Wk) dst[2u * fg + 1u] = (uint32_t) (b >> 32);
			}
		}
		__syncthreads();
		if (RST)
		{
			if (active)
				for (uint32_t j = 0; j < tc; ++j)
				{
					uint64_t const k = mt_pos[j];
					if (EXC) drain(k);
					gap_step(src_next, k);
					src_next = k + 1u;
					if (c0 + j == c_lo) { head = last; mine = true; }        // (uniform: what closed in front of P_g belongs to the segment before)
					uint32_t const code = (syms[j * rowbytes + (tid >> bsh)] >> ((tid & smask) * bits)) & cmask;
					col_step(k, code < sigma ? sets + ((size_t) j * sigma + code) * Wk : empty_set);
				}
		}
		else if (active)
			for (uint32_t j = 0; j < tc; ++j)
			{
				uint64_t const k = c0 + j;
				mine = k >= c_lo;                                            // (uniform: the closes in front of c_g belong to the segment before)
				if (k == c_lo) head = last;
				uint32_t const code = (syms[j * rowbytes + (tid >> bsh)] >> ((tid & smask) * bits)) & cmask;
				uint32_t const *const M = code < sigma ? sets + ((size_t) j * sigma + code) * Wk : empty_set;
				bool recheck = false;
				uint32_t any = 0;
				uint32_t nv[WR ? WR : 1];
				if (min_len != 0 && min_len <= k - lb) recheck = true;
				else
				{
					if (WR)
					{
						for (uint32_t i = 0; i < live.words(); ++i) { nv[i] = live.get(i) & M[i]; any |= nv[i]; }
					}
					else
					{
						for (uint32_t i = 0; i < live.words() && !any; ++i) any = live.get(i) & M[i];
					}
					if (!any) { if (min_len != 0 && mine) ++nshort; recheck = true; }
				}
				if (recheck)
				{
					if (mine) emit(k);
					lb = k;
					last = (uint32_t) k;
					any = 0;
					for (uint32_t i = 0; i < live.words(); ++i) { uint32_t const v = M[i]; live.set(i, v); any |= v; }
					if (!any && mine) ++nunc;
				}
				else if (WR)
				{
					for (uint32_t i = 0; i < live.words(); ++i) live.set(i, nv[i]);
				}
				else
				{
					for (uint32_t i = 0; i < live.words(); ++i) live.set(i, live.get(i) & M[i]);
				}
				alive = any != 0;
			}
		__syncthreads();
	}
	if (active)
	{
		if (RST)
		{
			// the exceptions and the identity columns up to the next segment's first position (the last segment: the source's end)
			if (EXC) drain(p_hi);
			gap_step(src_next, p_hi);
		}
		if (c_hi == n && alive) emit(RST ? A.n_src : n);
		if (!WRITE)
		{
			A.cnt[slot] = npieces; A.cnt[total + slot] = nunc; A.cnt[2u * total + slot] = nshort;
			S.head[slot] = head; S.tail[slot] = last;
		}
	}
}

// ------------------------------------------------------------------------------------------------
// The check of a split counting walk.  Workgroup: one group of 256 rows.  A row stands iff head[g] == tail[g - 1] for every
// g >= 1.  A group with a row that does not stand is flagged and joins the list (in no particular order), and its counts are
// cleared but for slot 0 of every row, which the fall-back walk writes.  info = {flagged groups, rows that do not stand};
// both zero before the launch.
// ------------------------------------------------------------------------------------------------
static __global__ __launch_bounds__(MT_T) void k_match_split_check(
	uint32_t const *__restrict__ head, uint32_t const *__restrict__ tail, uint32_t m, uint32_t G, uint32_t *__restrict__ cnt,
	uint32_t *__restrict__ flag, uint32_t *__restrict__ list, uint32_t *__restrict__ info)
{
	__shared__ uint32_t s_bad;
	uint32_t const grp = blockIdx.x, row = grp * MT_T + threadIdx.x;
	if (0 == threadIdx.x) s_bad = 0u;
	__syncthreads();
	bool bad = false;
	if (row < m)
		for (uint32_t g = 1; g < G && !bad; ++g) bad = head[(size_t) row * G + g] != tail[(size_t) row * G + g - 1u];
	if (bad) atomicAdd(&s_bad, 1u);
	__syncthreads();
	uint32_t const nbad = s_bad;
	if (0 == threadIdx.x)
	{
		flag[grp] = nbad ? 1u : 0u;
		if (nbad) { list[atomicAdd(&info[0], 1u)] = grp; atomicAdd(&info[1], nbad); }
	}
	if (!nbad) return;
	size_t const total = (size_t) m * G, lo = (size_t) grp * MT_T * G, hi = mt_min(total, lo + (size_t) MT_T * G);
	for (size_t i = lo + threadIdx.x; i < hi; i += MT_T)
		if (i % G) { cnt[i] = 0u; cnt[total + i] = 0u; cnt[2u * total + i] = 0u; }
}

// ------------------------------------------------------------------------------------------------
// k_match_scan for counts per (row, g), cnt[3][m x G]: off[0 .. m G] (off[m G] = all pieces) and the same four totals, the
// most pieces of a ROW among them.  One workgroup; a thread sums a run of whole rows.
// ------------------------------------------------------------------------------------------------
static __global__ __launch_bounds__(MT_SCAN_T) void k_match_scan_split(uint32_t const *__restrict__ cnt, uint32_t m, uint32_t G, uint64_t *__restrict__ off, uint64_t *__restrict__ tot)
{
	__shared__ uint64_t s_p[MT_SCAN_T], s_u[MT_SCAN_T], s_s[MT_SCAN_T], s_x[MT_SCAN_T];
	uint32_t const t = threadIdx.x, per = (m + MT_SCAN_T - 1u) / MT_SCAN_T;
	uint32_t const lo = min(m, t * per), hi = min(m, lo + per);
	size_t const total = (size_t) m * G;
	uint64_t p = 0, u = 0, s = 0, x = 0;
	for (uint32_t r = lo; r < hi; ++r)
	{
		uint64_t mine = 0;
		for (size_t i = (size_t) r * G; i < (size_t) (r + 1u) * G; ++i) { mine += cnt[i]; u += cnt[total + i]; s += cnt[2u * total + i]; }
		p += mine;
		x = mt_max(x, mine);
	}
	s_p[t] = p; s_u[t] = u; s_s[t] = s; s_x[t] = x;
	__syncthreads();
	if (t == 0)
	{
		uint64_t run = 0, su = 0, ss = 0, mx = 0;
		for (uint32_t i = 0; i < MT_SCAN_T; ++i)
		{
			uint64_t const v = s_p[i];
			s_p[i] = run; run += v;
			su += s_u[i]; ss += s_s[i]; mx = mt_max(mx, s_x[i]);
		}
		off[total] = run;
		tot[0] = run; tot[1] = su; tot[2] = ss; tot[3] = mx;
	}
	__syncthreads();
	uint64_t run = s_p[t];
	for (size_t i = (size_t) lo * G; i < (size_t) hi * G; ++i) { off[i] = run; run += cnt[i]; }
}

// ------------------------------------------------------------------------------------------------
// Query rows onto the device (fseq_match_rows).  raw: a staged chunk, row q's bytes of the columns [c0, c0 + cw) at
// raw[q * stride .. ] (stride a multiple of 16, the base 16-byte aligned).  Workgroup: 64 columns x 256 rows.  Every byte goes
// through lut (its code, or `sigma` for a byte outside the alphabet) into an LDS tile [column][row]; then a lane packs 16 output
// bytes of one column (16 << bsh rows) and stores them.  Rows beyond n_rows are code 0: the padding fields and the bytes up to
// ld are zeros (ld a multiple of 16 and at most the row groups' bytes: every byte of a column is written).
// ------------------------------------------------------------------------------------------------
constexpr uint32_t MT_PACK_COLS = 64;
constexpr uint32_t MT_PACK_LD = MT_T + 16;          // bytes of a column of the tile (16-byte aligned rows of it)

static __global__ __launch_bounds__(MT_T) void k_match_pack_rows(
	uint8_t const *__restrict__ raw, size_t stride, uint32_t n_rows, uint64_t c0, uint32_t cw, uint8_t const *__restrict__ code_of, uint32_t bsh,
	uint8_t *__restrict__ out, size_t ld)
{
	__shared__ uint8_t lut[256];
	__shared__ __attribute__((aligned(16))) uint8_t tile[MT_PACK_COLS][MT_PACK_LD];
	uint32_t const tid = threadIdx.x;
	lut[tid] = code_of[tid];
	__syncthreads();
	uint32_t const j0 = blockIdx.x * MT_PACK_COLS, r0 = blockIdx.y * MT_T;
	for (uint32_t i = tid; i < MT_T * (MT_PACK_COLS / 16u); i += MT_T)
	{
		uint32_t const r = i / (MT_PACK_COLS / 16u), part = i % (MT_PACK_COLS / 16u), j = j0 + part * 16u;
		uint4 v = make_uint4(0, 0, 0, 0);
		bool const in = r0 + r < n_rows && j < stride;
		if (in) v = *reinterpret_cast<uint4 const *>(raw + (size_t) (r0 + r) * stride + j);
		uint32_t const w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
		for (uint32_t b = 0; b < 16u; ++b)
			tile[part * 16u + b][r] = in ? lut[(w[b / 4u] >> (8u * (b % 4u))) & 0xFFu] : (uint8_t) 0;
	}
	__syncthreads();
	uint32_t const bits = 8u >> bsh, per = 1u << bsh, rowbytes = MT_T >> bsh, cpc = rowbytes / 16u;
	for (uint32_t i = tid; i < MT_PACK_COLS * cpc; i += MT_T)
	{
		uint32_t const col = i / cpc, ch = i - col * cpc;
		size_t const at = (size_t) blockIdx.y * rowbytes + (size_t) ch * 16u;
		if (j0 + col >= cw || at >= ld) continue;
		uint8_t const *const src = &tile[col][ch * 16u * per];
		uint32_t w[4] = {0u, 0u, 0u, 0u};
#pragma unroll
		for (uint32_t b = 0; b < 16u; ++b)
		{
			uint32_t byte = 0;
			for (uint32_t e = 0; e < per; ++e) byte |= (uint32_t) src[b * per + e] << (e * bits);
			w[b / 4u] |= byte << (8u * (b % 4u));
		}
		*reinterpret_cast<uint4 *>(out + (c0 + j0 + col) * ld + at) = make_uint4(w[0], w[1], w[2], w[3]);
	}
}

} // namespace fseq
