// fseq_chainsort.hpp -- phase B for orders that do not fit LDS (m > 11,264 rows): one chain step as a stable radix
// sort by the block rank plus range maxima, instead of ceil(log2(nkeys) / 2) two-bit partition passes.
//
// A chain step (k_chain, fseq_kernels.hpp, for LDS-resident rows) takes the order (a, d) in front of a key block
// {rank[row], keyd[key], nkeys} to the order behind it: a' = the stable sort of a by rank[a]; the row at new position p
// whose predecessor there has ANOTHER rank starts a block key and takes d' = keyd[rank]; a row whose predecessor has the
// SAME rank was, in the old order, the next row of that rank behind it, at positions q < r, and takes
// d' = max d(q, r] -- the column update of libbio::pbwt::pbwt_context (founder_sequences.hh:56-65, SURVEY.md Appendix A
// step 2) with nkeys buckets.  The two-bit digit passes of the partition step carry that maximum through every pass,
// which is what makes them exact -- and, for 100,000 rows and 17-bit ranks, nine passes of the whole tile machinery by
// ONE workgroup: 2.5 ms a step, and phase B is a chain of ~40 such steps whatever the chip (and whatever the rank count of
// a sharded run: its Amdahl floor).  Here:
//   1. pairs (rank[a[i]], i), stably sorted by rank with an LSD radix sort of <= 9-bit digits (two passes for ranks below
//      2^18).  A wave owns a contiguous chunk of the array: per-wave digit histograms in LDS, one prefix over (digit,
//      wave), then every wave scatters its chunk in order -- the rows of a 64-row group that share a digit found with
//      one ballot per digit bit (their rank within the group = a popcount below the lane) -- no barrier inside a sweep;
//   2. prefix and suffix maxima of d inside 64-blocks (one wave scan each) and a sparse table over the block maxima;
//   3. every new position: its row, and keyd or the range maximum between the old positions of the two rows (two
//      block-end look-ups and two table entries, or a scan of at most 63 values inside one block).
// Everything but the histograms lives in the workgroup's workspace (L2-resident: a few MB).
// Two forms of the step live here: one step on one workgroup (pass 2's k_chain_snap_grouped, which keeps its records in a
// workspace of its own, pass2_ws_words: pass2_step sorts the rows, pass2_runs the runs of equal class they form), and the k_cm_*
// kernels, phase B's steps spread over the chip (launch_chain in fseq_path_pass1.hip, the only streamed phase B).
#pragma once

#include <type_traits>

#include "fseq_stream.hpp"
#include "fseq_types.hpp"

namespace fseq {

constexpr uint32_t CS_MAX_DIGIT_BITS = 9;
constexpr uint32_t CS_BINS = 1u << CS_MAX_DIGIT_BITS;
constexpr uint32_t CS_LEVELS = 16;               // sparse table over at most 2^16 blocks of 64 rows

// workspace words of one workgroup: a0 d0 | a1 d1 (= pairs A during a sort) | pairs B | prefix max | suffix max | table
__host__ __device__ inline size_t chainsort_ws_words(uint32_t m)
{
	size_t const nblk = ((size_t) m + 63) / 64;
	return 8 * (size_t) m + CS_LEVELS * nblk + 64;
}

// lanes of the wave whose digit equals mine (in = this lane holds a row), nbits digit bits
__device__ __forceinline__ uint64_t cs_match(uint32_t dg, bool in, uint32_t nbits)
{
	uint64_t mask = __ballot(in);
#pragma unroll
	for (uint32_t b = 0; b < CS_MAX_DIGIT_BITS; ++b)
		if (b < nbits)
		{
			uint64_t const bal = __ballot(in && ((dg >> b) & 1u));
			mask &= ((dg >> b) & 1u) ? bal : ~bal;
		}
	return mask;
}

__device__ __forceinline__ uint32_t cs_below(uint64_t mask)
{
	return (uint32_t) __builtin_amdgcn_mbcnt_hi((uint32_t) (mask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t) mask, 0u));
}

// -DFSEQ_RUN_STAMPS: [r17] where a run step's time goes.  s_memrealtime stamps (100 MHz: units of 10 ns) behind the parts of
// pass2_runs and chainwg_runs, every part ending at a barrier; thread 0 of every 64th workgroup prints the sums over the run steps
// of the first blocks / the first chain it takes (k_chain_snap_grouped, k_chain_wg).
#ifdef FSEQ_RUN_STAMPS
struct RunStamps {
	unsigned long long last, acc[8];
	uint32_t steps;
	__device__ __forceinline__ void clear() { for (int i = 0; i < 8; ++i) acc[i] = 0; steps = 0; }
	__device__ __forceinline__ void start() { last = __builtin_amdgcn_s_memrealtime(); }
	__device__ __forceinline__ void mark(int part) { unsigned long long const t = __builtin_amdgcn_s_memrealtime(); acc[part] += t - last; last = t; }
};
#define FSEQ_RS_PARAM , RunStamps &rs
#define FSEQ_RS_ARG , rs
#define FSEQ_RS_MARK(part) rs.mark(part)
#else
#define FSEQ_RS_PARAM
#define FSEQ_RS_ARG
#define FSEQ_RS_MARK(part)
#endif

// ------------------------------------------------------------------------------------------------
// Pass 2 behind the reduced phase C, streamed rows (fseq_reduced.hpp): a boundary inside a block is ONE such step from
// the block's boundary state, keyed by the classes the block's representatives form at the boundary's column (the tables of
// k_columns_red): the key of a row is cls[rank[row]].  ncls[t] == 0: the boundary is the block's border (a copy);
// 0xFFFFFFFF: not this kernel's (k_colblock_stream<MODE_SNAP>).
// The step is the one at the head of this file, arranged for the bytes it moves (the workspaces of 512 workgroups are far beyond L2 and the
// Infinity Cache, so every sweep and every gather goes to HBM):
//   * a workgroup takes all tasks of one block (a group: consecutive tasks with one task_blk) and gathers r[i] =
//     rank[a0[i]] ONCE for them, as 16 bits (ranks index the task's class table of red_cap <= P2_CLS_CAP entries); every
//     task of the block then reads r in order, 2 B a row, instead of its own chain of dependent gathers;
//   * the task's class table (rank -> class, red_cap entries) sits in LDS: the key of a row is cls_lds[r[i]], in the
//     counting and in the scatter sweep alike (no key buffer);
//   * step 2 writes ONE 16-byte record per old position, {a0[i], d0[i], prefix max[i], suffix max[i + 1]}: step 3 gathers
//     rec[hi] only, and takes the suffix maximum at lo = (the previous new position's hi) + 1 from that neighbour's record
//     (the lane below; lane 0 reads it itself) -- one random access per row instead of four.  The records and the sparse table
//     depend on the block's boundary state only: they are built ONCE for the block's tasks, beside r (pass2_records);
//   * the divergence in front of a class (headd) and the sparse-table entries are loaded only by the rows that use them.
// Groups are taken from a counter, largest first (the host orders them), so that blocks with many boundaries spread.
// ------------------------------------------------------------------------------------------------
constexpr uint32_t P2_CLS_CAP = 11264;           // most representatives of a reduced block (red_plan's cap)

// [r8] Runs.  The state in front of a block is a pBWT order: rows that agree over the block's next columns already lie together
// in it, so the positions of one class form a few runs of consecutive positions (about two a class where no recombination
// boundary of the founders lies between the block's start and the boundary's column) and the sort by class moves runs, not rows.
// A task whose classes form at most run_cap runs takes the run path (pass2_runs): one descriptor per run, the descriptors sorted
// by class, the new order written run by run -- inside a run a copy of consecutive old positions, whose divergences are their
// own; only a run's head takes headd or a range maximum.  Every other task takes the radix path (pass2_step) as before.
constexpr uint32_t P2_RUN_CAP = 8832;            // most runs of a task on the run path (138 x 64: about two a class for 4,352 classes)
constexpr uint32_t P2_CLS_BITS = 14;             // bits of a class in a run's descriptor, class << position bits | start: up to 2^18 rows
static_assert(P2_CLS_CAP <= (1u << P2_CLS_BITS), "a class of a reduced block fits a descriptor");

// A workgroup's sweeps go to memory (the workspaces of a chip's worth of workgroups are far beyond the caches), sixteen waves a
// CU: what a step takes is the round trips of its sweeps, so the run steps' own sweeps (pass2_runs, chainwg_*) keep CW_U groups of 64 positions in flight a wave
constexpr uint32_t CW_U = 8;

// [r17] The run of a new position without a search.  The sorted runs' first new positions as a bitmap (bit p & 31 of word p >> 5:
// position p starts a run) and pre[w], the starts in front of the 64 positions w: a wave's 64 positions of the output sweep are
// consecutive and 64-aligned, so the run of position p is pre[p >> 6] + (the starts of its 64 up to and including p) - 1 -- two
// wave-uniform LDS reads and an mbcnt pair -- and p is a head where its own bit is set.  Sized for 2^18 rows; a step's runs are at
// most 16,384, so 16 bits hold a count of starts.
constexpr uint32_t SEL_ROWS = 1u << 18;
struct RunSelect {
	uint32_t bits[SEL_ROWS / 32];
	uint16_t pre[SEL_ROWS / 64];
};

// Clears the words of m positions.  The caller puts a barrier between this and sel_set.
__device__ __forceinline__ void sel_clear(RunSelect &B, uint32_t m)
{
	for (uint32_t w = threadIdx.x; w < 2u * ((m + 63u) / 64u); w += ST) B.bits[w] = 0u;
}
__device__ __forceinline__ void sel_set(RunSelect &B, uint32_t p) { atomicOr(&B.bits[p >> 5], 1u << (p & 31u)); }
// pre from the bits every thread has set (barriers before and inside; the caller puts one behind)
__device__ __forceinline__ void sel_scan(RunSelect &B, uint32_t m, uint32_t *scan)
{
	__syncthreads();
	constexpr uint32_t Q = SEL_ROWS / 64u / ST;
	uint32_t const nw = (m + 63u) / 64u, w0 = threadIdx.x * Q;
	uint32_t c[Q], sum = 0;
#pragma unroll
	for (uint32_t t = 0; t < Q; ++t)
	{
		c[t] = w0 + t < nw ? (uint32_t) __popc(B.bits[2u * (w0 + t)]) + (uint32_t) __popc(B.bits[2u * (w0 + t) + 1u]) : 0u;
		sum += c[t];
	}
	uint32_t all;
	uint32_t at = block_excl_add<ST>(sum, scan, &all);
#pragma unroll
	for (uint32_t t = 0; t < Q; ++t)
		if (w0 + t < nw) { B.pre[w0 + t] = (uint16_t) at; at += c[t]; }
}
// The run of new position p (its wave's positions: the 64 of p >> 6, lane = p & 63, or all of them at or behind m) and whether p is
// the run's head.  A position at or behind m gets a run of the step (of the last 64 positions) and is no head's business.
__device__ __forceinline__ uint32_t sel_run(RunSelect const &B, uint32_t p, uint32_t m, bool *head)
{
	uint32_t const w = __builtin_amdgcn_readfirstlane(min(p, m - 1u) >> 6);
	uint32_t const lo = __builtin_amdgcn_readfirstlane(B.bits[2u * w]), hi = __builtin_amdgcn_readfirstlane(B.bits[2u * w + 1u]);
	uint32_t const lane = lane_id();
	bool const h = (((lane < 32u ? lo : hi) >> (lane & 31u)) & 1u) != 0u;
	*head = h;
	// (position 0 starts a run: the count is at least one wherever p < m)
	return (uint32_t) B.pre[w] + (uint32_t) __builtin_amdgcn_mbcnt_hi(hi, __builtin_amdgcn_mbcnt_lo(lo, 0u)) + (h ? 1u : 0u) - 1u;
}

struct Pass2Lds {
	uint32_t scan[ST / WAVE + 1];
	uint32_t grp;                                // the group the workgroup took
	union {
		struct {
			uint32_t hist[ST / WAVE][CS_BINS];   // per wave: digit counts, then the wave's write offsets
			uint32_t total[CS_BINS];
			uint16_t cls[P2_CLS_CAP];            // the task's class of a rank
		};
		struct {                                 // the run path's output sweep (the sort is done, the classes are in the descriptors)
			uint32_t dlt[P2_RUN_CAP];            // the run's first old position less its first new one (modulo 2^32), runs by (class, start)
			RunSelect sel;                       // the runs' first new positions
		};
	};
};

__host__ __device__ inline size_t pass2_lds_bytes() { return carve_bytes(1, sizeof(Pass2Lds)); }

// workspace words of one workgroup: r (16-bit) | final pairs (up to 2 words each) | first-pass pairs (the same) | the block's
// records (4 words each) | sparse table; every part 16-byte aligned.  The records and the table are the block's (built once for
// its tasks); the pair buffers are a task's, and hold the run descriptors of a task on the run path (2 words a run, runs <= m).
__host__ __device__ inline size_t pass2_ws_r(uint32_t m) { return (((size_t) m + 1) / 2 + 3) & ~size_t(3); }
__host__ __device__ inline size_t pass2_ws_words(uint32_t m)
{
	size_t const nblk = ((size_t) m + 63) / 64;
	return pass2_ws_r(m) + 2 * (size_t) m + 2 * (size_t) m + 4 * (size_t) m + ((CS_LEVELS * nblk + 64 + 3) & ~size_t(3));
}
struct Pass2Ws {
	uint16_t *r;
	uint32_t *bufB, *bufA;                       // 2 m words each
	uint4 *rec;
	uint32_t *tab;
};
__device__ __forceinline__ Pass2Ws pass2_ws(uint32_t *w, uint32_t m)
{
	Pass2Ws W;
	W.r = reinterpret_cast<uint16_t *>(w);
	W.bufB = w + pass2_ws_r(m);
	W.bufA = W.bufB + 2u * (size_t) m;
	W.rec = reinterpret_cast<uint4 *>(W.bufA + 2u * (size_t) m);
	W.tab = W.bufA + 6u * (size_t) m;
	return W;
}

// digit passes of a sort by class: npass passes of db bits each
__device__ __forceinline__ void pass2_digits(uint32_t D, uint32_t &npass, uint32_t &db)
{
	uint32_t bits = 1;
	while (bits < 32u && ((D - 1u) >> bits) != 0u) ++bits;
	npass = (bits + CS_MAX_DIGIT_BITS - 1u) / CS_MAX_DIGIT_BITS;
	db = (bits + npass - 1u) / npass;
}

// The stable LSD radix sort of cnt items by key_of(item), npass passes of db bits.  Item i of the first pass is load0(i); the last
// pass lands in bufB (pass p writes bufB where npass - p is odd, else bufA, and reads the other).  Ends with a barrier.
// (Lds: Pass2Lds, or the chain kernel's ChainWgLds -- scan, hist and total)
// (U: groups of 64 a wave keeps in flight in a sweep)
template <typename PairT, uint32_t U = 4, typename Load0, typename KeyOf, typename Lds>
__device__ __forceinline__ void pass2_sort(uint32_t cnt, uint32_t npass, uint32_t db, Load0 load0, KeyOf key_of, PairT none, PairT *bufA, PairT *bufB, Lds &S)
{
	uint32_t const tid = threadIdx.x, lane = lane_id();
	uint32_t const wave = __builtin_amdgcn_readfirstlane(tid >> 6);
	constexpr uint32_t NW = ST / WAVE;
	uint32_t const nbins = 1u << db;
	// a wave's chunk: whole groups of 64 positions
	uint32_t const per = ((cnt + NW - 1u) / NW + 63u) & ~63u;
	uint32_t const c_lo = min(cnt, wave * per), c_hi = min(cnt, c_lo + per);
	for (uint32_t p = 0; p < npass; ++p)
	{
		uint32_t const shift = p * db;
		bool const first = p == 0;
		PairT const *src = ((npass - p) & 1u) ? bufA : bufB;            // (unused in the first pass)
		PairT *dst = ((npass - p) & 1u) ? bufB : bufA;
		// first pass: the items are made on the way, in both sweeps
		auto load = [&](uint32_t i) -> PairT { return first ? load0(i) : src[i]; };
		for (uint32_t b = lane; b < nbins; b += 64u) S.hist[wave][b] = 0;
		// (a wave's histogram row is its own: no barrier between clearing and counting; LDS operations of a wave stay in order)
		for (uint32_t i0 = c_lo; i0 < c_hi; i0 += 64u * U)
		{
			PairT pr[U];
#pragma unroll
			for (uint32_t u = 0; u < U; ++u) { uint32_t const i = i0 + u * 64u + lane; pr[u] = i < c_hi ? load(i) : none; }
#pragma unroll
			for (uint32_t u = 0; u < U; ++u)
				if (i0 + u * 64u + lane < c_hi) atomicAdd(&S.hist[wave][(key_of(pr[u]) >> shift) & (nbins - 1u)], 1u);
		}
		__syncthreads();
		// offsets: bins ascending, inside a bin the waves ascending (= the array order: the sort is stable)
		uint32_t tot = 0;
		if (tid < nbins)
			for (uint32_t v = 0; v < NW; ++v) { uint32_t const c = S.hist[v][tid]; S.hist[v][tid] = tot; tot += c; }
		uint32_t all;
		uint32_t const start = block_excl_add<ST>(tid < nbins ? tot : 0u, S.scan, &all);
		if (tid < nbins) S.total[tid] = start;
		__syncthreads();
		for (uint32_t b = lane; b < nbins; b += 64u) S.hist[wave][b] += S.total[b];
		for (uint32_t i0 = c_lo; i0 < c_hi; i0 += 64u * U)
		{
			PairT pr[U];
#pragma unroll
			for (uint32_t u = 0; u < U; ++u) { uint32_t const i = i0 + u * 64u + lane; pr[u] = i < c_hi ? load(i) : none; }
#pragma unroll
			for (uint32_t u = 0; u < U; ++u)
			{
				bool const in = i0 + u * 64u + lane < c_hi;
				uint32_t const dg = (key_of(pr[u]) >> shift) & (nbins - 1u);
				uint64_t const same = cs_match(dg, in, db);
				uint32_t const below = cs_below(same);
				uint32_t const base = S.hist[wave][dg];
				if (in) dst[base + below] = pr[u];
				// (the read above and this write are LDS operations of one wave: they execute in order)
				if (in && below == 0u) S.hist[wave][dg] = base + (uint32_t) __popcll(same);
			}
		}
		__syncthreads();
	}
}

// The records of a block's boundary state (a0, d0), once for all its tasks: rec[i] = {a0[i], d0[i], the prefix maximum of d0
// inside i's 64-block up to i, the suffix maximum from i + 1 (at a block's last position: the next block's maximum)}, and a
// sparse table over the block maxima.  Ends with a barrier.
// (UB blocks a wave and iteration: their loads in flight together)
__device__ __forceinline__ void pass2_records(uint32_t m, uint32_t const *__restrict__ a0, uint32_t const *__restrict__ d0, uint4 *rec, uint32_t *tab)
{
	uint32_t const tid = threadIdx.x, lane = lane_id();
	uint32_t const wave = __builtin_amdgcn_readfirstlane(tid >> 6);
	constexpr uint32_t NW = ST / WAVE;
	uint32_t const nblk = (m + 63u) / 64u;
	constexpr uint32_t UB = 4;
	for (uint32_t b0 = wave; b0 < nblk; b0 += NW * UB)
	{
		uint32_t v[UB], a[UB];
#pragma unroll
		for (uint32_t u = 0; u < UB; ++u)
		{
			uint32_t const i = (b0 + u * NW) * 64u + lane;
			v[u] = i < m ? d0[i] : 0u;
			a[u] = i < m ? a0[i] : 0u;
		}
#pragma unroll
		for (uint32_t u = 0; u < UB; ++u)
		{
			uint32_t const blk = b0 + u * NW, i = blk * 64u + lane;
			if (blk >= nblk) break;
			uint32_t const pre = wave_incl_max(v[u]);
			uint32_t const rev = (uint32_t) __builtin_amdgcn_ds_bpermute((int) ((63u - lane) << 2), (int) v[u]);
			uint32_t const sufr = wave_incl_max(rev);
			// the suffix maximum from i + 1: lane 62 - lane of the reversed scan (lane 63's is the next block's maximum, below)
			uint32_t const sufn = (uint32_t) __builtin_amdgcn_ds_bpermute((int) ((62u - min(lane, 62u)) << 2), (int) sufr);
			if (i < m) rec[i] = make_uint4(a[u], v[u], pre, lane == 63u ? 0u : sufn);
			if (lane == 63u) tab[blk] = pre;
		}
	}
	__syncthreads();                                                      // (the records and level 0 of the table are whole)
	for (uint32_t j = tid; j + 1u < nblk; j += ST) rec[j * 64u + 63u].w = tab[j + 1u];
	for (uint32_t k = 1; k < CS_LEVELS && (1u << k) <= nblk; ++k)
	{
		uint32_t const *lo = tab + (size_t) (k - 1u) * nblk;
		uint32_t *hi = tab + (size_t) k * nblk;
		for (uint32_t j = tid; j + (1u << k) <= nblk; j += ST) hi[j] = max(lo[j], lo[j + (1u << (k - 1u))]);
		__syncthreads();
	}
	__syncthreads();
}

// max d0[lo .. hi], 1 <= lo <= hi, from the records: the suffix maximum at lo, the blocks between, the prefix maximum at hi, or,
// where lo and hi share a 64-block, one of the two where it is the range's, else a scan of at most 63 values
__device__ __forceinline__ uint32_t pass2_range_max(uint32_t lo, uint32_t hi, uint4 const *rec, uint32_t const *tab, uint32_t nblk, uint32_t const *__restrict__ d0)
{
	uint32_t const bl = lo >> 6, bh = hi >> 6;
	uint4 const rc = rec[hi], q = rec[lo - 1u];
	uint32_t const pz = q.z, sv = q.w;                                    // prefix max at lo - 1, suffix max at lo
	uint32_t dv = max(sv, rc.z);
	if (bh > bl + 1u)
	{
		uint32_t const k = 31u - (uint32_t) __builtin_clz(bh - bl - 1u);
		uint32_t const *t = tab + (size_t) k * nblk;
		dv = max(dv, max(t[bl + 1u], t[bh - (1u << k)]));
	}
	if (bl == bh)
	{
		if ((lo & 63u) == 0u || rc.z > pz) dv = rc.z;
		else if ((hi & 63u) == 63u || sv > rc.w) dv = sv;
		else
		{
			dv = rc.y;
			for (uint32_t i = lo; i < hi; ++i) dv = max(dv, d0[i]);
		}
	}
	return dv;
}

// One task by runs: (a0, d0) -> (a1, d1), keys S.cls[r[i]], D classes with divergences kd[class]; the caller has checked that a
// class (P2_CLS_BITS) and a position share a word.  Returns false, having written nothing, where the classes form more than run_cap runs
// (*nrun: how many); else ends with a barrier.  LDS: the class table is gone afterwards.
__device__ __forceinline__ bool pass2_runs(
	uint32_t m, uint32_t const *__restrict__ kd, uint32_t D, Pass2Ws const &W, Pass2Lds &S, uint32_t run_cap, uint32_t *nrun,
	uint32_t const *__restrict__ a0, uint32_t const *__restrict__ d0, uint32_t *__restrict__ a1, uint32_t *__restrict__ d1 FSEQ_RS_PARAM)
{
	uint32_t const tid = threadIdx.x, lane = lane_id();
	uint32_t const wave = __builtin_amdgcn_readfirstlane(tid >> 6);
	constexpr uint32_t NW = ST / WAVE;
	uint16_t const *__restrict__ r = W.r;
	uint32_t pb = 1;
	while (pb < 32u && ((m - 1u) >> pb) != 0u) ++pb;
	uint32_t const pmask = (1u << pb) - 1u;                               // (pb < 32: a class shares the word)
	uint32_t const nblk = (m + 63u) / 64u;
	uint32_t const per = ((m + NW - 1u) / NW + 63u) & ~63u;
	uint32_t const c_lo = min(m, wave * per), c_hi = min(m, c_lo + per);
	constexpr uint32_t U = 4;

	// ---- a. the runs: position i starts one where its class is not the class at i - 1.  A wave sweeps its chunk in order (the
	// class in front of a group of 64: the last lane of the group before, in front of the chunk: looked up); sweep 0 counts the
	// starts, sweep 1 writes the descriptors {class << pb | start, end} in position order.
	// [r17] Where r is 16-byte aligned (the workspace's always; a block's handed-over keys where block x m is a multiple of 8) a lane
	// takes a piece of PC = 8 consecutive ranks in one load, UV pieces in flight: a position is a start where its class differs from
	// the one in front -- inside the piece, or the last class of the lane below (of the group before, of the chunk before) -- and
	// the starts of a group of 64 pieces are placed by one wave scan of their counts.  The same descriptors in the same order.
	bool const vec = (reinterpret_cast<uintptr_t>(r) & 15u) == 0u;
	constexpr uint32_t PC = 8, UV = 4;
	uint32_t npass, db;
	pass2_digits(D, npass, db);
	uint2 *const bufA = reinterpret_cast<uint2 *>(W.bufA), *const bufB = reinterpret_cast<uint2 *>(W.bufB);
	uint32_t *const pos_order = reinterpret_cast<uint32_t *>((npass & 1u) ? bufA : bufB);      // (the buffer the first pass of the sort does not write)
	uint32_t R = 0, wbase = 0;
	for (uint32_t sweep = 0; sweep < 2u; ++sweep)
	{
		uint32_t prev = 0xFFFFFFFFu;                                      // (no class: position 0 starts a run)
		if (c_lo > 0u && c_lo < c_hi) prev = (uint32_t) S.cls[r[c_lo - 1u]];
		uint32_t k0 = wbase;
		for (uint32_t i0 = c_lo; vec && i0 < c_hi; i0 += 64u * PC * UV)
		{
			uint4 rv[UV];
#pragma unroll
			for (uint32_t u = 0; u < UV; ++u)
			{
				uint32_t const ib = i0 + (u * 64u + lane) * PC;
				rv[u] = make_uint4(0u, 0u, 0u, 0u);
				if (ib + PC <= c_hi) rv[u] = *reinterpret_cast<uint4 const *>(r + ib);
				else if (ib < c_hi)
				{
					// the chunk's last piece: nothing behind c_hi is read
					uint32_t x[PC / 2u] = {0u, 0u, 0u, 0u};
#pragma unroll
					for (uint32_t e = 0; e < PC; ++e)
						if (ib + e < c_hi) x[e >> 1] |= (uint32_t) r[ib + e] << (16u * (e & 1u));
					rv[u] = make_uint4(x[0], x[1], x[2], x[3]);
				}
			}
#pragma unroll
			for (uint32_t u = 0; u < UV; ++u)
			{
				if (i0 + u * 64u * PC >= c_hi) break;
				uint32_t const ib = i0 + (u * 64u + lane) * PC;
				uint32_t const x[PC / 2u] = {rv[u].x, rv[u].y, rv[u].z, rv[u].w};
				uint32_t cl[PC];
#pragma unroll
				for (uint32_t e = 0; e < PC; ++e) cl[e] = (uint32_t) S.cls[(x[e >> 1] >> (16u * (e & 1u))) & 0xFFFFu];
				uint32_t const up = shfl_up_u32(cl[PC - 1u], 1);
				uint32_t front = lane ? up : prev, hm = 0;
#pragma unroll
				for (uint32_t e = 0; e < PC; ++e)
				{
					if (ib + e < c_hi && cl[e] != front) hm |= 1u << e;
					front = cl[e];
				}
				uint32_t const cnt = (uint32_t) __popc(hm), inc = wave_incl_add(cnt);
				if (sweep)
				{
					uint32_t k = k0 + inc - cnt;
#pragma unroll
					for (uint32_t e = 0; e < PC; ++e)
						if ((hm >> e) & 1u)
						{
							pos_order[2u * k] = (cl[e] << pb) | (ib + e);
							if (k) pos_order[2u * k - 1u] = ib + e;           // (the run before ends here)
							++k;
						}
				}
				k0 += readlane_u32(inc, 63);
				prev = readlane_u32(cl[PC - 1u], 63);                         // (a group that is not whole is the chunk's last)
			}
		}
		for (uint32_t i0 = c_lo; !vec && i0 < c_hi; i0 += 64u * U)
		{
			uint32_t rv[U];
#pragma unroll
			for (uint32_t u = 0; u < U; ++u) { uint32_t const i = i0 + u * 64u + lane; rv[u] = i < c_hi ? (uint32_t) r[i] : 0u; }
#pragma unroll
			for (uint32_t u = 0; u < U; ++u)
			{
				uint32_t const i = i0 + u * 64u + lane;
				if (i0 + u * 64u >= c_hi) break;
				bool const in = i < c_hi;
				uint32_t const cl = (uint32_t) S.cls[rv[u]];
				uint32_t const up = shfl_up_u32(cl, 1);
				bool const head = in && cl != (lane ? up : prev);
				uint64_t const heads = __ballot(head);
				if (sweep)
				{
					uint32_t const k = k0 + cs_below(heads);
					if (head)
					{
						pos_order[2u * k] = (cl << pb) | i;
						if (k) pos_order[2u * k - 1u] = i;                // (the run before ends here)
					}
				}
				k0 += (uint32_t) __popcll(heads);
				prev = readlane_u32(cl, 63);                              // (a group that is not whole is the chunk's last)
			}
		}
		if (sweep) break;
		uint32_t const before = block_excl_add<ST>(lane == 0u ? k0 : 0u, S.scan, &R);
		wbase = __builtin_amdgcn_readfirstlane(before);
		*nrun = R;
		if (R > run_cap) return false;
		FSEQ_RS_MARK(1);
	}
	if (tid == 0u) pos_order[2u * R - 1u] = m;
	__syncthreads();
	FSEQ_RS_MARK(2);

	// ---- b. the runs by (class, start): a stable sort by class of descriptors that are in start order
	pass2_sort<uint2>(R, npass, db, [&](uint32_t i) -> uint2 { return reinterpret_cast<uint2 const *>(pos_order)[i]; },
	                  [&](uint2 x) -> uint32_t { return x.x >> pb; }, make_uint2(0u, 0u), bufA, bufB, S);
	FSEQ_RS_MARK(3);
	// their first new positions: the prefix sum of their lengths (a thread takes consecutive runs)
	{
		uint32_t const q = (R + ST - 1u) / ST, j0 = min(R, tid * q), j1 = min(R, j0 + q);
		uint32_t sum = 0;
		for (uint32_t j = j0; j < j1; ++j) { uint2 const x = bufB[j]; sum += x.y - (x.x & pmask); }
		// (the sort's last barrier is behind every use of the histograms and of the class table, which these arrays lie over)
		sel_clear(S.sel, m);
		uint32_t all;
		uint32_t at = block_excl_add<ST>(sum, S.scan, &all);
		for (uint32_t j = j0; j < j1; ++j)
		{
			uint2 const x = bufB[j];
			S.dlt[j] = (x.x & pmask) - at; sel_set(S.sel, at);
			at += x.y - (x.x & pmask);
		}
		sel_scan(S.sel, m, S.scan);
	}
	// (the barrier behind the heads' pass is behind pre too)
#ifdef FSEQ_RUN_STAMPS
	__syncthreads();
#endif
	FSEQ_RS_MARK(4);

	// ---- c. the divergence of every run's head, in a pass of its own (as chainwg_runs d): the class's where the run is its class's
	// first, else the maximum of d0 from behind the end of the run before it (same class) up to its own first position.  The sort
	// has ended in bufB: the other pair buffer is free
	uint32_t *const rhead = reinterpret_cast<uint32_t *>(bufA);
	{
		constexpr uint32_t UH = 4;
		for (uint32_t j0 = tid; j0 < R; j0 += ST * UH)
		{
			uint2 me[UH], pv[UH];
			uint32_t hv[UH];
#pragma unroll
			for (uint32_t u = 0; u < UH; ++u)
			{
				uint32_t const j = min(j0 + u * ST, R - 1u);
				me[u] = bufB[j]; pv[u] = bufB[j ? j - 1u : 0u];
			}
#pragma unroll
			for (uint32_t u = 0; u < UH; ++u)
			{
				uint32_t const j = j0 + u * ST;
				hv[u] = 0u;
				if (j >= R) continue;
				if (j == 0u || (pv[u].x >> pb) != (me[u].x >> pb)) hv[u] = kd[me[u].x >> pb];
				else hv[u] = pass2_range_max(pv[u].y, me[u].x & pmask, W.rec, W.tab, nblk, d0);   // (runs of one class are not neighbours: lo < hi)
			}
#pragma unroll
			for (uint32_t u = 0; u < UH; ++u) { uint32_t const j = j0 + u * ST; if (j < R) rhead[j] = hv[u]; }
		}
	}
	__syncthreads();
	FSEQ_RS_MARK(7);

	// ---- d. the new order: position p lies in the run j the bitmap gives and takes the row at old position p + dlt[j]; behind the
	// run's head its divergence too, the head the one of c.
	for (uint32_t p0 = tid; p0 < m; p0 += ST * CW_U)
	{
		uint32_t jh[CW_U], hh[CW_U], av[CW_U], dv[CW_U];
#pragma unroll
		for (uint32_t u = 0; u < CW_U; ++u)
		{
			uint32_t const p = p0 + u * ST;
			bool head;
			uint32_t const j = sel_run(S.sel, p, m, &head);
			hh[u] = p < m ? p + S.dlt[j] : 0u;
			jh[u] = head && p < m ? j : 0xFFFFFFFFu;
		}
#pragma unroll
		for (uint32_t u = 0; u < CW_U; ++u) { av[u] = a0[hh[u]]; dv[u] = jh[u] != 0xFFFFFFFFu ? rhead[jh[u]] : d0[hh[u]]; }
#pragma unroll
		for (uint32_t u = 0; u < CW_U; ++u)
		{
			uint32_t const p = p0 + u * ST;
			if (p < m) { a1[p] = av[u]; d1[p] = dv[u]; }
		}
	}
	__syncthreads();
	FSEQ_RS_MARK(5);
	return true;
}

// The new order from the sorted pairs perm[p] = (key, old position) and the records of (a0, d0): position p takes the row of its
// record; the first of a key takes kd[key], any other the maximum of d0(lo .. hi] = max(suffix max at lo, the blocks between, prefix
// max at hi), or a scan of at most 63 values where lo and hi share a 64-block.  The positions of a wave are consecutive: the record
// of p - 1 is the lane below.  P4: a pair is ONE word, key << pb | position.  Ends with a barrier.
template <bool P4>
__device__ __forceinline__ void pass2_place(
	uint32_t m, uint32_t const *__restrict__ kd, std::conditional_t<P4, uint32_t, uint2> const *perm, uint4 const *rec, uint32_t const *tab,
	uint32_t const *__restrict__ d0, uint32_t *__restrict__ a1, uint32_t *__restrict__ d1)
{
	uint32_t const tid = threadIdx.x, lane = lane_id();
	using PairT = std::conditional_t<P4, uint32_t, uint2>;
	uint32_t pb = 1;
	while (pb < 32u && ((m - 1u) >> pb) != 0u) ++pb;
	uint32_t const pmask = pb < 32u ? (1u << pb) - 1u : 0xFFFFFFFFu;
	auto key_of = [&](PairT pr) -> uint32_t { if constexpr (P4) return pr >> pb; else return pr.x; };
	auto pos_of = [&](PairT pr) -> uint32_t { if constexpr (P4) return pr & pmask; else return pr.y; };
	uint32_t const nblk = (m + 63u) / 64u;
	{
		constexpr uint32_t U = 4;
		for (uint32_t p0 = tid; p0 < m; p0 += ST * U)
		{
			uint2 me[U], pv[U];
#pragma unroll
			for (uint32_t u = 0; u < U; ++u)
			{
				uint32_t const p = min(p0 + u * ST, m - 1u);
				PairT const pm_ = perm[p], pp_ = perm[p ? p - 1u : 0u];
				me[u] = make_uint2(key_of(pm_), pos_of(pm_));
				pv[u] = make_uint2(key_of(pp_), pos_of(pp_));
			}
			uint4 rc[U];
			uint32_t z0[U], w0[U], kdv[U], t0[U], t1[U];
#pragma unroll
			for (uint32_t u = 0; u < U; ++u)
			{
				uint32_t const p = p0 + u * ST;
				bool const first = p == 0u || pv[u].x != me[u].x;
				uint32_t const lo = pv[u].y + 1u, hi = me[u].y;
				uint32_t const bl = lo >> 6, bh = hi >> 6;
				rc[u] = rec[hi];
				z0[u] = 0u; w0[u] = 0u; kdv[u] = 0u; t0[u] = 0u; t1[u] = 0u;
				if (lane == 0u && !first) { uint4 const q = rec[pv[u].y]; z0[u] = q.z; w0[u] = q.w; }
				if (p < m && first) kdv[u] = kd[me[u].x];
				if (p < m && !first && bh > bl + 1u)
				{
					uint32_t const k = 31u - (uint32_t) __builtin_clz(bh - bl - 1u);
					uint32_t const *t = tab + (size_t) k * nblk;
					t0[u] = t[bl + 1u];
					t1[u] = t[bh - (1u << k)];
				}
			}
#pragma unroll
			for (uint32_t u = 0; u < U; ++u)
			{
				uint32_t const p = p0 + u * ST;
				// the record of p - 1 (old position lo - 1): from the lane below; lane 0 keeps its own load
				uint32_t const bz = (uint32_t) __builtin_amdgcn_ds_bpermute((int) ((lane - 1u) << 2), (int) rc[u].z);
				uint32_t const bw = (uint32_t) __builtin_amdgcn_ds_bpermute((int) ((lane - 1u) << 2), (int) rc[u].w);
				if (p < m)
				{
					bool const first = p == 0u || pv[u].x != me[u].x;
					uint32_t const lo = pv[u].y + 1u, hi = me[u].y;      // (same class:) max of d0[lo .. hi], lo <= hi
					uint32_t const bl = lo >> 6, bh = hi >> 6;
					uint32_t const pz = lane ? bz : z0[u], sv = lane ? bw : w0[u];   // prefix max at lo - 1, suffix max at lo
					uint32_t dv = max(sv, rc[u].z);
					if (bh > bl + 1u) dv = max(dv, max(t0[u], t1[u]));
					if (!first && bl == bh)
					{
						// lo and hi in one 64-block: the prefix maximum at hi is the range's if it grew behind lo - 1 (or lo starts
						// the block), the suffix maximum at lo if it is larger than the one behind hi (or hi ends the block); else a scan
						if ((lo & 63u) == 0u || rc[u].z > pz) dv = rc[u].z;
						else if ((hi & 63u) == 63u || sv > rc[u].w) dv = sv;
						else
						{
							dv = rc[u].y;
							for (uint32_t i = lo; i < hi; i += 4u)
							{
								uint32_t const x0 = d0[i], x1 = i + 1u < hi ? d0[i + 1u] : 0u;
								uint32_t const x2 = i + 2u < hi ? d0[i + 2u] : 0u, x3 = i + 3u < hi ? d0[i + 3u] : 0u;
								dv = max(dv, max(max(x0, x1), max(x2, x3)));
							}
						}
					}
					a1[p] = rc[u].x;
					d1[p] = first ? kdv[u] : dv;
				}
			}
		}
	}
	__syncthreads();
}

// One task by the sort of all its rows: (a0, d0) -> (a1, d1), keys S.cls[r[i]], D classes with divergences kd[class].  Ends with a barrier.
template <bool P4>
__device__ __forceinline__ void pass2_step(
	uint32_t m, uint32_t const *__restrict__ kd, uint32_t D, Pass2Ws const &W, Pass2Lds &S,
	uint32_t const *__restrict__ d0, uint32_t *__restrict__ a1, uint32_t *__restrict__ d1)
{
	// P4: a pair is ONE word, key << pb | position (the caller has checked that the bits fit)
	using PairT = std::conditional_t<P4, uint32_t, uint2>;
	uint32_t pb = 1;
	while (pb < 32u && ((m - 1u) >> pb) != 0u) ++pb;
	auto mk = [&](uint32_t key, uint32_t pos) -> PairT { if constexpr (P4) return (key << pb) | pos; else return make_uint2(key, pos); };
	auto key_of = [&](PairT pr) -> uint32_t { if constexpr (P4) return pr >> pb; else return pr.x; };
	uint16_t const *__restrict__ r = W.r;

	// ---- 1. the sort: the pairs are made on the way from r and the class table in LDS
	uint32_t npass, db;
	pass2_digits(D, npass, db);
	pass2_sort<PairT>(m, npass, db, [&](uint32_t i) -> PairT { return mk((uint32_t) S.cls[r[i]], i); }, key_of, mk(0u, 0u),
	                  reinterpret_cast<PairT *>(W.bufA), reinterpret_cast<PairT *>(W.bufB), S);
	// ---- 2. (the records: pass2_records, once for the block)
	// ---- 3. the new order
	pass2_place<P4>(m, kd, reinterpret_cast<PairT const *>(W.bufB), W.rec, W.tab, d0, a1, d1);
}

// stats (P2_STATS words, fseq_types.hpp): tasks on the run path, tasks on the radix path, border copies, the most runs a task had
// (of the tasks that counted theirs), those tasks by the power of two their run count reaches (P2_HIST buckets)
// [r15] hand_keys / hand_flag (or nullptr): phase B's hand-over (ChainMultiArgs) -- a group whose block has its flag set reads the
// block's r from hand_keys[block][m] and gathers nothing; hand_stats (or nullptr): two words, the groups that took handed-over keys
// and the groups that did not
__global__ __launch_bounds__(ST) void k_chain_snap_grouped(
	uint32_t const *__restrict__ bstate_a, uint32_t const *__restrict__ bstate_d, uint32_t const *__restrict__ rank, uint32_t m,
	uint32_t const *__restrict__ task_blk, uint32_t const *__restrict__ cls, uint32_t const *__restrict__ headd, uint32_t const *__restrict__ ncls,
	uint32_t cap, uint2 const *__restrict__ grps, uint32_t ngrp, uint32_t *__restrict__ grp_next, uint32_t *__restrict__ snap_a,
	uint32_t *__restrict__ snap_d, uint32_t *ws, uint32_t run_cap, uint32_t *__restrict__ stats,
	uint16_t const *hand_keys, uint32_t const *hand_flag, uint32_t *hand_stats)
{
	extern __shared__ __attribute__((aligned(16))) char smem[];
	Pass2Lds &S = *reinterpret_cast<Pass2Lds *>(smem);
	uint32_t const tid = threadIdx.x;
	Pass2Ws const W0 = pass2_ws(ws + (size_t) blockIdx.x * pass2_ws_words(m), m);
	uint32_t pbits = 1;
	while (pbits < 32u && ((m - 1u) >> pbits) != 0u) ++pbits;
#ifdef FSEQ_RUN_STAMPS
	RunStamps rs;
	uint32_t rs_groups = 0;
#endif
	for (;;)
	{
		if (tid == 0) S.grp = atomicAdd(grp_next, 1u);
		__syncthreads();
		uint32_t const g = S.grp;
		__syncthreads();                                                  // (S.grp is read by all before it is taken again)
		if (g >= ngrp) break;
		uint2 const gr = grps[g];
		uint32_t const blk = task_blk[gr.x];
		size_t const sb = (size_t) blk * m;
		uint32_t const *a0 = bstate_a + sb, *d0 = bstate_d + sb;
		// the block's r: phase B's, where it handed the block's keys over, else gathered into the workspace below
		bool const handed = hand_keys != nullptr && hand_flag[blk] != 0u;
		Pass2Ws W = W0;
		if (handed) W.r = const_cast<uint16_t *>(hand_keys) + sb;               // (read only from here on)
		if (hand_stats && tid == 0) atomicAdd(hand_stats + (handed ? 0 : 1), 1u);
		bool have_r = false;
#ifdef FSEQ_RUN_STAMPS
		rs.clear();
		uint32_t rs_sorted = 0;
		unsigned long long rs_runs = 0;
#endif
		for (uint32_t task = gr.x; task < gr.x + gr.y; ++task)
		{
			uint32_t const D = ncls[task];
			if (D == 0xFFFFFFFFu) continue;
			size_t const ob = (size_t) task * m;
			if (D == 0u)
			{
				for (uint32_t i = tid; i < m; i += ST) { snap_a[ob + i] = a0[i]; snap_d[ob + i] = d0[i]; }
				if (tid == 0) atomicAdd(stats + 2, 1u);
				continue;
			}
			if (!have_r)
			{
				// the block's ranks in the order in front of its boundaries, once for all of them (U loads in flight per thread)
				constexpr uint32_t U = 4;
				if (!handed)
					for (uint32_t i0 = tid; i0 < m; i0 += ST * U)
					{
						uint32_t rv[U];
#pragma unroll
						for (uint32_t u = 0; u < U; ++u) { uint32_t const i = i0 + u * ST; rv[u] = i < m ? rank[sb + a0[i]] : 0u; }
#pragma unroll
						for (uint32_t u = 0; u < U; ++u) { uint32_t const i = i0 + u * ST; if (i < m) W.r[i] = (uint16_t) rv[u]; }
					}
				// ... and the records and the table of its boundary state
#ifdef FSEQ_RUN_STAMPS
				__syncthreads();
				rs.start();
#endif
				pass2_records(m, a0, d0, W.rec, W.tab);
				FSEQ_RS_MARK(6);
				have_r = true;
			}
#ifdef FSEQ_RUN_STAMPS
			RunStamps const rs_before = rs;
			rs.start();
#endif
			for (uint32_t j = tid; j < cap; j += ST) S.cls[j] = (uint16_t) cls[(size_t) task * cap + j];
			__syncthreads();
			FSEQ_RS_MARK(0);
			// (the classes and the positions share a word where their bits fit: at most 11,264 classes, 2^18 rows)
			uint32_t kb = 1;
			while (kb < 32u && ((D - 1u) >> kb) != 0u) ++kb;
			bool const p4 = kb + pbits <= 32u;
			uint32_t const *kd = headd + (size_t) task * cap;
			uint32_t nrun = 0;
			// (a run's descriptor is a word of P2_CLS_BITS class bits over a position: with more than 2^18 rows every task sorts its rows)
			bool const by_runs = run_cap != 0u && P2_CLS_BITS + pbits <= 32u && pass2_runs(m, kd, D, W, S, run_cap, &nrun, a0, d0, snap_a + ob, snap_d + ob FSEQ_RS_ARG);
#ifdef FSEQ_RUN_STAMPS
			if (by_runs) { ++rs.steps; rs_runs += nrun; }
			else { rs = rs_before; ++rs_sorted; }                         // (a task that sorts its rows: not in the sums)
#endif
			if (!by_runs)
			{
				if (p4) pass2_step<true>(m, kd, D, W, S, d0, snap_a + ob, snap_d + ob);
				else pass2_step<false>(m, kd, D, W, S, d0, snap_a + ob, snap_d + ob);
			}
			if (tid == 0)
			{
				atomicAdd(stats + (by_runs ? 0 : 1), 1u);
				if (nrun)
				{
					atomicMax(stats + 3, nrun);
					atomicAdd(stats + 4 + min(P2_HIST - 1u, nrun > 1u ? 32u - (uint32_t) __builtin_clz(nrun - 1u) : 0u), 1u);
				}
			}
		}
#ifdef FSEQ_RUN_STAMPS
		if (tid == 0 && (blockIdx.x & 63u) == 0u && rs.steps != 0u && rs_groups++ < 3u)
			printf("p2 run stamps workgroup %u block %u (%u rows, %s keys, %u tasks by runs of %llu runs on average, %u sorted): records %llu, per task by runs: class table %llu, "
			       "sweep 0 %llu, sweep 1 %llu, descriptor sort %llu, prefix sums %llu, heads %llu, output sweep %llu (x 10 ns)\n",
			       blockIdx.x, blk, m, handed ? "handed-over" : "gathered", rs.steps, rs_runs / rs.steps, rs_sorted, rs.acc[6], rs.acc[0] / rs.steps, rs.acc[1] / rs.steps,
			       rs.acc[2] / rs.steps, rs.acc[3] / rs.steps, rs.acc[4] / rs.steps, rs.acc[7] / rs.steps, rs.acc[5] / rs.steps);
#endif
	}
}

// ================================================================================================
// The same step spread over the chip.  One workgroup per chain leaves 255 CUs idle on the levels of phase B's recursion
// that matter for its length -- the top ones, a handful of chains of four steps each -- and a step is bound by what ONE
// CU's texture path takes to gather and scatter 100,000 rows a dozen times (1.6 ms a step: BASELINE C4 phase B 95 -> 61 ms
// against a chain on one workgroup).  Here every sweep of a step is a launch over (parts of 1,024 positions) x
// (chains of the level): per radix pass  count  ->  offsets  ->  scatter, then the new order; a chain of G blocks is G
// such rounds, the chains of a level side by side.  A wave owns a part (16 groups of 64 positions in order); the digit
// histograms of the parts sit in a table of their own ([chain][part][bin]), whose prefix over (bin, part) one workgroup
// per chain takes -- it also builds the sparse table of the block maxima the count sweep of the first pass left.
// The number of passes a block needs (bits of nkeys) is device data: the host always queues the passes m needs and the
// kernels of a pass the block does not need return at once (the ping-pong of the pair buffers is by the block's own count).
// Pairs are (rank | row low 12 bits << 20, position | row high bits << 20): rows, positions and ranks are below 2^20.
// ================================================================================================
constexpr uint32_t CM_PART = 1024;               // positions per part (one wave: 16 groups of 64)
constexpr uint32_t CM_WG = 256;                  // threads per workgroup of the part kernels: four parts

// (ChainMultiArgs: fseq_types.hpp -- phase B builds one per chain launch, the kernels here take it as it is)

// [r5] Which (part group, chain) a workgroup of the part / row kernels takes.  The hardware hands consecutive workgroups to
// the eight XCDs in turn, so with (x, y) = (part group, chain) taken as they come the twenty-five workgroups of a chain land
// on all eight -- and each XCD's L2 fetches the chain's tables for an eighth of its gathers: rank[row] of the first count
// sweep, the pair buffers of the scatter sweeps, d0 / the block maxima of the output sweep are all addressed at random inside
// arrays of m words that belong to ONE chain (400 KB each at m = 100,000; an L2 is 4 MB).  Here workgroup L goes to XCD
// L mod 8 and takes chain 8 (slot / nx) + (L mod 8), slot = L / 8: the workgroups of a chain are consecutive slots of one XCD.
struct CmWg { uint32_t x, chain; bool ok; };
__device__ __forceinline__ CmWg cm_wg(ChainMultiArgs const &A)
{
	CmWg w;
	uint32_t const nx = gridDim.x, L = blockIdx.y * nx + blockIdx.x;
	uint32_t const xcd = L & 7u, slot = L >> 3;
	w.chain = (slot / nx) * 8u + xcd;
	w.x = slot % nx;
	w.ok = w.chain < A.nchains;
	return w;
}

__host__ __device__ inline uint32_t chainmulti_parts(uint32_t m) { return (m + CM_PART - 1u) / CM_PART; }
__host__ __device__ inline uint32_t chainmulti_passes(uint32_t m)
{
	uint32_t bits = 1;
	while (bits < 32u && ((m - 1u) >> bits) != 0u) ++bits;
	return (bits + CS_MAX_DIGIT_BITS - 1u) / CS_MAX_DIGIT_BITS;
}

struct ChainMultiGeom {
	uint32_t b, npass, db, nbins;
	uint32_t pb;                                 // bits of a position (m - 1)
	bool p4;                                     // [r5] a pair is one word, key << pb | position (the key's bits fit beside the position's)
	bool active;
	uint32_t *w;
	uint32_t const *a0, *d0;
	uint32_t *a1, *d1;
	uint2 *pairA, *pairB;
	uint32_t *pm, *sm, *tab;
	uint32_t *hist;
};

__device__ __forceinline__ ChainMultiGeom chainmulti_geom(ChainMultiArgs const &A, uint32_t chain)
{
	ChainMultiGeom g;
	uint32_t const grp = chain + A.grp0;
	uint32_t const b0 = grp * A.G, b1 = min(A.nb_total, b0 + A.G);
	g.b = b0 + A.step;
	// (an expansion -- states wanted, no composite keys -- does not step through a chain's last block unless that is the last
	// of all: the state behind it is the next chain's start state, k_chain in fseq_kernels.hpp)
	g.active = g.b < b1 && (A.out_rank != nullptr || g.b + 1u < b1 || g.b + 1u == A.nb_total);
	uint32_t const nk = g.active ? A.nkeys[g.b] : 1u;
	uint32_t bits = 1;
	while (bits < 32u && ((nk - 1u) >> bits) != 0u) ++bits;
	g.npass = (bits + CS_MAX_DIGIT_BITS - 1u) / CS_MAX_DIGIT_BITS;
	g.db = (bits + g.npass - 1u) / g.npass;
	g.nbins = 1u << g.db;
	uint32_t const cur = A.step & 1u, m = A.m;
	g.pb = 1;
	while (g.pb < 32u && ((m - 1u) >> g.pb) != 0u) ++g.pb;
	g.p4 = bits + g.pb <= 32u;
	g.w = A.ws + (size_t) chain * chainsort_ws_words(m);
	g.a0 = g.w + (size_t) cur * 2u * m; g.d0 = g.a0 + m;
	g.a1 = g.w + (size_t) (cur ^ 1u) * 2u * m; g.d1 = g.a1 + m;
	g.pairA = reinterpret_cast<uint2 *>(g.a1);
	g.pairB = reinterpret_cast<uint2 *>(g.w + 4u * (size_t) m);
	g.pm = g.w + 6u * (size_t) m; g.sm = g.w + 7u * (size_t) m; g.tab = g.w + 8u * (size_t) m;
	g.hist = A.hist + (size_t) chain * chainmulti_parts(m) * CS_BINS;
	return g;
}

__device__ __forceinline__ uint2 cm_pack(uint32_t key, uint32_t pos, uint32_t row) { return make_uint2(key | (row << 20), pos | ((row >> 12) << 20)); }
__device__ __forceinline__ uint32_t cm_key(uint2 p) { return p.x & 0xFFFFFu; }
__device__ __forceinline__ uint32_t cm_pos(uint2 p) { return p.y & 0xFFFFFu; }
__device__ __forceinline__ uint32_t cm_row(uint2 p) { return (p.x >> 20) | ((p.y >> 20) << 12); }

// [r5] P4: the pairs of a chain whose keys fit beside a position in ONE word (the key blocks of the alignment's own blocks:
// at most 12 x 1,024 keys; BASELINE C4: eleven of every twelve steps) are that word, key << pb | position, and the new order
// looks its row up at the old position -- half the bytes through the four sweeps of the sort for one gather more in the last
template <bool P4>
struct CmPair {
	using T = std::conditional_t<P4, uint32_t, uint2>;
	static __device__ __forceinline__ T pack(ChainMultiGeom const &g, uint32_t key, uint32_t pos, uint32_t row)
	{
		if constexpr (P4) { (void) row; return (key << g.pb) | pos; } else { (void) g; return cm_pack(key, pos, row); }
	}
	static __device__ __forceinline__ T none() { if constexpr (P4) return 0u; else return make_uint2(0u, 0u); }
	static __device__ __forceinline__ uint32_t key(ChainMultiGeom const &g, T p) { if constexpr (P4) return p >> g.pb; else { (void) g; return cm_key(p); } }
	static __device__ __forceinline__ uint32_t pos(ChainMultiGeom const &g, T p) { if constexpr (P4) return p & ((1u << g.pb) - 1u); else { (void) g; return cm_pos(p); } }
	static __device__ __forceinline__ uint32_t row(ChainMultiGeom const &g, T p) { if constexpr (P4) return g.a0[pos(g, p)]; else { (void) g; return cm_row(p); } }
	static __device__ __forceinline__ T *bufA(ChainMultiGeom const &g) { return reinterpret_cast<T *>(g.pairA); }
	static __device__ __forceinline__ T *bufB(ChainMultiGeom const &g) { return reinterpret_cast<T *>(g.pairB); }
	static __device__ __forceinline__ T *stage(ChainMultiGeom const &g) { return (g.npass & 1u) ? bufA(g) : bufB(g); }
	// pair of position i for the sweep kernels of pass p: made on the way in the first pass, else from the pass before
	static __device__ __forceinline__ T load(ChainMultiGeom const &g, uint32_t const *rk, uint32_t pass, uint32_t i)
	{
		if (pass == 0u) { uint32_t const r = g.a0[i]; return pack(g, rk[r], i, r); }
		T const *src = ((g.npass - pass) & 1u) ? bufA(g) : bufB(g);
		return src[i];
	}
};

// [r5] the first pass's pairs are made ONCE, by its count sweep, which leaves them in the pair buffer the pass does not
// write (dead until the second pass overwrites it): rank[row] is a gather at a random row of a table of m words per block --
// a 64-byte line from memory for 4 bytes, thousands of chains side by side -- and the scatter sweep used to make it again
// (BASELINE C4, 2,048 chains: 3.5 ms of every step's 9)
// (CmPair::stage)

// start state of every chain of the launch into its workspace (and out_state in front of its first block)
__global__ __launch_bounds__(CM_WG) void k_cm_init(ChainMultiArgs const A)
{
	CmWg const wg = cm_wg(A);
	if (!wg.ok) return;
	uint32_t const chain = wg.chain, grp = chain + A.grp0, m = A.m;
	uint32_t const b0 = grp * A.G;
	if (b0 >= A.nb_total) return;
	uint32_t const kstart = (uint32_t) ((uint64_t) b0 * A.cols_per_block);
	uint32_t *w = A.ws + (size_t) chain * chainsort_ws_words(m);
	uint32_t const i = wg.x * CM_WG + threadIdx.x;
	if (i >= m) return;
	uint32_t const av = A.start_a ? A.start_a[(size_t) grp * m + i] : i;
	uint32_t const dv = A.start_d ? A.start_d[(size_t) grp * m + i] : kstart;
	w[i] = av; w[(size_t) m + i] = dv;
	if (A.out_state_a) { A.out_state_a[(size_t) b0 * m + i] = av; A.out_state_d[(size_t) b0 * m + i] = dv; }
}

// count sweep of pass A.pass: digit histogram of every part; first pass: also prefix / suffix maxima of d inside the
// 64-blocks of the part and the block maxima (level 0 of the table)
__global__ __launch_bounds__(CM_WG) void k_cm_count(ChainMultiArgs const A)
{
	__shared__ uint32_t hist[CM_WG / WAVE][CS_BINS];
	CmWg const wg = cm_wg(A);
	if (!wg.ok) return;
	ChainMultiGeom const g = chainmulti_geom(A, wg.chain);
	if (!g.active || A.pass >= g.npass) return;
	uint32_t const lane = lane_id(), wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
	uint32_t const part = wg.x * (CM_WG / WAVE) + wave, m = A.m;
	uint32_t const lo = part * CM_PART;
	if (lo >= m) return;
	uint32_t const hi = min(m, lo + CM_PART);
	uint32_t const *rk = A.rank + (size_t) g.b * m;
	uint32_t const shift = A.pass * g.db;
	for (uint32_t b = lane; b < g.nbins; b += 64u) hist[wave][b] = 0;
	auto sweep = [&](auto p4_) {
		using P = CmPair<decltype(p4_)::value>;
		constexpr uint32_t U = 4;
		for (uint32_t i0 = lo; i0 < hi; i0 += 64u * U)
		{
			typename P::T pr[U];
#pragma unroll
			for (uint32_t u = 0; u < U; ++u) { uint32_t const i = i0 + u * 64u + lane; pr[u] = i < hi ? P::load(g, rk, A.pass, i) : P::none(); }
			if (A.pass == 0u)
			{
				typename P::T *const stage = P::stage(g);
#pragma unroll
				for (uint32_t u = 0; u < U; ++u) { uint32_t const i = i0 + u * 64u + lane; if (i < hi) stage[i] = pr[u]; }
			}
#pragma unroll
			for (uint32_t u = 0; u < U; ++u)
				if (i0 + u * 64u + lane < hi) atomicAdd(&hist[wave][(P::key(g, pr[u]) >> shift) & (g.nbins - 1u)], 1u);
		}
	};
	if (g.p4) sweep(std::true_type{}); else sweep(std::false_type{});
	if (A.pass == 0u)
	{
		uint32_t const nblk = (m + 63u) / 64u;
		for (uint32_t i0 = lo; i0 < hi; i0 += 64u)
		{
			uint32_t const i = i0 + lane;
			uint32_t const v = i < m ? g.d0[i] : 0u;
			uint32_t const pre = wave_incl_max(v);
			uint32_t const rev = (uint32_t) __builtin_amdgcn_ds_bpermute((int) ((63u - lane) << 2), (int) v);
			uint32_t const sufr = wave_incl_max(rev);
			uint32_t const suf = (uint32_t) __builtin_amdgcn_ds_bpermute((int) ((63u - lane) << 2), (int) sufr);
			if (i < m) { g.pm[i] = pre; g.sm[i] = suf; }
			if (lane == 63u && (i0 >> 6) < nblk) g.tab[i0 >> 6] = pre;
		}
	}
	uint32_t *out = g.hist + (size_t) part * CS_BINS;
	for (uint32_t b = lane; b < g.nbins; b += 64u) out[b] = hist[wave][b];
}

// one workgroup per chain: the parts' histograms -> their write offsets (bins ascending, inside a bin the parts ascending);
// first pass: the levels of the sparse table over the block maxima
__global__ __launch_bounds__(ST) void k_cm_offsets(ChainMultiArgs const A)
{
	__shared__ uint32_t scan[ST / WAVE + 1];
	__shared__ uint32_t start_of[CS_BINS];
	ChainMultiGeom const g = chainmulti_geom(A, blockIdx.x);
	if (!g.active || A.pass >= g.npass) return;
	uint32_t const tid = threadIdx.x, m = A.m;
	uint32_t const nparts = chainmulti_parts(m);
	// (a thread per bin walks the parts in batches of independent loads: one load per round trip to L2 made this kernel --
	// a single workgroup per chain -- the longest of a step)
	constexpr uint32_t PB = 16;
	uint32_t tot = 0;
	if (tid < g.nbins)
		for (uint32_t p0 = 0; p0 < nparts; p0 += PB)
		{
			uint32_t c[PB];
#pragma unroll
			for (uint32_t q = 0; q < PB; ++q) c[q] = p0 + q < nparts ? g.hist[(size_t) (p0 + q) * CS_BINS + tid] : 0u;
#pragma unroll
			for (uint32_t q = 0; q < PB; ++q) tot += c[q];
		}
	uint32_t all;
	uint32_t const start = block_excl_add<ST>(tid < g.nbins ? tot : 0u, scan, &all);
	(void) start_of;
	if (tid < g.nbins)
	{
		uint32_t run = start;
		for (uint32_t p0 = 0; p0 < nparts; p0 += PB)
		{
			uint32_t c[PB];
#pragma unroll
			for (uint32_t q = 0; q < PB; ++q) c[q] = p0 + q < nparts ? g.hist[(size_t) (p0 + q) * CS_BINS + tid] : 0u;
#pragma unroll
			for (uint32_t q = 0; q < PB; ++q)
			{
				if (p0 + q < nparts) g.hist[(size_t) (p0 + q) * CS_BINS + tid] = run;
				run += c[q];
			}
		}
	}
	if (A.pass == 0u)
	{
		uint32_t const nblk = (m + 63u) / 64u;
		for (uint32_t k = 1; k < CS_LEVELS && (1u << k) <= nblk; ++k)
		{
			__syncthreads();
			uint32_t const *lo = g.tab + (size_t) (k - 1u) * nblk;
			uint32_t *hi = g.tab + (size_t) k * nblk;
			for (uint32_t j = tid; j + (1u << k) <= nblk; j += ST) hi[j] = max(lo[j], lo[j + (1u << (k - 1u))]);
		}
	}
}

// scatter sweep of pass A.pass: every part in order, the rows of a 64-row group that share a digit found by ballots
__global__ __launch_bounds__(CM_WG) void k_cm_scatter(ChainMultiArgs const A)
{
	__shared__ uint32_t offs[CM_WG / WAVE][CS_BINS];
	CmWg const wg = cm_wg(A);
	if (!wg.ok) return;
	ChainMultiGeom const g = chainmulti_geom(A, wg.chain);
	if (!g.active || A.pass >= g.npass) return;
	uint32_t const lane = lane_id(), wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
	uint32_t const part = wg.x * (CM_WG / WAVE) + wave, m = A.m;
	uint32_t const lo = part * CM_PART;
	if (lo >= m) return;
	uint32_t const hi = min(m, lo + CM_PART);
	uint32_t const *rk = A.rank + (size_t) g.b * m;
	uint32_t const shift = A.pass * g.db;
	uint32_t const *in_offs = g.hist + (size_t) part * CS_BINS;
	for (uint32_t b = lane; b < g.nbins; b += 64u) offs[wave][b] = in_offs[b];
	auto sweep = [&](auto p4_) {
		using P = CmPair<decltype(p4_)::value>;
		typename P::T *dst = ((g.npass - A.pass) & 1u) ? P::bufB(g) : P::bufA(g);
		constexpr uint32_t U = 4;
		for (uint32_t i0 = lo; i0 < hi; i0 += 64u * U)
		{
			typename P::T pr[U];
#pragma unroll
			for (uint32_t u = 0; u < U; ++u)
			{
				uint32_t const i = i0 + u * 64u + lane;
				pr[u] = i < hi ? (A.pass == 0u ? P::stage(g)[i] : P::load(g, rk, A.pass, i)) : P::none();
			}
#pragma unroll
			for (uint32_t u = 0; u < U; ++u)
			{
				bool const in = i0 + u * 64u + lane < hi;
				uint32_t const dg = (P::key(g, pr[u]) >> shift) & (g.nbins - 1u);
				uint64_t const same = cs_match(dg, in, g.db);
				uint32_t const below = cs_below(same);
				uint32_t const base = offs[wave][dg];
				if (in) dst[base + below] = pr[u];
				// (the read above and this write are LDS operations of one wave: they execute in order)
				if (in && below == 0u) offs[wave][dg] = base + (uint32_t) __popcll(same);
			}
		}
	};
	if (g.p4) sweep(std::true_type{}); else sweep(std::false_type{});
}

// the new order of every chain (and out_state behind the block, where the contract asks for it)
__global__ __launch_bounds__(CM_WG) void k_cm_output(ChainMultiArgs const A)
{
	CmWg const wg = cm_wg(A);
	if (!wg.ok) return;
	ChainMultiGeom const g = chainmulti_geom(A, wg.chain);
	if (!g.active) return;
	uint32_t const m = A.m, p = wg.x * CM_WG + threadIdx.x;
	if (p >= m) return;
	uint32_t const nblk = (m + 63u) / 64u;
	uint32_t const *kd = A.keyd + (size_t) g.b * m;
	uint32_t key_me, key_pv, pos_me, pos_pv, row;
	if (g.p4)
	{
		using P = CmPair<true>;
		P::T const me = P::bufB(g)[p], pv = P::bufB(g)[p ? p - 1u : 0u];
		key_me = P::key(g, me); key_pv = P::key(g, pv); pos_me = P::pos(g, me); pos_pv = P::pos(g, pv); row = P::row(g, me);
	}
	else
	{
		using P = CmPair<false>;
		P::T const me = P::bufB(g)[p], pv = P::bufB(g)[p ? p - 1u : 0u];
		key_me = P::key(g, me); key_pv = P::key(g, pv); pos_me = P::pos(g, me); pos_pv = P::pos(g, pv); row = P::row(g, me);
	}
	bool const first = p == 0u || key_pv != key_me;
	uint32_t dv;
	if (first) dv = kd[key_me];
	else
	{
		uint32_t const lo = pos_pv + 1u, hi = pos_me;                     // max of d0[lo .. hi], lo <= hi
		uint32_t const bl = lo >> 6, bh = hi >> 6;
		if (bl == bh)
		{
			dv = g.d0[hi];
			for (uint32_t i = lo; i < hi; ++i) dv = max(dv, g.d0[i]);
		}
		else
		{
			dv = max(g.sm[lo], g.pm[hi]);
			if (bh > bl + 1u)
			{
				uint32_t const k = 31u - (uint32_t) __builtin_clz(bh - bl - 1u);
				uint32_t const *t = g.tab + (size_t) k * nblk;
				dv = max(dv, max(t[bl + 1u], t[bh - (1u << k)]));
			}
		}
	}
	g.a1[p] = row; g.d1[p] = dv;
	uint32_t const grp = wg.chain + A.grp0;
	uint32_t const b1 = min(A.nb_total, grp * A.G + A.G);
	// out_state: the state in front of every block of the chain, and behind the last block of the whole sequence
	if (A.out_state_a && (g.b + 1u < b1 || g.b + 1u == A.nb_total))
	{
		A.out_state_a[(size_t) (g.b + 1u) * m + p] = row; A.out_state_d[(size_t) (g.b + 1u) * m + p] = dv;
	}
}

// the chains' composite key blocks (rank / keyd / nkeys of the order behind the last block of every chain)
__global__ __launch_bounds__(ST) void k_cm_emit(ChainMultiArgs const A, uint32_t steps_done)
{
	extern __shared__ __attribute__((aligned(16))) char smem[];
	Carver cv{smem};
	StreamLds &L = *cv.take<StreamLds>(1);
	uint32_t const chain = blockIdx.x, grp = chain + A.grp0, m = A.m;
	uint32_t const b0 = grp * A.G;
	if (b0 >= A.nb_total) return;
	uint32_t const b1 = min(A.nb_total, b0 + A.G);
	uint32_t const cur = (b1 - b0) & 1u;                          // the chain made b1 - b0 steps
	(void) steps_done;
	uint32_t const *w = A.ws + (size_t) chain * chainsort_ws_words(m);
	uint32_t const *a = w + (size_t) cur * 2u * m, *d = a + m;
	uint32_t const kstart = (uint32_t) ((uint64_t) b0 * A.cols_per_block);
	stream_emit_ranks(m, a, d, kstart, A.out_rank + (size_t) grp * m, A.out_keyd + (size_t) grp * m, A.out_nkeys + grp, L.red);
}

// ================================================================================================
// [r14] A wide level's chains on ONE workgroup each.  Where a launch has a chain per CU and more (level 0 of phase B's
// recursion: BASELINE C4, 256 chains of 24 blocks) the chip is full without spreading a step over it, and a workgroup that
// owns its chain can do what the spread kernels cannot without chip-wide hand-overs: look at the step's data and move RUNS.
// The order in front of a block is a pBWT order, so behind the chain's first step the rows of one key lie in a few runs of
// consecutive positions (C4: ~8,000 runs of ~12 rows a step, but for the block with a recombination point of the founders).
// k_chain_wg walks a chain's steps in one launch, chains taken by a fixed stride, and decides per step on device data:
//   * from the identity (the first step of a chain without a start state): a0[i] = i, d0 = kstart -- the rows are sorted by
//     rank[i] itself, the first row of a key takes keyd[key], every other kstart: no gather through a0, no range maxima;
//   * by runs, where a key and a position share a word and the step has at most run_cap runs: the keys rank[a0[i]] are gathered
//     once; one descriptor per run {key << pb | start, run index}, the run's start and -- in the sweep that reads d0 -- its
//     maximum of d0; the descriptors sorted by key (pass2_sort), prefix sums of their lengths, the new order written run by run:
//     inside a run a' and d' are copies of consecutive old positions, a head takes keyd[key] or max(d0[its own position], the
//     maxima of the whole runs between the previous run of its key and itself) -- a range maximum over RUN indices: prefix /
//     suffix maxima inside blocks of 64 runs and a sparse table over the blocks (a few hundred KB of the workspace);
//   * by sorting the rows otherwise: pass 2's radix step (pass2_records, pass2_sort, pass2_place) on the gathered keys.
// An expansion writes a step's output once, into out_state, and the next step reads it there; a composition ping-pongs in the
// workspace and emits the chain's composite key block itself.
// ================================================================================================
// One workgroup of ST = 1,024 threads a CU: the step's code (pass 2's, for ST threads) takes up to 128 registers a thread without
// scratch, which is what sixteen waves a CU leave each of them; two such workgroups a CU would have to live in 64 (180 registers
// spilled, profiles/r14_kernel_resource_usage.txt).  The one workgroup has the CU's 160 KiB of LDS to itself: 16,384 runs take 128 KiB.
constexpr uint32_t CW_RUN_CAP = 16384;           // most runs of a step on the run path (off + dlt: 8 bytes a run)
constexpr uint32_t CW_RBLK = CW_RUN_CAP / 64;    // blocks of 64 runs
constexpr uint32_t CW_RLEVELS = 9;               // sparse table over at most 2^8 blocks of runs: levels 0 .. 8
static_assert(CW_RUN_CAP % 64u == 0u && CW_RBLK <= (1u << (CW_RLEVELS - 1u)), "the table over the blocks of runs");

struct ChainWgLds {
	uint32_t scan[ST / WAVE + 1];
	union {
		struct {
			uint32_t hist[ST / WAVE][CS_BINS];   // per wave: digit counts, then the wave's write offsets
			uint32_t total[CS_BINS];
		};
		struct {                                 // the run path's output sweep
			union {
				RunSelect sel;                   // the runs' first new positions, runs by (key, start): up to SEL_ROWS rows a bitmap ...
				uint32_t off[CW_RUN_CAP + 1];    // ... above, the positions themselves, m behind the last: a search per position
			};
			uint32_t dlt[CW_RUN_CAP];            // a run's first old position less its first new one (modulo 2^32)
		};
	};
};
static_assert(sizeof(ChainWgLds) + 16u <= 160u * 1024u, "a workgroup a CU");

__host__ __device__ inline size_t chainwg_lds_bytes() { return carve_bytes(1, sizeof(ChainWgLds)); }

// workspace words of one workgroup, every part 16-byte aligned: records (4 words a row) | pairs B | pairs A (2 words a row each) |
// the state, twice (a, d) | keys | the table over the 64-blocks of d0 | the runs: start, maximum, prefix and suffix maxima, the heads'
// divergences, table
__host__ __device__ inline size_t chainwg_ws_rows(uint32_t m) { return ((size_t) m + 3) & ~size_t(3); }
__host__ __device__ inline size_t chainwg_ws_tab(uint32_t m) { return (CS_LEVELS * (((size_t) m + 63) / 64) + 64 + 3) & ~size_t(3); }
__host__ __device__ inline size_t chainwg_ws_words(uint32_t m)
{
	return 13 * chainwg_ws_rows(m) + chainwg_ws_tab(m) + 5 * (size_t) (CW_RUN_CAP + 64) + (size_t) CW_RLEVELS * CW_RBLK;
}
struct ChainWgWs {
	uint4 *rec;
	uint32_t *bufB, *bufA, *state, *keys, *tab;       // state: a, d, a, d of chainwg_ws_rows(m) words each
	uint32_t *rstart, *rmax, *rpre, *rsuf, *rhead, *rtab;
};
__device__ __forceinline__ ChainWgWs chainwg_ws(uint32_t *w, uint32_t m)
{
	size_t const M = chainwg_ws_rows(m);
	ChainWgWs W;
	W.rec = reinterpret_cast<uint4 *>(w);
	W.bufB = w + 4 * M; W.bufA = w + 6 * M;
	W.state = w + 8 * M;
	W.keys = w + 12 * M;
	W.tab = w + 13 * M;
	W.rstart = W.tab + chainwg_ws_tab(m);
	W.rmax = W.rstart + (CW_RUN_CAP + 64); W.rpre = W.rmax + (CW_RUN_CAP + 64); W.rsuf = W.rpre + (CW_RUN_CAP + 64);
	W.rhead = W.rsuf + (CW_RUN_CAP + 64);
	W.rtab = W.rhead + (CW_RUN_CAP + 64);
	return W;
}

// a run's maximum: the word the sweep's atomics built in L2 (a load that does not stop at the CU's vector cache, which may still
// hold the word's line from the step before)
__device__ __forceinline__ uint32_t chainwg_rmax(uint32_t const *rmax, uint32_t k)
{
	return __hip_atomic_load(rmax + k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// max of rmax[lo .. hi] (run indices, lo <= hi < R)
__device__ __forceinline__ uint32_t chainwg_run_max(uint32_t lo, uint32_t hi, uint32_t R, ChainWgWs const &W)
{
	uint32_t const bl = lo >> 6, bh = hi >> 6;
	if (bl == bh)
	{
		if ((lo & 63u) == 0u) return W.rpre[hi];
		if ((hi & 63u) == 63u || hi + 1u == R) return W.rsuf[lo];
		uint32_t v = 0;
		for (uint32_t k = lo; k <= hi; ++k) v = max(v, chainwg_rmax(W.rmax, k));
		return v;
	}
	uint32_t v = max(W.rsuf[lo], W.rpre[hi]);
	if (bh > bl + 1u)
	{
		uint32_t const k = 31u - (uint32_t) __builtin_clz(bh - bl - 1u);
		uint32_t const *t = W.rtab + (size_t) k * CW_RBLK;
		v = max(v, max(t[bl + 1u], t[bh - (1u << k)]));
	}
	return v;
}



// The keys of the old positions, W.keys[i] = rk[a0[i]], and the runs they form, counted on the way: position i starts a run where
// its key is not the key at i - 1.  A wave sweeps its chunk in order (the key in front of a group of 64: the last lane of the group
// before; in front of the chunk: looked up).  *R: the runs of the step; returns the runs in front of this wave's chunk.  Ends with
// a barrier.  hk (or nullptr): where the step hands its keys over to pass 2, 16 bits a row, beside W.keys.
__device__ __forceinline__ uint32_t chainwg_keys(uint32_t m, uint32_t const *__restrict__ rk, uint32_t const *a0, ChainWgWs const &W, ChainWgLds &S, uint16_t *hk,
                                                 uint32_t *R)
{
	uint32_t const tid = threadIdx.x, lane = lane_id();
	uint32_t const wave = __builtin_amdgcn_readfirstlane(tid >> 6);
	constexpr uint32_t NW = ST / WAVE;
	uint32_t const per = ((m + NW - 1u) / NW + 63u) & ~63u;
	uint32_t const c_lo = min(m, wave * per), c_hi = min(m, c_lo + per);
	uint32_t prev = 0xFFFFFFFFu;                                          // (no key: position 0 starts a run)
	if (c_lo > 0u && c_lo < c_hi) prev = rk[a0[c_lo - 1u]];
	uint32_t k0 = 0;
	for (uint32_t i0 = c_lo; i0 < c_hi; i0 += 64u * CW_U)
	{
		uint32_t av[CW_U], kv[CW_U];
#pragma unroll
		for (uint32_t u = 0; u < CW_U; ++u) { uint32_t const i = i0 + u * 64u + lane; av[u] = i < c_hi ? a0[i] : 0u; }
#pragma unroll
		for (uint32_t u = 0; u < CW_U; ++u) { uint32_t const i = i0 + u * 64u + lane; kv[u] = i < c_hi ? rk[av[u]] : 0u; }
#pragma unroll
		for (uint32_t u = 0; u < CW_U; ++u)
		{
			uint32_t const i = i0 + u * 64u + lane;
			if (i0 + u * 64u >= c_hi) break;
			bool const in = i < c_hi;
			if (in) W.keys[i] = kv[u];
			if (hk && in) hk[i] = (uint16_t) kv[u];
			uint32_t const up = shfl_up_u32(kv[u], 1);
			k0 += (uint32_t) __popcll(__ballot(in && kv[u] != (lane ? up : prev)));
			prev = readlane_u32(kv[u], 63);                               // (a group that is not whole is the chunk's last)
		}
	}
	uint32_t const before = block_excl_add<ST>(lane == 0u ? k0 : 0u, S.scan, R);
	__syncthreads();                                                      // (the keys are whole)
	return __builtin_amdgcn_readfirstlane(before);
}

// One step by runs: (a0, d0) -> (a1, d1), the keys of the old positions in W.keys (chainwg_keys: they form R <= CW_RUN_CAP runs, wbase of
// them in front of this wave's chunk), nk keys with divergences kd[key]; the caller has checked that a key and a position share a
// word.  Ends with a barrier.
__device__ __forceinline__ void chainwg_runs(
	uint32_t m, uint32_t const *__restrict__ kd, uint32_t nk, ChainWgWs const &W, ChainWgLds &S, uint32_t R, uint32_t wbase,
	uint32_t const *a0, uint32_t const *d0, uint32_t *a1, uint32_t *d1 FSEQ_RS_PARAM)
{
	uint32_t const tid = threadIdx.x, lane = lane_id();
	uint32_t const wave = __builtin_amdgcn_readfirstlane(tid >> 6);
	constexpr uint32_t NW = ST / WAVE;
	uint32_t const *keys = W.keys;
	uint32_t pb = 1;
	while (pb < 32u && ((m - 1u) >> pb) != 0u) ++pb;
	uint32_t const pmask = (1u << pb) - 1u;                               // (pb < 32: a key shares the word)
	uint32_t const per = ((m + NW - 1u) / NW + 63u) & ~63u;
	uint32_t const c_lo = min(m, wave * per), c_hi = min(m, c_lo + per);
	uint32_t npass, db;
	pass2_digits(nk, npass, db);
	uint2 *const bufA = reinterpret_cast<uint2 *>(W.bufA), *const bufB = reinterpret_cast<uint2 *>(W.bufB);
	uint2 *const pos_order = (npass & 1u) ? bufA : bufB;                  // (the buffer the first pass of the sort does not write)
	bool const by_select = m <= SEL_ROWS;                                 // (the debug entry takes more rows than the bitmap holds)

	// ---- a. one descriptor per run, {key << pb | start, run}, in position order, the runs' starts, and the runs' maxima of d0: a
	// scan inside the group of 64 that does not cross a start, the last lane of every piece to the run's word
	for (uint32_t k = tid; k < R; k += ST) W.rmax[k] = 0u;
	__syncthreads();
	{
		uint32_t prev = 0xFFFFFFFFu;
		if (c_lo > 0u && c_lo < c_hi) prev = keys[c_lo - 1u];
		uint32_t k0 = wbase;
		for (uint32_t i0 = c_lo; i0 < c_hi; i0 += 64u * CW_U)
		{
			uint32_t kv[CW_U], dv[CW_U];
#pragma unroll
			for (uint32_t u = 0; u < CW_U; ++u)
			{
				uint32_t const i = i0 + u * 64u + lane;
				kv[u] = i < c_hi ? keys[i] : 0u;
				dv[u] = i < c_hi ? d0[i] : 0u;
			}
#pragma unroll
			for (uint32_t u = 0; u < CW_U; ++u)
			{
				uint32_t const i = i0 + u * 64u + lane;
				if (i0 + u * 64u >= c_hi) break;
				bool const in = i < c_hi;
				uint32_t const up = shfl_up_u32(kv[u], 1);
				bool const head = in && kv[u] != (lane ? up : prev);
				uint64_t const heads = __ballot(head);
				// the run of this lane: starts counted up to and including it, less one (a group that does not begin with a
				// start continues run k0 - 1: position 0 is a start, so k0 >= 1 there)
				uint32_t const k = k0 + cs_below(heads) + (head ? 1u : 0u) - 1u;
				if (head) { pos_order[k] = make_uint2((kv[u] << pb) | i, k); W.rstart[k] = i; }
				// the lane this lane's piece of its run starts at: the highest start at or below it, else lane 0
				uint64_t const upto = heads & (lane == 63u ? ~0ull : ((2ull << lane) - 1ull));
				uint32_t const s0 = upto ? 63u - (uint32_t) __builtin_clzll(upto) : 0u;
				uint32_t v = dv[u];
#pragma unroll
				for (uint32_t o = 1; o < 64u; o <<= 1)
				{
					uint32_t const t = shfl_up_u32(v, (int) o);
					if (lane >= s0 + o) v = max(v, t);
				}
				uint64_t const ins = __ballot(in);
				bool const last = in && (lane == 63u || !((ins >> (lane + 1u)) & 1ull) || ((heads >> (lane + 1u)) & 1ull));
				if (last) atomicMax(&W.rmax[k], v);
				k0 += (uint32_t) __popcll(heads);
				prev = readlane_u32(kv[u], 63);
			}
		}
	}
	if (tid == 0u) W.rstart[R] = m;
	__syncthreads();
	FSEQ_RS_MARK(1);

	// ---- b. prefix and suffix maxima of the runs' maxima inside blocks of 64 runs, a sparse table over the blocks
	uint32_t const nrb = (R + 63u) / 64u;
	for (uint32_t blk = wave; blk < nrb; blk += NW)
	{
		uint32_t const k = blk * 64u + lane;
		uint32_t const v = k < R ? chainwg_rmax(W.rmax, k) : 0u;
		uint32_t const pre = wave_incl_max(v);
		uint32_t const rev = (uint32_t) __builtin_amdgcn_ds_bpermute((int) ((63u - lane) << 2), (int) v);
		uint32_t const sufr = wave_incl_max(rev);
		uint32_t const suf = (uint32_t) __builtin_amdgcn_ds_bpermute((int) ((63u - lane) << 2), (int) sufr);
		if (k < R) { W.rpre[k] = pre; W.rsuf[k] = suf; }
		if (lane == 63u) W.rtab[blk] = pre;
	}
	__syncthreads();
	for (uint32_t k = 1; k < CW_RLEVELS && (1u << k) <= nrb; ++k)
	{
		uint32_t const *lo = W.rtab + (size_t) (k - 1u) * CW_RBLK;
		uint32_t *hi = W.rtab + (size_t) k * CW_RBLK;
		for (uint32_t j = tid; j + (1u << k) <= nrb; j += ST) hi[j] = max(lo[j], lo[j + (1u << (k - 1u))]);
		__syncthreads();
	}
	FSEQ_RS_MARK(2);

	// ---- c. the runs by (key, start): a stable sort by key of descriptors that are in start order
	pass2_sort<uint2>(R, npass, db, [&](uint32_t i) -> uint2 { return pos_order[i]; }, [&](uint2 x) -> uint32_t { return x.x >> pb; },
	                  make_uint2(0u, 0u), bufA, bufB, S);
	FSEQ_RS_MARK(3);
	// their first new positions: the prefix sum of their lengths (a thread takes consecutive runs, all its loads at once)
	{
		constexpr uint32_t Q = CW_RUN_CAP / ST;
		static_assert(Q * ST == CW_RUN_CAP, "a thread's runs");
		uint32_t const q = (R + ST - 1u) / ST, j0 = min(R, tid * q), j1 = min(R, j0 + q);
		uint32_t st[Q], len[Q];
#pragma unroll
		for (uint32_t t = 0; t < Q; ++t)
		{
			uint2 const x = j0 + t < j1 ? bufB[j0 + t] : make_uint2(0u, 0u);
			st[t] = x.x & pmask; len[t] = x.y;
		}
#pragma unroll
		for (uint32_t t = 0; t < Q; ++t) len[t] = j0 + t < j1 ? W.rstart[len[t] + 1u] - st[t] : 0u;
		uint32_t sum = 0;
#pragma unroll
		for (uint32_t t = 0; t < Q; ++t) sum += len[t];
		// (the sort's last barrier is behind every use of the histograms, which these arrays lie over)
		if (by_select) sel_clear(S.sel, m);
		uint32_t all;
		uint32_t at = block_excl_add<ST>(sum, S.scan, &all);
#pragma unroll
		for (uint32_t t = 0; t < Q; ++t)
			if (j0 + t < j1)
			{
				if (by_select) sel_set(S.sel, at); else S.off[j0 + t] = at;
				S.dlt[j0 + t] = st[t] - at; at += len[t];
			}
		if (by_select) sel_scan(S.sel, m, S.scan);
		else if (tid == 0u) S.off[R] = m;
	}
#ifdef FSEQ_RUN_STAMPS
	__syncthreads();
#endif
	FSEQ_RS_MARK(4);

	// ---- d. the divergence of every run's head: the key's where the run is the key's first, else the maximum of its own d0 and of
	// the whole runs between the run before it (same key) and itself
	{
		constexpr uint32_t UH = 4;
		for (uint32_t j0 = tid; j0 < R; j0 += ST * UH)
		{
			uint2 me[UH], pv[UH];
			uint32_t hv[UH];
#pragma unroll
			for (uint32_t u = 0; u < UH; ++u)
			{
				uint32_t const j = min(j0 + u * ST, R - 1u);
				me[u] = bufB[j]; pv[u] = bufB[j ? j - 1u : 0u];
			}
#pragma unroll
			for (uint32_t u = 0; u < UH; ++u)
			{
				uint32_t const j = j0 + u * ST;
				hv[u] = 0u;
				if (j >= R) continue;
				if (j == 0u || (pv[u].x >> pb) != (me[u].x >> pb)) hv[u] = kd[me[u].x >> pb];
				else
				{
					hv[u] = d0[me[u].x & pmask];
					uint32_t const k_lo = pv[u].y + 1u, k_me = me[u].y;          // (k_lo < k_me: neighbouring runs differ in key)
					if (k_lo < k_me) hv[u] = max(hv[u], chainwg_run_max(k_lo, k_me - 1u, R, W));
				}
			}
#pragma unroll
			for (uint32_t u = 0; u < UH; ++u) { uint32_t const j = j0 + u * ST; if (j < R) W.rhead[j] = hv[u]; }
		}
	}
	__syncthreads();
	FSEQ_RS_MARK(5);

	// ---- e. the new order: position p lies in the run j the bitmap gives (more than SEL_ROWS rows: the one with off[j] <= p <
	// off[j + 1]) and takes the row at old position p + dlt[j]; behind the run's head its divergence too, the head the one of d.
	uint32_t top = 1;
	while (top * 2u < R) top *= 2u;
	for (uint32_t p0 = tid; p0 < m; p0 += ST * CW_U)
	{
		uint32_t jh[CW_U], hh[CW_U], av[CW_U], dv[CW_U];
		if (by_select)
		{
#pragma unroll
			for (uint32_t u = 0; u < CW_U; ++u)
			{
				uint32_t const p = p0 + u * ST;
				bool head;
				uint32_t const j = sel_run(S.sel, p, m, &head);
				hh[u] = p < m ? p + S.dlt[j] : 0u;
				jh[u] = head && p < m ? j : 0xFFFFFFFFu;
			}
		}
		else
		{
#pragma unroll
			for (uint32_t u = 0; u < CW_U; ++u)
			{
				uint32_t const p = min(p0 + u * ST, m - 1u);
				uint32_t j = 0;
				for (uint32_t step = top; step; step >>= 1) { uint32_t const t = j + step; if (t < R && S.off[t] <= p) j = t; }
				hh[u] = p + S.dlt[j];
				jh[u] = S.off[j] == p ? j : 0xFFFFFFFFu;
			}
		}
#pragma unroll
		for (uint32_t u = 0; u < CW_U; ++u) { av[u] = a0[hh[u]]; dv[u] = jh[u] != 0xFFFFFFFFu ? W.rhead[jh[u]] : d0[hh[u]]; }
#pragma unroll
		for (uint32_t u = 0; u < CW_U; ++u)
		{
			uint32_t const p = p0 + u * ST;
			if (p < m) { a1[p] = av[u]; d1[p] = dv[u]; }
		}
	}
	__syncthreads();
	FSEQ_RS_MARK(6);
}

// One step by the sort of all its rows: the keys from W.keys (ident: from rk itself -- the order is the identity, every divergence
// kstart, and neither records nor range maxima are needed).  Ends with a barrier.
template <bool P4>
__device__ __forceinline__ void chainwg_sort(
	uint32_t m, uint32_t const *__restrict__ rk, uint32_t const *__restrict__ kd, uint32_t nk, ChainWgWs const &W, ChainWgLds &S, bool ident, uint32_t kstart,
	uint32_t const *a0, uint32_t const *d0, uint32_t *a1, uint32_t *d1)
{
	using PairT = std::conditional_t<P4, uint32_t, uint2>;
	uint32_t pb = 1;
	while (pb < 32u && ((m - 1u) >> pb) != 0u) ++pb;
	uint32_t const pmask = pb < 32u ? (1u << pb) - 1u : 0xFFFFFFFFu;
	auto mk = [&](uint32_t key, uint32_t pos) -> PairT { if constexpr (P4) return (key << pb) | pos; else return make_uint2(key, pos); };
	auto key_of = [&](PairT pr) -> uint32_t { if constexpr (P4) return pr >> pb; else return pr.x; };
	auto pos_of = [&](PairT pr) -> uint32_t { if constexpr (P4) return pr & pmask; else return pr.y; };
	uint32_t npass, db;
	pass2_digits(nk, npass, db);
	PairT *const bufA = reinterpret_cast<PairT *>(W.bufA), *const bufB = reinterpret_cast<PairT *>(W.bufB);
	if (ident)
	{
		pass2_sort<PairT, CW_U>(m, npass, db, [&](uint32_t i) -> PairT { return mk(rk[i], i); }, key_of, mk(0u, 0u), bufA, bufB, S);
		for (uint32_t p0 = threadIdx.x; p0 < m; p0 += ST * CW_U)
		{
			PairT me[CW_U], pv[CW_U];
			uint32_t dv[CW_U];
#pragma unroll
			for (uint32_t u = 0; u < CW_U; ++u) { uint32_t const p = min(p0 + u * ST, m - 1u); me[u] = bufB[p]; pv[u] = bufB[p ? p - 1u : 0u]; }
#pragma unroll
			for (uint32_t u = 0; u < CW_U; ++u)
			{
				uint32_t const p = p0 + u * ST;
				dv[u] = (p < m && (p == 0u || key_of(pv[u]) != key_of(me[u]))) ? kd[key_of(me[u])] : kstart;
			}
#pragma unroll
			for (uint32_t u = 0; u < CW_U; ++u) { uint32_t const p = p0 + u * ST; if (p < m) { a1[p] = pos_of(me[u]); d1[p] = dv[u]; } }
		}
		__syncthreads();
		return;
	}
	uint32_t const *keys = W.keys;
	pass2_records(m, a0, d0, W.rec, W.tab);
	pass2_sort<PairT, CW_U>(m, npass, db, [&](uint32_t i) -> PairT { return mk(keys[i], i); }, key_of, mk(0u, 0u), bufA, bufB, S);
	pass2_place<P4>(m, kd, bufB, W.rec, W.tab, d0, a1, d1);
}

// stats (CW_STATS words, fseq_types.hpp; nullptr: none kept): steps by runs, steps by the sort of the rows, steps from the identity,
// the most runs a step had (of the steps that may go by runs: the knob is not 0, a key and a position share a word), those steps
// by the power of two their run count reaches
__global__ __launch_bounds__(ST) void k_chain_wg(ChainMultiArgs const A, uint32_t *ws, uint32_t run_cap, uint32_t *stats)
{
	extern __shared__ __attribute__((aligned(16))) char smem[];
	ChainWgLds &S = *reinterpret_cast<ChainWgLds *>(smem);
	uint32_t const tid = threadIdx.x, m = A.m;
	ChainWgWs const W = chainwg_ws(ws + (size_t) blockIdx.x * chainwg_ws_words(m), m);
	uint32_t pbits = 1;
	while (pbits < 32u && ((m - 1u) >> pbits) != 0u) ++pbits;
#ifdef FSEQ_RUN_STAMPS
	RunStamps rs;
#endif
	for (uint32_t chain = blockIdx.x; chain < A.nchains; chain += gridDim.x)
	{
		uint32_t const grp = chain + A.grp0;
		uint32_t const b0 = grp * A.G;
		if (b0 >= A.nb_total) continue;
		uint32_t const b1 = min(A.nb_total, b0 + A.G);
		uint32_t const kstart = (uint32_t) ((uint64_t) b0 * A.cols_per_block);
#ifdef FSEQ_RUN_STAMPS
		rs.clear();
		unsigned long long rs_runs = 0;
#endif
		// the state in front of the chain: the caller's, or the identity (never stored unless out_state asks for it)
		bool ident = A.start_a == nullptr;
		uint32_t const *a0 = ident ? nullptr : A.start_a + (size_t) grp * m, *d0 = ident ? nullptr : A.start_d + (size_t) grp * m;
		if (A.out_state_a)
			for (uint32_t i = tid; i < m; i += ST)
			{
				A.out_state_a[(size_t) b0 * m + i] = ident ? i : a0[i];
				A.out_state_d[(size_t) b0 * m + i] = ident ? kstart : d0[i];
			}
		uint32_t pp = 0;
		for (uint32_t b = b0; b < b1; ++b)
		{
			// (an expansion -- states wanted, no composite keys -- does not step through a chain's last block unless that is the last
			// of all: the state behind it is the next chain's start state, chainmulti_geom)
			bool const keep = b + 1u < b1 || b + 1u == A.nb_total;
			if (!A.out_rank && !keep) break;
			uint32_t *a1, *d1;
			if (A.out_state_a && keep) { a1 = A.out_state_a + (size_t) (b + 1u) * m; d1 = A.out_state_d + (size_t) (b + 1u) * m; }
			else { a1 = W.state + (size_t) pp * 2u * chainwg_ws_rows(m); d1 = a1 + chainwg_ws_rows(m); pp ^= 1u; }
			uint32_t const *rk = A.rank + (size_t) b * m, *kd = A.keyd + (size_t) b * m;
			uint32_t const nk = A.nkeys[b];
			uint32_t kb = 1;
			while (kb < 32u && ((nk - 1u) >> kb) != 0u) ++kb;
			bool const p4 = kb + pbits <= 32u;
			uint32_t nrun = 0;
			bool by_runs = false;
			// [r15] the hand-over to pass 2 (A.hand_keys: the host sets it for the expansion of the alignment's own blocks alone): this step
			// goes through block b from the exact state in front of it, so its keys rk[a0[i]] are pass 2's r of the block, word for
			// word.  Not from the identity (the keys are rk itself) and not where a key does not fit 16 bits: the flag stays clear
			uint16_t *const hk = A.hand_keys && A.out_state_a && !A.out_rank && !ident && nk <= 65536u ? A.hand_keys + (size_t) b * m : nullptr;
			if (!ident)
			{
				// the keys in the order in front of the block, once for the step, and their runs
				uint32_t R = 0;
#ifdef FSEQ_RUN_STAMPS
				RunStamps const rs_before = rs;
				rs.start();
#endif
				uint32_t const wbase = chainwg_keys(m, rk, a0, W, S, hk, &R);
				FSEQ_RS_MARK(0);
				bool const may = run_cap != 0u && p4;
				nrun = may ? R : 0u;
				by_runs = may && R <= run_cap;
				if (by_runs) chainwg_runs(m, kd, nk, W, S, R, wbase, a0, d0, a1, d1 FSEQ_RS_ARG);
#ifdef FSEQ_RUN_STAMPS
				if (by_runs) { ++rs.steps; rs_runs += R; }
				else rs = rs_before;                                          // (a step that sorts its rows: not in the sums)
#endif
			}
			if (!by_runs)
			{
				if (p4) chainwg_sort<true>(m, rk, kd, nk, W, S, ident, kstart, a0, d0, a1, d1);
				else chainwg_sort<false>(m, rk, kd, nk, W, S, ident, kstart, a0, d0, a1, d1);
			}
			if (hk && tid == 0u) A.hand_flag[b] = 1u;                         // (behind the step's last barrier: the keys are whole)
			if (stats && tid == 0)
			{
				atomicAdd(stats + (ident ? 2 : by_runs ? 0 : 1), 1u);
				if (nrun)
				{
					atomicMax(stats + 3, nrun);
					atomicAdd(stats + 4 + min(P2_HIST - 1u, nrun > 1u ? 32u - (uint32_t) __builtin_clz(nrun - 1u) : 0u), 1u);
				}
			}
			ident = false;
			a0 = a1; d0 = d1;
		}
#ifdef FSEQ_RUN_STAMPS
		if (tid == 0 && (blockIdx.x & 63u) == 0u && chain == blockIdx.x && rs.steps != 0u)
			printf("cw run stamps workgroup %u chain %u (%u rows, %s, %u steps by runs of %llu runs on average), per step by runs: keys and run count %llu, "
			       "a descriptors and maxima %llu, b table %llu, c descriptor sort %llu, prefix sums %llu, d heads %llu, e new order %llu (x 10 ns)\n",
			       blockIdx.x, chain, m, A.out_rank ? "composition" : "expansion", rs.steps, rs_runs / rs.steps, rs.acc[0] / rs.steps, rs.acc[1] / rs.steps,
			       rs.acc[2] / rs.steps, rs.acc[3] / rs.steps, rs.acc[4] / rs.steps, rs.acc[5] / rs.steps, rs.acc[6] / rs.steps);
#endif
		// the chain's composite key block (a composition steps through every block: a0 is the order behind the last)
		if (A.out_rank)
		{
			stream_emit_ranks(m, a0, d0, kstart, A.out_rank + (size_t) grp * m, A.out_keyd + (size_t) grp * m, A.out_nkeys + grp, S.scan);
			__syncthreads();
		}
	}
}

} // namespace fseq
