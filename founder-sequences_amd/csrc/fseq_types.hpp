// fseq_types.hpp -- the few plain types the context (fseq_ctx.hpp) holds by value or names in a signature, apart from the
// kernel headers that use them.
#pragma once

#include "fseq_redplan.hpp"     // RED_NONE, and the plan the context holds by value

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

namespace fseq {

// Phase D's arrays (fseq_dp.hpp): M (segment_max_size = the key), LB, SZ per DP entry; K[t]: 64-bit stack mask over the
// 64-block of t; Tb[p][j] / Tbv[p][j]: sparse-table sample (index / key) of rmq.hh's m_precalc[p][j].
struct DpArrays {
	uint32_t *M, *LB, *SZ, *Tb, *Tbv;
	unsigned long long *K;
	uint32_t tstride;
};

// ---- The path's device words (fseq_ctx::d_flags): what the kernels of a run report in single words, every region named here
// and nowhere else.  A kernel keeps its pointer parameter and is handed the address of its own region.
// phase A's counters: the key-space tree's `counters` are the first two, the trie's the third
struct PhaseACounters {
	uint32_t tree_sliced;                // blocks whose merges the key-space tree sliced
	uint32_t tree_given_up;              // blocks it handed to the column sweep
	uint32_t trie_given_up;              // blocks the trie handed to the tree
};
struct PathWords {
	uint32_t dp[4];                      // k_dp's `flags`: bit 0 of [0] = a list too short to prove a cell, [1] = the lowest entry read; cleared and read as 16 bytes
	PhaseACounters phase_a;
	uint32_t dense_columns;              // k_column_presence: columns with at most four codes
	// diagnostic builds, behind the production words: -DFSEQ_DP_STAMPS (cycle stamps, 3 per wave: the waves' own schedule, then
	// the classic one), -DFSEQ_DP_STATS (list entries a cell needed: 0 .. 32, more)
	unsigned long long dp_stamps[96];
	uint32_t dp_hist[34];
};
// what the diagnostic k_dp adds to its `flags` (= PathWords::dp), in words: the kernel and the host's read-back use these
constexpr uint32_t DP_STAMPS_AT = (uint32_t) ((offsetof(PathWords, dp_stamps) - offsetof(PathWords, dp)) / 4);
constexpr uint32_t DP_HIST_AT = (uint32_t) ((offsetof(PathWords, dp_hist) - offsetof(PathWords, dp)) / 4);
static_assert(offsetof(PathWords, dp) + sizeof(PathWords::dp) <= offsetof(PathWords, phase_a)
              && offsetof(PathWords, phase_a) + sizeof(PhaseACounters) <= offsetof(PathWords, dense_columns)
              && offsetof(PathWords, dense_columns) + 4 <= offsetof(PathWords, dp_stamps)
              && offsetof(PathWords, dp_stamps) + sizeof(PathWords::dp_stamps) <= offsetof(PathWords, dp_hist)
              && offsetof(PathWords, dp_hist) + sizeof(PathWords::dp_hist) <= sizeof(PathWords)
              && offsetof(PathWords, dp_stamps) % 8 == 0, "the path's device words: no region overlaps another");

// the two words behind d_red_invalid[nblocks] (red_flags, fseq_path.hpp): k_reduce_prep clears both, the reduced column kernels
// set the first with invalid[b], k_reduce_check the second
struct RedFlags {
	uint32_t unproven;                   // a block's lists took an entry its representatives cannot vouch for
	uint32_t plan_stale;                 // the counts are not the ones the plan was made from
};

// what an attempt reads back at its end (pinned, run_long_path)
struct AttemptWords {
	uint32_t dp[4];
	PhaseACounters phase_a;
	RedFlags red;
};

// ---- What the launchers of the path take (the kernel tables of fseq_ctx.hpp, the launch_* functions): plain host-side views
// of a context's buffers and geometry.  A kernel's positional parameter list is written out at one place, its launcher, from
// these by name; the kernels themselves keep their scalar and __restrict__ pointer parameters (fseq_path.hpp builds the
// views of a context).

// bytes of m rows of a packed column: 8 >> bsh bits per dense symbol code (the storage: fseq_kernels.hpp)
__host__ __device__ inline uint32_t sym_bytes(uint32_t m, uint32_t bsh) { return (m + (1u << bsh) - 1u) >> bsh; }

// the alignment as a kernel sees it: column k at msa + k * ld, in nblocks blocks of B columns
struct MsaArgs {
	uint8_t const *msa = nullptr;
	size_t ld = 0;
	uint32_t m = 0;
	uint64_t n = 0;
	uint32_t B = 0, nblocks = 0;
	uint32_t N2 = 0;                     // slots of the sort in k_columns' prologue (the power of two above m)
	uint32_t npass = 1, bsh = 0;         // digit passes of a column; packing: 8 >> bsh bits per symbol
};

// the lists of phase C: column k at ent + k * stride, its header at hdr + k
struct ListArgs {
	uint32_t L = 0, X = 0, stride = 0;   // segment length, list capacity, entries between two columns' lists
	uint2 *ent = nullptr;
	uint4 *hdr = nullptr;
};

// one launch of k_relump_lists (fseq_lengthscan.hpp): the lists of the columns [k0, k0 + ncols), built or folded at a segment length
// <= lists.L, folded in place to what the DP reads at lists.L (lists.X is not used: the capacity stays what the lists were built at)
struct RelumpArgs {
	ListArgs lists;
	uint64_t k0 = 0, ncols = 0;
};

// the stride states: the state at column q * snap_stride at ss_* + q * (words of a state); phase C drops them, pass 2 starts from them
struct StrideStates {
	uint32_t snap_stride = 0;
	uint32_t *ss_a = nullptr, *ss_d = nullptr;
	uint32_t ss_pack = 0;                // streamed rows: bits of a row id when the states are packed to 5 bytes per row
	bool ids = false;                    // ... and hold value ids, not divergences (the tile step, fseq_stream2.hpp)
};

// phase A: the key blocks a launch writes -- its first block starts at column col0; rank / keyd / nkeys point at that block --
// and what the kernel that writes them works in
struct PhaseAArgs {
	MsaArgs A;
	uint32_t *rank = nullptr, *keyd = nullptr, *nkeys = nullptr;
	uint64_t col0 = 0;
	uint32_t nblk = 0;                   // blocks of the launch (the trie and the streamed tree hand them to their workgroups in turn)
	uint32_t const *only = nullptr;      // per-block filter: a block whose word is zero is skipped (nullptr: every block)
	uint32_t *todo = nullptr;            // per block: set where the kernel gives the block up (the next kernel's `only`)
	uint32_t T = 0;                      // the key-space tree and the trie: threads of a workgroup
	void *work = nullptr;                // ... their scratch (the tree on LDS-resident rows: halfwords; else words), work_per elements a block / a workgroup
	size_t work_per = 0;
	uint32_t cap_words = 0;              // the tree: words of its LDS bitmap
	uint32_t wide = 0;                   // the streamed tree: bit 0 = 32-bit ids from the start, bit 1 = leaves one by one
	uint32_t *counters = nullptr;        // blocks sliced (the tree) / given up (the trie)
	uint8_t *cls = nullptr;              // the trie: the class columns it writes for the blocks it ranks (column k at cls + k * ldc; nullptr: none) ...
	size_t ldc = 0;
	uint32_t *cls_have = nullptr;        // ... and, per block of the launch, 1 where it wrote them
};

// pass 2: the states at the boundaries task_rb, each group of boundaries (task_grp: {first, count}) swept from one start state
// (task_src: a block's boundary state, or -- bit 63 -- a stride state)
struct SnapArgs {
	MsaArgs A;
	uint32_t const *bstate_a = nullptr, *bstate_d = nullptr;
	uint64_t const *task_rb = nullptr;
	uint2 const *task_grp = nullptr;
	uint64_t const *task_src = nullptr;
	uint32_t *snap_a = nullptr, *snap_d = nullptr;       // [boundary][m]
	StrideStates ss;
	uint32_t keyed = 0;                  // LDS-resident rows: what the partition steps scan (scan_keyed)
	uint32_t const *task_blk = nullptr;  // behind the reduced phase C: [boundary] its block (the chain step, k_chain_snap)
	// on the streamed tile step (S2SnapArgs, fseq_stream2.hpp): a workgroup per block that has boundaries
	uint32_t *ws = nullptr;              // the blocks' workspaces (block b at ws + b * words per block)
	uint32_t const *wg_block = nullptr;  // [grid] block of every workgroup
	uint2 const *wg_groups = nullptr;    // [grid] {first group, groups}
	uint32_t const *bs_w = nullptr;      // the blocks' start states in id form
	uint8_t const *bs_h = nullptr;
};

// one launch of phase C on all rows: the blocks block0 .. (or blocklist[i]), from their boundary states
struct ColumnsArgs {
	MsaArgs A;
	uint32_t const *bstate_a = nullptr, *bstate_d = nullptr;
	ListArgs lists;
	StrideStates ss;
	uint32_t *ws = nullptr;              // streamed rows: the blocks' workspaces (block b at ws + b * words per block)
	uint32_t block0 = 0;
	uint32_t *done_host = nullptr;
	uint32_t epoch = 0;
	uint32_t const *blocklist = nullptr; // workgroup i owns block blocklist[i] instead of block0 + i
	uint32_t const *colmask = nullptr;   // 4-bit symbols: the codes present in every column (k_column_presence), or nullptr
};

// One chain launch of phase B: grid chains grp0 .. grp0 + grid - 1, chain g over the key blocks [g * G, min(nb_total, (g + 1) * G))
// of a level; from start_* (nullptr: the identity) to the states in front of every key block (out_state_*) and / or the
// chain's composite key block (out_rank / out_keyd / out_nkeys).  The streamed chain kernels take it as it is (fseq_chainsort.hpp).
struct ChainMultiArgs {
	uint32_t const *rank, *keyd, *nkeys;         // the key blocks of the level below
	uint32_t m, nb_total, G;
	uint64_t cols_per_block;
	uint32_t *ws;                                // [chains of the launch][chainsort_ws_words(m)]
	uint32_t *hist;                              // [chains of the launch][parts][CS_BINS]
	uint32_t const *start_a, *start_d;
	uint32_t *out_state_a, *out_state_d, *out_rank, *out_keyd, *out_nkeys;
	uint32_t grp0;
	uint32_t step;                               // block b0 + step of every chain
	uint32_t pass;                               // radix pass of the sweep kernels
	uint32_t nchains;                            // chains of the launch (the grid's y is rounded up to the XCDs: cm_wg)
	// the hand-over to pass 2 (k_chain_wg alone; nullptr: none): hand_keys[b][m], 16 bits a row, the keys of block b in the order in
	// front of it where hand_flag[b] is set (k_chain_snap_grouped takes them for its r)
	uint16_t *hand_keys;
	uint32_t *hand_flag;
};

// the reduced alignment k_reduce_msa writes: the listed blocks' representative rows (rows[block][cap], cnt[block] of them), column k at red + k * ldr
struct ReducedMsaArgs {
	uint8_t *red = nullptr;
	size_t ldr = 0;
	uint32_t const *cnt = nullptr, *rows = nullptr;
	uint32_t cap = 0;
	uint32_t const *blocks = nullptr;    // [nlisted] the reduced blocks
	uint32_t nlisted = 0, max_rows = 0;  // ... and the most representatives among them
	uint32_t const *flag = nullptr;      // per block, or nullptr: only the listed blocks with flag[block] == want (the others take the other source)
	uint32_t want = 0;
	uint32_t const *pad = nullptr;       // the row whose symbol fills the last byte behind the last representative: pad[block * pad_per] (nullptr: row 0)
	size_t pad_per = 0;
	uint32_t const *skip = nullptr;      // per block, or nullptr: the blocks with skip[block] are left out (from the class columns: the column kernel stages theirs itself)
};

// phase A's class columns (k_blocktrie, fseq_blocktrie.hpp), the other source of the reduced alignment: column k at cls + k * ldc holds at row rho the
// symbol of the block key of rank rho; have[block] = 1 where the block has them; leaf[block][cap]: the rank of every representative's key
struct ClassColumnArgs {
	uint8_t const *cls = nullptr;
	size_t ldc = 0;
	uint32_t const *have = nullptr, *leaf = nullptr;
	uint32_t const *rank = nullptr;      // [block][m]: block-key rank of every row
};

// [r5] Phase C on a block's REPRESENTATIVE rows (fseq_reduced.hpp): what k_reduce_prep left for every block and where a
// workgroup of the reduced column kernel finds it.  Plain pointers into device memory.
constexpr uint32_t P2_HIST = 19;                 // ... tasks by run count: bucket b counts those with more than 2^(b - 1) and at most 2^b runs (bucket 0: one run)
constexpr uint32_t CW_STATS = 4 + P2_HIST;       // counters of phase B's chain-per-workgroup kernel (k_chain_wg): steps by runs, by the sort of the rows, from the identity, the most runs, steps by run count
constexpr uint32_t P2_STATS = 4 + P2_HIST;       // counters of pass 2's streamed chain step (k_chain_snap_grouped; fseq_debug_pass2_paths)
constexpr uint32_t P2_HAND = 2;                  // ... and behind them in the path's buffers: the groups that took phase B's keys, the groups that gathered their own
constexpr uint32_t RED_WIDE = 2u;               // invalid[b]: the block has more distinct start values than its configuration's table holds
struct RedArgs {
	uint32_t const *cnt = nullptr;      // [block] representatives of the block
	uint32_t const *vmin = nullptr;     // [block] the values >= vmin are those of the run on all rows (1: every value is)
	uint32_t const *a = nullptr;        // [block][cap] start state: representative index (place among the block's representatives by row id) ...
	uint32_t const *d = nullptr;        // [block][cap] ... and the maximum of d0 over the positions skipped since the last kept row
	uint32_t const *leaf = nullptr;     // [block][cap] block-key rank of representative i (pass 2)
	uint32_t const *blocks = nullptr;   // [workgroup] block of workgroup i of the launch
	uint32_t *invalid = nullptr;        // [block] 1 when a list of the block took an entry the representatives cannot vouch for (RED_WIDE: see there)
	uint32_t cap = 0;                   // row stride of a / d / leaf (and of cls / headd)
	uint32_t m_true = 0;                // rows of the alignment
	uint32_t direct = 0;                // 1: a[] holds ROW IDS and msa / ld are the alignment itself (its whole column is staged: colbytes);
	                                    // 0: a[] holds representative indices and msa / ld are the reduced alignment (k_reduce_msa)
	uint32_t colbytes = 0;              // direct: bytes of a packed column of the alignment
	uint32_t symcap = 0;                // bytes of each of the two staged-column buffers in LDS (whole kilobytes)
	uint32_t const *rank = nullptr;     // direct, pass 2: [block][m_true] block-key rank of every row (leaf[] is not used)
	uint32_t *any_invalid = nullptr;    // one word: set with invalid[b]
	// [r10] phase A's class columns staged directly (streamed rows; a launch whose staged-column buffers hold a class column: cls_have
	// set): a block with cls_src[b] (the plan: both of its configurations take the class width) and cls_have[b] (this run's phase A
	// wrote its columns) stages column k from cls_msa + k * cls_ld, ceil16(sym_bytes(nkeys[b])) bytes of it, and the ids of its order are
	// leaf[] -- cls[k][leaf[i]] == msa[k][rows[i]] -- so a[] is translated once at the block's first column and the reduced stride
	// states hold leaf ids; every other block reads the reduced alignment by representative index as before
	uint32_t const *cls_have = nullptr, *cls_src = nullptr, *nkeys = nullptr;
	uint8_t const *cls_msa = nullptr;
	size_t cls_ld = 0;
	// pass 2: instead of lists, the class tables at the task columns of the block
	uint32_t const *wg_tasks = nullptr; // [workgroup][3] {first task, tasks, column of the start state (the block's first column, or a stride state's)}
	// the reduced states phase C drops every ss_stride columns (the state at column q * ss_stride at [q][ss_cap], where that
	// column lies strictly inside a block): where pass 2's sweeps start from.  [r16] Two 16-bit arrays: the order as the column
	// kernel holds it, and every divergence as its column into the block (0: at or in front of the block's first column)
	uint16_t *ss_a = nullptr, *ss_d = nullptr;
	uint32_t ss_stride = 0, ss_cap = 0;
	unsigned long long const *task_rb = nullptr;   // [task] column (ascending inside a workgroup)
	uint32_t *cls = nullptr;            // [task][cap] class (rank among the distinct key prefixes) of every block key
	uint32_t *headd = nullptr;          // [task][cap] divergence in front of every class
	uint32_t *ncls = nullptr;           // [task]
};

// what k_reduce_prep reads and leaves (fseq_reduced.hpp)
struct RedPrepArgs {
	uint32_t const *bstate_a, *bstate_d;     // [blocks + 1][m]: the exact states in front of the blocks and behind the last
	uint32_t const *rank;                    // [blocks][m]: block-key rank of every row (phase A)
	uint32_t const *blocks;                  // [workgroup] block of workgroup i, or nullptr: block0 + i
	uint32_t m, B, L, Xp, cap, block0, leaf_only, direct;      // direct: a[] = row ids (else: indices among the block's representatives)
	uint32_t *invalid, *flags;               // invalid[b] = 0; flags[0 .. 1] = 0 (workgroup 0): what the column kernels and the plan check set
	uint64_t n;
	uint32_t *cnt, *vmin, *rows, *leaf, *a, *d;
};

} // namespace fseq
