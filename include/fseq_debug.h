/* fseq_debug.h -- intermediate state of the HIP segmentation path, for parity tests and diagnostics.
 * Not part of the drop-in boundary (include/fseq.h): nothing here replaces a call of the reference; the entry points
 * are exported by the same library. */
#ifndef FSEQ_DEBUG_H
#define FSEQ_DEBUG_H

#include "fseq.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The DP's round schedule (debug / tests of the host logic; no device needed): number of rounds for (L, n),
 * cells per round, and how many leading rounds only need the lists of columns < col_hi (what the host hands
 * to a resumed DP launch while later columns are still being produced). */
int  fseq_debug_dp_schedule(uint64_t segment_length, uint64_t n, uint64_t col_hi, uint32_t *n_rounds, uint32_t *cells_per_round,
                            uint32_t *rounds_within, int *pipelined);
/* Whole DP array (debug / parity of intermediate state): n - L + 1 entries, rb = index + L.
 * A rank of a sharded run computes the entries [*first, *last) (and the final cell's, entry n - L, when *final_cell);
 * since round 4 it holds the other ranks' entries only for a window in front of its own (*whole_arrays == 0), so
 * fseq_debug_dp is meaningful there for its own entries only (FSEQ_SHARD_DP_FULL keeps whole arrays on every rank). */
int  fseq_debug_dp(fseq_ctx *ctx, uint32_t *lb, uint32_t *max_size, uint32_t *size);
int  fseq_debug_dp_owned(fseq_ctx *ctx, uint64_t *first, uint64_t *last, int *final_cell, int *whole_arrays);
/* Exact (a,d) at column block_idx*block_len (block_idx <= n_blocks). */
int  fseq_debug_block_state(fseq_ctx *ctx, uint64_t block_idx, uint32_t *a_out, uint32_t *d_out);
/* Per-column divergence list after column c: descending (value,count), up to list_cap+1 entries;
 * *n_entries, *cnt0 (count of value 0) and *complete (list reaches the smallest value). */
int  fseq_debug_column_list(fseq_ctx *ctx, uint64_t c, uint32_t *values, uint32_t *counts,
                            uint32_t *n_entries, uint32_t *cnt0, uint32_t *complete);
/* What the last run did with the lists (fseq_set_list_memory): bytes of device memory the list buffer held, columns of a
 * window (n when every list was held), windows of pass 1 (1: every list held; 0: short path) and windows the merge's second
 * pass ran again.  After a windowed run only the lists of the window last held are there: fseq_debug_column_list returns
 * FSEQ_E_ARG for any other column. */
int  fseq_debug_list_windows(fseq_ctx *ctx, uint64_t *bytes_held, uint64_t *columns_per_window, uint32_t *windows,
                             uint32_t *merge_windows);

/* The restated rmq.hh (rmq<..., 64>, include/founder_sequences/rmq.hh:61-118, quirks included) on caller-supplied
 * keys, straight on the device routines the DP uses (debug / tests): the stack masks and the sparse table are
 * built in closed form from the keys, every query [beg, end) is answered by the HBM path (index_hbm) and, when
 * the array fits the LDS rings (count <= 4096), by the LDS path (index_lds, else 0xFFFFFFFF). */
int  fseq_debug_rmq(int device, uint32_t const *keys, uint32_t count, uint32_t const *beg, uint32_t const *end, uint32_t n_queries,
                    uint32_t *index_hbm, uint32_t *index_lds);

/* Phase ranges (roctx: rocprofv3 --marker-trace) pushed and popped by this process so far, and whether the library was built
 * against roctx: a run of the long path adds four of each (phases A + B, phases C + D, traceback + merge, pass 2). */
int  fseq_debug_ranges(uint64_t *pushes, uint64_t *pops, int *with_roctx);

/* Diagnostic builds only (-DFSEQ_CLOCK_STAMPS; FSEQ_E_UNSUPPORTED otherwise): the clock phase C's kernel held in the last run,
 * d(s_memtime) / d(s_memrealtime) x 100 MHz stamped once around every workgroup, the median over the workgroups
 * (MI355X_MICROARCH.md, "DVFS give-back" item 6).  tools/clock_probe.py. */
int  fseq_debug_clock(fseq_ctx *ctx, double *ghz, uint32_t *workgroups);

/* The library's diagnostic knobs (FSEQ_* names, listed in csrc/fseq_ctx.hpp `struct Tuning`): a context reads them
 * from the environment once, at fseq_create; this sets one afterwards (value NULL = off).  Every knob selects among
 * exact alternatives; results never depend on them.  Call before the first fseq_run_segmentation (a later call drops the work buffers and
 * the result of the context: the geometry may change -- but for FSEQ_SCAN_REBUILD, which fseq_scan_segment_lengths alone reads); on a sharded context before the input is set, identically on
 * every rank (FSEQ_E_ARG afterwards: the input is laid out for the block partition in force when it was set). */
int  fseq_debug_set_tuning(fseq_ctx *ctx, char const *name, char const *value);

/* Which way the last fseq_join_greedy of the context went (*path): 0 the all-host joiner, 1 the device front with the pair's
 * counters in one LDS matrix (up to 181 classes), 2 the wide device front (strips of left classes; FSEQ_JOIN_WIDE forces it).
 * FSEQ_E_ARG before any fseq_join_greedy has finished. */
int  fseq_debug_join_path(fseq_ctx *ctx, int *path);

/* Which way the last fseq_join_bipartite of the context went (*path): 0 the host joiner, 1 the device form with the pair's
 * weights in LDS (up to 181 texts a segment), 2 the wide device form (weights in slabs of device memory, up to 4,096 texts;
 * FSEQ_JOIN_BIP_WIDE forces it at any count up to that, FSEQ_JOIN_BIP_SLABS caps its slabs = persistent workgroups).
 * FSEQ_E_ARG before any fseq_join_bipartite has finished since the context's input was set: a new input clears it. */
int  fseq_debug_bipartite_path(fseq_ctx *ctx, int *path);

/* Device memory the context holds through its own buffers now (*now) and the most it has held since it was made or since the
 * last call with reset_peak != 0 (*peak; the reset happens after the report, to the bytes held now).  Accounting of the
 * context's allocations, not a measurement of the device: borrowed columns and the runtime's own memory are not in it. */
int  fseq_debug_device_bytes(fseq_ctx *ctx, uint64_t *now, uint64_t *peak, int reset_peak);

/* The alphabet of the input the context holds: *sigma codes of *bits bits, code_to_byte[code] (256 bytes, or NULL) the byte a
 * code stands for (entries from *sigma on are not defined).  FSEQ_E_ARG while the context holds no input. */
int  fseq_debug_alphabet(fseq_ctx *ctx, uint32_t *sigma, uint32_t *bits, uint8_t *code_to_byte);

/* The resident alignment as it is stored: the bytes of the columns [c0, c1), *ld bytes a column (padding included), codes of
 * *bits bits.  out == NULL: *ld and *bits only.  Not for sharded contexts (a rank holds its own columns only). */
int  fseq_debug_packed_columns(fseq_ctx *ctx, uint64_t c0, uint64_t c1, uint8_t *out, uint64_t *ld, uint32_t *bits);

/* Which way the boundaries of the last run went through pass 2's chain step on streamed rows behind the reduced phase C
 * (k_chain_snap_grouped): boundaries moved as runs of equal class (*by_runs), boundaries whose rows were all sorted
 * (*by_sort: more runs than FSEQ_P2_RUN_CAP, the knob at 0, or a class and a position that do not share a 32-bit word),
 * boundaries on a block border (*copies) and the most runs a boundary formed, over those that counted theirs (*max_runs);
 * runs_hist (19 words, or NULL): those boundaries by run count, [b] = how many formed more than 2^(b - 1) and at most 2^b
 * runs ([0]: one run).  All zero where the last run did not go through that kernel (LDS-resident rows, no representatives). */
int  fseq_debug_pass2_paths(fseq_ctx *ctx, uint32_t *by_runs, uint32_t *by_sort, uint32_t *copies, uint32_t *max_runs, uint32_t *runs_hist);

/* Pass 2's sweeps of the last run at caller-chosen columns: after a finished run whose phase C went through the blocks'
 * representatives, the class tables (k_columns_red in its sweep form, from the reduced state phase C dropped in front of the column
 * or from the block's first column) at columns[0 .. count), ascending and each strictly inside a block -- the task construction and
 * the launches of pass 2 itself, on buffers of this call.  By rows of the alignment, m words a column: cls[i * m + r] the class of
 * row r at columns[i] (the class of its block key), headd[i * m + c] the divergence in front of class c for c < ncls[i] (0xFFFFFFFF
 * behind them), ncls[i] the classes.  FSEQ_E_UNSUPPORTED where the last run was not reduced (or sharded), or a column lies in a block
 * without representatives; FSEQ_E_ARG for columns on a block border, out of order or outside the alignment. */
int  fseq_debug_class_tables(fseq_ctx *ctx, uint64_t const *columns, uint32_t count, uint32_t *cls, uint32_t *headd, uint32_t *ncls);

/* Where the reduced alignment of the last run came from (streamed rows behind the reduced phase C): *from_classes blocks took their
 * representatives' columns from phase A's class columns (the block trie's, csrc/fseq_blocktrie.hpp), *from_alignment blocks
 * from the alignment itself (blocks the trie gave up; every block with FSEQ_CLASS_COLUMNS=0, or where the class columns did not
 * fit the memory budget).  Both zero where the run built no reduced alignment (LDS-resident rows, no representatives).
 * block != UINT32_MAX: that block's class columns as well -- *have (1: it has them), *nkeys (its distinct keys), *ldc (bytes a class
 * column) and, where out != NULL and it has them, the columns of the block one after the other, *ldc bytes each, into out
 * (out_bytes: its size; FSEQ_E_ARG when too small): row rho of a column is the symbol of the key of rank rho, packed like the
 * alignment. */
int  fseq_debug_class_columns(fseq_ctx *ctx, uint32_t *from_classes, uint32_t *from_alignment, uint32_t block, uint32_t *have, uint32_t *nkeys,
                              uint64_t *ldc, uint8_t *out, uint64_t out_bytes);

/* How the listed blocks of the last run (the blocks with representatives; streamed rows behind the reduced phase C) came by their
 * columns: *staged blocks had phase A's class columns staged by the reduced column kernel itself, *gathered blocks read the reduced
 * alignment (gathered from the class columns or from the alignment: fseq_debug_class_columns tells which).  A block is staged where it
 * has class columns and every configuration it runs on takes staged-column buffers of the class width at no cost in LDS or resident
 * workgroups; never with FSEQ_CLASS_GATHER=1 or FSEQ_CLASS_COLUMNS=0.  block != UINT32_MAX: *block_staged for that block as well.
 * Both zero where the run built neither (LDS-resident rows, no representatives). */
int  fseq_debug_column_sources(fseq_ctx *ctx, uint32_t *staged, uint32_t *gathered, uint32_t block, uint32_t *block_staged);

/* The direct-or-gather rule of one configuration of the reduced column kernel (red_cls_direct, csrc/fseq_redplan.hpp), as a run of m
 * rows in blocks of B columns at `bits` bits a symbol with class columns of cls_ld bytes applies it -- host arithmetic, no device:
 * *lds_rows / *lds_cls the configuration's LDS with staged-column buffers for its rows / of the class width, *direct whether it stages
 * the class columns itself given the workgroups per CU the device reports at either size (resident_rows, resident_cls: the run asks
 * the occupancy query).  FSEQ_E_ARG: m, B, cls_ld >= 1, bits 2 / 4 / 8, config below the number fseq_debug_red_plan reports. */
int  fseq_debug_red_cls_direct(uint32_t m, uint32_t B, uint32_t bits, uint64_t cls_ld, uint32_t config, uint32_t resident_rows, uint32_t resident_cls,
                               uint64_t *lds_rows, uint64_t *lds_cls, int *direct);

/* Which way the last fseq_join_random since the input was set went: 0 the host joiner (every boundary state copied), 1 the class
 * tables from the device.  FSEQ_E_ARG while none has finished. */
int  fseq_debug_random_path(fseq_ctx *ctx, int *path);

/* Which way the last fseq_join_score since the input was set went: 0 the host form (every boundary state copied), 1 the device
 * form.  FSEQ_E_ARG while none has finished. */
int  fseq_debug_join_score_path(fseq_ctx *ctx, int *path);

/* k_join_score and k_join_score_founders (csrc/fseq_joinscore.hpp) on caller-built class arrays, through the launcher
 * fseq_join_score itself uses (debug / tests; needs no context): of[S][m] the class of every row in every segment;
 * perm_cls_left / perm_cls_right [S - 1][X] the classes of every slot's left and right row at every junction, 0xFFFF a gap.
 * Out, each may be NULL: junctions [S - 1] (rb is 0), breaks [X], support [(S - 1) x X], summary.  Everything an index or a key
 * is formed from is checked on the host before the first call of the runtime, FSEQ_E_ARG otherwise: the three arrays given;
 * 1 <= m < 2^31; 1 <= X <= 4,096; 2 <= S <= 65,536; every class in of below 0xFFFF (a slot's class may be any value: one that
 * no row has finds no row). */
int  fseq_debug_join_score(int device, uint32_t m, uint32_t X, uint32_t S, uint16_t const *of, uint16_t const *perm_cls_left,
                           uint16_t const *perm_cls_right, fseq_join_score_entry *junctions, uint32_t *breaks, uint32_t *support,
                           fseq_join_score_summary *summary);

/* The bounds of merged segments in the source's co-ordinates (restored_segment_bounds, csrc/fseq_restored_bounds.hpp), as
 * fseq_get_segments_restored and fseq_write_segments_restored apply them -- host arithmetic, no device, no context.  kept[n]: the
 * source column of every kept column; lb / rb [n_segments]: the merged segments in kept columns.  Out: src_lb / src_rb
 * [n_segments]: src_lb[0] = 0, else kept[lb[s]]; src_rb[last] = n_src, else kept[rb[s]].  FSEQ_E_ARG, with nothing written: a
 * NULL array, no segment, kept not strictly ascending or an entry not below n_src, segments that do not tile [0, n). */
int  fseq_debug_restored_bounds(uint64_t const *kept, uint64_t n, uint64_t n_src, uint64_t const *lb, uint64_t const *rb, uint64_t n_segments,
                                uint64_t *src_lb, uint64_t *src_rb);

/* Which entries of a kept-column list fall inside a chunk of source columns (debug / tests; no device, no context): the pure
 * host function behind fseq_input_kept_columns and fseq_input_columns_kept (input_kept_range, csrc/fseq_input_kept_range.hpp).
 * kept[0 .. n_kept) ascend strictly; [*k0, *k1) are the entries with c0 <= kept[k] < c0 + ncols, *k0 == *k1 (where one would
 * stand) if there is none.  FSEQ_E_ARG: a NULL out pointer, or kept NULL with n_kept > 0. */
int  fseq_debug_input_kept_range(uint64_t const *kept, uint64_t n_kept, uint64_t c0, uint64_t ncols, uint64_t *k0, uint64_t *k1);

/* The last file fseq_write_segments_device or fseq_write_segments_restored wrote on this context: the batches that left the device (0: greedy, the header
 * alone), the file's bytes, the bytes of its longest line and its lines -- both with the header, a line with its newline.
 * Each out pointer may be NULL.  FSEQ_E_ARG while none has been written. */
int  fseq_debug_segments_file(fseq_ctx *ctx, uint64_t *batches, uint64_t *bytes, uint64_t *longest_line, uint64_t *lines);

/* The last file fseq_write_block_graph wrote on this context, by section -- [0] the S lines, [1] the L lines, [2] the P lines
 * (all zero without FSEQ_GRAPH_PATHS): the batches that left the device, the lines and their bytes, a line with its newline.
 * The header line (11 bytes) goes through no batch and is in no count: the file has 11 + bytes[0] + bytes[1] + bytes[2] bytes.
 * FSEQ_GRAPH_BATCH=bytes sets the most a batch holds (a longer line is a batch of its own; fseq_debug_set_tuning takes it at any
 * time: nothing of a run depends on it).  FSEQ_E_ARG while none has been written. */
typedef struct fseq_graph_file_stats {
	uint64_t batches[3], lines[3], bytes[3];
} fseq_graph_file_stats;
int  fseq_debug_graph_file(fseq_ctx *ctx, fseq_graph_file_stats *stats);

/* The last fseq_graph_thread_rows / fseq_graph_thread_held_out that finished on this context: the bits of a node key
 * (FSEQ_GRAPH_THREAD_KEY_BITS=b, 1 .. 64, by itself 64, truncates the keys; fseq_debug_set_tuning takes it at any time: nothing
 * of a run depends on it, and the threading's results never do), the slots of a workgroup's LDS table, the candidates -- table
 * entries whose key equals a query's -- that were compared code by code and those among them that failed the comparison, and the
 * (query, segment) cells left unmatched because the query carries a byte outside the alphabet there.  A probe runs to the empty
 * slot that ends its chain, so the counts do not depend on where the entries lie.  FSEQ_E_ARG while no call has finished. */
typedef struct fseq_graph_thread_info {
	uint32_t key_bits, table_slots;
	uint64_t candidates_verified, candidates_rejected, queries_out_of_alphabet;
} fseq_graph_thread_info;
int  fseq_debug_graph_thread(fseq_ctx *ctx, fseq_graph_thread_info *info);

/* The last fseq_graph_nearest_rows / fseq_graph_nearest_held_out that finished on this context: the batches of whole segments
 * its class representatives were packed in, the representatives' packed words over all batches, the packed words of ONE query,
 * and the bits of a packed code (the queries' width).  FSEQ_GRAPH_NEAREST_BATCH=bytes sets the most representative words a
 * batch holds (by itself 256 MiB; a segment above it is a batch of its own; fseq_debug_set_tuning takes it at any time: nothing
 * of a run depends on it, and the results never do).  FSEQ_E_ARG while no call has finished. */
typedef struct fseq_graph_nearest_info {
	uint64_t batches, packed_words, query_words;
	uint32_t bits, reserved;
} fseq_graph_nearest_info;
int  fseq_debug_graph_nearest_info(fseq_ctx *ctx, fseq_graph_nearest_info *info);
/* The batch cut alone (graph_nearest_words and graph_nearest_plan, csrc/fseq_graphnearest_plan.hpp; no device, no context):
 * n_segments segments [lb[s], rb[s]) of count[s] classes at `bits` bits a code.  words[s] (n_segments + 1 entries) is the sum of
 * count * ceil(columns / (32 / bits)) over the segments in front of s; batch b is the segments [first[b], first[b + 1]), of
 * first's n_segments + 1 entries *n_batches + 1 are written.  FSEQ_E_ARG, with nothing written, for a NULL array, no segments,
 * bits not 2, 4 or 8, a budget of 0 bytes, an empty or backward segment and a segment without a class; FSEQ_E_UNSUPPORTED for a
 * segment of 2^32 - 1 columns or more. */
int  fseq_debug_graph_nearest_plan(uint64_t const *lb, uint64_t const *rb, uint32_t const *count, uint64_t n_segments, uint32_t bits,
                                   uint64_t budget_bytes, uint64_t *words, uint64_t *first, uint64_t *n_batches);
/* The pack and distance kernels through the production launcher on caller-supplied tables (debug / tests; needs no context).
 * cols: an alignment of m rows and n columns, column-major and packed at `bits` bits a code, ld bytes a column (pack_columns);
 * qcols: n_queries queries the same way at qbits, qld bytes a column.  n_segments segments [seg_lb[s], seg_rb[s]) with count[s]
 * classes whose representative rows are rep[s][0 .. count[s]) (rep is [n_segments][X]): the caller's, so duplicate or equidistant
 * representatives can be planted.  nodes (as CLASS indices), distances and ties are [n_segments][n_queries]; info as
 * fseq_debug_graph_nearest_info's; batch_bytes 0: the budget by itself.  Refuses with FSEQ_E_ARG, before a device is touched,
 * whatever a kernel could form an index from: a NULL array, m, n, n_segments, X or n_queries = 0, rep >= m, count = 0 or > X,
 * bounds outside n or out of order, bits / qbits not in {2, 4, 8}, qbits < bits, ld or qld too short for the rows. */
int  fseq_debug_graph_nearest(int device, uint8_t const *cols, uint64_t ld, uint32_t m, uint64_t n, uint32_t bits,
                              uint64_t const *seg_lb, uint64_t const *seg_rb, uint32_t const *count, uint32_t const *rep,
                              uint32_t n_segments, uint32_t X, uint8_t const *qcols, uint64_t qld, uint32_t n_queries, uint32_t qbits,
                              uint32_t sigma, uint64_t batch_bytes, uint32_t *nodes, uint32_t *distances, uint32_t *ties,
                              fseq_graph_nearest_info *info);

/* One launch of pass 2's chain step on streamed rows (k_chain_snap_grouped, csrc/fseq_chainsort.hpp) on caller-supplied states
 * (debug / tests; needs no context).  nblocks boundary states a0 / d0 [nblocks][m] with the block-key rank of every row,
 * rank[nblocks][m] < cap; ntasks tasks, task t one step from the state of block task_blk[t], the key of a row cls[t][rank[row]],
 * the divergence in front of a class headd[t][class] (cls / headd [ntasks][cap]), ncls[t] classes: 0 is a border copy, 0xFFFFFFFF a
 * task the kernel leaves alone.  The tasks of a block are consecutive and form one group; the groups go to the kernel largest
 * first, taken from a counter by `workgroups` workgroups.  run_cap: the most runs of equal class a task may form and still be moved
 * by runs (0: every task sorts its rows).  Out: snap_a / snap_d [ntasks][m] (0xFFFFFFFF where the kernel wrote nothing) and the
 * kernel's counters, stats[23]: tasks by runs, tasks by sort, copies, the most runs, 19 words of runs_hist (fseq_debug_pass2_paths).
 * Everything an index is formed from is checked on the host before the first call of the runtime, FSEQ_E_ARG otherwise:
 * 11,265 <= m <= 589,824; every a0 a permutation of 0 .. m - 1; rank < cap <= 11,264; task_blk < nblocks, a block's tasks
 * together; ncls <= cap and all cap entries of such a task's cls below its ncls; run_cap <= 8,832; 1 <= workgroups <= 1,024;
 * at most 4,096 blocks and tasks. */
int  fseq_debug_pass2_step(int device, uint32_t m, uint32_t nblocks, uint32_t const *a0, uint32_t const *d0, uint32_t const *rank, uint32_t cap,
                           uint32_t ntasks, uint32_t const *task_blk, uint32_t const *cls, uint32_t const *headd, uint32_t const *ncls,
                           uint32_t run_cap, uint32_t workgroups, uint32_t *snap_a, uint32_t *snap_d, uint32_t *stats);

/* One chain launch of phase B on streamed rows (k_cm_*, csrc/fseq_chainsort.hpp, through the launcher phase B itself uses) on
 * caller-supplied key blocks (debug / tests; needs no context): the level's key blocks rank[nb_total][m], keyd[nb_total][m],
 * nkeys[nb_total], cols_per_block columns each; the chains first_chain .. first_chain + chains - 1 of G blocks each, from
 * start_a / start_d [chains][m] (both NULL: the identity, every divergence the chain's first column).  Out, either or both:
 * the states in front of every block and behind the last, out_state_a / out_state_d [nb_total + 1][m] (0xFFFFFFFF where the
 * launch wrote nothing; without composite keys a chain does not step through its last block unless that is the last of all),
 * and the chains' composite key blocks out_rank / out_keyd [chains][m], out_nkeys[chains] (out_keyd: 0xFFFFFFFF behind the keys).
 * Checked on the host before the first call of the runtime, FSEQ_E_ARG otherwise: 11,265 <= m <= 589,824; 1 <= nkeys[b] <= m and
 * rank[b][row] < nkeys[b]; 1 <= G <= nb_total <= 4,096; the chains inside ceil(nb_total / G); every start_a a permutation of
 * 0 .. m - 1; start_a and start_d, and the outputs of a kind, together. */
int  fseq_debug_chain_launch(int device, uint32_t m, uint32_t nb_total, uint32_t G, uint64_t cols_per_block, uint32_t const *rank, uint32_t const *keyd,
                             uint32_t const *nkeys, uint32_t first_chain, uint32_t chains, uint32_t const *start_a, uint32_t const *start_d,
                             uint32_t *out_state_a, uint32_t *out_state_d, uint32_t *out_rank, uint32_t *out_keyd, uint32_t *out_nkeys);

/* The same launch with a chain per workgroup (k_chain_wg, csrc/fseq_chainsort.hpp: the form phase B takes for launches of at least
 * a chain per CU): `workgroups` workgroups take the chains by a fixed stride and walk each through its steps -- a step from the
 * identity, by runs of equal key (at most run_cap of them, and a key and a position in one 32-bit word) or by the sort of its rows.
 * Arguments, outputs and checks as for fseq_debug_chain_launch, and: run_cap <= 16,384 (0: no step goes by runs),
 * 1 <= workgroups <= 1,024, and the kernel's counters, stats[23]: steps by runs, steps by the sort of their rows, steps from the
 * identity, the most runs of a step that counted its runs, 19 words of those steps by run count (bucket b: more than 2^(b - 1) and
 * at most 2^b runs; bucket 0: one run). */
int  fseq_debug_chain_launch_wg(int device, uint32_t m, uint32_t nb_total, uint32_t G, uint64_t cols_per_block, uint32_t const *rank, uint32_t const *keyd,
                                uint32_t const *nkeys, uint32_t first_chain, uint32_t chains, uint32_t const *start_a, uint32_t const *start_d,
                                uint32_t run_cap, uint32_t workgroups, uint32_t *out_state_a, uint32_t *out_state_d, uint32_t *out_rank,
                                uint32_t *out_keyd, uint32_t *out_nkeys, uint32_t *stats);

/* fseq_debug_chain_launch_wg with the hand-over to pass 2: hand_keys[nb_total][m] (16 bits a row; in: any pattern, out: what the
 * launch left of it) and hand_flag[nb_total] (out).  Where hand_flag[b] is set, hand_keys[b][i] = rank[b][a[i]] for the state a
 * in front of block b: an expansion's run or sort step through b whose keys fit 16 bits.  Every other block keeps its pattern and
 * a clear flag -- a composition hands nothing over.  Takes m from 65 on (the other entries: the streamed regime's 11,265). */
int  fseq_debug_chain_launch_wg_keys(int device, uint32_t m, uint32_t nb_total, uint32_t G, uint64_t cols_per_block, uint32_t const *rank,
                                     uint32_t const *keyd, uint32_t const *nkeys, uint32_t first_chain, uint32_t chains, uint32_t const *start_a,
                                     uint32_t const *start_d, uint32_t run_cap, uint32_t workgroups, uint32_t *out_state_a, uint32_t *out_state_d,
                                     uint32_t *out_rank, uint32_t *out_keyd, uint32_t *out_nkeys, uint32_t *stats, uint16_t *hand_keys,
                                     uint32_t *hand_flag);

/* fseq_debug_pass2_step with phase B's hand-over: hand_keys[nblocks][m] and hand_flag[nblocks]; a group whose block has its flag set
 * reads the block's ranks in the order of its state from hand_keys and gathers none (FSEQ_E_ARG where such a key is not below cap).
 * hand_stats[2] (out): the groups that took handed-over keys, the groups that gathered their own. */
int  fseq_debug_pass2_step_keys(int device, uint32_t m, uint32_t nblocks, uint32_t const *a0, uint32_t const *d0, uint32_t const *rank, uint32_t cap,
                                uint32_t ntasks, uint32_t const *task_blk, uint32_t const *cls, uint32_t const *headd, uint32_t const *ncls,
                                uint32_t run_cap, uint32_t workgroups, uint16_t const *hand_keys, uint32_t const *hand_flag, uint32_t *snap_a,
                                uint32_t *snap_d, uint32_t *stats, uint32_t *hand_stats);

/* The plan of phase B (csrc/fseq_chainplan.hpp; debug / tests; touches no device): the fan of the recursion over the key blocks, the
 * items of every level, and every chain launch in the order a run queues it -- up the levels, the top chain, down the levels -- with the
 * kernel the rule gives it.  A launch: the level whose key blocks its chains walk (0: the alignment's own blocks), its kind (0 a
 * composition from the identity, 1 the top chain, 2 an expansion), its chains, the key blocks of a chain (the last chain of a level may
 * hold fewer), its first chain among the level's, and the workgroups of k_chain_wg it runs on -- 0: the spread kernels (k_cm_*), or,
 * LDS-resident rows, the chain kernel of those rows. */
typedef struct fseq_chain_launch_info {
	uint32_t level, kind, chains, blocks, first_chain, workgroups;
} fseq_chain_launch_info;
#define FSEQ_DEBUG_CHAIN_LEVELS 40
#define FSEQ_DEBUG_CHAIN_LAUNCHES 80
typedef struct fseq_chain_plan {
	uint32_t fan;                 /* the fan in force */
	uint32_t fan_round5;          /* the fan before turns of workgroups were looked at (round 5's cost model on streamed rows) */
	uint32_t turns;               /* the turns of workgroups the model counted for level 0 at `fan`; 0: it counted none */
	uint32_t shard_k, shard_q;    /* sharded: a rank is shard_q groups of fan^shard_k blocks ... */
	uint32_t blocks_per_rank;     /* ... = this many blocks; */
	uint32_t n_hyper;             /* the ranks that own blocks; */
	uint32_t b_lo, b_hi;          /* the blocks of the rank asked for */
	uint32_t n_levels, n_launches, reserved;
	/* one GPU: the items of level 0 .. n_levels - 1 ([0] = nblocks; the top chain takes the last).  Sharded: the rank's items of the
	 * levels 0 .. shard_k, n_levels = shard_k + 1 */
	uint32_t level_items[FSEQ_DEBUG_CHAIN_LEVELS];
	fseq_chain_launch_info launches[FSEQ_DEBUG_CHAIN_LAUNCHES];
} fseq_chain_plan;
/* One GPU: m rows in nblocks blocks; streamed != 0: the rows take the streamed kernels (more than 11,264 rows); cus: the device's
 * CUs; chain_wg: FSEQ_CHAIN_WG (0 the rule: a launch of at least a chain per CU goes to k_chain_wg; 1 every streamed launch; 2 none --
 * 1 and 2 keep round 5's fan); chain_fan: FSEQ_CHAIN_FAN (0: none; a forced fan reports no turns); fit, resident: the cap on the
 * workgroups of a launch on k_chain_wg, min(chains, fit, max(cus, 1) x max(resident, 1)) -- the workgroups whose workspaces the run's
 * workspace holds and the workgroups a CU holds at once (fseq_debug_phase_b reports both; fit == 0: the launch takes the spread
 * kernels).  FSEQ_E_ARG: plan NULL, m or nblocks 0, chain_wg not 0, 1 or 2, chain_fan 1. */
int  fseq_debug_chain_plan(uint32_t m, int streamed, uint32_t nblocks, uint32_t cus, int chain_wg, uint32_t chain_fan, uint64_t fit, uint32_t resident,
                           fseq_chain_plan *plan);
/* A rank of a sharded run: nblocks blocks over `world` ranks at fan chain_fan (0: the 4 a sharded run takes by itself): (k, q) with
 * the fewest serial steps among those that keep every rank busy, the blocks of rank `rank`, its items a level and its launches -- up
 * its own range, its q composites into its hyper key block (level shard_k, one chain), the chain over the n_hyper hyper key blocks
 * (level shard_k + 1, kind 1; every rank, also one without blocks), and down again.  fan and fan_round5 are the fan, turns is 0.
 * FSEQ_E_ARG: plan NULL, nblocks 0, world 0 or above 4,096, rank >= world, chain_wg not 0, 1 or 2, chain_fan 1. */
int  fseq_debug_chain_plan_sharded(uint32_t nblocks, uint32_t world, uint32_t rank, uint32_t chain_fan, int streamed, uint32_t cus, int chain_wg,
                                   uint64_t fit, uint32_t resident, fseq_chain_plan *plan);
/* What phase B of the last run on this context did (a sharded rank: its own): the CUs it saw, the blocks and the fan, the chain
 * launches it queued, in order (n_launches of them), `fit` and `resident` as chain_wg_groups applied them (fseq_debug_chain_plan;
 * both 0 on LDS-resident rows), whether the hand-over of level 0's keys to pass 2 was armed, the counters of k_chain_wg where they
 * were kept (stats_kept: FSEQ_DEBUG was set and FSEQ_CHAIN_WG is not 2; cw_stats as fseq_debug_chain_launch_wg's stats), and of pass
 * 2's streamed chain step the groups it ran, those that took the keys phase B handed over and those that gathered their own (all 0
 * where the run did not go through that kernel).  FSEQ_E_ARG while the context holds no result of the long path. */
typedef struct fseq_phase_b_info {
	uint32_t cus, nblocks, fan, n_launches;
	uint32_t resident, hand_armed, stats_kept, reserved;
	uint64_t fit;
	uint32_t p2_groups, p2_groups_took_keys, p2_groups_gathered, reserved2;
	uint32_t cw_stats[23];
	uint32_t reserved3;
	fseq_chain_launch_info launches[FSEQ_DEBUG_CHAIN_LAUNCHES];
} fseq_phase_b_info;
int  fseq_debug_phase_b(fseq_ctx *ctx, fseq_phase_b_info *info);

/* The plan of phase C on representative rows (plan_reduced, csrc/fseq_redplan.hpp) on caller-supplied counts (debug / tests; touches
 * no device).  The configurations are the library's, judged as a run of m rows in blocks of B columns at `bits` bits a symbol would
 * judge them (direct != 0: LDS-resident rows, which stage the alignment's own columns).  cnt[nblocks]: the representatives of every
 * block (0xFFFFFFFF: not reduced); force[nblocks] or NULL: 0, 1 (the block on all rows) or 2 (the block skips the slim
 * configuration); [b_lo, b_hi): the blocks planned for; no_block_list: the kernel on all rows takes no block list.
 * Out, each or NULL: configs[FSEQ_DEBUG_RED_CONFIGS][6] = {rows, values, threads, rows per thread, list wave, fits} and *n_configs;
 * *verdict (0 use, 1 declined, 2 no block list); full / config_of / config_snap_of [nblocks]; blocks[3 nblocks], the list that goes to
 * the device, and *n_blocks; bins[n_configs][3] = {configuration, first, count} into blocks and *n_bins; summary[6] = {full_at,
 * nfull, listed, max_rows, reduced_blocks, rows_mean}.  Checked before anything is indexed, FSEQ_E_ARG otherwise: m, B >= 1; bits 2,
 * 4 or 8; b_lo <= b_hi <= nblocks <= 2^24; every count <= m or 0xFFFFFFFF; every force mark 0, 1 or 2. */
#define FSEQ_DEBUG_RED_CONFIGS 64
int  fseq_debug_red_plan(uint32_t m, uint32_t B, uint32_t bits, int direct, uint32_t nblocks, uint32_t b_lo, uint32_t b_hi, uint32_t const *cnt,
                         uint8_t const *force, int reduced_always, int no_block_list, uint32_t *configs, uint32_t *n_configs, int *verdict,
                         uint8_t *full, int32_t *config_of, int32_t *config_snap_of, uint32_t *blocks, uint32_t *n_blocks, uint32_t *bins,
                         uint32_t *n_bins, uint32_t *summary);

/* The order of work of fseq_scan_segment_lengths (plan_length_scan, csrc/fseq_scanplan.hpp) for an alignment of n columns
 * (debug / tests; touches no device): the distinct lengths of the long path (n >= 2L), ascending, into long_lengths[count] and
 * *n_long; slot[i], the place of lengths[i] among them, or -1 where it takes the short path (n < 2L); *n_short, the entries that
 * do.  FSEQ_E_ARG: a NULL pointer, count == 0, n == 0, a length of 0. */
int  fseq_debug_scan_plan(uint64_t n, uint64_t const *lengths, uint32_t count, uint64_t *long_lengths, uint32_t *n_long, int32_t *slot,
                          uint32_t *n_short);

/* One launch of k_relump_lists (csrc/fseq_lengthscan.hpp) on caller-supplied lists (debug / tests; needs no context): the lists
 * of the columns [k0, k0 + ncols) as phase C leaves them at segment length L_from -- ent[ncols][stride] {value, count} pairs,
 * entry 0 the lump {k + 1, count of the values >= k + 2 - L_from}, then the distinct values below, descending; hdr[ncols][4] =
 * {entries, count of value 0, complete, cumulative count} -- are folded in place to what the DP reads at L_to: the leading
 * entries from index 1 on whose value is >= k + 2 - L_to (0 where k + 2 <= L_to) join the lump, the rest moves down, the header's
 * first word falls by their number; the words behind the new end and the other header words stay.
 * Refused before a device is touched, FSEQ_E_ARG: a NULL array, ncols == 0, stride == 0, L_from == 0, L_to < L_from, a header
 * whose entries are 0 or more than stride, k0 + ncols beyond 2^32. */
int  fseq_debug_relump_lists(int device, uint64_t k0, uint32_t ncols, uint32_t stride, uint64_t L_from, uint64_t L_to, uint32_t *ent, uint32_t *hdr);

/* How the last match of the context walked (csrc/fseq_match.hpp, k_match_walk_split): the segments G the columns were split
 * into (1: unsplit) and the overlap in use (clamped to the longest segment; 0 where G = 1), the groups of 256 rows, how many of
 * them were flagged by the check and walked again unsplit, and the rows that did not stand (head[g] != tail[g - 1] for some g).
 * FSEQ_MATCH_SPLIT=g (1..4,096) and FSEQ_MATCH_OVERLAP=columns force the shape for the entries that take query rows --
 * fseq_match_rows, fseq_match_held_out, fseq_match_held_out_restored, fseq_match_rows_restored, which otherwise choose it by
 * themselves -- and, with FSEQ_MATCH_SPLIT set, for fseq_match_founders, fseq_match_founder_rows and fseq_match_founders_restored,
 * which walk unsplit otherwise (fseq_debug_set_tuning takes both at any time: nothing of a run depends on them; so it does
 * FSEQ_MATCH_STAGE_BYTES=bytes, the most a staged chunk of fseq_match_rows_restored's query rows takes -- 64 MiB by itself, at
 * least 64 columns).  For the three restored entries the segments and the overlap, forced and reported, are counted in the
 * context's columns, the kept ones of the source; a restored match of query rows that chooses one segment by itself (fewer than
 * 32,768 kept columns) walks through the unsplit kernel and reports one segment.  FSEQ_E_ARG before a match. */
typedef struct fseq_match_split_info {
	uint32_t segments, row_groups, flagged_groups, reserved;
	uint64_t overlap, rows_not_standing;
} fseq_match_split_info;
int  fseq_debug_match_split(fseq_ctx *ctx, fseq_match_split_info *info);

/* The held-out rows of a context made by fseq_create_without_rows as they are stored (the twin of fseq_debug_packed_columns): the
 * bytes of the columns [c0, c1), *ld bytes a column (padding included), codes of *bits bits; row q of a column is held_rows[q].
 * out == NULL: *ld and *bits only.  FSEQ_E_ARG on any other context. */
int  fseq_debug_held_out_columns(fseq_ctx *ctx, uint64_t c0, uint64_t c1, uint8_t *out, uint64_t *ld, uint32_t *bits);

/* The plan of a split along the rows (row_split_plan, csrc/fseq_rowsplit_plan.hpp) for m rows at `bits` = 2, 4 or 8 bits a code
 * with the n_held rows of `held` set aside (debug / tests; touches no device).  per = 32 / bits.  Out, each array or NULL:
 * kept[m - n_held], the rows that stay, ascending; one descriptor per 32-bit word of a kept column, base / keep [*n_words],
 * *n_words = ceil((m - n_held) / per): word w holds the kept rows w per .. w per + per - 1, base[w] is the source row of the first,
 * and bit i of keep[w] is set iff source row base[w] + i is one of them -- the word is the 2 per fields from base[w] on compressed
 * by keep[w].  A word whose rows span more than 2 per source rows has keep[w] = 0 (bit 0 is set otherwise) and is built field by
 * field from kept; *n_slow counts those.  FSEQ_E_ARG, as fseq_create_without_rows refuses it: bits not 2, 4 or 8, held NULL,
 * n_held outside 1 .. m - 1, an entry not below m, an entry twice; n_words or n_slow NULL. */
int  fseq_debug_row_split_plan(uint32_t m, uint32_t bits, uint32_t const *held, uint32_t n_held, uint32_t *kept, uint32_t *base, uint32_t *keep,
                               uint32_t *n_words, uint32_t *n_slow);

/* Whether the DP may read caller-supplied lists (debug / tests; touches no device): ent[n][stride] {value, count} pairs and
 * hdr[n][4] = {entries, count of value 0, complete, cumulative count}, the format of k_columns (fseq_debug_relump_lists above),
 * for m rows, n columns and segment length L, n >= 2L.  Checked for every column a cell reads, L - 1 .. n - L - 1 and n - 1
 * -- what a kernel could form an index or a wrong proof from --, FSEQ_E_ARG at the first column that fails, *bad_column (or
 * NULL) that column and *rule (or NULL) the rule it broke:
 *   1  entries in 1 .. stride                          5  every count behind the lump >= 1
 *   2  entry 0's value is k + 1                        6  the cumulative count is the sum of the counts, at most m
 *   3  values strictly descending                      7  complete (0 or 1) iff the sum is m; the count of value 0 is at most m
 *   4  value 0 in the last place only, its count the header's and the list complete; a complete list without it has a
 *      header count of 0
 * rule 0 (no column): a NULL array, m == 0, L == 0, n < 2L, n >= 2^32 - 16, stride == 0 or n * stride beyond 2^28 entries. */
int  fseq_debug_dp_lists_check(uint32_t m, uint64_t n, uint64_t segment_length, uint32_t stride, uint32_t const *ent, uint32_t const *hdr,
                               uint64_t *bad_column, uint32_t *rule);

/* Phase D alone on caller-supplied lists, through the launchers a run uses (debug / tests): k_dp in its three modes and the
 * kernels of the speculative sweeps (csrc/fseq_dp.hpp, csrc/fseq_dpspec.hpp).  ctx: an unsharded context without a list budget
 * whose input is set (m x n at the context's segment length, n >= 2L; the bytes of the rows are never read).  ent / hdr as for
 * fseq_debug_dp_lists_check with stride = (list_cap + 3) & ~1, which refuses them here before the device is touched.  The work
 * buffers are made at capacity list_cap, the lists copied over the context's, the DP's words and arrays cleared.  Then
 *   n_cuts == 0: the DP as a run at this length chooses it (long_dp_on_lists): the speculative sweeps under spec_plan's plan or
 *     the one FSEQ_DP_SPEC_ROUNDS / _WIN / _MAX_SWEEPS force, one whole launch of the serial kernel under FSEQ_DP_SERIAL or
 *     where the plan has fewer than three chunks;
 *   n_cuts > 0: resumed launches of the serial kernel over the rounds [0, cuts[0]), [cuts[0], cuts[1]), ... [cuts[n_cuts - 1],
 *     rounds), as a run under a list budget chains them; the cuts ascend strictly inside (0, rounds) (fseq_debug_dp_schedule).
 * Out: lb / max_size / size, n - L + 1 words each (the entries 0 .. n - 2L and n - L are written, the others read 0), and
 * info = {a list was too short to prove a cell, chunks of the sweeps' plan (0: serial), sweeps compared (1000 + the sweeps
 * where the budget ran out and the serial kernel took over), launches of the serial kernel this call queued itself}.
 * The context holds no result afterwards and no lists fseq_debug_column_list would answer for; a following run is unaffected. */
typedef struct fseq_dp_lists_info {
	uint32_t unproven, dp_chunks, dp_sweeps, launches;
} fseq_dp_lists_info;
int  fseq_debug_dp_on_lists(fseq_ctx *ctx, uint32_t list_cap, uint32_t const *ent, uint32_t const *hdr, uint32_t const *cuts, uint32_t n_cuts,
                            uint32_t *lb, uint32_t *max_size, uint32_t *size, fseq_dp_lists_info *info);

/* The traceback and the greedy merge alone on caller-supplied DP arrays and lists, through follow_traceback and the merge half
 * of long_traceback_and_merge as an unsharded run calls them (debug / tests): k_tb_windows, k_tb_chain, k_tb_emit, k_seg_tau_tb,
 * k_seg_tau, k_seg_count (csrc/fseq_kernels.hpp).  ctx, list_cap, ent and hdr as for fseq_debug_dp_on_lists, with the same
 * refusals and the same fseq_debug_dp_lists_check.  lb / max_size / size: n - L + 1 words each, copied over the DP's arrays.  Of
 * lb only the chain from entry n - L is checked, on the host before any runtime call (csrc/fseq_tbcheck.hpp): an entry t on it has
 * lb == 0 or L <= lb <= t, and the chain ends in lb == 0 within n / L + 2 entries; FSEQ_E_ARG with a message naming the entry
 * otherwise.  Entries off the chain may hold anything.
 *   flags bit 0 clear: the thresholds ride with the traceback (k_seg_tau_tb), as an unsharded run takes them; col_splits are refused;
 *   flags bit 0 set: they come from launches of k_seg_tau of their own, and the merged sizes from k_seg_count, once per column range
 *     [0, s0), [s0, s1), ... [s_last, n) of col_splits[n_splits] (strictly ascending inside (0, n); none: one range), summed element
 *     by element on the host -- what the exchange of a sharded run does with the zeros the ownership rule leaves.
 * Out, each or NULL: the traceback (room for n / L + 2), first segment first, and its count; the thresholds tau[count][2] =
 * {tau, kind} in the traceback's order and *n_tau, how many were taken (entry 0 is the first segment's own column, which no
 * boundary reads; flag set: 0 where the traceback has one entry or max_size[n - L] >= m, and no launch was made); the merged
 * segments (room for n / L + 2) and their count (0 where max_size[n - L] >= m, and on overflow); info = {a list ended before a
 * threshold could be told, flags bit 0, launches of k_seg_tau, launches of k_seg_count}.
 * The context holds no result afterwards and no lists fseq_debug_column_list would answer for; a following run is unaffected. */
typedef struct fseq_merge_lists_info {
	uint32_t overflow, tau_separate, threshold_launches, count_launches;
} fseq_merge_lists_info;
int  fseq_debug_merge_on_lists(fseq_ctx *ctx, uint32_t list_cap, uint32_t const *ent, uint32_t const *hdr, uint32_t const *lb, uint32_t const *max_size,
                               uint32_t const *size, uint32_t flags, uint64_t const *col_splits, uint32_t n_splits, fseq_dp_arg *traceback,
                               uint64_t *n_traceback, uint32_t *tau, uint64_t *n_tau, fseq_segment *segments, uint64_t *n_segments,
                               fseq_merge_lists_info *info);

/* The traceback as a sharded run in window mode follows it, part by part in one process without ranks (debug / tests; no
 * context).  lb / max_size / size: n - L + 1 words each (the chain check of fseq_debug_merge_on_lists runs first; *bad_entry, or
 * NULL, the entry it names).  part_lo[n_parts], n_parts <= 64, strictly ascending from part_lo[0] == 0: part g holds the entries
 * [part_lo[g], part_lo[g + 1]), the last one up to n - L + 1.  Every part makes its view of lb -- its own entries, every other entry
 * from foreign[n - L + 1], or 0xFFFFFFFF where foreign is NULL -- and runs k_tb_windows(vlo, vhi) on it; the part the chain stands
 * in runs k_tb_chain_part and k_tb_emit(vlo), and its two words go to the host walk a sharded run drives (in place of the
 * exchange).  Out, each or NULL: the whole traceback (room for n / L + 2), first segment first, and its count; part_entries /
 * part_windows [n_parts]: the entries and windows of the chain in each part (0: not visited).  FSEQ_E_HIP where the walk
 * refuses what a part reports, as a sharded run would.  Everything is freed on every exit. */
int  fseq_debug_traceback_parts(int device, uint64_t n, uint64_t segment_length, uint32_t const *lb, uint32_t const *max_size, uint32_t const *size,
                                uint32_t const *part_lo, uint32_t n_parts, uint32_t const *foreign, fseq_dp_arg *traceback, uint64_t *n_traceback,
                                uint32_t *part_entries, uint32_t *part_windows, uint64_t *bad_entry);

/* The packed local pass of phase C's partition step alone (csrc/fseq_localpass.hpp; debug / tests; no context): one workgroup of
 * `threads` threads (a multiple of 64, at most 1024), thread t over the positions [t * E, (t + 1) * E), E = rows_per_thread one of
 * 11, 12, 15.  d / s: threads * E values below 2^16 and symbols 0 .. 4, an unused position (symbol 4) with the value 0;
 * FSEQ_E_ARG otherwise, before the device is touched.  Out: dnew[threads * E], the rows' new values (0 for an unused position),
 * and tails[threads * 4], every thread's maximum behind its last row of each symbol (over all its rows where the symbol is absent). */
int  fseq_debug_local_pass(int device, uint32_t threads, uint32_t rows_per_thread, uint32_t const *d, uint32_t const *s, uint32_t *dnew, uint32_t *tails);

#ifdef __cplusplus
}
#endif
#endif
