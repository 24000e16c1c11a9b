/*
 * fseq.h -- C ABI of the MI355X-native segmentation engine (libfseq_hip.so).
 *
 * Drop-in boundary for ONE path of tsnorri/founder-sequences: everything
 * founder_sequences::segmentation_lp_context does (pBWT pass 1 + minimum-segmentation DP +
 * traceback + pass 2 + greedy segment merge) and segmentation_sp_context::process.
 * The reference has no FFI for this path; its boundary is the C++ delegate pair
 *   segmentation_lp_context_delegate          include/founder_sequences/segmentation_lp_context.hh:45-58
 *   segmentation_context / _delegate          include/founder_sequences/segmentation_context.hh:14-33
 * and the hand-off type
 *   segmentation_container                    include/founder_sequences/segmentation_container.hh:15-20
 * Each entry point below names the reference interface it replaces.  Plain pointers and sizes
 * only; no exceptions and no exit() cross this ABI.  All paths are relative to /root/reference.
 */
#ifndef FSEQ_H
#define FSEQ_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 2: fseq_timings grew (dp_chunks .. reserved), FSEQ_E_PEER, fseq_set_memory_budget, fseq_set_progress /
 *    fseq_step_max / fseq_current_step; the fseq_debug_* entry points moved to include/fseq_debug.h */
/* 3: fseq_shard_abort */
/* 4: fseq_timings grew (phase_a_trie_given_up: 120 -> 128 bytes): a host that calls fseq_get_timings must be rebuilt */
/* 5: fseq_timings grew (reduced_blocks, reduced_rows_mean, reduced_redone: 128 -> 136 bytes) */
#define FSEQ_ABI_VERSION 5

enum {
	FSEQ_OK             = 0,
	FSEQ_E_ARG          = 1,   /* bad argument / call order */
	FSEQ_E_NO_REDUCTION = 2,   /* max segment size >= m: generate_context.cc:192-200 */
	FSEQ_E_HIP          = 3,   /* HIP runtime error, see fseq_last_error */
	FSEQ_E_OOM          = 4,   /* a device (or pinned host) allocation failed; fseq_last_error has the sizes.  Typically the
	                            * per-column lists of a very diverse input: n x (X + 3) x 8 bytes at list capacity X (DESIGN.md
	                            * section 7).  Nothing was written; other contexts of the process are not affected.
	                            * fseq_set_list_memory bounds what the lists of a run may take (the run then holds them in column
	                            * windows); a budget too small for one window fails with this code and names the bytes needed */
	FSEQ_E_UNSUPPORTED  = 5,   /* shape outside what this build's kernels cover (fails loudly, no CPU fallback) */
	FSEQ_E_PEER         = 6    /* sharded run: another rank failed; every rank returns from the same exchange */
};

typedef struct fseq_ctx fseq_ctx;

/* Construction parameters = what segmentation_lp_context reads from its delegate
 * (segmentation_lp_context.hh:47-50): sequence_count(), sequences().front().size(),
 * segment_length(), pbwt_sample_rate(). */
typedef struct fseq_params {
	uint32_t m;                 /* sequence_count()                                   */
	uint64_t n;                 /* sequence length (columns)                           */
	uint64_t segment_length;    /* L, --segment-length-bound (cmdline.ggo:16-17)       */
	uint64_t pbwt_sample_rate;  /* accepted for interface parity; results do not depend on it. The
	                               engine keeps an exact (a,d) state every block_len columns instead. */
	uint32_t block_len;         /* column-block length B; 0 = choose automatically     */
	uint32_t list_cap;          /* X: per-column divergence list covers the X largest entries; 0 = default.
	                               Too small a value is detected and retried internally (results stay exact). */
	int32_t  device;            /* HIP device ordinal                                  */
} fseq_params;

/* Synthetic founder-mosaic input, generated on the device. */
typedef struct fseq_synth_spec {
	uint64_t seed;
	uint32_t n_founders;
	uint32_t block_len;         /* recombination block length */
	uint64_t mut_threshold;     /* mutation iff hash < mut_threshold (= mu * 2^64) */
	uint32_t kind;              /* 0: "ACGT" uniform; 1: "ACGTRYSWKMBDHVN-", P(ACGT)=0.9 */
} fseq_synth_spec;

/* One reduced segment: segmentation_container::reduced_traceback entry
 * (segmentation_dp_arg.hh:18-23 built by the 3-argument constructor at
 * segmentation_lp_context.cc:368,380). */
typedef struct fseq_segment {
	uint64_t lb;                /* inclusive */
	uint64_t rb;                /* exclusive */
	uint32_t segment_size;
	uint32_t reserved;
} fseq_segment;

/* One traceback entry before merging (segmentation_lp_context.cc:191-224). */
typedef struct fseq_dp_arg {
	uint64_t lb, rb;
	uint32_t segment_max_size, segment_size;
} fseq_dp_arg;

typedef struct fseq_result {
	uint32_t max_segment_size;      /* segmentation_container::max_segment_size           */
	uint32_t short_path;            /* 1 if n < 2L (generate_context.cc:386-389)          */
	uint64_t dp_segment_count;      /* S reported by context_did_finish_traceback (:221-223) */
	uint64_t segment_count;         /* S' = reduced_traceback.size()                       */
} fseq_result;

typedef struct fseq_timings {
	double ms_total;                /* wall, whole fseq_run_segmentation call                       */
	double ms_phase_a, ms_phase_b, ms_phase_c, ms_dp, ms_pass2, ms_host;   /* device phases: HIP event time */
	double ms_colstep_kernels;      /* summed HIP-event time of the column-update kernels (A + C + pass 2) */
	uint64_t colstep_launches;      /* number of those launches                            */
	uint64_t colstep_cells;         /* cells (rows x columns) those launches processed     */
	uint64_t pass2_cells;           /* R: cells re-processed for the boundary snapshots    */
	uint32_t list_cap_used;         /* X that produced the result                          */
	uint32_t retries;               /* list_cap retries                                    */
	uint32_t block_len;             /* B in use                                            */
	uint32_t n_blocks;
	uint32_t dp_chunks;             /* chunks of the speculative DP (0: the serial kernel ran)               */
	uint32_t dp_sweeps;             /* sweeps it compared until no key changed (>= 1000: serial fallback took over) */
	uint32_t phase_a_fallbacks;     /* blocks in which a merge of the key-space tree exceeded the LDS bitmap and ran in slices */
	uint32_t phase_a_given_up;      /* blocks the key-space tree handed to the column sweep (their merges would have sliced past the budget) */
	uint32_t phase_a_trie_given_up; /* streamed rows: blocks the trie over 16-column words handed to the key-space tree (too many distinct keys) */
	uint32_t reduced_blocks;        /* [ABI 5] blocks whose column updates ran on their representative rows (0: every block on all rows) */
	uint32_t reduced_rows_mean;     /* ... representatives per such block, mean                                  */
	uint32_t reduced_redone;        /* ... blocks run again on all rows because a list could not be proven on the representatives */
} fseq_timings;

uint32_t    fseq_abi_version(void);
char const *fseq_strerror(int code);

/* replaces: new segmentation_lp_context(delegate, ...)  generate_context.cc:184 */
int  fseq_create(fseq_params const *params, fseq_ctx **out);
/* replaces: segmentation_lp_context::cleanup  segmentation_lp_context.hh:117 */
void fseq_destroy(fseq_ctx *ctx);
char const *fseq_last_error(fseq_ctx const *ctx);

/* ---- a new input on a live context ----
 * Every input setter -- fseq_set_rows, fseq_set_matrix, fseq_set_device_columns, fseq_set_device_columns_packed,
 * fseq_generate_synthetic and the chunked input (fseq_input_begin .. fseq_input_end, fseq_set_rows_streamed) -- may be called
 * again on a context that has run; m and n stay those of fseq_create, the segment length that of fseq_create or of the last fseq_set_segment_length.  Once its arguments are in order the
 * call takes the context for the new alignment:
 *   - the result of the last run is dropped: until the next fseq_run_segmentation, fseq_get_traceback, fseq_get_segments,
 *     fseq_boundary_state, fseq_short_path_runs, the joiners, fseq_write_segments, fseq_write_founders(_device) and
 *     fseq_match_founders return FSEQ_E_ARG, and fseq_last_error says that no run has finished since the input was set;
 *   - the last match is dropped: fseq_get_match and fseq_write_match return FSEQ_E_ARG until the next match;
 *   - the device work buffers of the runs before are released (the next run lays them out for the new alphabet and packing:
 *     a context that cycles through inputs holds no more after the third than after the second) and what runs had learnt of
 *     the old input is forgotten, so the first run on the new input costs what a first run on a fresh context costs;
 *   - a context made by fseq_create_without_identity_columns REFUSES (FSEQ_E_ARG, nothing it holds changes): its identity
 *     relation belongs to the columns it was made from.  Make a new one from the new source.
 * A setter that fails after this point leaves the context without a result, and without an input where it says so.
 *
 * Input = delegate->sequences() (m spans of n raw bytes, founder_sequences.hh:38-40) plus
 * delegate->alphabet() (generate_context.cc:135-147).  rows[r] points at n bytes.  The bytes
 * are mapped to dense codes in ascending byte order and stored column-major in HBM. */
int  fseq_set_rows(fseq_ctx *ctx, uint8_t const *const *rows);
/* Same, from one host buffer: sym(r,c) = base[r*row_stride + c*col_stride]. */
int  fseq_set_matrix(fseq_ctx *ctx, uint8_t const *base, size_t row_stride, size_t col_stride);
/* Input already resident in HBM: column-major dense codes, one per byte, column c at d_codes + c*ld,
 * ld >= m.  sigma = number of codes (codes are < sigma: checked with one pass over the columns, FSEQ_E_ARG if a
 * larger code is found).  The buffer is borrowed, not copied (and not repacked: inputs the library uploads itself
 * are stored at 2 / 4 / 8 bits per cell by sigma).  The code check is one pass over the columns plus a stream
 * synchronisation per call, and only when sigma is below what the code width can hold (sigma = 2^bits: no pass). */
int  fseq_set_device_columns(fseq_ctx *ctx, void const *d_codes, size_t ld, uint32_t sigma);
/* The same for columns that are already packed the way the library stores them: bits = 2, 4 or 8 per
 * code (codes < sigma <= 2^bits), row r of a column in byte r / (8 / bits) at bit (r mod (8 / bits)) * bits,
 * column c at d_packed + c * ld_bytes, ld_bytes a multiple of 16 and >= ceil(m * bits / 8). */
int  fseq_set_device_columns_packed(fseq_ctx *ctx, void const *d_packed, size_t ld_bytes, uint32_t sigma, uint32_t bits);
/* Generate the alignment on the device (bench / large configs). */
int  fseq_generate_synthetic(fseq_ctx *ctx, fseq_synth_spec const *spec);
/* Copy columns [c0,c1) back as raw bytes, out[r*row_stride + (c-c0)*col_stride] (tests, writers). */
int  fseq_get_matrix(fseq_ctx *ctx, uint64_t c0, uint64_t c1, uint8_t *out, size_t row_stride, size_t col_stride);

/* ---- one alignment over several GPUs (one process per GPU) ----
 * replaces: the reference's only parallel axis for this path, independent update_pbwt_task's over column ranges
 * on the global concurrent queue (segmentation_lp_context.cc:319-332, update_pbwt_task.cc:13-35), extended to
 * pass 1: rank r of `world` owns a contiguous range of column blocks -- its share of the alignment, of phases A
 * and C, of the DP chunks and of pass 2.  The exchange steps (the W composite key blocks of phase B, the DP keys
 * after every sweep, the merge thresholds: a few MB in all) go through ONE caller-supplied all-reduce over a
 * caller-owned device buffer; a C++ host passes a function that calls ncclAllReduce on it, the Python mirror one
 * that calls torch.distributed.all_reduce (RCCL) on the tensor that owns the buffer.
 *   fn(user, offset_words, count_words, op): all-reduce xbuf[offset .. offset + count) (uint32 words; op 0 = sum,
 *   1 = max) over all ranks, IN PLACE, and return 0 once the result is visible to work submitted afterwards on
 *   any stream of this device (the library has synchronised its own stream before the call).
 * Call before the input is set (each rank then generates / uploads / borrows only its own columns; borrowed
 * device columns hold the columns [first, last) fseq_shard_columns reports, column `first` at the base pointer).
 * Every rank must make the same calls in the same order; results (fseq_result, traceback, segments, timings)
 * are identical on all ranks, fseq_boundary_state(i) answers on the rank that owns segments[i].rb
 * (fseq_shard_owner) and returns FSEQ_E_ARG elsewhere. */
typedef int (*fseq_allreduce_fn)(void *user, uint64_t offset_words, uint64_t count_words, int op);
/* device words (uint32) the exchange buffer must hold for this context's shape on `world` ranks */
uint64_t fseq_shard_xbuf_words(fseq_ctx const *ctx, uint32_t world);
int  fseq_set_shard(fseq_ctx *ctx, uint32_t rank, uint32_t world, void *xbuf_device, uint64_t xbuf_words,
                    fseq_allreduce_fn fn, void *user);
/* A rank whose HOST failed between two library calls (it could not read its input, allocate a buffer of its own, ...) and
 * will make no further calls on this context: tells the other ranks, who learn of it in the exchange they make next and
 * return FSEQ_E_PEER instead of waiting in a collective.  One status exchange, at most once per context; failures inside
 * the library's own calls (fseq_set_rows, fseq_generate_synthetic, fseq_run_segmentation) are posted by the library
 * itself.  code: what the others see as this rank's error code (0 = FSEQ_E_HIP).  Nothing to do on unsharded contexts. */
int  fseq_shard_abort(fseq_ctx *ctx, int code);
/* columns [*first, *last) this rank holds (its block range plus the few columns of the next rank that its last
 * DP round reads) */
int  fseq_shard_columns(fseq_ctx const *ctx, uint64_t *first, uint64_t *last);
/* rank that owns the boundary state at column rb */
int  fseq_shard_owner(fseq_ctx const *ctx, uint64_t rb, uint32_t *rank);

/* ---- Row-sharded pBWT sweep: BASELINE.json north_star's partition, as a conformance path ----------------------
 * "Rows shard across the GPUs with a per-column sigma-bucket-histogram all-reduce and a boundary exchange for the
 * divergence scan": rank g of `world` owns the positions [m g / world, m (g + 1) / world) of the order (a_k, d_k)
 * and supplies the symbols of the rows fseq_rowshard_rows reports; every column (and 2-bit digit of a wider
 * alphabet) costs two all-reduces through the same fseq_allreduce_fn as above -- the column itself plus the scattered
 * (a, d), and one 12-word summary per rank (bucket counts, running maxima, symbols seen).  The sweep therefore runs
 * at the latency of the collective (DESIGN.md section 6 has the measured curve); the production split of one
 * alignment over GPUs is fseq_set_shard's column blocks, which exchange per phase, not per column.
 * Computes what the per-column update of libbio::pbwt_context computes when founder_sequences.hh:56-65 drives it
 *  over the columns [0, ncols) from the identity order: bit-identical to the single-GPU path.
 * d_cols: device, column-major packed codes < sigma (the layout of fseq_set_device_columns_packed: `bits` per row,
 * row r of a column in byte r * bits / 8, ld bytes from column to column, ld a multiple of 4); only this rank's rows
 * are read.  a_out / d_out: host, m entries each; the entries [*pos_lo, *pos_hi) are written. */
typedef struct fseq_rowshard {
	int32_t  device;
	uint32_t rank, world;
	uint32_t m, sigma, bits;
	uint64_t ncols;
	void const *d_cols;
	size_t   ld;
	void    *xbuf;                 /* device, fseq_rowshard_xbuf_words uint32 words; every rank its own */
	uint64_t xbuf_words;
	fseq_allreduce_fn fn;          /* may be NULL when world == 1 */
	void    *user;
} fseq_rowshard;
uint64_t fseq_rowshard_xbuf_words(uint32_t m, uint32_t bits, uint32_t world);
int  fseq_rowshard_rows(uint32_t m, uint32_t bits, uint32_t rank, uint32_t world, uint32_t *row_lo, uint32_t *row_hi);
int  fseq_rowshard_pbwt(fseq_rowshard const *args, uint32_t *a_out, uint32_t *d_out, uint32_t *pos_lo, uint32_t *pos_hi,
                        double *ms, uint64_t *n_exchanges);

/* replaces: generate_traceback + update_samples_to_traceback_positions + find_segments_greedy
 * (segmentation_lp_context.cc:26-390) or segmentation_sp_context::process
 * (segmentation_sp_context.cc:21-28) when n < 2L.  Returns FSEQ_E_NO_REDUCTION exactly when the
 * reference would print "Unable to reduce the number of sequences" (the traceback is still
 * available then). */
int  fseq_run_segmentation(fseq_ctx *ctx, fseq_result *res);
/* Several independent alignments (chromosomes, windows) at once: one host thread and one stream per
 * context, all in flight together -- the DP of one alignment keeps a single CU busy, so the chip is
 * shared (measured: 8 alignments of BASELINE C2 shape in flight give 3.5x the throughput of one after
 * the other; beyond 4 in flight set GPU_MAX_HW_QUEUES -- the HIP runtime's default of 4 hardware queues
 * makes contexts that share a queue take turns).  results[i] / return_codes[i] are what fseq_run_segmentation(ctxs[i], ...) gives; the
 * return value is FSEQ_OK when every call was made (look at return_codes for their outcomes). */
int  fseq_run_segmentation_batch(fseq_ctx *const *ctxs, size_t count, fseq_result *results, int *return_codes);

/* segmentation_lp_context::m_segmentation_traceback_res (before merging), dp_segment_count entries. */
int  fseq_get_traceback(fseq_ctx *ctx, fseq_dp_arg *out);
/* segmentation_container::reduced_traceback, segment_count entries. */
int  fseq_get_segments(fseq_ctx *ctx, fseq_segment *out);
/* segmentation_container::reduced_pbwt_samples[i]: input_permutation() / input_divergence() at
 * sequence_idx() == segments[i].rb (greedy_matcher.cc:242-257, join_context.cc:73).  m uint32 each. */
int  fseq_boundary_state(fseq_ctx *ctx, uint64_t i, uint32_t *a_out, uint32_t *d_out);
/* Short path result (segmentation_sp_context.hh:28): one (first row id, copy number) per distinct
 * row in pBWT order; returns max_segment_size entries. */
int  fseq_short_path_runs(fseq_ctx *ctx, uint32_t *first_idx, uint32_t *run_len);

/* ---- segment joining on the host ----
 * replaces: join_context::join_greedy -> greedy_matcher::match (join_context.cc:211-229,
 * greedy_matcher.cc:204-465).  permutations: segment_count x max_segment_size uint32, row-major;
 * permutations[s][r] = index of the input sequence whose [lb_s, rb_s) substring is founder r's
 * content in segment s.
 * The class tables and the co-occurrence edges are built on the device, where the boundary states are, and the host hands out
 * the copies and draws the edges: up to 181 classes a segment with the pair's counters in one LDS matrix, above that (up to
 * 65,535), from 16 MiB of boundary states on, in strips of left classes.  Everything else -- smaller inputs above 181 classes,
 * a failed device allocation -- goes through the all-host joiner; the permutations are the same entry for entry
 * (fseq_debug_join_path tells which ran). */
int  fseq_join_greedy(fseq_ctx *ctx, uint32_t *permutations);
/* The same matcher on caller-supplied boundary states (no context, no device): segments given as
 * lb[i], rb[i]; a, d: n_segments x m.  Used by the CPU tests of the host logic. */
int  fseq_greedy_match_host(uint32_t m, uint32_t max_segment_size, uint64_t n_segments, uint64_t const *lb, uint64_t const *rb,
                            uint32_t const *a, uint32_t const *d, uint32_t *permutations);
/* ---- the non-greedy joiners, host C++ as in the reference ----
 * replaces: join_context::join_with_bipartite_matching -> bipartite_matcher::match (join_context.cc:231-236,
 * bipartite_matcher.cc:17-151, create_segment_texts_task.cc:15-81, merge_segments_task.cc:133-195 with
 * INTERSECTION scoring, main.cc:126).  Lemon's MaxWeightedPerfectMatching is replaced by an own
 * Kuhn-Munkres: every matching has the optimal total weight; which optimal matching Lemon picks is
 * not reproduced (parity unpinned).  Texts of equal size keep their classes' pBWT order
 * (the reference's std::sort leaves it to its standard library).  [r5] fseq_join_bipartite runs on the
 * device where the boundary states are while the run is not sharded and the merged segments tile the columns -- the same
 * permutations, entry for entry, as the host form below.  Up to 181 texts a segment a pair's weight matrix and its
 * Kuhn-Munkres state are one workgroup's LDS (csrc/fseq_joinbip.hpp).  Above that and up to 4,096 texts, from 16 MiB of
 * boundary states (segments x m x 8 bytes) on, the wide form runs (csrc/fseq_joinbipw.hpp): the weights of a pair in a slab
 * of max_segment_size^2 words of device memory, one slab per persistent workgroup, which solves its pairs one after the
 * other with 64-bit potentials in LDS; as many slabs as the pairs, the CUs, half of the free device memory and of what is left
 * of fseq_set_memory_budget allow.  Everything else goes through the host joiner, which copies every boundary state to the
 * host: more than 4,096 texts, smaller inputs above 181 texts, a failed device allocation (not one slab fits), implausible
 * class counts (a sharded run is refused there, as before).  fseq_debug_bipartite_path (fseq_debug.h) tells which ran. */
int  fseq_join_bipartite(fseq_ctx *ctx, uint32_t *permutations);
/* replaces: join_context::join_random_order_and_output (join_context.cc:259-289): std::mt19937(seed),
 * one std::shuffle per segment.  The joiner reads nothing of a boundary state but its classes' first rows and sizes, so
 * while the run is not sharded, the merged segments tile the columns and max_segment_size is at most 65,535 the class
 * tables are made where the boundary states are (k_join_classes_wide) and segments x max_segment_size x 8 + segments x 4
 * bytes come to the host instead of segments x m x 8; the host part -- copy numbers, slots, shuffles -- is the same code on
 * the same vectors, so the permutations are the host joiner's entry for entry.  A failed device allocation or a class
 * count outside [1, max_segment_size] goes through the host joiner (FSEQ_JOIN_HOST forces it), which refuses a sharded
 * run.  fseq_debug_random_path (fseq_debug.h) tells which ran. */
int  fseq_join_random(fseq_ctx *ctx, uint32_t seed, uint32_t *permutations);
/* The same joiners on caller-supplied boundary states (no context, no device).  weights (optional):
 * n_segments - 1 total matching weights. */
int  fseq_bipartite_match_host(uint32_t m, uint32_t max_segment_size, uint64_t n_segments, uint64_t const *lb, uint64_t const *rb,
                               uint32_t const *a, uint32_t const *d, uint32_t *permutations, int64_t *weights);
int  fseq_random_join_host(uint32_t m, uint32_t max_segment_size, uint64_t n_segments, uint64_t const *lb, uint64_t const *rb,
                           uint32_t const *a, uint32_t const *d, uint32_t seed, uint32_t *permutations);
/* The random joiner from the runs on (join_context.cc:259-289 behind unique_substring_count_idxs_lhs), on caller-supplied
 * class tables (no context, no device): count[s] classes of segment s in pBWT order, rep / size [n_segments][max_segment_size]
 * their first rows in that order and their row counts.  What fseq_join_random runs behind its device front.
 * FSEQ_E_ARG: a null pointer, m or max_segment_size 0, a count outside [1, max_segment_size]. */
int  fseq_random_join_classes_host(uint32_t m, uint32_t max_segment_size, uint64_t n_segments, uint32_t const *count, uint32_t const *rep,
                                   uint32_t const *size, uint32_t seed, uint32_t *permutations);
/* ---- what a join is worth: junction support per adjacent segment pair and founder slot (no counterpart in the reference) ----
 * A finished run has S merged segments that tile the columns; X is max_segment_size; permutations is [S][X], an entry < m the
 * input row whose substring the founder of that slot takes in that segment, an entry >= m a gap (fseq_write_founders_device
 * prints '-').  cls_s(i) is the class of row i in segment s: two rows are in one class iff they agree on [lb_s, rb_s).  At the
 * junction p = (s, s + 1) slot r has L = permutations[s][r] and R = permutations[s + 1][r], and
 *   support[p][r] = the rows i with cls_s(i) = cls_s(L) and cls_{s+1}(i) = cls_{s+1}(R); 0 where L or R is a gap
 * -- the input rows that carry the founder's substring on both sides of the border, the quantity every joiner works on.
 * A junction's entry: supported -- slots with support > 0; unsupported -- slots with support 0 that are no gaps; gaps -- slots
 * where L or R is a gap (the three add up to X); weight -- the sum of support over the slots; rows_through -- the rows i for
 * which some slot has (cls_s(L), cls_{s+1}(R)) = (cls_s(i), cls_{s+1}(i)): the rows that can cross the junction without
 * changing founder, a pair of classes that several slots share counted once; rb -- the border's column, rb_s.
 * breaks[r]: the junctions at which slot r is unsupported.  The summary: the totals of the five fields over the junctions, the
 * smallest rows_through and the first junction it is at (m and 0 where S = 1), the largest breaks, and the call's wall time. */
typedef struct {
	uint64_t rb;
	uint64_t weight;
	uint32_t supported, unsupported, gaps, rows_through;
} fseq_join_score_entry;
typedef struct {
	uint64_t junctions;                     /* S - 1 */
	uint64_t supported, unsupported, gaps, rows_through, weight;
	uint64_t min_rows_through_junction;
	uint32_t min_rows_through, max_breaks;
	double   ms_device;
} fseq_join_score_summary;
/* The score of any permutations -- a joiner's or the caller's own -- on the context of a finished run.  junctions [S - 1],
 * breaks [X], support [(S - 1) x X] and summary may each be NULL.  While the merged segments tile the columns, X <= 4,096,
 * m and S < 2^31 and FSEQ_JOIN_HOST is not set, the score is computed where the boundary states are (csrc/fseq_joinscore.hpp):
 * the class tables of k_join_classes_wide, then one workgroup per junction with the slots' class pairs in an LDS table and
 * one pass over the rows' classes; permutations go to the device (S x X x 4 bytes), the results come back.  Everything else --
 * X > 4,096, a failed device allocation, class counts outside [1, X] read back -- copies every boundary state and runs the
 * host form below, with the same results entry for entry (fseq_debug_join_score_path, fseq_debug.h, tells which ran).
 * FSEQ_E_ARG: no permutations, no finished run; FSEQ_E_UNSUPPORTED: a sharded context (collect the boundary states and use
 * fseq_join_score_host).  Existing results and buffers of the context are left as they are. */
int  fseq_join_score(fseq_ctx *ctx, uint32_t const *permutations, fseq_join_score_entry *junctions, uint32_t *breaks, uint32_t *support,
                     fseq_join_score_summary *summary);
/* The same on caller-supplied boundary states (no context, no device), the arguments of fseq_greedy_match_host and the
 * permutations: classes by the rule of the joiners' host forms (a pBWT position i starts a class iff i = 0 or d[i] > lb).
 * Any max_segment_size.  FSEQ_E_ARG: a NULL input, m or max_segment_size 0, no segment, an entry of a that is no row. */
int  fseq_join_score_host(uint32_t m, uint32_t max_segment_size, uint64_t n_segments, uint64_t const *lb, uint64_t const *rb,
                          uint32_t const *a, uint32_t const *d, uint32_t const *permutations, fseq_join_score_entry *junctions,
                          uint32_t *breaks, uint32_t *support, fseq_join_score_summary *summary);
/* replaces: join_context::output_segments -> output_segments (segmentation_dp_arg.cc:13-104): the
 * --output-segments text file for the given joining method (greedy: the header line only, SURVEY.md
 * F5; bipartite: one line per segment text; random: one line per distinct substring with its copy
 * number).  path NULL or "-" = stdout. */
enum { FSEQ_JOIN_GREEDY = 0, FSEQ_JOIN_BIPARTITE = 1, FSEQ_JOIN_RANDOM = 2 };
int  fseq_write_segments(fseq_ctx *ctx, uint8_t const *const *rows, int joining, char const *path);
/* The same with the boundary states supplied by the caller (S' x m words each, segment-major): a sharded run, where
 * they sit on their owner ranks (fseq_shard_owner / fseq_boundary_state) and the host collects them. */
int  fseq_write_segments_host(fseq_ctx *ctx, uint8_t const *const *rows, int joining, uint32_t const *a, uint32_t const *d, char const *path);
/* replaces: the same (segmentation_dp_arg.cc:13-104) from what the device holds (csrc/fseq_segfile.hpp): the bytes are those
 * fseq_write_segments writes when given the raw rows of the alignment the context holds -- uploaded, streamed, generated or
 * borrowed (one code per byte or packed); on a context made by fseq_create_without_identity_columns the reduced
 * co-ordinates and the reduced rows' bytes.  No host rows and no copy of the boundary states (segments x m x 8 bytes): the
 * class tables, the texts, the sorted row list of every text, the decoded substrings and the decimal text are made where
 * the boundary states are, and the file leaves in batches of whole lines of at most 256 MiB (FSEQ_SEGFILE_BATCH), one copy
 * and one write a batch.  For random joining the lines' order is the host's own std::sort on the device's class tables.
 * Greedy: the header line only, no device work.  Refuses, each with fseq_last_error set and no other bytes written:
 * FSEQ_E_ARG -- no run since the input was set, no resident alignment, an unknown joining, an output file that cannot be
 * opened; FSEQ_E_UNSUPPORTED -- a sharded context, merged segments that do not tile the columns, bipartite joining with
 * more than 4,096 texts a segment, random joining with more than 65,535, a class count outside [1, max_segment_size] read
 * back from the device (fseq_write_segments serves these from host rows); FSEQ_E_OOM -- a failed allocation, which leaves
 * nothing behind and the context usable.  fseq_debug_segments_file (fseq_debug.h) reports the batches.
 * path NULL or "-" = stdout. */
int  fseq_write_segments_device(fseq_ctx *ctx, int joining, char const *path);
/* ---- the founder block graph of a finished run (no counterpart in the reference) ----
 * A finished run has S merged segments that tile the columns.  The graph's nodes are the classes of every segment -- the
 * distinct substrings of the rows over [lb_s, rb_s) --, its edges join class l of segment s to class r of segment s + 1 and
 * weigh the input rows that carry both; every input row is a path of S nodes.  Node ids are 0-based, id(s, c) = the classes of
 * the segments in front of s plus c, where c is the class number the joiners, the segments file and the join score share
 * (k_join_classes_wide, csrc/fseq_joinprep.hpp: the classes in the order of their first pBWT position at rb_s).  A node:
 * its segment and class, the segment's [lb, rb), rep_row -- the first row of the class in that order, whose bytes the
 * label is taken from --, rows -- the size of the class.  An edge: from / to are node ids, rows its weight, junction = the left
 * segment; the edges are ordered by junction, then (l, r) ascending.  The weights of a junction add up to m, and so do the
 * rows of a segment's nodes. */
typedef struct { uint64_t lb, rb; uint32_t segment, cls, rep_row, rows; } fseq_graph_node;      /* 32 bytes */
typedef struct { uint32_t from, to, rows, junction; } fseq_graph_edge;                           /* 16 bytes */
typedef struct { uint64_t segments, nodes, edges; double ms_device; } fseq_graph_summary;
/* The graph as arrays, computed where the boundary states are (the class tables and the edge kernel of fseq_join_greedy's
 * device front): nodes [summary.nodes], edges [summary.edges], row_nodes [S][m] -- the node of every row in every segment --
 * and summary may each be NULL; with the three arrays NULL the call counts, so that a caller can size them.  On a context
 * made by fseq_create_without_identity_columns lb / rb are in reduced co-ordinates, as fseq_write_segments_device's.
 * Refuses, each with fseq_last_error set and the context and its results left as they were: FSEQ_E_ARG -- no finished
 * long-path run; FSEQ_E_UNSUPPORTED -- a sharded context, merged segments that do not tile the columns, more than 65,535
 * classes in a segment, a right segment of more than 32,768 (the edge kernel reports none), 2^32 nodes or edges or more, 2^31
 * rows or segments or more, a class count outside [1, max_segment_size] read back; FSEQ_E_OOM -- a failed allocation, with
 * nothing left behind.  There is no host form. */
int  fseq_block_graph(fseq_ctx *ctx, fseq_graph_node *nodes, fseq_graph_edge *edges, uint32_t *row_nodes, fseq_graph_summary *summary);
/* The graph as a GFA 1.0 file, written from the device (csrc/fseq_graph.hpp).  Tab-separated, '\n'-terminated:
 *   H	VN:Z:1.0
 *   S	<id+1>	<label>	LN:i:<len>	RC:i:<rows>	sg:i:<segment>	lb:i:<lb>	rb:i:<rb>     one per node, in id order
 *   L	<from+1>	+	<to+1>	+	0M	RC:i:<rows>                                      one per edge, in edge order
 *   P	<row>	<id+1>+,<id+1>+,...	*                                                one per input row 0 .. m - 1, with FSEQ_GRAPH_PATHS
 * <label> is the representative row's bytes over [lb, rb) without every byte equal to gap_byte (gap_byte < 0: every byte
 * stays); <len> its length; an empty label prints '*' with LN:i:0.  The bytes are the alignment's own, decoded through the
 * context's code table: keeping them inside GFA's sequence alphabet is the caller's business.  The concatenated labels of a P
 * line spell the row without its gap bytes.  The file leaves in batches of whole lines of at most 256 MiB (FSEQ_GRAPH_BATCH),
 * one copy and one write a batch (fseq_debug_graph_file, fseq_debug.h, reports them).  Needs the alignment resident on the
 * device and no rows on the host: contexts filled in chunks, made by fseq_create_without_rows or by
 * fseq_create_without_identity_columns (reduced co-ordinates and the reduced rows' bytes) are served.
 * Refuses as fseq_block_graph, and FSEQ_E_ARG for no resident alignment, gap_byte > 255, a flag bit other than
 * FSEQ_GRAPH_PATHS and an output file that cannot be opened -- each with no byte written.  path NULL or "-" = stdout. */
enum { FSEQ_GRAPH_PATHS = 1 };
int  fseq_write_block_graph(fseq_ctx *ctx, uint32_t flags, int gap_byte, char const *path);
/* ---- rows that are NOT the graph's own threaded through it (no counterpart in the reference) ----
 * For query row q and segment s, node[s][q] is the id (fseq_block_graph's numbering) of the node of segment s whose rows' codes
 * over [lb_s, rb_s) equal the query's there -- code by code, a gap a symbol like any other, a query byte outside the
 * alignment's alphabet equal to nothing --, or FSEQ_GRAPH_NONE where the segment has no such node.  For junction p (segments p
 * and p + 1), step[p][q] is the index into fseq_block_graph's edges of the edge (node[p][q], node[p + 1][q]), or
 * FSEQ_GRAPH_NONE where either side is unmatched or the graph has no such edge; both sides matched and no edge is a NOVEL
 * junction: the row recombines there as no input row does.  A WALK is a maximal run of consecutive matched segments with every
 * junction between them linked; a row is ON THE GRAPH iff it is one walk of S segments.
 * Per row: the matched segments and their columns, the linked and the novel junctions, the walks, and the most segments and the
 * most columns a walk of the row has (each its own maximum).  Per segment: the queries matched in it and, for the junction
 * behind it, those linked and those novel (0 for the last segment).  The summary adds up the rows'; its ms_device is the wall time
 * of the call behind the upload: the class tables and edges, the kernels, the copies back.
 * nodes is [S][n_rows] (row_nodes' layout), steps [S - 1][n_rows]; every output pointer may be NULL, and with nodes and steps
 * NULL only the statistics leave the device.  fseq_graph_thread_rows takes n raw bytes per query; they go up in column chunks
 * through at most 64 MiB of staging into a buffer of the call's own, through the context's code table, packed at the narrowest
 * of 2 / 4 / 8 bits that leaves the code `sigma` for a byte outside the alphabet.  fseq_graph_thread_held_out threads the
 * held-out rows of a context made by fseq_create_without_rows where they lie on the device: nothing is uploaded, query q is
 * held_rows[q].  Everything is a temporary of the call: the run's results and the context's last match (fseq_get_match,
 * fseq_write_match) stay as they were.  The node of a (query, segment) is found through a 64-bit key of the codes, and every
 * candidate is compared code by code with the class's representative row: the result is exact whatever the keys do
 * (FSEQ_GRAPH_THREAD_KEY_BITS truncates them; fseq_debug_graph_thread, fseq_debug.h, counts the candidates).
 * Refuses, each with fseq_last_error set and nothing left behind: as fseq_block_graph, with its codes; FSEQ_E_UNSUPPORTED --
 * more than 4,096 classes in a segment (there is no host form), a context made by fseq_create_without_identity_columns or its
 * _held form (source co-ordinates with exception cells are not served); FSEQ_E_ARG -- rows NULL, a NULL row, n_rows = 0, no
 * alignment resident on the device, fseq_graph_thread_held_out on a context not made by fseq_create_without_rows. */
enum { FSEQ_GRAPH_NONE = 0xFFFFFFFFu };
typedef struct { uint64_t columns_matched, longest_walk_columns;
                 uint32_t segments_matched, junctions_linked, junctions_novel, walks, longest_walk_segments, reserved; } fseq_graph_thread_row;      /* 40 bytes */
typedef struct { uint32_t matched, linked, novel, reserved; } fseq_graph_thread_segment;   /* 16 bytes; linked / novel: the junction behind the segment, 0 for the last */
typedef struct { uint64_t rows, segments, segments_matched, junctions_linked, junctions_novel, walks, rows_on_graph; double ms_device; } fseq_graph_thread_summary;
int  fseq_graph_thread_rows(fseq_ctx *ctx, uint8_t const *const *rows, uint32_t n_rows,
                            uint32_t *nodes /* [S][n_rows] */, uint32_t *steps /* [S-1][n_rows] */,
                            fseq_graph_thread_row *per_row /* [n_rows] */, fseq_graph_thread_segment *per_segment /* [S] */,
                            fseq_graph_thread_summary *summary);
int  fseq_graph_thread_held_out(fseq_ctx *ctx, uint32_t *nodes, uint32_t *steps, fseq_graph_thread_row *per_row,
                                fseq_graph_thread_segment *per_segment, fseq_graph_thread_summary *summary);
/* ---- the block graph in the SOURCE's co-ordinates on an identity-reduced context (no counterpart in the reference) ----
 * ctx was made by fseq_create_without_identity_columns, its _held form or the reduce-on-upload input
 * (fseq_set_rows_streamed_without_identity_columns, fseq_input_end_kept), and has a finished long-path run whose S merged
 * segments tile the kept columns.  Segment s owns the source range [src_lb_s, src_rb_s) of fseq_get_segments_restored.  The
 * classes, node ids, edges, row_nodes and the P and L lines are the reduced graph's, unchanged: rows that agree on the kept
 * columns of a segment agree on its whole source range, and identity columns do not move the pBWT order.  So fseq_block_graph
 * serves these contexts as it is; the `segment` of its nodes indexes fseq_get_segments_restored, whose lb / rb are the node's
 * source range.
 * The RESTORED LABEL of node (s, j) has, for p ascending over [src_lb_s, src_rb_s): row 0's byte of the source where p is an
 * identity column, otherwise the representative row's byte at the kept column c with kept[c] == p; bytes equal to the gap
 * byte left out; '*' if nothing is left.
 * fseq_write_block_graph_restored writes fseq_write_block_graph's file -- the header, every L line and every P line equal
 * that call's byte for byte -- with the restored label, its LN and lb / rb = src_lb_s / src_rb_s in every S line: the
 * concatenated labels of a P line spell the source's row without its gap bytes.  Batches, FSEQ_GRAPH_BATCH and
 * fseq_debug_graph_file as there.
 * A query of n_src bytes CARRIES node (s, j) iff its codes at the kept columns of the segment equal the node's (the rule of
 * fseq_graph_thread_rows: a byte outside the alphabet equals nothing) and it has no exception cell in [src_lb_s, src_rb_s) --
 * an identity column in which it differs from row 0, by a byte outside the alphabet as by any other.
 * fseq_graph_thread_rows_restored takes n_src raw bytes per query (uploaded once: the kept columns packed, the exception cells
 * listed, both in temporaries of the call); fseq_graph_thread_held_out_restored threads the held-out rows a context made by
 * fseq_create_without_identity_columns_held carries, with the exception cells it was made with.  Outputs as their twins';
 * columns_matched and longest_walk_columns count SOURCE columns.  Both leave the run's results and the context's last match
 * as they were, the exception lists of a restored match included (fseq_get_match_exceptions answers as before).
 * Refuse, each with nothing written and nothing left behind: what the reduced twin refuses, with its code (but that the context
 * is identity-reduced); FSEQ_E_ARG -- a context that is not identity-reduced, the held-out form on a context without carried
 * held-out rows; FSEQ_E_UNSUPPORTED -- where fseq_get_segments_restored refuses (a source of 2^32 - 1 columns or more), for
 * the threads more than 4,096 classes in a segment.  Not for sharded contexts; there is no host form. */
int  fseq_write_block_graph_restored(fseq_ctx *ctx, uint32_t flags, int gap_byte, char const *path);
int  fseq_graph_thread_rows_restored(fseq_ctx *ctx, uint8_t const *const *rows /* n_src bytes each */, uint32_t n_rows,
                                     uint32_t *nodes /* [S][n_rows] */, uint32_t *steps /* [S-1][n_rows] */,
                                     fseq_graph_thread_row *per_row /* [n_rows] */, fseq_graph_thread_segment *per_segment /* [S] */,
                                     fseq_graph_thread_summary *summary);
int  fseq_graph_thread_held_out_restored(fseq_ctx *ctx, uint32_t *nodes, uint32_t *steps, fseq_graph_thread_row *per_row,
                                         fseq_graph_thread_segment *per_segment, fseq_graph_thread_summary *summary);
/* ---- the NEAREST node of every segment, and how far it is, for rows threaded through the graph (no counterpart in the reference) ----
 * The threading above is all or nothing per (row, segment): a query with one private variant in a segment is reported like one
 * that matches nothing there.  These entries answer how far the row is from the graph, which node it is nearest to, whether that
 * node is unique, and how the row walks if up to max_distance mismatches a segment are forgiven.  The context is one
 * fseq_graph_thread_rows accepts: a finished long-path run, unsharded, not identity-reduced, merged segments tiling the columns;
 * node ids, classes, representative rows and edges are fseq_block_graph's.
 *   dist(q, s, j)    the number of columns k in [lb_s, rb_s) where the code of query q differs from the code of the
 *                    representative row of class j of segment s -- by code, as in the threading: a gap is a symbol like any
 *                    other, a query byte outside the alignment's alphabet differs from every code
 *   distance[s][q]   min over j of dist(q, s, j)
 *   nodes[s][q]      noff[s] + the smallest j that attains the minimum (noff[s]: the id of the segment's class 0)
 *   ties[s][q]       the number of classes of segment s that attain the minimum, at least 1
 * Every segment has a class, so all three are always defined: none is ever FSEQ_GRAPH_NONE.  Cell (s, q) is ADMITTED iff
 * distance[s][q] <= max_distance, and EXACT iff the distance is 0.  steps[p][q] is the index into fseq_block_graph's edges of the
 * edge (nodes[p][q], nodes[p + 1][q]) if both cells are admitted and the edge exists, FSEQ_GRAPH_NONE otherwise.  Novel junction,
 * walk and on-the-graph are the threading's with "matched" read as "admitted".  With max_distance = 0, nodes where the distance
 * is 0 (FSEQ_GRAPH_NONE elsewhere), steps and every walk statistic equal fseq_graph_thread_rows' entry for entry.
 * Per row: the admitted cells' columns, the most columns and the most segments of a walk, the sum of the distances over the
 * admitted cells and over all cells, the admitted and the exact cells, the linked and the novel junctions, the walks and the
 * row's largest distance.  Per segment: the sum of the distances over the queries, the queries admitted and exact in it, those
 * linked and novel at the junction behind it (0 for the last), and the largest distance.  The summary adds up the rows'; its
 * ms_device is measured as the threading's.  nodes, distances and ties are [S][n_rows], steps [S - 1][n_rows]; every output
 * pointer may be NULL, and with the four arrays NULL only statistics leave the device.
 * The rows form uploads its queries as fseq_graph_thread_rows does (the narrowest of 2 / 4 / 8 bits that leaves the code `sigma`
 * free); the held-out form reads the held-out rows where they lie.  The class representatives of a batch of whole segments and
 * the queries are packed into row-major words at the queries' width, every segment on a word boundary, and compared 32 / width
 * codes an operation (csrc/fseq_graphnearest.hpp); a batch holds at most FSEQ_GRAPH_NEAREST_BATCH bytes (by itself 256 MiB) of
 * representative words, a segment above that is a batch of its own (fseq_debug_graph_nearest_info, fseq_debug.h).  Everything
 * is a temporary of the call: the run's results, the last match and fseq_debug_graph_thread's record stay as they were.
 * Refuses, each with fseq_last_error set, nothing written and nothing left behind: what fseq_graph_thread_rows / _held_out
 * refuse, but for the 4,096 classes a segment (there is no table in LDS here: the limits are fseq_block_graph's), and
 * FSEQ_E_UNSUPPORTED a segment of 2^32 - 1 columns or more (distances are 32-bit).  Out of scope: identity-reduced contexts
 * (source co-ordinates with exception cells), sharded contexts and a host form.  Detected by symbol; FSEQ_ABI_VERSION stays 5. */
typedef struct { uint64_t columns_admitted, longest_walk_columns, mismatches_admitted, mismatches;
                 uint32_t segments_admitted, segments_exact, junctions_linked, junctions_novel, walks, longest_walk_segments,
                          max_distance, reserved; } fseq_graph_nearest_row;                 /* 64 bytes */
typedef struct { uint64_t mismatches; uint32_t admitted, exact, linked, novel, max_distance, reserved; } fseq_graph_nearest_segment;   /* 32 bytes */
typedef struct { uint64_t rows, segments, segments_admitted, segments_exact, junctions_linked, junctions_novel, walks, rows_on_graph,
                          mismatches; double ms_device; } fseq_graph_nearest_summary;
int  fseq_graph_nearest_rows(fseq_ctx *ctx, uint8_t const *const *rows, uint32_t n_rows, uint32_t max_distance,
                             uint32_t *nodes /* [S][n_rows] */, uint32_t *distances /* [S][n_rows] */, uint32_t *ties /* [S][n_rows] */,
                             uint32_t *steps /* [S-1][n_rows] */, fseq_graph_nearest_row *per_row /* [n_rows] */,
                             fseq_graph_nearest_segment *per_segment /* [S] */, fseq_graph_nearest_summary *summary);
int  fseq_graph_nearest_held_out(fseq_ctx *ctx, uint32_t max_distance, uint32_t *nodes, uint32_t *distances, uint32_t *ties, uint32_t *steps,
                                 fseq_graph_nearest_row *per_row, fseq_graph_nearest_segment *per_segment, fseq_graph_nearest_summary *summary);
/* replaces: join_context::output_in_permutation_order (join_context.cc:333-356): max_segment_size
 * lines; line r = concatenation over segments of rows[permutations[s][r]][lb_s, rb_s).  rows = the
 * raw input sequences.  path NULL or "-" = stdout. */
int  fseq_write_founders(fseq_ctx *ctx, uint8_t const *const *rows, uint32_t const *permutations, char const *path);
/* [ABI 5] the same from the alignment the device holds (uploaded, generated or borrowed): the lines are put together on the
 * device and leave in one copy per batch of rows; no host rows needed.  Not for sharded runs (a rank holds its own columns). */
int  fseq_write_founders_device(fseq_ctx *ctx, uint32_t const *permutations, char const *path);

/* ---- matching the input rows against founders on the device ----
 * replaces: match-sequences-to-founders (match_founder_sequences.cc:108-259, match-sequences-to-founders/cmdline.ggo): every
 * input row is threaded through the founders greedily -- keep the set of founders that still agree with the row; when it would
 * run empty, or, with min_segment_length != 0, as soon as the running piece has that length, close the piece [lb, rb) with the
 * set as it was and start again from all founders.  A cell whose symbol no founder has at its column (an uncovered cell) closes
 * the running piece and gives a one-column piece with an empty set, except in the last column, where the tool prints none; a
 * piece that a mismatch closes while it is shorter than min_segment_length is a short piece (the tool's "under the given
 * limit" line).  The corners are the tool's (an uncovered cell in column 0 first closes the piece [0, 0) of all founders).
 * The alignment the context holds (uploaded, generated or borrowed) is the input; at most 2,048 founders
 * (FSEQ_E_UNSUPPORTED beyond, csrc/fseq_match.hpp); not for sharded contexts (a rank holds its own columns only).  Pieces are
 * ordered by row, then lb; a founder set is set_words = ceil(K / 32) words, founder f at bit f % 32 of word f / 32.  Nothing
 * of the segmentation's state is touched, and nothing is allocated before the first match. */
typedef struct fseq_match_piece { uint64_t lb, rb; uint32_t row, n_founders; } fseq_match_piece;     /* 24 bytes */
typedef struct fseq_match_summary {
	uint64_t pieces, uncovered_cells, short_pieces, max_pieces_per_row;
	uint32_t n_founders, set_words;          /* K, W */
	double   ms_device;                      /* HIP event time of the founders' columns + both walks */
} fseq_match_summary;
/* founders = what fseq_write_founders_device would write for these permutations (a slot >= m is a line of '-'); needs a
 * finished long-path run (FSEQ_E_ARG before one and on a short-path result, which has no permutations: its founders are the
 * rows fseq_short_path_runs names, to be handed to fseq_match_founder_rows) */
int  fseq_match_founders(fseq_ctx *ctx, uint32_t const *permutations, uint64_t min_segment_length, fseq_match_summary *out);
/* founders = K caller-supplied rows of n raw bytes (--founders with --founders-format text, cmdline.ggo); needs only the
 * alignment (no run).  A byte outside the alignment's alphabet matches no row. */
int  fseq_match_founder_rows(fseq_ctx *ctx, uint8_t const *const *founders, uint32_t K, uint64_t min_segment_length, fseq_match_summary *out);
/* result of the last match on the context: `pieces` entries, pieces x set_words mask words (either may be NULL) */
int  fseq_get_match(fseq_ctx *ctx, fseq_match_piece *pieces, uint32_t *founder_sets);
/* the tool's stdout, byte for byte (header line, then SEQUENCE_INDEX LB RB FOUNDER_INDICES per piece,
 * match_founder_sequences.cc:125-136, :220); path NULL or "-" = stdout */
int  fseq_write_match(fseq_ctx *ctx, char const *path);
/* Rows that are NOT the alignment's (held-out validation): n_rows query rows of n raw bytes each, rows[q] the bytes of query q,
 * matched against the founders of the finished run (permutations, as fseq_match_founders) or against K raw founder rows
 * (founders / K, as fseq_match_founder_rows) -- exactly one of the two is given, FSEQ_E_ARG otherwise.  The queries go through the
 * context's code table; a byte outside the alignment's alphabet is an uncovered cell, as in the tool.  They are uploaded in
 * column chunks through a temporary of at most 64 MiB and held packed like the alignment.  The walk is split along the
 * columns over workgroups and checked for exactness (csrc/fseq_match.hpp; fseq_debug_match_split tells how it went).
 * fseq_match_piece::row is the query index; the report of fseq_write_match is match-sequences-to-founders' stdout for these
 * sequences and founders.  Refusals as the other entries (sharded context, no alignment, K > 2,048, n >= 2^32 - 1, permutations
 * without a finished long-path run); FSEQ_E_ARG also for rows == NULL, a NULL row, n_rows == 0 and a context made by
 * fseq_create_without_identity_columns (its columns are the kept ones of a longer source: fseq_match_rows_restored takes
 * full-length queries there).  The result replaces the context's last match.  Detected by symbol: FSEQ_ABI_VERSION stays 5. */
int  fseq_match_rows(fseq_ctx *ctx, uint32_t const *permutations, uint8_t const *const *founders, uint32_t K,
                     uint8_t const *const *rows, uint32_t n_rows, uint64_t min_segment_length, fseq_match_summary *out);

/* ---- identity columns dropped and put back on the device ----
 * replaces: remove-identity-columns (remove-identity-columns/main.cc:105-153 the comparison of a chunk of every text,
 * :157-227 the driver that writes m reduced files and the 0 / 1 string) in front of founder_sequences, and
 * insert-identity-columns (insert-identity-columns/main.cc:138-195) behind it.  An identity column is one in which all m
 * rows carry the same symbol (m == 1: every column).  The alignment the context holds is the input; the entry points are
 * detected by symbol (FSEQ_ABI_VERSION is unchanged: no struct of the boundary changed). */
typedef struct fseq_identity_summary {
	uint64_t n, identity, kept;     /* columns of the source, identity columns, n - identity */
	double   ms_device;             /* HIP event time of the mask pass (+ scan and gather when a context was made) */
} fseq_identity_summary;
/* replaces: main.cc:105-153 over the whole alignment.  mask[k] = 1 iff column k is an identity column; mask (n bytes) may
 * be NULL (the summary alone).  The source is any context with a resident alignment -- uploaded, generated, borrowed one code
 * per byte or borrowed packed -- and needs no run.  Read-only on the context: nothing of the segmentation's state is touched,
 * and what the call allocates it frees.  A sharded context returns FSEQ_E_UNSUPPORTED (a rank holds its own columns only). */
int  fseq_identity_columns(fseq_ctx *ctx, uint8_t *mask /* n bytes */, fseq_identity_summary *out);
/* replaces: main.cc:157-227 without the m reduced files: a new, ordinary context over the kept columns only.
 * params->n must be 0 and params->m 0 or the source's (FSEQ_E_ARG otherwise): n becomes `kept`, m is the source's;
 * segment_length, block_len, list_cap and pbwt_sample_rate are taken from params, and params->device must be the source's
 * device.  The new context owns its alignment (columns padded to 16 bytes, padding zeroed) and keeps the source's sigma,
 * code table and code width as they are: a symbol that occurred only in identity columns keeps its code, and since the order
 * of the codes is unchanged every result (segments, traceback, boundary states, permutations) is what the reduced rows give
 * when uploaded afresh.  Segments, traceback, boundary states and the segments file of the new context are in REDUCED
 * co-ordinates, as in the reference's chain of tools; kept_columns[j] (fseq_get_identity_columns) maps reduced column j back.
 * It also keeps the mask, the kept-column list and row 0 of the source as raw bytes on the device, so src may be destroyed
 * right afterwards.  Every column an identity column: FSEQ_E_ARG ("every column is an identity column"), nothing is created;
 * none: a plain copy.  A failed allocation returns FSEQ_E_OOM with the sizes (fseq_last_error(src)), leaves nothing behind
 * and src usable.  fseq_get_matrix, fseq_run_segmentation, the joiners, fseq_write_segments (given the reduced rows),
 * fseq_write_founders_device (reduced founders) and the matcher work on the new context unchanged.  summary may be NULL.
 * The new context takes no other input: every input setter returns FSEQ_E_ARG on it and leaves it as it is (the mask, the
 * kept columns and the reference row describe the alignment it was made from; see "a new input on a live context"). */
int  fseq_create_without_identity_columns(fseq_ctx *src, fseq_params const *params, fseq_ctx **out, fseq_identity_summary *summary);
/* On a context made by the call above (FSEQ_E_ARG on any other): the mask over the source's columns (source n bytes) and
 * the source column of every column of this context (`kept` entries, ascending); either may be NULL. */
int  fseq_get_identity_columns(fseq_ctx *ctx, uint8_t *mask, uint64_t *kept_columns);
/* ... the stdout of remove-identity-columns (main.cc:139-146, :225): '0' / '1' per source column ('1' = identity), then
 * '\n'.  path NULL or "-" = stdout. */
int  fseq_write_identity_columns(fseq_ctx *ctx, char const *path);
/* replaces: insert-identity-columns (main.cc:138-195) with --reference = input row 0, on what fseq_write_founders_device
 * writes: max_segment_size lines of source-n bytes plus '\n'; at a kept column the founder's byte ('-' for a slot >= m), at
 * an identity column row 0's byte.  Needs a finished long-path run (FSEQ_E_ARG before one and on a short-path result, whose
 * founders are input rows).  path NULL or "-" = stdout. */
int  fseq_write_founders_restored(fseq_ctx *ctx, uint32_t const *permutations, char const *path);
/* replaces: segmentation_container::reduced_traceback mapped through the identity-column string, which the reference's chain
 * leaves to the user: fseq_get_segments with lb / rb in the SOURCE's co-ordinates, segment_size unchanged.  Segment s covers
 * the source columns from its first kept column up to the next segment's first kept column; segment 0 begins at 0 and the last
 * one ends at the source's n, so the ranges tile the source and the identity columns behind a segment's last kept column are
 * that segment's (csrc/fseq_restored_bounds.hpp).  These are the ranges whose bytes a line of fseq_write_founders_restored
 * takes from one row.  FSEQ_E_ARG on a context not made by fseq_create_without_identity_columns, before a run and on a
 * short-path result. */
int  fseq_get_segments_restored(fseq_ctx *ctx, fseq_segment *out);
/* replaces: the --output-segments file (segmentation_dp_arg.cc:13-104) of a run on the FULL-LENGTH alignment's columns, which
 * the reference's chain does not give (its file is in reduced co-ordinates): fseq_write_segments_device with LB / RB those of
 * fseq_get_segments_restored and every substring at the source's length -- the line's row at the kept columns of the segment,
 * input row 0's byte at the identity columns of its range.  Header, SEGMENT, SIZE, the row lists, COPIED_FROM, the copy numbers
 * and the order of the lines are those of fseq_write_segments_device on the same context, byte for byte; greedy joining writes
 * the header alone.  Written where the alignment, the boundary states and the identity state are: no host rows, the same
 * batches (FSEQ_SEGFILE_BATCH).  Refuses, each with fseq_last_error set and no file created: FSEQ_E_ARG -- a context not made
 * by fseq_create_without_identity_columns, no finished long-path run, no resident alignment, an unknown joining, an output
 * file that cannot be opened; FSEQ_E_UNSUPPORTED -- merged segments that do not tile the columns, bipartite joining with more
 * than 4,096 texts a segment, random joining with more than 65,535, a source of 2^32 - 1 columns or more.  path NULL or
 * "-" = stdout. */
int  fseq_write_segments_restored(fseq_ctx *ctx, int joining, char const *path);
/* replaces: match-sequences-to-founders (match_founder_sequences.cc:108-259) as the last step of the reference's chain
 * remove-identity-columns | founder_sequences | insert-identity-columns | match-sequences-to-founders: the FULL-LENGTH input
 * rows matched against the FULL-LENGTH founders, on a context made by fseq_create_without_identity_columns (FSEQ_E_ARG on any
 * other) after a long-path run.  The founders are what fseq_write_founders_restored writes for these permutations; the rows
 * are the source's, that is the context's rows with row 0's byte in every identity column.  Neither is built: every founder
 * agrees with every row in every identity column, so the walk of fseq_match_founders visits the kept columns only, at their
 * source positions, and accounts for the identity columns between two of them in a closed form (csrc/fseq_match.hpp; DESIGN.md
 * section 7).  Pieces, founder sets, uncovered cells, short pieces and the most pieces in a row are the tool's on those rows
 * and founders, lb and rb in SOURCE co-ordinates: an uncovered cell in the last kept column gives its one-column piece when an
 * identity column follows, and with min_segment_length != 0 a piece closes once it has that many source columns, inside a run
 * of identity columns too.  Refusals as fseq_match_founders (before a run, short-path result, segments that do not tile the
 * columns: FSEQ_E_ARG; more than 2,048 founders, a source of 2^32 - 1 columns or more: FSEQ_E_UNSUPPORTED).  The result
 * replaces the context's last match: fseq_get_match and fseq_write_match serve it unchanged.  The walk is unsplit unless
 * FSEQ_MATCH_SPLIT is set, as fseq_match_founders'; the segments and FSEQ_MATCH_OVERLAP are then counted in kept columns.
 * Detected by symbol, as the entry points above. */
int  fseq_match_founders_restored(fseq_ctx *ctx, uint32_t const *permutations, uint64_t min_segment_length, fseq_match_summary *out);

/* ---- rows held out of a resident alignment and matched on the device ----
 * replaces: nothing of the reference, where a sequence is held out of a reconstruction by removing its line from the list file
 * and running the chain again on the shorter file; here the alignment that is already resident -- uploaded, streamed, generated
 * or borrowed, one code per byte or packed -- is split along its rows on the device (csrc/fseq_rowsplit.hpp): leave-rows-out and
 * k-fold validation of a founder set cost one upload.  The entry points are detected by symbol; FSEQ_ABI_VERSION stays 5. */
typedef struct fseq_hold_out_summary {
	uint32_t m_src, held, kept, reserved;   /* rows of the source, rows held out, m_src - held */
	double   ms_device;                      /* HIP event time of the split pass */
} fseq_hold_out_summary;                     /* 24 bytes */
/* A new, ordinary context on the source's device over the rows of src that are NOT in held_rows: the kept rows stay in the
 * source's order and are numbered 0 .. kept - 1.  held_rows: n_held distinct row indices below the source's m, in any order,
 * 1 <= n_held <= m - 1; anything else is FSEQ_E_ARG with a message (fseq_last_error(src)) before a device is touched.
 * params->m must be 0 (it becomes `kept`), params->n 0 or the source's, params->device the source's device, segment_length
 * positive; block_len, list_cap and pbwt_sample_rate are taken from params.  The new context owns its alignment (columns padded
 * to 16 bytes, padding zeroed) and keeps the source's sigma, code table and code width as they are: a symbol that occurs only
 * in held-out rows keeps its code, and since the order of the codes is unchanged every result is what a fresh upload of the
 * kept rows gives.  Segments, traceback, boundary states, permutations, the founders writers and the segments file are all in
 * the KEPT rows' numbering: exactly what the reference's chain produces from a list file with those lines removed;
 * fseq_get_held_out maps the numbers back.  The held-out rows live in the new context as a second column-major buffer, n
 * columns of ld_h bytes (n_held fields at the source's width, rounded up to 16, padding zeroed), in the order of held_rows: row
 * q of it is held_rows[q].  The source may be destroyed as soon as the call returns; nothing of its segmentation state is read
 * or written, and it may be the source of further calls (one per fold).  FSEQ_E_UNSUPPORTED: a sharded source (a rank holds its
 * own columns only), a source made by fseq_create_without_identity_columns (its identity state would have to be carried along;
 * the other way round works: a context made here may be the source of that call, which knows nothing of the held-out rows and
 * makes a plain context, or of fseq_create_without_identity_columns_held, which carries them along).  FSEQ_E_ARG: no alignment resident.  A failed allocation returns FSEQ_E_OOM with the sizes, leaves
 * nothing behind, *out NULL and src as it was.  The new context takes no other input (every input setter returns FSEQ_E_ARG, as
 * on a context made by fseq_create_without_identity_columns); fseq_set_segment_length is allowed.  summary may be NULL. */
int  fseq_create_without_rows(fseq_ctx *src, uint32_t const *held_rows, uint32_t n_held, fseq_params const *params, fseq_ctx **out,
                              fseq_hold_out_summary *summary);
/* On a context made by the call above (FSEQ_E_ARG on any other): the source row of every row of this context (`kept` entries,
 * ascending) and the held-out rows in the caller's order (`held` entries); either may be NULL. */
int  fseq_get_held_out(fseq_ctx *ctx, uint32_t *kept_rows /* [kept] or NULL */, uint32_t *held_rows /* [held] or NULL */);
/* fseq_match_rows with the context's own held-out rows as the queries: how the rows that took no part in the reconstruction
 * thread through its founders -- the permutations of the finished run or K raw founder rows, exactly one of the two.  Nothing
 * is uploaded or packed: the split walk runs on the held-out buffer as it is.  fseq_match_piece::row is the index into
 * held_rows.  Refusals and the limit of 2,048 founders as fseq_match_rows; FSEQ_E_ARG on a context not made by
 * fseq_create_without_rows.  The result replaces the context's last match: fseq_get_match, fseq_write_match and
 * fseq_debug_match_split serve it as they do after fseq_match_rows. */
int  fseq_match_held_out(fseq_ctx *ctx, uint32_t const *permutations, uint8_t const *const *founders, uint32_t K,
                         uint64_t min_segment_length, fseq_match_summary *out);

/* ---- query rows matched against the RESTORED founders: leave-rows-out validation of a reconstruction made with the
 * identity columns removed ----
 * replaces: match-sequences-to-founders (match_founder_sequences.cc:108-259) run on the full-length query sequences and the
 * file fseq_write_founders_restored writes: the report is byte for byte the tool's, lb and rb in SOURCE co-ordinates.  A match
 * in reduced co-ordinates cannot give it: a column is an identity column among the rows of the reconstruction only, and a query
 * that differs from row 0 there -- an EXCEPTION cell -- carries a byte no restored founder has: an uncovered cell that closes two
 * pieces.  The walk is fseq_match_founders_restored's over the kept columns, merged with every row's own ascending list of
 * exception columns (csrc/fseq_match.hpp, csrc/fseq_exceptions.hpp).  It is split along the KEPT columns as
 * fseq_match_rows' walk is split along the columns: by itself where the context has 32,768 kept columns or more, or as
 * FSEQ_MATCH_SPLIT / FSEQ_MATCH_OVERLAP say, both counted in kept columns; the result is the unsplit walk's in every case and
 * fseq_debug_match_split reports how it walked.
 * Founders are given by permutations only (K raw full-length rows need not agree with row 0 in the identity columns).
 * Detected by symbol; FSEQ_ABI_VERSION stays 5. */
/* fseq_create_without_identity_columns for a source made by fseq_create_without_rows (FSEQ_E_ARG on any other source) that
 * carries the held-out rows along.  The alignment, the identity state and every result of the new context are those of
 * fseq_create_without_identity_columns(src, ...), bit for bit; it also holds the held-out rows' KEPT columns, the two row maps
 * (fseq_get_held_out answers on it) and the held-out rows' exception cells.  fseq_match_held_out on it is the match in reduced
 * co-ordinates, as fseq_match_founders is on a reduced context; fseq_set_segment_length is allowed (nothing carried depends on
 * the segment length).  Refusals and the out-of-memory contract as the plain call: nothing is left behind, *out is NULL and src
 * is as it was.  ms_device does not cover the held-out rows' part. */
int  fseq_create_without_identity_columns_held(fseq_ctx *src, fseq_params const *params, fseq_ctx **out, fseq_identity_summary *summary);
/* On a context made by the call above, after a long-path run: its held-out rows, full length, against the restored founders
 * of these permutations.  fseq_match_piece::row indexes the hold-out list.  Nothing is uploaded.  Refusals as
 * fseq_match_founders_restored, each before a device is touched, the context and its last match left as they were; FSEQ_E_ARG on
 * a context of another kind.  The result replaces the context's last match: fseq_get_match and fseq_write_match serve it. */
int  fseq_match_held_out_restored(fseq_ctx *ctx, uint32_t const *permutations, uint64_t min_segment_length, fseq_match_summary *out);
/* ... rows from the host, on a context made by either identity-column create call: rows[q] points at the SOURCE-n raw bytes of
 * query q.  They go up in column chunks through a staging of at most 64 MiB, every byte once; the kept columns are held packed
 * as fseq_match_rows holds its queries, the others are compared with row 0's byte.  A byte outside the alphabet is an uncovered
 * cell in either kind of column.  FSEQ_E_ARG also for rows == NULL, a NULL row and n_rows == 0. */
int  fseq_match_rows_restored(fseq_ctx *ctx, uint32_t const *permutations, uint8_t const *const *rows, uint32_t n_rows,
                              uint64_t min_segment_length, fseq_match_summary *out);
/* The exception cells of the last match, where it was made by one of the two calls above (FSEQ_E_ARG otherwise): offsets
 * [rows + 1], row r's cells are columns[offsets[r] .. offsets[r + 1]), source columns in ascending order; *total = offsets[rows].
 * These are the query rows' private variants in the reconstruction's identity columns.  Any pointer may be NULL. */
int  fseq_get_match_exceptions(fseq_ctx *ctx, uint64_t *offsets, uint32_t *columns, uint64_t *total);

int  fseq_get_timings(fseq_ctx const *ctx, fseq_timings *out);

/* Host time of the last fseq_join_* call on this context (wall, milliseconds): the boundary states' way to the host,
 * then -- greedy joiner -- the class tables (greedy_matcher.cc:31-68), the co-occurrence edges (:295-343) and the rounds
 * that draw them (:353-439); the other joiners report their matching under ms_draw. */
typedef struct fseq_join_profile {
	double ms_d2h, ms_classes, ms_edges, ms_draw, ms_total;
	uint64_t bytes_d2h;
} fseq_join_profile;
int  fseq_get_join_profile(fseq_ctx const *ctx, fseq_join_profile *out);

/* replaces: segmentation_lp_context::step_max() / current_step() (segmentation_lp_context.hh:122-127), which the
 * reference's progress indicator polls from another thread, and the per-stage timestamps of generate_context.cc.
 * The stages are the reference's: generate_traceback (pass 1 + DP; steps = columns), find_segments_greedy (steps =
 * traceback entries), update_samples_to_traceback_positions (steps = merged boundaries).  Pass 1 runs as phases over
 * all columns at once, so current_step moves at the phase boundaries (A, B, C, DP), scaled to columns.  Both counters
 * may be read from any thread while fseq_run_segmentation runs; the optional callback is made from the calling thread
 * at the same points (fn == NULL: none).  With the library built against roctx (the default build), every phase is
 * also an roctx range (rocprofv3 --marker-trace). */
enum { FSEQ_STAGE_TRACEBACK = 0, FSEQ_STAGE_MERGE = 1, FSEQ_STAGE_SAMPLES = 2 };
typedef void (*fseq_progress_fn)(void *user, int stage, uint64_t current_step, uint64_t step_max);
int      fseq_set_progress(fseq_ctx *ctx, fseq_progress_fn fn, void *user);
uint64_t fseq_step_max(fseq_ctx const *ctx);
uint64_t fseq_current_step(fseq_ctx const *ctx);

/* A context that shares its device with other contexts or ranks keeps its device allocations -- the pass-2 stride
 * states are sized from what is free -- inside `bytes` in all (0 = whatever is free on the device, the default). */
int  fseq_set_memory_budget(fseq_ctx *ctx, uint64_t bytes);

/* Device memory the per-column divergence lists of a long-path run may occupy: the list ring and its halo, not the
 * per-column headers (16 bytes a column) or the DP arrays.  0 (the default): every list is held until the merge walk is
 * done, n x (X + 3) x 8 bytes at list capacity X.  Otherwise, when those do not fit the budget, pass 1 and the DP run in
 * windows of consecutive column blocks: a window's lists are written, the DP rounds they feed run, and the next window
 * takes their place (the few columns the next rounds still read move to the front); the merge walk then takes its
 * thresholds in a second pass over the windows, which writes the same lists again.  Results are the same bit for bit as
 * without a budget; the time is that of about one more phase C plus the DP in one serial launch per window.  A budget that
 * cannot hold one column block plus the halo at the list capacity in use -- also one grown by a retry -- makes the run
 * return FSEQ_E_OOM with the bytes needed; the context stays usable.  The setting persists for later runs on the context;
 * the short path (n < 2L) ignores it; a sharded context (fseq_set_shard, before or after) returns FSEQ_E_UNSUPPORTED.
 * The reference's knob for memory against time is --pbwt-sample-rate (generate_context.cc:121-124): it keeps one
 * column's divergence_value_counts live (segmentation_lp_context.cc:78,119) and a pBWT sample every q sqrt(n) columns,
 * from which its later steps replay columns.  This engine keeps an exact (a, d) state every block_len columns whatever
 * that rate is (fseq_params.pbwt_sample_rate is accepted and not used), so the samples are not the memory that grows with
 * the input's diversity: the lists are, and this budget is what bounds them, at the price of replaying phase C once. */
int  fseq_set_list_memory(fseq_ctx *ctx, uint64_t bytes);

/* The input rows in column chunks of bounded memory: the device holds the packed alignment and a fixed staging buffer, never
 * the m x n raw bytes fseq_set_rows stages, and the host may hold one chunk at a time.  replaces: nothing of the reference,
 * which reads every sequence whole (generate_context.cc:64-106); it is what lets an alignment whose raw bytes exceed the card
 * be loaded when its packed form fits.
 *   fseq_input_begin    discards the context's input and result (as a second fseq_set_rows does) and allocates the staging:
 *                       two halves of staging_bytes / 2 (0 = 256 MiB in all).  alphabet: the byte values that may occur, in any
 *                       order, no duplicates (else FSEQ_E_ARG), or NULL: the alphabet is collected by fseq_input_scan calls.
 *                       A staging too small for 16 columns of m rows in a half returns FSEQ_E_ARG and names the bytes needed.
 *   fseq_input_chunk_columns   the most columns one call below may carry: floor(staging_bytes / 2 / m), rounded down to whole
 *                       16-byte pieces of a staged row; 0 before fseq_input_begin and on a NULL context.
 *   fseq_input_scan     rows[r] points at the ncols bytes of row r from column c0 on.  The calls tile [0, n) in ascending,
 *                       contiguous chunks; only without a supplied alphabet.
 *   fseq_input_columns  the same chunks again (after the scans have covered [0, n) when there is no supplied alphabet).  The
 *                       first call fixes the code table -- dense codes in ascending byte order, as fseq_set_rows; with a
 *                       supplied alphabet a listed byte that never occurs keeps its code, which changes no result (the order
 *                       of the codes is all the pBWT sees) but may widen the codes -- and allocates the packed alignment.
 *                       Padding bytes and padding fields of every column are written as zeros.
 *   fseq_input_end      after column n has arrived: the context holds the input, the staging is released.  A byte outside a
 *                       supplied alphabet is recorded on the device (no round trip per chunk) and reported here: FSEQ_E_ARG,
 *                       fseq_last_error names the byte value, and the context is left without an input (it takes a new
 *                       fseq_input_begin or fseq_set_rows).
 * When fseq_input_scan or fseq_input_columns returns, the host bytes of that call have been read (the copy is waited for, not
 * the kernel: chunk i is encoded while chunk i + 1 is copied into the other half), so the caller may reuse its buffers.
 * Between begin and end the context's device allocations stay within packed alignment + staging_bytes + 1 MiB.  A chunk out
 * of order, overlapping, gapped or wider than fseq_input_chunk_columns, a scan after a supplied alphabet, columns before the
 * scans are complete, an end before column n, and any of these calls without a begin return FSEQ_E_ARG.  NOT for sharded
 * contexts (fseq_set_shard before or after fseq_input_begin): FSEQ_E_UNSUPPORTED -- a rank's alphabet exchange is not built
 * for this path.  Detected by symbol; FSEQ_ABI_VERSION stays 5. */
int      fseq_input_begin(fseq_ctx *ctx, uint8_t const *alphabet, uint32_t alphabet_size, uint64_t staging_bytes);
uint64_t fseq_input_chunk_columns(fseq_ctx const *ctx);
int      fseq_input_scan(fseq_ctx *ctx, uint64_t c0, uint64_t ncols, uint8_t const *const *rows);
int      fseq_input_columns(fseq_ctx *ctx, uint64_t c0, uint64_t ncols, uint8_t const *const *rows);
int      fseq_input_end(fseq_ctx *ctx);
/* All of the above for rows that are in host memory (rows[r]: the n bytes of row r): the scan pass, the encode pass and the
 * end, in chunks of fseq_input_chunk_columns rounded down to a multiple of 64 where that leaves at least 64.  Results are
 * those of fseq_set_rows on the same rows, bit for bit. */
int      fseq_set_rows_streamed(fseq_ctx *ctx, uint8_t const *const *rows, uint64_t staging_bytes);

/* The chunked input with the identity columns dropped on the way: the context fseq_set_rows_streamed followed by
 * fseq_create_without_identity_columns gives, bit for bit, without the source's packed alignment (ld x n bytes) ever existing.
 * replaces: remove-identity-columns in front of founder_sequences for an alignment whose packed form exceeds the card while its
 * variable columns fit.  src is an ordinary fseq_create context with n = the source's columns; it never holds an alignment.
 *   fseq_input_begin    as above.
 *   fseq_input_scan_identity   the scan pass: fseq_input_scan's chunks (same rules), finding besides the byte values, for every
 *                       column, whether all m rows carry row 0's byte, and row 0's byte.  Allowed, and needed for this path, with a
 *                       supplied alphabet too.  One scan entry per input: after fseq_input_scan this one returns FSEQ_E_ARG, and
 *                       the other way round.
 *   fseq_input_reduce   after the scan has covered [0, n): fixes the code table -- alphabet, sigma and code width are those of the
 *                       WHOLE source, so a byte that occurs only in identity columns takes a code, as in the chain above; a found
 *                       byte outside a supplied alphabet is refused here with fseq_input_end's message and effect, wherever it
 *                       lies --, makes the kept-column list and creates the context over the kept columns with its alignment of
 *                       ld x kept bytes.  params as for fseq_create_without_identity_columns (n must be 0, m 0 or the source's,
 *                       device the source's); summary may be NULL (ms_device: the scan of the mask).  Every column an identity
 *                       column: FSEQ_E_ARG ("every column is an identity column"), no context is made and what the identity scan
 *                       allocated is released; src holds what fseq_input_begin allocated, and the input may go on as an ordinary
 *                       one (fseq_input_columns) or give way to a new one.  A failed allocation: FSEQ_E_OOM with the sizes, src
 *                       stays usable (the call may be repeated).  The new context belongs to src's input until
 *                       fseq_input_end_kept: a new fseq_input_begin, any other input set on src and fseq_destroy(src) destroy it.
 *   fseq_input_kept_columns    *count = the kept columns in [c0, c0 + ncols).  Host only, after the reduce: a caller may skip
 *                       reading a chunk that holds none.
 *   fseq_input_columns_kept    the second pass: the same tiling of [0, n), ascending.  Only the kept columns of a chunk are
 *                       encoded, into their final place in the new alignment (padding written as zeros).  A chunk without a
 *                       kept column returns without a copy or a launch, and rows may be NULL for it.
 *   fseq_input_end_kept after column n: *out is the finished context -- it has its input and answers as one made by
 *                       fseq_create_without_identity_columns everywhere (the run, the joiners, the restored writers and matchers,
 *                       fseq_set_segment_length, the length scan; no other input) --, the staging is released and src is left
 *                       without an input.  A byte outside a supplied alphabet in a kept cell: FSEQ_E_ARG as fseq_input_end, *out
 *                       NULL, the new context destroyed.
 * Device memory, by the accounts of the two contexts (fseq_debug_device_bytes): src holds the staging, 320 bytes of tables and
 * during the scan 2 n bytes (mask, reference row), min(n, chunk columns) + at most 256 bytes of accumulators and, inside
 * fseq_input_reduce, 4 bytes per 2,048 columns; the new context ld x kept + 16, 4 x kept and the 2 n bytes src hands over.  The
 * peaks of both together stay within staging + ld x kept + 16 + 4 x kept + 6 n for n >= 1,024.
 * Wrong order -- a reduce before the scan is complete or a second one, columns or an end before the reduce, an end before the
 * columns are complete, fseq_input_columns or fseq_input_end after a reduce -- returns FSEQ_E_ARG and names the step.  Sharded
 * contexts: FSEQ_E_UNSUPPORTED.  Sources of 2^32 - 1 columns or more are refused (fseq_create).  Not served: held-out rows
 * (they need the resident source: fseq_create_without_identity_columns_held).  Detected by symbol; FSEQ_ABI_VERSION stays 5. */
int      fseq_input_scan_identity(fseq_ctx *src, uint64_t c0, uint64_t ncols, uint8_t const *const *rows);
int      fseq_input_reduce(fseq_ctx *src, fseq_params const *params, fseq_identity_summary *summary);
int      fseq_input_kept_columns(fseq_ctx *src, uint64_t c0, uint64_t ncols, uint64_t *count);
int      fseq_input_columns_kept(fseq_ctx *src, uint64_t c0, uint64_t ncols, uint8_t const *const *rows);
int      fseq_input_end_kept(fseq_ctx *src, fseq_ctx **out);
/* All of the above for rows that are in host memory, in fseq_set_rows_streamed's chunks: both passes, the reduce between them
 * and the end.  On any failure *out is NULL and src is left without an input. */
int      fseq_set_rows_streamed_without_identity_columns(fseq_ctx *src, uint8_t const *const *rows, uint64_t staging_bytes, fseq_params const *params,
                                                         fseq_ctx **out, fseq_identity_summary *summary);

/* Another segment length bound L on the alignment the context holds.  replaces: nothing of the reference, which is run once
 * per L (generate_context.cc:121-124 reads the bound once); here a second L needs neither a second context nor a second
 * upload.  The context keeps the resident alignment, its alphabet and -- a context made by
 * fseq_create_without_identity_columns, on which the call is allowed -- its identity relation.  It drops the result and the
 * last match as a new input does: the getters return FSEQ_E_ARG until the next fseq_run_segmentation.  What runs learnt that
 * depends on L is forgotten (the list capacity that worked, the representatives' plan, the traceback's length); the block
 * geometry of an unsharded context does not depend on L, so what phase A learnt stays.  No buffer that still fits is released:
 * the DP arrays grow when L shrinks and never shrink, so a context cycled between two lengths settles on the larger arrays.
 * The next fseq_run_segmentation gives, bit for bit, what a fresh context created with that L gives on the same rows; n < 2L
 * takes the short path as there.  FSEQ_E_ARG and nothing changes: L == 0 (what fseq_create refuses for L), a chunked input
 * under way (fseq_input_begin without its end).  FSEQ_E_UNSUPPORTED: a sharded context (fseq_set_shard, before or after) --
 * its geometry and halo depend on L.  Detected by symbol; FSEQ_ABI_VERSION stays 5. */
int      fseq_set_segment_length(fseq_ctx *ctx, uint64_t segment_length);

/* The maximum segment size at several segment length bounds in one call: "how many founders at which L".  replaces: nothing
 * of the reference (one run of the program per L).  Phases A and B and the capacity estimate run once -- on an unsharded
 * context they do not depend on L --; the lists are built (phase C) at the smallest long-path length, and for every further
 * length, ascending, folded in place (the entries a larger L clips to the same cut bound join the list's first entry) and
 * the DP alone runs again.  The DP itself tells where a folded list is too short to prove a cell: the lists are then built
 * at that length (FSEQ_SCAN_LISTS_BUILT) and the scan goes on from there, so no value rests on the folding.  Measured (DESIGN.md
 * section 7): folded lists prove whole lengths where the lists are complete (capacity >= m); lists cut at their capacity end at
 * the first value that many rows share, and on the benchmark's inputs every length was built -- the scan then costs one phase C
 * a length, what runs on the one context cost without their traceback, merge and pass 2.  All entries with
 * n < 2L share one short-path sweep.  Under a list budget that puts the lists into windows (fseq_set_list_memory), and with
 * the knob FSEQ_SCAN_REBUILD, every long-path entry is built.  No traceback, merge or pass 2 is run.
 * Entries may come in any order and may repeat; every entry is filled in place (a repeat carries ms_device 0; the entries of
 * the short path share one sweep, whose time the first of them carries).
 * Afterwards the context keeps its own segment length and holds no result (the DP arrays and the lists are those of the last
 * entry): the getters return FSEQ_E_ARG until the next fseq_run_segmentation, which gives what it gave before the scan.
 * Refusals, each with fseq_last_error set and nothing written to the entries: no input, a NULL pointer, count == 0 or a
 * segment_length of 0: FSEQ_E_ARG; a sharded context: FSEQ_E_UNSUPPORTED; a failed allocation: FSEQ_E_OOM, the context stays
 * usable.  Detected by symbol; FSEQ_ABI_VERSION stays 5. */
enum { FSEQ_SCAN_LISTS_BUILT = 0, FSEQ_SCAN_LISTS_FOLDED = 1, FSEQ_SCAN_LISTS_NONE = 2 };
typedef struct fseq_length_scan_entry {
	uint64_t segment_length;    /* in */
	uint32_t max_segment_size;  /* out: what fseq_run_segmentation reports at this L (m where the reference cannot reduce) */
	uint32_t short_path;        /* out: 1 if n < 2L */
	uint32_t lists;             /* out: BUILT (phase C ran at this L), FOLDED (from the previous entry's lists), NONE (short path) */
	uint32_t list_cap;          /* out: X of the lists the value was proven on */
	uint32_t dp_chunks;         /* out: as fseq_timings.dp_chunks */
	uint32_t reserved;
	double   ms_device;         /* out: event time spent on this entry alone */
} fseq_length_scan_entry;        /* 40 bytes */
typedef struct fseq_length_scan_summary {
	uint32_t lists_built, lists_folded, short_entries, retries;     /* distinct lengths built / folded, entries on the short path, capacities doubled */
	double ms_phase_a, ms_phase_b, ms_total;                         /* event times of the one phase A and B; host time of the call */
} fseq_length_scan_summary;      /* 40 bytes */
int      fseq_scan_segment_lengths(fseq_ctx *ctx, fseq_length_scan_entry *entries, size_t count, fseq_length_scan_summary *summary);

#ifdef __cplusplus
}
#endif
#endif
