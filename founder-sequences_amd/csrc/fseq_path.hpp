// fseq_path.hpp -- what the units of the segmentation path share, and nothing else of the library needs: the state of one
// long-path run, the aliases and ranges of its phases, the path's constants, the views of a context that the launchers take
// (msa_args, list_args, stride_states), and the functions that cross a unit.
//   csrc/fseq_api.hip         the entry points of include/fseq.h, what a new input or knob makes a context forget
//   csrc/fseq_api_debug.hip   the entry points of include/fseq_debug.h, the row-sharded conformance sweep
//   csrc/fseq_path_setup.hip  pinned staging, geometry, work buffers, the row upload, the shard exchange
//   csrc/fseq_path_dp.hip     the DP drivers, the tracebacks, the merge (the one unit that instantiates k_dp<>)
//   csrc/fseq_path_pass1.hip  phases A and B, the list capacity, phase C's launchers on all rows (the one unit that instantiates
//                             k_colblock_stream<> / k_columns_stream<> and includes fseq_chainsort.hpp)
//   csrc/fseq_path_reduced.hip  phase C on representative rows: the stages around the plan (plan_reduced, fseq_redplan.hpp), the
//                             configurations' launches side by side, the redo marking (instantiates no kernel)
//   csrc/fseq_path_attempt.hip  one attempt at a list capacity as stages with one verdict, the list windows, the loop over attempts,
//                             the short path (instantiates no kernel)
//   csrc/fseq_path_pass2.hip  the boundary states at the merged boundaries
//   csrc/fseq_lengthscan.hip  another segment length on a resident alignment, the scan over segment lengths (the one unit that
//                             includes fseq_lengthscan.hpp: k_relump_lists)
// A kernel template is instantiated, and a header that defines plain __global__ kernels (fseq_dpspec.hpp, fseq_chainsort.hpp,
// fseq_rowshard.hpp) is included, by one unit only: the others reach those kernels through the launchers declared here.  A unit
// may include a header of templates for the sizes and schedules it computes on the host (stream_lds_bytes, ...); the DP's round
// schedule is a header without kernels (fseq_dpschedule.hpp).
// Everything a unit does not declare here is in its anonymous namespace.  Internal: none of this is exported.
#pragma once

#include "fseq_ctx.hpp"

#ifdef FSEQ_WITH_ROCTX
#include <rocprofiler-sdk-roctx/roctx.h>
#endif

namespace fseq { struct DpSchedule; }          // fseq_dpschedule.hpp

#pragma GCC visibility push(hidden)

namespace fseq {

// One range per phase (rocprofv3 --marker-trace shows them when the library is built against roctx).  The pushes and pops
// are counted, so a test can tell that the ranges are there and balanced without a profiler (fseq_debug_ranges).
extern std::atomic<uint64_t> g_range_pushes, g_range_pops;       // (csrc/fseq_path_pass1.hip)
#ifdef FSEQ_WITH_ROCTX
#define FSEQ_RANGE_PUSH(name) do { fseq::g_range_pushes.fetch_add(1, std::memory_order_relaxed); (void) roctxRangePushA(name); } while (0)
#define FSEQ_RANGE_POP() do { fseq::g_range_pops.fetch_add(1, std::memory_order_relaxed); (void) roctxRangePop(); } while (0)
#else
#define FSEQ_RANGE_PUSH(name) do { fseq::g_range_pushes.fetch_add(1, std::memory_order_relaxed); } while (0)
#define FSEQ_RANGE_POP() do { fseq::g_range_pops.fetch_add(1, std::memory_order_relaxed); } while (0)
#endif

// a phase's range: popped where the phase ends -- or where the function leaves early (a retry with a larger list capacity, an
// attempt that runs again, an error), so that pushes and pops stay balanced on every path
struct RangeScope {
	bool open = true;
	explicit RangeScope(char const *name) { FSEQ_RANGE_PUSH(name); (void) name; }
	void end() { if (open) { FSEQ_RANGE_POP(); open = false; } }
	~RangeScope() { end(); }
	RangeScope(RangeScope const &) = delete;
	RangeScope &operator=(RangeScope const &) = delete;
};

constexpr size_t LDS_LIMIT = 160 * 1024;
constexpr uint64_t STREAM_BLOCK_TARGET_ALL_ROWS = 1600;   // columns per block the streamed regime aims for (prepare_geometry / block_geometry) ...
// [r5] ... and when phase C runs on the blocks' representatives: a block of ~800 columns of BASELINE C4 has ~6,600 of them, and
// the ~10,700 of a block in which the founders recombine still fit the largest configuration (11,264)
constexpr uint64_t STREAM_BLOCK_TARGET_REDUCED = 800;
constexpr size_t RED_SIDE_STREAMS = 3;                    // side streams the reduced configurations' launches may use (red_launch_all)
#define STREAM_BLOCK_TARGET (c->tune.no_reduced ? STREAM_BLOCK_TARGET_ALL_ROWS : STREAM_BLOCK_TARGET_REDUCED)
#ifndef FSEQ_X_FLOOR_VALUE
#define FSEQ_X_FLOOR_VALUE 63u
#endif
constexpr uint32_t FSEQ_X_FLOOR = FSEQ_X_FLOOR_VALUE;   // smallest per-column list capacity tried (the estimate and the retries raise it)

// what the phases of one long-path run share (run_long_path)
struct LongRun {
	uint32_t X = 0, retries = 0;
	double ms_c = 0, ms_dp = 0, ms_host = 0, ms_p2 = 0;
	uint64_t pass2_cells = 0;
	bool keyspace = false;
	bool tree_ran = false;                   // phase A ran the key-space tree at all (else: the column sweep did every block, as last time)
	bool tree_alone = false;                 // phase A ran the key-space tree without the column sweep behind it (no block was given up last time)
	bool trie_ran = false, trie_alone = false;   // ... the trie over 16-column words (streamed rows); ... without the key-space tree behind it
	uint32_t redone = 0;                     // blocks whose lists could not be proven on their representatives: their attempt ran again, they on all rows
	bool range_ab_open = false;              // the roctx range of phases A + B spans two functions
};

// the aliases every phase uses
#define FSEQ_LONG_LOCALS(c)                                                                           \
	fseq_params const &p = (c)->p;                                                                    \
	uint32_t const m = p.m;                                                                           \
	uint64_t const n = p.n;                                                                           \
	uint64_t const L = p.segment_length;                                                              \
	hipStream_t st = (c)->stream;                                                                     \
	KernelSet const &ks = (c)->ks;                                                                    \
	Shard const &sh = (c)->sh;                                                                        \
	bool const sharded = sh.on;                                                                       \
	uint32_t const b_lo = sharded ? sh.b_lo : 0u, b_hi = sharded ? sh.b_hi : (c)->nblocks;            \
	uint32_t const my_blocks = b_hi - b_lo;                                                           \
	int rc = FSEQ_OK;                                                                                 \
	(void) m; (void) n; (void) L; (void) st; (void) ks; (void) sharded; (void) b_lo; (void) my_blocks; (void) rc

// columns this context holds: all of them, or the rank's share of a sharded run
inline uint64_t held_lo(fseq_ctx const *c) { return c->sh.on ? c->sh.c_lo : 0; }
inline uint64_t held_hi(fseq_ctx const *c) { return c->sh.on ? c->sh.c_end : c->p.n; }

// the path's device words and the two behind d_red_invalid[nblocks] (fseq_types.hpp); device addresses: for their members' addresses only
inline PathWords *path_words(fseq_ctx const *c) { return c->d_flags; }
inline RedFlags *red_flags(fseq_ctx const *c) { return reinterpret_cast<RedFlags *>(c->d_red_invalid + c->nblocks); }

// diagnostic ("ABC" in FSEQ_SYNC_PHASES): synchronise behind a phase, so that a fault shows up at the phase that caused it
inline bool sync_at(fseq_ctx const *c, char ph) { return c->tune.sync_phases.find(ph) != std::string::npos; }

// ---- the views of a context that the launchers take (fseq_types.hpp)
// the alignment: all of it in the context's blocks, or the columns [0, n) in nblocks blocks of B (a rank of a sharded run
// covers its own columns and the halo; the short path takes all columns as one block)
inline MsaArgs msa_args(fseq_ctx const *c, uint64_t n, uint32_t B, uint32_t nblocks)
{
	MsaArgs A;
	A.msa = c->d_msa; A.ld = c->ld; A.m = c->p.m; A.n = n; A.B = B; A.nblocks = nblocks; A.N2 = c->N2; A.npass = c->npass; A.bsh = c->bsh;
	return A;
}
inline MsaArgs msa_args(fseq_ctx const *c) { return msa_args(c, c->p.n, c->B, c->nblocks); }
inline ListArgs list_args(fseq_ctx const *c) { return ListArgs{(uint32_t) c->p.segment_length, c->X, c->stride, c->d_ent, c->d_hdr}; }
inline StrideStates stride_states(fseq_ctx const *c) { return StrideStates{c->snap_stride, c->d_ss_a, c->d_ss_d, c->ss_pack, c->ss_ids}; }

// ---- csrc/fseq_api.hip
void forget_run_history(fseq_ctx *c);

// ---- csrc/fseq_path_setup.hip
// Pinned host staging.  A copy between the device and pageable host memory is staged by the runtime -- one blocking round
// trip of 20-50 microseconds each, and a step had a dozen of them (flags, counts, the traceback, thresholds: a fifth of a
// BASELINE C2 step).  pin_reserve(bytes) opens a stage (what the previous one handed out is dead), pin_take carves it.
int pin_reserve(fseq_ctx *c, size_t bytes);
template <typename U>
U *pin_take(fseq_ctx *c, size_t count)
{
	size_t const at = (c->pin_used + 15) & ~size_t(15);
	c->pin_used = at + count * sizeof(U);
	return c->pin_used <= c->pin_cap ? reinterpret_cast<U *>(c->h_pin + at) : nullptr;      // (nullptr: the stage was reserved too small -- a bug)
}
void free_msa(fseq_ctx *c);
int alloc_msa(fseq_ctx *c);
void block_geometry(fseq_ctx *c);
int prepare_geometry(fseq_ctx *c);
int ensure_work_buffers(fseq_ctx *c, uint32_t X, bool want_ss = true);
void free_work(fseq_ctx *c);
int upload_rows_device(fseq_ctx *c, uint8_t const *const *rows);
int set_alphabet_and_upload(fseq_ctx *c, uint8_t const *base, size_t rs, size_t cs);
int shard_exchange(fseq_ctx *c, uint64_t words, int op);
void shard_post_failure(fseq_ctx *c, int code);

// ---- csrc/fseq_path_dp.hip
// The chunk plan of the speculative DP (fseq_dpspec.hpp): chunk k runs the rounds [r0[k], r0[k + 1]) (the last one
// also the drain round and the final cell); no chunks = use the serial kernel.  Sharded: a round belongs to the
// rank that owns its first column; every rank cuts its own rounds into chunks and every rank computes the same table.
struct SpecPlan {
	std::vector<uint32_t> r0;                // nchunks + 1 entries
	uint32_t mine_lo = 0, mine_hi = 0;       // my chunks
	std::vector<uint32_t> rank_lo;           // sharded: rank g runs the chunks [rank_lo[g], rank_lo[g + 1]) (active + 1 entries)
	uint32_t nchunks() const { return r0.empty() ? 0u : (uint32_t) r0.size() - 1u; }
};
SpecPlan spec_plan(fseq_ctx *c, DpSchedule const &S);
bool shard_dp_plan_ok(fseq_ctx *c);          // fseq_set_shard: every rank that owns blocks owns DP rounds
int dp_spec_reset(fseq_ctx *c, SpecPlan const &P, hipStream_t s);
int run_dp_spec(fseq_ctx *c, DpSchedule const &S, SpecPlan const &P, hipStream_t st, uint32_t *overflow, uint32_t *sweeps_out, bool reset_done = false);
int prepare_dp_kernels(fseq_ctx *c);         // prepare_geometry: the LDS of every k_dp<>
// the serial DP over the rounds [r_lo, r_hi): k_dp<DP_WHOLE> or k_dp<DP_PARTIAL> (fseq_dp.hpp)
void launch_dp_serial(fseq_ctx *c, int mode, hipStream_t st, uint32_t r_lo, uint32_t r_hi);
int long_traceback_and_merge(fseq_ctx *c, double th0, bool *overflow_out);
// The two halves of long_traceback_and_merge on DP arrays and lists a caller laid over the context (fseq_debug_merge_on_lists).
// separate: the thresholds do not ride with the traceback (k_seg_tau_tb) but come from launches of their own, they and the
// merged sizes once per column range [bounds[r], bounds[r + 1]) and summed on the host.  Out: the thresholds in the host's
// order (empty where none were taken) and the launches made.
struct MergeProbe {
	bool separate = false;
	std::vector<uint64_t> bounds;
	std::vector<uint2> tau;
	uint32_t threshold_launches = 0, count_launches = 0;
};
int probe_traceback_and_merge(fseq_ctx *c, MergeProbe *probe, bool *overflow_out);

// ---- csrc/fseq_path_pass1.hip
uint32_t scan_keyed(fseq_ctx const *c);
int prepare_stream_kernels(fseq_ctx *c, size_t lds);  // prepare_geometry: the LDS of the streamed kernels this unit instantiates ...
int prepare_stream2_prologue(fseq_ctx *c);            // ... and of the static kernels it launches (an attribute set on another unit's
int prepare_blockkeys_stream(fseq_ctx *c);            //     copy of a static kernel would not reach the one launched)
size_t chain_hist_words(uint32_t m);                 // digit histogram words of one chain of the streamed phase B (fseq_chainsort.hpp)
// the streamed replay sweep of pass 2 (k_colblock_stream<MODE_SNAP>): the groups [0, groups) of tasks.task_grp / task_src, as
// many per launch as the workspace holds
void launch_replay_stream(fseq_ctx *c, size_t groups, SnapArgs const &tasks);
int launch_chain_snap_grouped(fseq_ctx *c, uint32_t ngrp, uint32_t *stats);       // pass 2 behind the reduced phase C, streamed rows: the chain steps
int long_phase_a(fseq_ctx *c, LongRun &R);
int phase_a_take_counts(fseq_ctx *c, LongRun const &R, PhaseACounters counts);    // what an attempt read back of phase A's counters
int long_phase_b(fseq_ctx *c, LongRun &R);
int long_list_capacity(fseq_ctx *c, LongRun &R);
int short_phase_a(fseq_ctx *c, uint32_t *d_rank, uint32_t *d_keyd, uint32_t *d_nkeys);      // the short path's one block [0, n), ranked
// phase C on all rows of the blocks b0 .. b0 + nb - 1 (list: workgroup i owns block list[i] -- the blocks the plan hands to all rows)
void launch_columns(fseq_ctx *c, uint32_t b0, uint32_t nb, uint32_t const *list = nullptr);

// ---- csrc/fseq_path_reduced.hip
// the plan of an attempt at list capacity X into c->red.plan (*use: phase C goes by it); what later runs need of it into c->red.memory
int red_plan(fseq_ctx *c, uint32_t X, bool *use);
int red_columns(fseq_ctx *c);                         // the lists of the plan's reduced blocks, the largest configurations first
void red_fill_args(fseq_ctx *c, RedArgs &RA);
struct RedLaunch { int config; uint32_t first, count; };
// (base.blocks / base.wg_tasks: the lists the launches' [first, first + count) index; lists: the segment length alone in pass 2)
int red_launch_all(fseq_ctx *c, std::vector<RedLaunch> const &ls, RedArgs const &base, ListArgs const &lists);
// the blocks of [b_lo, b_hi) whose lists could not be proven on their representatives get their force marks (*count; *wide: of them, reduced still)
int red_take_invalid(fseq_ctx *c, uint32_t b_lo, uint32_t b_hi, uint32_t *count, uint32_t *wide);

// ---- csrc/fseq_path_attempt.hip
void set_list_window(fseq_ctx *c, uint32_t lo_w);
int window_phase_c(fseq_ctx *c, uint32_t lo, uint32_t hi);
int run_long_path(fseq_ctx *c, fseq_result *res);
int run_short_path(fseq_ctx *c, fseq_result *res);
// what a scan over segment lengths shares with a run: the attempts up to a proven DP result (stages 1 to 5 of an attempt, the
// capacity grown by the ordinary rule), and the DP alone on the lists the context holds (*unproven: a list was too short)
struct DpProof { uint32_t max_segment_size = 0, dp_chunks = 0, dp_sweeps = 0; };
int long_attempts_to_proof(fseq_ctx *c, LongRun &R, DpProof *proof);
int long_dp_on_lists(fseq_ctx *c, DpProof *proof, bool *unproven);

// ---- csrc/fseq_lengthscan.hip
// another segment length on the context: dp_size and the DP arrays' sizes follow (grow-only; allocated where the geometry's buffers are)
int apply_segment_length(fseq_ctx *c, uint64_t L);
void launch_relump_lists(hipStream_t st, RelumpArgs const &lists);     // (k_relump_lists, fseq_lengthscan.hpp)

// ---- csrc/fseq_path_pass2.hip
int long_pass2(fseq_ctx *c, LongRun &R);

} // namespace fseq

#pragma GCC visibility pop
