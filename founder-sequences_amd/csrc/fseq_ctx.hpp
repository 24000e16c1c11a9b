// fseq_ctx.hpp -- the context behind the C ABI (include/fseq.h) and the small helpers every translation unit of the library
// shares: csrc/fseq_api.hip (the ABI's entry points) and csrc/fseq_api_debug.hip (the debug entry points, the row-sharded sweep),
// the units of the segmentation path (csrc/fseq_path_setup.hip, _dp, _pass1, _reduced, _attempt, _pass2: geometry, buffers, phases, sharding; what
// only they share is csrc/fseq_path.hpp), csrc/fseq_api_join.hip (the host joiners, their device front and the output
// writers), csrc/fseq_api_graph.hip (the founder block graph), csrc/fseq_api_match.hip (the rows matched against founders), csrc/fseq_api_identity.hip (identity columns dropped
// and put back), csrc/fseq_api_rowsplit.hip (rows held out of the resident alignment) and csrc/fseq_api_input.hip (the input rows in column chunks).  Internal: nothing here is part of the boundary.
#pragma once

#include "../../include/fseq.h"
#include "../../include/fseq_debug.h"
#include "fseq_types.hpp"
#include "fseq_chainplan.hpp"    // ChainLaunch: what a context remembers of its last phase B

#include <hip/hip_runtime.h>

#include <algorithm>
#include <array>
#include <atomic>
#include <chrono>
#include <climits>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <thread>
#include <unordered_map>
#include <vector>

namespace fseq {

struct KernelSet {
	uint32_t T, E, sigma, cap;
	size_t lds_colblock, lds_snap;
	uint32_t scan_shift;                     // partition steps of this configuration may scan keys while every divergence is < 2^scan_shift
	// (the launchers take the views of fseq_types.hpp and write out the kernel's parameter list)
	void (*rank)(hipStream_t st, uint32_t grid, size_t lds, PhaseAArgs const &keys);
	void (*snap)(hipStream_t st, uint32_t grid, size_t lds, SnapArgs const &tasks);
	size_t (*columns_lds)(uint32_t B);
	void (*columns)(hipStream_t st, uint32_t grid, size_t lds, ColumnsArgs const &cols);      // (cols.colmask: the kernel that takes dense columns in one digit pass)
	uint32_t (*columns_resident)(size_t lds);                 // workgroups of k_columns one CU holds
	size_t lds_chain;
	void (*chain)(hipStream_t st, uint32_t grid, size_t lds, ChainMultiArgs const &chains, uint32_t keyed);
	hipError_t (*prepare)();
	hipError_t (*prepare_columns)(size_t lds_columns);
};

template <typename K>
inline hipError_t allow_lds(K kernel, size_t bytes)
{
	if (bytes <= 64 * 1024) return hipSuccess;
	return hipFuncSetAttribute(reinterpret_cast<void const *>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int) bytes);
}

struct Stream2Config { uint32_t T, E, key_shift; size_t (*lds)(uint32_t colbytes); hipError_t (*prepare)(size_t lds);
	void (*launch)(hipStream_t st, uint32_t grid, size_t lds, ColumnsArgs const &cols);
	uint32_t (*resident)(size_t lds);
	// pass 2 on the same tile step: k_columns_stream2<.., S2_SNAP>
	void (*launch_snap)(hipStream_t st, uint32_t grid, size_t lds, SnapArgs const &tasks); };
// [r5] phase C on representative rows (fseq_reduced.hpp; the kernels live in csrc/fseq_reduced.hip)
struct ReducedSet {
	uint32_t T, E, rows, values;             // rows: representatives a workgroup holds; values: distinct start values (fewer than rows: the slim configuration)
	bool pk, ew;
	size_t (*lds)(uint32_t B, uint32_t symcap);   // symcap: bytes of each staged-column buffer (RedArgs).  Phase C's form: what planning counts with
	// [r16] pass 2's sweep form (k_columns_red<.., SW>: no value table, no id histogram) asks for less.  A configuration has the forms
	// the plan can send it: phase C's with a list wave or at most 128 threads, the sweep form without a list wave
	size_t (*lds_sweep)(uint32_t B, uint32_t symcap);
	// sweep: the form asked for (an error where the configuration does not have it)
	hipError_t (*prepare)(size_t lds, bool sweep);
	// (cols: the alignment the representatives' symbols are read from -- RedArgs::direct -- and the lists; the rest comes with red:
	// the sweep form where red.cls is set)
	// hipErrorInvalidDeviceFunction, and nothing launched, for a form the configuration does not have
	hipError_t (*launch)(hipStream_t st, uint32_t grid, size_t lds, ColumnsArgs const &cols, RedArgs const &red);
	uint32_t (*resident)(size_t lds);          // (of phase C's form where the configuration has it, else of the sweep form: see LaunchRed)
	bool phase_form() const { return T <= 128u || ew; }
};
// the smallest configuration that holds `rows` representatives (index into the list; -1: none)
int reduced_config_count();
bool reduced_config(int index, ReducedSet *out);
// pass 2's chain step for the base configuration <T, E> of a KernelSet
struct ChainSnapSet {
	size_t lds;
	hipError_t (*prepare)();
	// (tasks: the blocks' boundary states, task_blk, the snapshots, keyed; red: rank, m_true, cap and the class tables)
	void (*launch)(hipStream_t st, uint32_t grid, size_t lds, SnapArgs const &tasks, RedArgs const &red);
};
bool select_chain_snap(uint32_t T, uint32_t E, ChainSnapSet *out);

// the kernel configurations and their launchers (csrc/fseq_kernelsets.hip)
bool select_kernels(uint32_t m, uint32_t sigma, KernelSet *out);
Stream2Config stream2_config();
void launch_blockkeys(hipStream_t st, uint32_t grid, size_t lds, PhaseAArgs const &keys);       // (k_blockkeys<keys.T>)
hipError_t prepare_blockkeys(uint32_t T, size_t lds, bool debug);
uint32_t blocktrie_threads(uint32_t m, bool stream);
size_t blocktrie_lds(uint32_t T);
hipError_t launch_blocktrie(hipStream_t st, uint32_t groups, PhaseAArgs const &keys);           // (k_blocktrie<8 >> bsh, keys.T>)
hipError_t launch_reduce_prep(hipStream_t, uint32_t grid, RedPrepArgs const &);
void launch_reduce_check(hipStream_t, uint32_t const *cnt, uint32_t const *planned, uint32_t count, uint32_t *flags);
void launch_reduce_msa(hipStream_t st, MsaArgs const &A, ReducedMsaArgs const &red, bool gather_only);
bool launch_reduce_cls(hipStream_t st, MsaArgs const &A, ReducedMsaArgs const &red, ClassColumnArgs const &classes);      // (false: not this shape, nothing launched)

inline double now_ms()
{
	using namespace std::chrono;
	return duration<double, std::milli>(steady_clock::now().time_since_epoch()).count();
}


} // namespace fseq

// Diagnostic / test knobs of the library.  They are read from the environment ONCE, when a context is created
// (fseq_create), and can be set per context with fseq_debug_set_tuning (include/fseq_debug.h); nothing on the run
// path looks at the environment.  Every knob selects among exact alternatives (results never depend on them).
struct Tuning {
	bool debug = false;                  // FSEQ_DEBUG: progress notes on stderr
	bool dp_serial = false;              // FSEQ_DP_SERIAL: the serial DP instead of the speculative sweeps
	int  dp_spec_win = 0, dp_spec_rounds = 0, dp_spec_max_sweeps = 0;      // FSEQ_DP_SPEC_*: tail window, chunk length, sweep budget
	bool stream_plain_scan = false;      // FSEQ_STREAM_PLAIN_SCAN: streamed phase C with the has-based scan (first form)
	bool plain_scan = false;             // FSEQ_PLAIN_SCAN: phase B / pass 2 never scan keys
	bool occurrence_keys = false;        // FSEQ_OCCURRENCE_KEYS: ... scan occurrence keys even where row counts fit the keys
	bool phase_a_classic = false;        // FSEQ_PHASE_A_CLASSIC: phase A as a column sweep
	int  chain_fan = 0;                  // FSEQ_CHAIN_FAN: group size of phase B's recursion
	bool blockkeys_wide = false;         // FSEQ_BLOCKKEYS_WIDE: 32-bit ids in the streamed key-space tree from the start
	bool blockkeys_single = false;       // FSEQ_BLOCKKEYS_SINGLE: its leaves one by one (no pair leaves)
	bool no_dense_columns = false;       // FSEQ_NO_DENSE_COLUMNS: every column of 4-bit symbols in two digit passes (by itself: one pass where at most four codes are present)
	bool no_blocktrie = false;           // FSEQ_NO_BLOCKTRIE: the streamed phase A without the trie over 16-column words (fseq_blocktrie.hpp): the key-space tree on every block
	bool blocktrie_always = false;       // FSEQ_BLOCKTRIE_ALWAYS: the trie for LDS-resident rows of any count (by itself: from 6,145 rows on)
	int  blockkeys_cap = 0;              // FSEQ_BLOCKKEYS_CAP: words of the key-space tree's LDS bitmap
	bool ss_unpacked = false;            // FSEQ_SS_UNPACKED: 8-byte stride states in the streamed regime
	bool ss_absolute = false;            // FSEQ_SS_ABSOLUTE: stride states hold divergences and pass 2 runs the first form's tile step (the form before round 4)
	bool poison_lists = false;           // FSEQ_POISON_LISTS: lists and headers filled with 0xFF before phase C
	bool join_host = false;              // FSEQ_JOIN_HOST: the joiners' class tables and edges, and the join score, on the host
	bool join_wide = false;              // FSEQ_JOIN_WIDE: ... through the wide device front (strips of left classes) at any max_segment_size; FSEQ_JOIN_HOST wins
	bool join_bip_wide = false;          // FSEQ_JOIN_BIP_WIDE: fseq_join_bipartite through the wide device form (weights in slabs of device memory) at any max_segment_size up to 4,096; FSEQ_JOIN_HOST wins
	int  join_bip_slabs = 0;             // FSEQ_JOIN_BIP_SLABS: most slabs (= persistent workgroups) of the wide form (by itself: from the CU count and the memory)
	int  segfile_batch = 0;              // FSEQ_SEGFILE_BATCH: most bytes of a batch of fseq_write_segments_device / fseq_write_segments_restored (by itself: 256 MiB; tests: batches of a line or two)
	int  graph_batch = 0;                // FSEQ_GRAPH_BATCH: most bytes of a batch of fseq_write_block_graph (by itself: 256 MiB; tests: batches of a line or two)
	bool shard_dp_full = false;          // FSEQ_SHARD_DP_FULL: the sharded DP gathers the whole key array after every sweep (round 2-3 form)
	int  shard_dp_window = 0;            // FSEQ_SHARD_DP_WINDOW: entries of the other ranks a rank holds in front of its own (tests: small windows)
	int  inject_failure_rank = -1;       // FSEQ_INJECT_FAILURE_RANK: this rank of a sharded run fails after phase A
	std::string sync_phases;             // FSEQ_SYNC_PHASES: "ABC": synchronise after these phases (a fault shows where it happened)
	bool check_phase_a = false;          // FSEQ_CHECK_PHASE_A: validate the key blocks on the host before phase B
	bool no_reduced = false;             // FSEQ_NO_REDUCED: phase C and pass 2 on all rows of every block (the form before round 5)
	int  reduced_margin = -1;            // FSEQ_REDUCED_MARGIN: counts beyond the list capacity the choice of vmin allows for (tests: 0 makes lists dig below it)
	bool reduced_always = false;         // FSEQ_REDUCED_ALWAYS: the representatives whenever some block has fewer of them than rows (tests of the mixed runs)
	bool reduced_msa_gather = false;     // FSEQ_REDUCED_MSA_GATHER: the reduced alignment by gathers from memory (by itself: the column through LDS where it fits)
	int  red_ss_stride = 0;              // FSEQ_RED_SS_STRIDE: columns between the reduced states phase C drops for pass 2's sweeps (a power of two, 4..64; by itself: 16 streamed, 8 LDS-resident)
	int  reduced_cap = 0;                // FSEQ_REDUCED_CAP: most representatives a block may have (tests: small values send blocks to the run on all rows)
	bool class_gather = false;           // FSEQ_CLASS_GATHER: the class columns are gathered into the reduced alignment for every block (the form before the column kernel staged them itself)
	int  class_columns = 1;              // FSEQ_CLASS_COLUMNS=0: the reduced alignment is gathered from the alignment (a second read of it: the form before phase A wrote class columns)
	int  p2_run_cap = -1;                // FSEQ_P2_RUN_CAP: most runs of equal class a task of the streamed pass 2 moves by runs (0: every task sorts its rows; clamped to P2_RUN_CAP)
	int  chain_run_cap = -1;             // FSEQ_CHAIN_RUN_CAP: most runs of equal key a step of phase B's chain-per-workgroup kernel moves by runs (0: every step sorts its rows; clamped to CW_RUN_CAP)
	int  p2_keys = 0;                    // FSEQ_P2_KEYS: unset or 0: phase B's chain-per-workgroup kernel hands the keys of the blocks it steps through to pass 2's streamed chain step; 2: it writes none and pass 2 gathers its own
	int  chain_wg = 0;                   // FSEQ_CHAIN_WG: streamed phase B's chains on one workgroup each (k_chain_wg): unset or 0: launches of at least a chain per CU; 1: every launch; 2: none
	bool scan_rebuild = false;           // FSEQ_SCAN_REBUILD: fseq_scan_segment_lengths builds the lists at every length (by itself: folds them from the length before, builds where the DP asks)
	int  match_split = 0;                // FSEQ_MATCH_SPLIT: segments the matcher's walk is split into along the columns (1..4,096; 1 = unsplit; by itself: the entries that take query rows choose, those over the alignment's rows walk unsplit)
	int  match_overlap = 0;              // FSEQ_MATCH_OVERLAP: columns (of a restored match: kept columns) a segment's cold walk starts in front of its range (by itself: 16,384)
	int  match_stage = 0;                // FSEQ_MATCH_STAGE_BYTES: most bytes of a staged chunk of fseq_match_rows_restored's query rows (by itself: 64 MiB; tests: chunks of 64 columns)
	int  graph_thread_key_bits = 0;      // FSEQ_GRAPH_THREAD_KEY_BITS: bits of a node key of fseq_graph_thread_rows / _held_out (1..64; by itself: 64; tests: a bit or two, so that classes share keys)
	int  graph_nearest_batch = 0;        // FSEQ_GRAPH_NEAREST_BATCH: most bytes of packed class representatives in a batch of fseq_graph_nearest_rows / _held_out (by itself: 256 MiB; tests: a segment a batch)

	// Every knob once, by name: a flag (set = on), a number (set: at least lo; unset: off) or a string.
	struct Knob {
		char const *name;
		bool Tuning::*flag;
		int Tuning::*num;
		int lo, off;
		std::string Tuning::*str;
	};
	static std::vector<Knob> const &knobs()
	{
		static std::vector<Knob> const table = {
			{"FSEQ_DEBUG", &Tuning::debug, nullptr, 0, 0, nullptr},
			{"FSEQ_DP_SERIAL", &Tuning::dp_serial, nullptr, 0, 0, nullptr},
			{"FSEQ_DP_SPEC_WIN", nullptr, &Tuning::dp_spec_win, 1, 0, nullptr},
			{"FSEQ_DP_SPEC_ROUNDS", nullptr, &Tuning::dp_spec_rounds, 1, 0, nullptr},
			{"FSEQ_DP_SPEC_MAX_SWEEPS", nullptr, &Tuning::dp_spec_max_sweeps, 1, 0, nullptr},
			{"FSEQ_STREAM_PLAIN_SCAN", &Tuning::stream_plain_scan, nullptr, 0, 0, nullptr},
			{"FSEQ_PLAIN_SCAN", &Tuning::plain_scan, nullptr, 0, 0, nullptr},
			{"FSEQ_OCCURRENCE_KEYS", &Tuning::occurrence_keys, nullptr, 0, 0, nullptr},
			{"FSEQ_PHASE_A_CLASSIC", &Tuning::phase_a_classic, nullptr, 0, 0, nullptr},
			{"FSEQ_CHAIN_FAN", nullptr, &Tuning::chain_fan, 2, 0, nullptr},
			{"FSEQ_BLOCKKEYS_WIDE", &Tuning::blockkeys_wide, nullptr, 0, 0, nullptr},
			{"FSEQ_BLOCKKEYS_SINGLE", &Tuning::blockkeys_single, nullptr, 0, 0, nullptr},
			{"FSEQ_NO_DENSE_COLUMNS", &Tuning::no_dense_columns, nullptr, 0, 0, nullptr},
			{"FSEQ_NO_BLOCKTRIE", &Tuning::no_blocktrie, nullptr, 0, 0, nullptr},
			{"FSEQ_BLOCKTRIE_ALWAYS", &Tuning::blocktrie_always, nullptr, 0, 0, nullptr},
			{"FSEQ_BLOCKKEYS_CAP", nullptr, &Tuning::blockkeys_cap, 2048, 0, nullptr},
			{"FSEQ_SS_UNPACKED", &Tuning::ss_unpacked, nullptr, 0, 0, nullptr},
			{"FSEQ_SS_ABSOLUTE", &Tuning::ss_absolute, nullptr, 0, 0, nullptr},
			{"FSEQ_POISON_LISTS", &Tuning::poison_lists, nullptr, 0, 0, nullptr},
			{"FSEQ_JOIN_HOST", &Tuning::join_host, nullptr, 0, 0, nullptr},
			{"FSEQ_JOIN_WIDE", &Tuning::join_wide, nullptr, 0, 0, nullptr},
			{"FSEQ_JOIN_BIP_WIDE", &Tuning::join_bip_wide, nullptr, 0, 0, nullptr},
			{"FSEQ_JOIN_BIP_SLABS", nullptr, &Tuning::join_bip_slabs, 1, 0, nullptr},
			{"FSEQ_SEGFILE_BATCH", nullptr, &Tuning::segfile_batch, 1, 0, nullptr},
			{"FSEQ_GRAPH_BATCH", nullptr, &Tuning::graph_batch, 1, 0, nullptr},
			{"FSEQ_SHARD_DP_FULL", &Tuning::shard_dp_full, nullptr, 0, 0, nullptr},
			{"FSEQ_SHARD_DP_WINDOW", nullptr, &Tuning::shard_dp_window, 64, 0, nullptr},
			{"FSEQ_INJECT_FAILURE_RANK", nullptr, &Tuning::inject_failure_rank, INT_MIN, -1, nullptr},
			{"FSEQ_SYNC_PHASES", nullptr, nullptr, 0, 0, &Tuning::sync_phases},
			{"FSEQ_CHECK_PHASE_A", &Tuning::check_phase_a, nullptr, 0, 0, nullptr},
			{"FSEQ_NO_REDUCED", &Tuning::no_reduced, nullptr, 0, 0, nullptr},
			{"FSEQ_REDUCED_MARGIN", nullptr, &Tuning::reduced_margin, 0, -1, nullptr},
			{"FSEQ_REDUCED_ALWAYS", &Tuning::reduced_always, nullptr, 0, 0, nullptr},
			{"FSEQ_REDUCED_MSA_GATHER", &Tuning::reduced_msa_gather, nullptr, 0, 0, nullptr},
			{"FSEQ_REDUCED_CAP", nullptr, &Tuning::reduced_cap, 1, 0, nullptr},
			{"FSEQ_RED_SS_STRIDE", nullptr, &Tuning::red_ss_stride, 4, 0, nullptr},
			{"FSEQ_P2_RUN_CAP", nullptr, &Tuning::p2_run_cap, 0, -1, nullptr},
			{"FSEQ_CHAIN_RUN_CAP", nullptr, &Tuning::chain_run_cap, 0, -1, nullptr},
			{"FSEQ_CHAIN_WG", nullptr, &Tuning::chain_wg, 0, 0, nullptr},
			{"FSEQ_P2_KEYS", nullptr, &Tuning::p2_keys, 0, 0, nullptr},
			{"FSEQ_CLASS_COLUMNS", nullptr, &Tuning::class_columns, 0, 1, nullptr},
			{"FSEQ_CLASS_GATHER", &Tuning::class_gather, nullptr, 0, 0, nullptr},
			{"FSEQ_SCAN_REBUILD", &Tuning::scan_rebuild, nullptr, 0, 0, nullptr},
			{"FSEQ_MATCH_SPLIT", nullptr, &Tuning::match_split, 1, 0, nullptr},
			{"FSEQ_MATCH_OVERLAP", nullptr, &Tuning::match_overlap, 1, 0, nullptr},
			{"FSEQ_MATCH_STAGE_BYTES", nullptr, &Tuning::match_stage, 64, 0, nullptr},
			{"FSEQ_GRAPH_THREAD_KEY_BITS", nullptr, &Tuning::graph_thread_key_bits, 1, 0, nullptr},
			{"FSEQ_GRAPH_NEAREST_BATCH", nullptr, &Tuning::graph_nearest_batch, 1, 0, nullptr},
		};
		return table;
	}

	void apply(Knob const &k, char const *value)
	{
		bool const on = value != nullptr;
		if (k.flag) this->*k.flag = on;
		else if (k.num) this->*k.num = on ? std::max(k.lo, atoi(value)) : k.off;
		else this->*k.str = on ? value : "";
	}

	// returns false for a name it does not know
	bool set(char const *name, char const *value)
	{
		for (Knob const &k : knobs())
			if (!strcmp(k.name, name)) { apply(k, value); return true; }
		return false;
	}

	void from_environment()
	{
		for (Knob const &k : knobs())
			if (char const *v = getenv(k.name)) apply(k, v);
	}
};

struct fseq_ctx;

namespace fseq {

// A device buffer of T that a context owns.  Every device allocation of a context is one of these: fseq_ctx::alloc_total is
// what the context holds (the memory plan of the stride states stays inside fseq_set_memory_budget's figure when ranks share
// a card), so an allocation is always of exactly the elements asked for.  A failed allocation leaves the buffer empty.
// The buffer converts to the pointer its users address it by: `base`, or -- rebase / alloc_range -- a pointer below it, so
// that item i of an array of which the context holds a range only sits at + i * per (a rank of a sharded run holds its own
// column blocks, addressed by their place in the whole alignment).
template <typename T>
struct DevBuf {
	T *base = nullptr;                       // what was allocated (nullptr: empty)
	size_t cap = 0;                          // elements asked for
	ptrdiff_t shift = 0;                     // bytes from the pointer handed out up to base
	operator T *() const { return base ? reinterpret_cast<T *>(reinterpret_cast<char *>(base) - shift) : nullptr; }
	template <typename U> U *as() const { return reinterpret_cast<U *>(static_cast<T *>(*this)); }
	void rebase(ptrdiff_t elements) { shift = elements * (ptrdiff_t) sizeof(T); }
	int alloc(fseq_ctx *c, size_t count);                     // exactly `count` elements in place of what is held
	bool try_alloc(fseq_ctx *c, size_t count);                // the same for a buffer the run can do without: false, and no error on the context, where the device has no room
	int ensure(fseq_ctx *c, size_t count) { return cap >= count ? FSEQ_OK : alloc(c, count); }      // grow-only
	int alloc_range(fseq_ctx *c, size_t lo, size_t hi, size_t per)      // items [lo, hi) of `per` elements each
	{
		int const rc = alloc(c, (hi > lo ? hi - lo : 0) * per);
		rebase((ptrdiff_t) (lo * per));
		return rc;
	}
	void release(fseq_ctx *c);
};

// ... of one call: released on every way out of its scope
template <typename T>
struct DevTemp : DevBuf<T> {
	fseq_ctx *const c;
	explicit DevTemp(fseq_ctx *c_) : c(c_) {}
	DevTemp(DevTemp const &) = delete;
	~DevTemp() { this->release(c); }
	int alloc(size_t count) { return DevBuf<T>::alloc(c, count); }
};

template <typename... B>
inline void release_all(fseq_ctx *c, B &...bufs) { (bufs.release(c), ...); }

} // namespace fseq

// One alignment over several ranks (include/fseq.h, fseq_set_shard): which blocks / columns / DP chunks are mine
struct Shard {
	bool on = false;
	uint32_t rank = 0, world = 1;
	uint32_t *xbuf = nullptr;               // caller-owned exchange buffer (device)
	uint64_t xwords = 0;
	fseq_allreduce_fn fn = nullptr;
	void *user = nullptr;
	uint32_t bpr = 0;                       // blocks per rank = shard_q * chain_fan^shard_k (a rank is one hyper-block of phase B)
	uint32_t active = 1;                    // ranks that own blocks
	uint32_t b_lo = 0, b_hi = 0;            // my blocks
	uint64_t c_lo = 0, c_hi = 0, c_end = 0; // my columns [c_lo, c_hi); held: [c_lo, c_end) (halo for my last DP round)
	bool posted = false;                    // this rank has told the others that it failed (once per context)
	bool closed = false;                    // the run's last exchange is done: nobody is left to hear of a failure
};

struct fseq_ctx {
	fseq_params p{};
	Tuning tune;                             // read from the environment once, at fseq_create
	template <typename T> using DevBuf = fseq::DevBuf<T>;
	std::unordered_map<void *, size_t> alloc_sizes;   // device allocations of this context (DevBuf)
	size_t alloc_total = 0;
	size_t alloc_peak = 0;                    // the most alloc_total has been (fseq_debug_device_bytes)
	uint64_t mem_budget = 0;                  // fseq_set_memory_budget: 0 = whatever is free on the device
	// fseq_set_list_memory: the lists of a long-path run in column windows (csrc/fseq_path_attempt.hip, plan_list_windows).  The buffer
	// holds the columns [lo_w B - H, hi_w B) of window w: d_ent is rebased to (lo_w B - H) stride.
	struct ListWindows {
		uint64_t budget = 0;                  // bytes (0: every list held, the default)
		bool on = false;                      // the last long-path run went through windows
		uint32_t wb = 0, H = 0, nwin = 0;     // blocks per window, halo columns, windows
		uint32_t merge_windows = 0;           // windows the merge's second pass ran phase C on again
		uint64_t bytes = 0;                   // the list buffer's size
		uint64_t col_lo = 0, col_hi = 0;      // columns whose lists the buffer holds now (fseq_debug_column_list)
		std::vector<hipEvent_t> ev;           // per window: DP begin / end
	} lw;
	std::atomic<uint64_t> step_max{0}, current_step{0};      // fseq_step_max / fseq_current_step (segmentation_lp_context.hh:122-127)
	fseq_join_profile jp{};                  // the last joiner call (fseq_get_join_profile)
	int join_path = -1;                      // the last fseq_join_greedy (fseq_debug_join_path): 0 host, 1 the LDS front, 2 the wide front; -1: none yet
	int bip_path = -1;                       // the last fseq_join_bipartite since the input was set (fseq_debug_bipartite_path): 0 host, 1 the LDS form, 2 the wide form; -1: none yet
	int rand_path = -1;                      // the last fseq_join_random since the input was set (fseq_debug_random_path): 0 host, 1 the class tables from the device; -1: none yet
	int score_path = -1;                     // the last fseq_join_score since the input was set (fseq_debug_join_score_path): 0 host, 1 the device form; -1: none yet
	struct SegFileStats { bool have = false; uint64_t batches = 0, bytes = 0, longest_line = 0, lines = 0; } segfile;      // the last fseq_write_segments_device or fseq_write_segments_restored (fseq_debug_segments_file)
	struct GraphFileStats { bool have = false; uint64_t batches[3] = {}, lines[3] = {}, bytes[3] = {}; } graphfile;      // the last fseq_write_block_graph (fseq_debug_graph_file): the S, L and P sections
	struct GraphThreadStats { bool have = false; fseq_graph_thread_info info{}; } graphthread;      // the last fseq_graph_thread_rows / fseq_graph_thread_held_out (fseq_debug_graph_thread)
	struct GraphNearestStats { bool have = false; fseq_graph_nearest_info info{}; } graphnearest;      // the last fseq_graph_nearest_rows / fseq_graph_nearest_held_out (fseq_debug_graph_nearest_info)
	fseq_progress_fn progress_fn = nullptr;
	void *progress_user = nullptr;
	hipStream_t stream = nullptr;
	std::string err;
	Shard sh;
	DevBuf<uint8_t> d_msa_own;               // the alignment when the context allocated it; d_msa = d_msa_own.base - c_lo * ld (column k at d_msa + k * ld)
	DevBuf<uint32_t> d_bkws;                 // ... streamed rows: per-workgroup workspace (id arrays, group ids)
	DevBuf<uint16_t> d_bk;                   // phase A in key space (fseq_blockkeys.hpp): per-block scratch (leaf words, group ids)
	size_t bk_per_block = 0;                 // ... halfwords of a block in it
	uint32_t bk_cap_words = 0;
	uint32_t bk_T = 0;                       // threads of k_blockkeys (LDS-resident rows)
	DevBuf<uint32_t> d_todo;                 // phase A: blocks the key-space tree gave up on (the column sweep does them)
	int bk_given_up = -1;                    // ... in the last run on this input (-1: not run yet): later runs skip the sweep's launch when
	                                         // it was none, and the tree altogether when it was most blocks
	size_t bk_lds = 0;
	DevBuf<uint32_t> d_colmask;              // 4-bit symbols: the codes present in every held column (k_column_presence), once per input (column k at d_colmask[k])
	bool colmask_ready = false, colmask_use = false;      // ... computed for this input; ... enough dense columns for the kernel that looks at it
	DevBuf<uint32_t> d_btws;                 // phase A, streamed rows, the trie (fseq_blocktrie.hpp): per-workgroup workspace (the nodes of the levels)
	DevBuf<uint32_t> d_only;                 // ... blocks the trie gave up on (the key-space tree does them)
	int bt_given_up = -1;                    // ... in the last run on this input (-1: not run yet)
	DevBuf<uint32_t> d_chunk_r0;             // speculative DP: first round of every chunk (+ the end)
	DevBuf<uint2> d_tau;                     // merge thresholds (k_seg_tau) / counts
	std::vector<int64_t> snap_slot;          // segment index -> slot in d_snap_* (-1: another rank's)
	// sharded DP (run_dp_spec): the DP entries [own_lo[g], own_hi[g]) belong to rank g (the last active rank also owns the
	// final cell's); dp_window_mode: a rank holds its own entries and a window of the others' in front of them, not the
	// whole arrays (the traceback then runs rank by rank, follow_traceback_sharded)
	std::vector<uint32_t> own_lo, own_hi;
	bool dp_window_mode = false;
	bool shard_dp_full_sticky = false;       // a sweep of this input read below its window once: whole-array exchanges from then on
	uint64_t dp_exchange_words = 0;          // words the DP's sweep exchanges moved in the last run (diagnostics)

	// input
	uint8_t *d_msa = nullptr;                // (not a DevBuf: the caller's own columns when the input was borrowed, fseq_set_device_columns)
	size_t ld = 0;
	bool have_input = false;
	uint32_t sigma = 0;
	uint8_t code_to_byte[256]{};

	// geometry
	uint32_t B = 0, nblocks = 0, N2 = 0, npass = 1;
	uint32_t auto_B = 0;                     // block length fitted to whole rounds of phase C's workgroups (short inputs)
	fseq::Stream2Config s2{};                      // streamed phase C, second form (T = 0: not in use)
	size_t s2_lds = 0;
	bool stream_staged = false;              // streamed kernels lay tiles out in LDS before writing them (needs 64 KiB more)
	uint32_t bsh = 0;                        // alignment packing: 8 >> bsh bits per symbol (fseq_kernels.hpp sym_bytes)
	fseq::KernelSet ks{};
	bool kernels_ready = false;
	bool use_stream = false;             // m too large for an LDS-resident order: HBM-streamed kernels (fseq_stream.hpp)
	size_t tb_guess = 0;                 // traceback entries of the last run (sizes the speculative copy of the next)
	std::vector<uint2> tau_host;         // merge thresholds that came back with the traceback (not sharded)
	DevBuf<uint32_t> d_ws;               // their per-block workspaces: streamed phase C's of block b at d_ws + b * (words per block); phase A's column
	                                     // sweep, phase B and pass 2 index the same memory by workgroup, from d_ws.base
	size_t lds_columns = 0;

	// device work buffers
	// per column block: key blocks (phase A) and boundary states (phase B), indexed by the block's place in the whole
	// alignment.  A rank of a sharded run allocates its own blocks [b_lo, b_hi] only and shifts the pointer
	// (block b at d_rank + b * m as before): memory per rank falls with the rank count
	DevBuf<uint32_t> d_rank, d_keyd, d_nkeys;
	DevBuf<uint32_t> d_bstate_a, d_bstate_d;
	DevBuf<uint32_t> d_cshist;               // streamed phase B spread over the chip (fseq_chainsort.hpp): digit histograms [chain][part][bin]
	int dev_cus = -1;                        // the device's CUs (device_cus: asked once a context)
	int cw_resident = 0;                     // workgroups of k_chain_wg a CU holds at once (prepare_stream_kernels)
	// [r15] phase B's hand-over to pass 2 (ChainMultiArgs::hand_keys): the keys of block b in the order in front of it at
	// d_p2keys + b * m where d_p2keys_flag[b] is set.  Buffers the run can do without (empty: pass 2 gathers its own)
	DevBuf<uint16_t> d_p2keys;
	DevBuf<uint32_t> d_p2keys_flag;
	bool p2keys_live = false;                // the flags are those of the boundary states the context holds (phase B cleared and set them)
	uint32_t p2_hand[2]{};                   // pass 2's groups of the last run that took handed-over keys, and those that gathered
	DevBuf<uint32_t> d_cw_stats;             // FSEQ_DEBUG: the counters of phase B's chain-per-workgroup kernel (CW_STATS words; empty otherwise: the kernel keeps none)
	// what the last phase B did (fseq_debug_phase_b): its chain launches in the order they were queued, the counters of k_chain_wg where
	// they were kept, whether the hand-over to pass 2 was armed, and the groups pass 2's streamed chain step then ran
	std::vector<fseq::ChainLaunch> pb_launches;
	uint32_t pb_cw_stats[fseq::CW_STATS]{};
	bool pb_cw_stats_have = false;
	bool pb_hand = false;
	uint64_t pb_fit = 0;                     // workgroups of k_chain_wg the workspace held (streamed rows; chain_wg_groups)
	uint32_t p2_groups = 0;
	DevBuf<uint32_t> d_hrank, d_hkeyd, d_hnkeys, d_hstate_a, d_hstate_d;
	// not sharded: phase B over any number of levels (levels[i - 1] = the composites of chain_fan level-(i - 1) key blocks)
	struct ChainLevel { uint32_t count = 0; uint64_t cols = 0; DevBuf<uint32_t> rank, keyd, nkeys, state_a, state_d; };
	std::vector<ChainLevel> levels;
	uint32_t chain_fan = 0;
	uint32_t shard_k = 0, shard_q = 0;       // sharded: a rank's hyper-block = shard_q groups of chain_fan^shard_k blocks
	uint32_t chain_G = 0, n_super = 0;       // sharded: super-blocks of chain_G blocks
	uint32_t chain_G2 = 0, n_hyper = 0;      // third level: hyper-blocks of chain_G2 super-blocks (0 = two levels only)
	DevBuf<uint2> d_ent;                     // the lists: column k at d_ent + k * stride
	DevBuf<uint4> d_hdr;
	uint32_t X = 0, stride = 0;
	uint32_t X_hint = 0;                     // list capacity that worked on the last run of this input
	struct Dp {                              // phase D's arrays; the kernels take them as DpArrays (fseq_types.hpp)
		DevBuf<uint32_t> M, LB, SZ, Tb, Tbv;
		DevBuf<unsigned long long> K;
		uint32_t tstride = 0;
		operator fseq::DpArrays() const { return fseq::DpArrays{M, LB, SZ, Tb, Tbv, K, tstride}; }
	} dp;
	DevBuf<uint32_t> d_Mprev;                // chunk-speculative DP: the iterate the last sweep started from
	DevBuf<uint32_t> d_spec;                 // its per-chunk words (active, changed, tailmin, floor, lift, 2 x ovf) + SpecCtl
	DevBuf<fseq::PathWords> d_flags;        // the path's device words, one PathWords (fseq_types.hpp; path_words in fseq_path.hpp)
	DevBuf<uint32_t> d_recent;               // k_boundary_recent counts, one per block boundary
	uint64_t dp_size = 0;
	DevBuf<uint64_t> d_cols;                 // scratch: column / rb lists
	DevBuf<uint2> d_grp;
	DevBuf<uint64_t> d_src;
	uint32_t snap_stride = 16;            // phase C drops the exact (a,d) every snap_stride columns for pass 2
	DevBuf<uint32_t> d_ss_a, d_ss_d;      // the stride states: the state at column q * snap_stride at d_ss_* + q * (words of a state)
	uint32_t ss_pack = 0;                 // streamed rows: stride states packed to 5 bytes per row (bits of a row id; fseq_stream.hpp)
	bool ss_ids = false;                  // ... and in ID form: the packed rows of phase C's workspace; pass 2 replays them on the same tile step (fseq_stream2.hpp, S2_SNAP)
	DevBuf<uint32_t> d_bs_w;              // ... with every block's start state in the same form (block b at d_bs_w + b * m)
	DevBuf<uint8_t> d_bs_h;
	DevBuf<uint32_t> d_wgblk;             // pass 2 on the tile step: block and groups of every workgroup
	DevBuf<uint2> d_wggrp;
	DevBuf<uint32_t> d_snap_a, d_snap_d;

	// [r5] phase C / pass 2 on representative rows (fseq_reduced.hpp): per block [red_cap] representatives (ascending row id),
	// their block keys, the reduced start state; the reduced alignment (column k at d_red_msa + k * red_ld)
	DevBuf<uint32_t> d_red_cnt, d_red_vmin, d_red_rows, d_red_leaf, d_red_a, d_red_d;      // (a rank holds its own blocks' rows)
	DevBuf<uint32_t> d_red_invalid, d_red_blocks;
	uint32_t red_cap = 0;
	DevBuf<uint8_t> d_red_msa;
	size_t red_ld = 0;
	// phase A's class columns (fseq_blocktrie.hpp, phase 3), what the reduced alignment of a block the trie ranked is gathered from: column k at
	// d_cls + k * cls_ld (a rank holds its own columns), d_cls_have[block] = 1 where this run's phase A wrote them
	DevBuf<uint8_t> d_cls;
	DevBuf<uint32_t> d_cls_have;
	size_t cls_ld = 0;
	bool cls_on = false;                     // this run's phase A wrote class columns
	bool cls_every = false;                  // ... for every block of mine (the trie ran alone: it gave no block up in the run before on this input)
	bool cls_read = false;                   // this run's reduced alignment took them where a block has them (fseq_debug_class_columns)
	// [r10] ... or the reduced column kernel staged them itself (RedArgs::cls_have): d_red_src[block] = red.plan.from_cls, uploaded with the plan's
	// block lists; cls_staged: this run's launches went so (FSEQ_CLASS_GATHER: never -- every block through the reduced alignment)
	DevBuf<uint32_t> d_red_src;
	bool cls_staged = false;
	// the plan of the representatives (fseq_redplan.hpp; red_plan, csrc/fseq_path_reduced.hip): every result of a planning is in
	// `plan`, everything a run remembers of this input for the next in `memory` (DESIGN.md section 1 has the table of what each
	// forget_* clears, by the site that calls it)
	struct Red {
		fseq::RedPlan plan;                  // of the last planning: read where red_active says this run's phase C went by it
		std::vector<uint8_t> cls_config;     // ... [configuration] RedConfig::cls as that planning saw it (the launches size their buffers by it)
		struct Memory {
			std::vector<uint8_t> force;      // [block] RED_FORCE_FULL / RED_FORCE_WIDE marks (RedPlanInput::force); of another input's size: none
			// `plan` is the plan (which block on which configuration) of the last run on this input at capacity plan_X: the next run
			// launches by it without waiting for the counts, and checks on the device that they are what the plan was made from
			bool plan_holds = false;
			uint32_t plan_X = 0;
			bool declined = false;           // the last run on this input (at capacity declined_X) found too many representatives: no prep this time
			uint32_t declined_X = 0;
			bool cls_unread = false;         // the plan of this input takes a path that reads no reduced alignment: phase A writes no class columns for it
			void forget_plan() { plan_holds = false; }                                     // the next attempt plans afresh
			void forget_verdicts() { plan_holds = false; declined = false; cls_unread = false; }      // ... and asks again whether the representatives pay (the buffers are gone)
			void forget_input() { forget_verdicts(); force.clear(); }                      // ... with no block marked (another input, or another geometry)
		} memory;
	} red;
	bool red_active = false;                 // this run's phase C went through the representatives (pass 2 follows it)
	DevBuf<uint32_t> d_red_cls, d_red_headd, d_red_ncls, d_red_taskblk, d_red_wgtasks;
	DevBuf<uint32_t> d_red_p2grp;            // streamed pass 2: its groups {first task, count}, the counter they are taken by and the kernel's counters
	uint32_t p2_stats[fseq::P2_STATS]{};                // ... of the last run (fseq_debug_pass2_paths): tasks by runs, tasks by the sort of all rows, border copies, most runs, tasks by run count
	bool p2_stats_have = false;              // the last run went through that kernel
	DevBuf<uint16_t> d_red_ss_a, d_red_ss_d; // the reduced states phase C drops every red_ss_stride columns ([q][red_ss_cap] halfwords: RedArgs)
	uint32_t red_ss_stride = 0, red_ss_cap = 0;
	uint32_t *h_red_pin = nullptr;           // pinned host staging of a planning's two copies (counts back, red.plan.blocks out): nothing reads it afterwards
	size_t red_pin_words = 0;
	bool red_direct = false;                 // the representatives' symbols are read from the alignment's own columns (LDS-resident row counts): no reduced alignment
	DevBuf<uint32_t> d_red_cnt_plan;         // the counts red.plan was made from (k_reduce_check)
	hipStream_t red_st[2]{};                 // the configurations' launches side by side: the context's second stream, then these
	struct RedEvents {                       // (no timing)
		hipEvent_t fork = nullptr;           // the context's stream has reached the launches: the side streams wait for it
		hipEvent_t join_stream2 = nullptr, join_side0 = nullptr, join_side1 = nullptr;     // a side stream's launch is queued: the context's stream waits for it
		std::array<hipEvent_t *, 3> joins() { return {&join_stream2, &join_side0, &join_side1}; }      // by side stream: stream2, red_st[0], red_st[1]
		std::array<hipEvent_t *, 4> all() { return {&fork, &join_stream2, &join_side0, &join_side1}; }
	} red_ev;
	uint8_t *h_red_pin2 = nullptr;           // pass 2's task lists (pinned)
	size_t red_pin2_bytes = 0;

	// results
	bool have_result = false;
	bool scan_lists = false;                 // no result, but the lists of a scan's last long-path entry (fseq_scan_segment_lengths): fseq_debug_column_list answers
	fseq_result res{};
	DevBuf<uint4> d_tb;                      // the traceback kernels' output {entry, lb, key, size} per segment, window heads, counts
	std::vector<fseq_dp_arg> traceback;
	std::vector<fseq_segment> segments;
	std::vector<uint32_t> sp_first, sp_len;
	fseq_timings tm{};
	// the path's events, by what they bracket; all on the context's stream but dp_reset
	struct PathEvents {
		hipEvent_t a_begin = nullptr, a_end_b_begin = nullptr, b_end = nullptr;      // phases A and B (once a run)
		hipEvent_t c_begin = nullptr, c_end = nullptr, dp_begin = nullptr, dp_end = nullptr;     // phase C and the DP of an attempt
		hipEvent_t pass2_begin = nullptr, pass2_end = nullptr;
		hipEvent_t dp_reset = nullptr;       // (no timing) the arrays of the speculative DP were reset on stream2
		std::array<hipEvent_t *, 9> timed() { return {&a_begin, &a_end_b_begin, &b_end, &c_begin, &c_end, &dp_begin, &dp_end, &pass2_begin, &pass2_end}; }
	} ev;
	hipStream_t stream2 = nullptr;           // beside the context's stream: the reset of the DP's arrays while phase C runs, the first side
	                                         // stream of the reduced configurations' launches, the chunked input's copies
	uint8_t *h_pin = nullptr;                // pinned host staging of a step's small transfers (pin_reserve / pin_take)
	size_t pin_cap = 0, pin_used = 0;

	// matching the rows against founders (fseq_match_founders, csrc/fseq_api_match.hip): nothing is allocated before the first
	// match; a run of the segmentation does not touch these
	struct Match {
		DevBuf<uint8_t> fcols;               // the founders as columns: the code of founder f at column k in fcols[k * Kp + f]
		DevBuf<uint32_t> cnt;                // counting pass: pieces, uncovered cells, short pieces of every row ([3][m])
		DevBuf<uint64_t> off;                // first piece of every row (+ the total), then the four totals of the summary
		DevBuf<fseq_match_piece> pieces;     // the last match: pieces by row, then lb
		DevBuf<uint32_t> sets;               // ... their founder sets, set_words each
		DevBuf<uint8_t> qrows;               // fseq_match_rows: the query rows, column-major and packed like the alignment
		DevBuf<uint32_t> split;              // the split walk: head and tail of every (row, g), flag and list of the row groups, {flagged groups, rows that do not stand}
		DevBuf<uint64_t> exc_off;            // fseq_match_rows_restored: the queries' exception cells (csrc/fseq_exceptions.hpp), [rows + 1]
		DevBuf<uint32_t> exc_cols;           // ... their source columns, exactly exc_total entries
		uint64_t exc_total = 0;
		int exc_from = 0;                    // whose exception cells the last match walked (fseq_get_match_exceptions): 0 none, 1 hold's, 2 the ones above
		uint32_t exc_rows = 0;               // ... and of how many query rows
		bool have = false;
		fseq_match_summary sum{};
		fseq_match_split_info split_info{};  // how the last match walked (fseq_debug_match_split)
		hipEvent_t ev[4]{};
	} match;
	void free_match()
	{
		fseq::release_all(this, match.fcols, match.cnt, match.off, match.pieces, match.sets, match.qrows, match.split, match.exc_off, match.exc_cols);
		for (auto &e : match.ev) if (e) { (void) hipEventDestroy(e); e = nullptr; }
		match.have = false;
		match.exc_from = 0;
	}

	// a context over the kept columns of another (fseq_create_without_identity_columns, csrc/fseq_api_identity.hip): what it
	// needs to put the identity columns back after its source is gone.  Empty on every other context
	struct Identity {
		bool have = false;
		uint64_t n_src = 0, identity = 0;    // columns of the source, identity columns among them
		DevBuf<uint8_t> mask;                // [n_src] 1 = identity column
		DevBuf<uint32_t> kept;               // [n]: source column of this context's column j (ascending)
		DevBuf<uint8_t> ref;                 // [n_src] row 0 of the source as raw bytes
	} idn;
	void free_identity()
	{
		fseq::release_all(this, idn.mask, idn.kept, idn.ref);
		idn.have = false;
	}

	// a context over some rows of another (fseq_create_without_rows, csrc/fseq_api_rowsplit.hip): the rows that were held out,
	// packed like the alignment, and the two maps back into the source's row numbers.  Empty on every other context
	struct HeldOut {
		bool have = false;
		uint32_t m_src = 0, n_held = 0;      // rows of the source, rows held out of it
		size_t ld = 0;                       // bytes of a held-out column: n_held fields rounded up to 16
		DevBuf<uint8_t> cols;                // column k at cols + k * ld; row q of it is held_rows[q]
		std::vector<uint32_t> kept_rows, held_rows;      // source row of this context's row j (ascending); the caller's list
		// fseq_create_without_identity_columns_held: cols holds the KEPT columns, and the held-out rows' exception cells (where one
		// differs from row 0 in an identity column; csrc/fseq_exceptions.hpp) are kept beside them
		bool have_exc = false;
		DevBuf<uint64_t> exc_off;            // [n_held + 1]
		DevBuf<uint32_t> exc_cols;           // source columns, ascending per row, exactly exc_total entries
		uint64_t exc_total = 0;
	} hold;
	void free_held_out()
	{
		fseq::release_all(this, hold.cols, hold.exc_off, hold.exc_cols);
		hold.have = hold.have_exc = false;
	}

	// the input in column chunks (fseq_input_begin .. fseq_input_end, csrc/fseq_api_input.hip): alive between begin and end only
	struct Input {
		bool open = false;
		bool given = false;                  // the alphabet came with begin (no scans)
		bool table_ready = false;            // the first fseq_input_columns has fixed the code table and allocated the alignment
		uint64_t half_bytes = 0, chunk_cols = 0;
		uint64_t scanned = 0, encoded = 0;   // columns [0, scanned) have been scanned, [0, encoded) encoded
		uint64_t calls = 0;                  // chunks so far: chunk i goes through half i & 1
		uint32_t present[8]{};               // the alphabet: supplied, or what the scans have found
		DevBuf<uint8_t> stage;               // the two halves
		DevBuf<uint32_t> words;              // [0, 8): bytes the scans found; [8, 16): bytes outside the alphabet the encode met
		DevBuf<uint8_t> table;               // [256] code of a byte (0xFF: not in the alphabet, where sigma < 256)
		hipEvent_t copied[2]{}, used[2]{};   // per half: its copies are done; the kernel that read it is done
		// the identity columns dropped on the way (fseq_input_scan_identity .. fseq_input_end_kept): the packed form of the source never exists
		int scan_mode = 0;                   // which scan entry this input uses: 0 none yet, 1 fseq_input_scan, 2 fseq_input_scan_identity
		DevBuf<uint8_t> id_mask, id_ref;     // [n] each, filled chunk by chunk; fseq_input_reduce hands them to the new context (idn.mask, idn.ref)
		DevBuf<uint32_t> id_acc;             // the chunk under way: OR over the rows of (piece ^ row 0's piece), 4 words a 16-column piece; zero between chunks
		bool reduced = false;                // fseq_input_reduce has made `half`
		fseq_ctx *half = nullptr;            // the context over the kept columns while it is filled: this input's until fseq_input_end_kept hands it out
		std::vector<uint32_t> kept;          // host copy of half->idn.kept (csrc/fseq_input_kept_range.hpp searches it)
	} in;
	void free_input()
	{
		if (in.half) { fseq_destroy(in.half); in.half = nullptr; }
		fseq::release_all(this, in.stage, in.words, in.table, in.id_mask, in.id_ref, in.id_acc);
		in.kept = std::vector<uint32_t>();
		in.reduced = false;
		for (auto &e : in.copied) if (e) { (void) hipEventDestroy(e); e = nullptr; }
		for (auto &e : in.used) if (e) { (void) hipEventDestroy(e); e = nullptr; }
		in.open = false;
	}
};


namespace fseq {

// the CUs of the context's device (0 where the runtime does not say)
inline int device_cus(fseq_ctx *c)
{
	if (c->dev_cus < 0 && hipDeviceGetAttribute(&c->dev_cus, hipDeviceAttributeMultiprocessorCount, c->p.device) != hipSuccess) c->dev_cus = 0;
	return c->dev_cus;
}

inline int fail(fseq_ctx *c, int code, char const *what, hipError_t e = hipSuccess)
{
	char buf[512];
	if (e != hipSuccess)
		snprintf(buf, sizeof(buf), "%s: %s", what, hipGetErrorString(e));
	else
		snprintf(buf, sizeof(buf), "%s", what);
	c->err = buf;
	return code;
}

// progress (include/fseq.h, fseq_set_progress): counters another thread may poll + the caller's callback
inline void progress(fseq_ctx *c, int stage, uint64_t current, uint64_t max)
{
	c->step_max.store(max, std::memory_order_relaxed);
	c->current_step.store(current, std::memory_order_relaxed);
	if (c->progress_fn) c->progress_fn(c->progress_user, stage, current, max);
}

// csrc/fseq_api.hip: a new input takes the context (every input setter, before it touches the alignment): the work buffers,
// the result and the last match are dropped and what runs remember of the last input is forgotten; a context over the kept
// columns of another refuses.  discard_input: the same and the alignment too (the chunked input's begin).
int take_new_input(fseq_ctx *c);
int discard_input(fseq_ctx *c);
void forget_input_history(fseq_ctx *c);

// what hands out a run's results asks this first: no run yet, or none since an input or a tuning knob was set
inline int need_result(fseq_ctx *c, bool long_path = true)
{
	if (!c->have_result)
		return fail(c, FSEQ_E_ARG, "no result on this context: no run has finished since its input or a tuning knob was set (fseq_run_segmentation)");
	if (long_path && c->res.short_path)
		return fail(c, FSEQ_E_ARG, "the last run took the short path (n < 2L): this call serves a long-path result");
	return FSEQ_OK;
}

// csrc/fseq_api_match.hip: n_rows query rows of n raw bytes onto the device -- column chunks through a bounded temporary, through
// the context's code table (a byte outside the alphabet: the code `sigma`), packed at `bsh` / `ld` into dst, which is grown to
// n * ld bytes (fseq_match_rows: the match's own buffer; fseq_graph_thread_rows: a temporary of the call)
int upload_queries(fseq_ctx *c, uint8_t const *const *rows, uint32_t n_rows, uint32_t bsh, size_t ld, DevBuf<uint8_t> &dst);
// ... and n_rows query rows of n_src raw bytes onto an identity-reduced context: their kept columns packed into dst the same
// way, and their exception cells (csrc/fseq_exceptions.hpp) into exc_off [n_rows + 1] / exc_cols [*exc_total], each grown or
// replaced as the lists need (fseq_match_rows_restored: the match's own buffers; fseq_graph_thread_rows_restored: temporaries of
// the call)
int upload_queries_restored(fseq_ctx *c, uint8_t const *const *rows, uint32_t n_rows, uint32_t bsh, size_t ld, DevBuf<uint8_t> &dst,
                            DevBuf<uint64_t> &exc_off, DevBuf<uint32_t> &exc_cols, uint64_t *exc_total);
// csrc/fseq_api_join.hip: the merged segments of an identity-reduced context in the source's co-ordinates (restored_segment_bounds,
// csrc/fseq_restored_bounds.hpp, on the kept columns copied to the host); FSEQ_E_UNSUPPORTED where the pure function refuses
int restored_bounds_of(fseq_ctx *c, std::vector<uint64_t> &src_lb, std::vector<uint64_t> &src_rb);

#define HIP_TRY(c, expr)                                                   \
	do {                                                                   \
		hipError_t e_ = (expr);                                            \
		if (e_ != hipSuccess) return fail((c), FSEQ_E_HIP, #expr, e_);     \
	} while (0)

template <typename T>
void DevBuf<T>::release(fseq_ctx *c)
{
	if (base)
	{
		auto it = c->alloc_sizes.find(static_cast<void *>(base));
		if (it != c->alloc_sizes.end()) { c->alloc_total -= it->second; c->alloc_sizes.erase(it); }
		(void) hipFree(base);
	}
	*this = DevBuf<T>{};
}

template <typename T>
bool DevBuf<T>::try_alloc(fseq_ctx *c, size_t count)
{
	release(c);
	size_t const bytes = std::max<size_t>(count, 1) * sizeof(T);
	if (hipMalloc(reinterpret_cast<void **>(&base), bytes) != hipSuccess)
	{
		base = nullptr;
		(void) hipGetLastError();          // (as in alloc: the runtime must not remember the failure)
		return false;
	}
	cap = count;
	c->alloc_sizes[static_cast<void *>(base)] = bytes;
	c->alloc_total += bytes;
	c->alloc_peak = std::max(c->alloc_peak, c->alloc_total);
	return true;
}

template <typename T>
int DevBuf<T>::alloc(fseq_ctx *c, size_t count)
{
	release(c);
	size_t const bytes = std::max<size_t>(count, 1) * sizeof(T);
	hipError_t e = hipMalloc(reinterpret_cast<void **>(&base), bytes);
	if (e != hipSuccess)
	{
		base = nullptr;
		size_t free_b = 0, total_b = 0;
		(void) hipMemGetInfo(&free_b, &total_b);
		(void) hipGetLastError();          // the runtime remembers the failure: the checks behind later launches (of this or any
		                                   // other context of the thread) must not find it
		char what[160];
		snprintf(what, sizeof(what), "hipMalloc of %zu bytes (%zu of %zu bytes free on the device)", bytes, free_b, total_b);
		return fail(c, e == hipErrorOutOfMemory ? FSEQ_E_OOM : FSEQ_E_HIP, what, e);
	}
	cap = count;
	c->alloc_sizes[static_cast<void *>(base)] = bytes;
	c->alloc_total += bytes;
	c->alloc_peak = std::max(c->alloc_peak, c->alloc_total);
	return FSEQ_OK;
}

} // namespace fseq
