"""founder-sequences_amd: MI355X-native segmentation engine (host-side Python mirror of the C ABI).

The compute lives in libfseq_hip.so (hand-written HIP for gfx950, built in-tree by build.py) behind
the C ABI declared in include/fseq.h.  This module is a thin ctypes mirror of that ABI, named after
the reference's interface for the path (segmentation_lp_context / segmentation_container,
include/founder_sequences/segmentation_lp_context.hh:45-121, segmentation_container.hh:15-20).

There is NO CPU fallback: if the library is missing, or no GPU is visible, calls raise.
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libfseq_hip.so")

FSEQ_OK, FSEQ_E_ARG, FSEQ_E_NO_REDUCTION, FSEQ_E_HIP, FSEQ_E_OOM, FSEQ_E_UNSUPPORTED = range(6)


class FseqError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("fseq error %d: %s" % (code, msg))
        self.code = code


class NoReduction(FseqError):
    """generate_context.cc:192-200: max segment size equals the number of input sequences."""


class Params(C.Structure):
    _fields_ = [("m", C.c_uint32), ("n", C.c_uint64), ("segment_length", C.c_uint64),
                ("pbwt_sample_rate", C.c_uint64), ("block_len", C.c_uint32), ("list_cap", C.c_uint32),
                ("device", C.c_int32)]


class SynthSpec(C.Structure):
    _fields_ = [("seed", C.c_uint64), ("n_founders", C.c_uint32), ("block_len", C.c_uint32),
                ("mut_threshold", C.c_uint64), ("kind", C.c_uint32)]


class Segment(C.Structure):
    _fields_ = [("lb", C.c_uint64), ("rb", C.c_uint64), ("segment_size", C.c_uint32), ("reserved", C.c_uint32)]


class DpArg(C.Structure):
    _fields_ = [("lb", C.c_uint64), ("rb", C.c_uint64), ("segment_max_size", C.c_uint32), ("segment_size", C.c_uint32)]


class Result(C.Structure):
    _fields_ = [("max_segment_size", C.c_uint32), ("short_path", C.c_uint32),
                ("dp_segment_count", C.c_uint64), ("segment_count", C.c_uint64)]


class Timings(C.Structure):
    _fields_ = [("ms_total", C.c_double), ("ms_phase_a", C.c_double), ("ms_phase_b", C.c_double),
                ("ms_phase_c", C.c_double), ("ms_dp", C.c_double), ("ms_pass2", C.c_double), ("ms_host", C.c_double),
                ("ms_colstep_kernels", C.c_double), ("colstep_launches", C.c_uint64), ("colstep_cells", C.c_uint64),
                ("pass2_cells", C.c_uint64), ("list_cap_used", C.c_uint32), ("retries", C.c_uint32),
                ("block_len", C.c_uint32), ("n_blocks", C.c_uint32),
                ("dp_chunks", C.c_uint32), ("dp_sweeps", C.c_uint32), ("phase_a_fallbacks", C.c_uint32), ("phase_a_given_up", C.c_uint32), ("phase_a_trie_given_up", C.c_uint32),
                ("reduced_blocks", C.c_uint32), ("reduced_rows_mean", C.c_uint32), ("reduced_redone", C.c_uint32)]


CHAIN_LEVELS_MAX, CHAIN_LAUNCHES_MAX = 40, 80      # include/fseq_debug.h, FSEQ_DEBUG_CHAIN_LEVELS / _LAUNCHES
CHAIN_COMPOSE, CHAIN_TOP, CHAIN_EXPAND = 0, 1, 2    # fseq_chain_launch_info.kind


class ChainLaunchInfo(C.Structure):
    _fields_ = [(f, C.c_uint32) for f in ("level", "kind", "chains", "blocks", "first_chain", "workgroups")]


class ChainPlan(C.Structure):
    _fields_ = [(f, C.c_uint32) for f in ("fan", "fan_round5", "turns", "shard_k", "shard_q", "blocks_per_rank", "n_hyper", "b_lo", "b_hi",
                                          "n_levels", "n_launches", "reserved")] + \
               [("level_items", C.c_uint32 * CHAIN_LEVELS_MAX), ("launches", ChainLaunchInfo * CHAIN_LAUNCHES_MAX)]


class PhaseBInfo(C.Structure):
    _fields_ = [(f, C.c_uint32) for f in ("cus", "nblocks", "fan", "n_launches", "resident", "hand_armed", "stats_kept", "reserved")] + \
               [("fit", C.c_uint64)] + [(f, C.c_uint32) for f in ("p2_groups", "p2_groups_took_keys", "p2_groups_gathered", "reserved2")] + \
               [("cw_stats", C.c_uint32 * 23), ("reserved3", C.c_uint32), ("launches", ChainLaunchInfo * CHAIN_LAUNCHES_MAX)]


class JoinProfile(C.Structure):
    _fields_ = [("ms_d2h", C.c_double), ("ms_classes", C.c_double), ("ms_edges", C.c_double), ("ms_draw", C.c_double), ("ms_total", C.c_double),
                ("bytes_d2h", C.c_uint64)]


class MatchPiece(C.Structure):
    _fields_ = [("lb", C.c_uint64), ("rb", C.c_uint64), ("row", C.c_uint32), ("n_founders", C.c_uint32)]


class MatchSummary(C.Structure):
    _fields_ = [("pieces", C.c_uint64), ("uncovered_cells", C.c_uint64), ("short_pieces", C.c_uint64), ("max_pieces_per_row", C.c_uint64),
                ("n_founders", C.c_uint32), ("set_words", C.c_uint32), ("ms_device", C.c_double)]


class MatchSplitInfo(C.Structure):
    _fields_ = [("segments", C.c_uint32), ("row_groups", C.c_uint32), ("flagged_groups", C.c_uint32), ("reserved", C.c_uint32),
                ("overlap", C.c_uint64), ("rows_not_standing", C.c_uint64)]


class IdentitySummary(C.Structure):
    _fields_ = [("n", C.c_uint64), ("identity", C.c_uint64), ("kept", C.c_uint64), ("ms_device", C.c_double)]


class HoldOutSummary(C.Structure):
    _fields_ = [("m_src", C.c_uint32), ("held", C.c_uint32), ("kept", C.c_uint32), ("reserved", C.c_uint32), ("ms_device", C.c_double)]


class JoinScoreSummary(C.Structure):
    _fields_ = [("junctions", C.c_uint64), ("supported", C.c_uint64), ("unsupported", C.c_uint64), ("gaps", C.c_uint64), ("rows_through", C.c_uint64),
                ("weight", C.c_uint64), ("min_rows_through_junction", C.c_uint64), ("min_rows_through", C.c_uint32), ("max_breaks", C.c_uint32),
                ("ms_device", C.c_double)]


class GraphSummary(C.Structure):
    _fields_ = [("segments", C.c_uint64), ("nodes", C.c_uint64), ("edges", C.c_uint64), ("ms_device", C.c_double)]


class GraphFileStats(C.Structure):
    _fields_ = [("batches", C.c_uint64 * 3), ("lines", C.c_uint64 * 3), ("bytes", C.c_uint64 * 3)]


class GraphThreadSummary(C.Structure):
    _fields_ = [("rows", C.c_uint64), ("segments", C.c_uint64), ("segments_matched", C.c_uint64), ("junctions_linked", C.c_uint64),
                ("junctions_novel", C.c_uint64), ("walks", C.c_uint64), ("rows_on_graph", C.c_uint64), ("ms_device", C.c_double)]


class GraphThreadInfo(C.Structure):
    _fields_ = [("key_bits", C.c_uint32), ("table_slots", C.c_uint32), ("candidates_verified", C.c_uint64), ("candidates_rejected", C.c_uint64),
                ("queries_out_of_alphabet", C.c_uint64)]


class GraphNearestSummary(C.Structure):
    _fields_ = [("rows", C.c_uint64), ("segments", C.c_uint64), ("segments_admitted", C.c_uint64), ("segments_exact", C.c_uint64),
                ("junctions_linked", C.c_uint64), ("junctions_novel", C.c_uint64), ("walks", C.c_uint64), ("rows_on_graph", C.c_uint64),
                ("mismatches", C.c_uint64), ("ms_device", C.c_double)]


class GraphNearestInfo(C.Structure):
    _fields_ = [("batches", C.c_uint64), ("packed_words", C.c_uint64), ("query_words", C.c_uint64), ("bits", C.c_uint32), ("reserved", C.c_uint32)]


class DpListsInfo(C.Structure):
    _fields_ = [("unproven", C.c_uint32), ("dp_chunks", C.c_uint32), ("dp_sweeps", C.c_uint32), ("launches", C.c_uint32)]


class MergeListsInfo(C.Structure):
    _fields_ = [("overflow", C.c_uint32), ("tau_separate", C.c_uint32), ("threshold_launches", C.c_uint32), ("count_launches", C.c_uint32)]


class LengthScanSummary(C.Structure):
    _fields_ = [("lists_built", C.c_uint32), ("lists_folded", C.c_uint32), ("short_entries", C.c_uint32), ("retries", C.c_uint32),
                ("ms_phase_a", C.c_double), ("ms_phase_b", C.c_double), ("ms_total", C.c_double)]


# fseq_length_scan_entry (include/fseq.h), 40 bytes
LENGTH_SCAN_DTYPE = np.dtype([("segment_length", "<u8"), ("max_segment_size", "<u4"), ("short_path", "<u4"), ("lists", "<u4"), ("list_cap", "<u4"),
                              ("dp_chunks", "<u4"), ("reserved", "<u4"), ("ms_device", "<f8")])
SCAN_LISTS_BUILT, SCAN_LISTS_FOLDED, SCAN_LISTS_NONE = 0, 1, 2

# fseq_join_score_entry (include/fseq.h), 32 bytes
JOIN_SCORE_DTYPE = np.dtype([("rb", "<u8"), ("weight", "<u8"), ("supported", "<u4"), ("unsupported", "<u4"), ("gaps", "<u4"), ("rows_through", "<u4")])
JOIN_SCORE_MAX_SLOTS = 4096    # csrc/fseq_joinscore.hpp, JS_MAX_SLOTS: the device form's cap on max_segment_size
JOIN_SCORE_GAP = 0xFFFF        # ... JS_GAP: a slot's class where its row is a gap (debug_join_score)

# fseq_graph_node (include/fseq.h), 32 bytes, and fseq_graph_edge, 16 bytes
GRAPH_NODE_DTYPE = np.dtype([("lb", "<u8"), ("rb", "<u8"), ("segment", "<u4"), ("cls", "<u4"), ("rep_row", "<u4"), ("rows", "<u4")])
GRAPH_EDGE_DTYPE = np.dtype([("from", "<u4"), ("to", "<u4"), ("rows", "<u4"), ("junction", "<u4")])
GRAPH_PATHS = 1                # fseq_write_block_graph's flag: the P lines
GRAPH_NONE = 0xFFFFFFFF        # FSEQ_GRAPH_NONE: no node of a segment carries the query's substring / no edge joins the two nodes
# fseq_graph_thread_row (include/fseq.h), 40 bytes, and fseq_graph_thread_segment, 16 bytes
GRAPH_THREAD_ROW_DTYPE = np.dtype([("columns_matched", "<u8"), ("longest_walk_columns", "<u8"), ("segments_matched", "<u4"), ("junctions_linked", "<u4"),
                                   ("junctions_novel", "<u4"), ("walks", "<u4"), ("longest_walk_segments", "<u4"), ("reserved", "<u4")])
GRAPH_THREAD_SEGMENT_DTYPE = np.dtype([("matched", "<u4"), ("linked", "<u4"), ("novel", "<u4"), ("reserved", "<u4")])
GRAPH_THREAD_MAX_CLASSES = 4096    # csrc/fseq_graphthread.hpp, GT_MAX_CLASSES
# fseq_graph_nearest_row (include/fseq.h), 64 bytes, and fseq_graph_nearest_segment, 32 bytes
GRAPH_NEAREST_ROW_DTYPE = np.dtype([("columns_admitted", "<u8"), ("longest_walk_columns", "<u8"), ("mismatches_admitted", "<u8"), ("mismatches", "<u8"),
                                    ("segments_admitted", "<u4"), ("segments_exact", "<u4"), ("junctions_linked", "<u4"), ("junctions_novel", "<u4"),
                                    ("walks", "<u4"), ("longest_walk_segments", "<u4"), ("max_distance", "<u4"), ("reserved", "<u4")])
GRAPH_NEAREST_SEGMENT_DTYPE = np.dtype([("mismatches", "<u8"), ("admitted", "<u4"), ("exact", "<u4"), ("linked", "<u4"), ("novel", "<u4"),
                                        ("max_distance", "<u4"), ("reserved", "<u4")])
GRAPH_NEAREST_BATCH_BYTES = 256 << 20   # csrc/fseq_graphnearest_plan.hpp, GN_BATCH_BYTES

MATCH_PIECE_DTYPE = np.dtype([("lb", "<u8"), ("rb", "<u8"), ("row", "<u4"), ("n_founders", "<u4")])
MATCH_MAX_FOUNDERS = 2048      # csrc/fseq_match.hpp, MT_MAX_FOUNDERS

SEGMENT_DTYPE = np.dtype([("lb", "<u8"), ("rb", "<u8"), ("segment_size", "<u4"), ("reserved", "<u4")])
DPARG_DTYPE = np.dtype([("lb", "<u8"), ("rb", "<u8"), ("segment_max_size", "<u4"), ("segment_size", "<u4")])

# every symbol include/fseq.h declares
EXPORTS = [
    "fseq_abi_version", "fseq_strerror", "fseq_create", "fseq_destroy", "fseq_last_error",
    "fseq_set_rows", "fseq_set_matrix", "fseq_set_device_columns", "fseq_generate_synthetic", "fseq_get_matrix",
    "fseq_run_segmentation", "fseq_get_traceback", "fseq_get_segments", "fseq_boundary_state",
    "fseq_short_path_runs", "fseq_join_greedy", "fseq_greedy_match_host", "fseq_write_founders", "fseq_write_founders_device", "fseq_debug_dp", "fseq_debug_block_state", "fseq_debug_column_list", "fseq_get_timings",
    "fseq_rowshard_xbuf_words", "fseq_rowshard_rows", "fseq_rowshard_pbwt",
    "fseq_debug_rmq", "fseq_shard_xbuf_words", "fseq_set_shard", "fseq_shard_columns", "fseq_shard_owner",
    "fseq_set_device_columns_packed", "fseq_debug_dp_schedule", "fseq_run_segmentation_batch", "fseq_join_bipartite", "fseq_join_random", "fseq_bipartite_match_host", "fseq_random_join_host", "fseq_write_segments",
    "fseq_set_progress", "fseq_step_max", "fseq_current_step", "fseq_set_memory_budget", "fseq_write_segments_host", "fseq_get_join_profile", "fseq_debug_set_tuning",
    "fseq_shard_abort", "fseq_debug_dp_owned", "fseq_debug_clock", "fseq_debug_ranges",
    "fseq_set_list_memory", "fseq_debug_list_windows",
    "fseq_match_founders", "fseq_match_founder_rows", "fseq_get_match", "fseq_write_match",
    "fseq_identity_columns", "fseq_create_without_identity_columns", "fseq_get_identity_columns", "fseq_write_identity_columns", "fseq_write_founders_restored", "fseq_match_founders_restored",
    "fseq_input_begin", "fseq_input_chunk_columns", "fseq_input_scan", "fseq_input_columns", "fseq_input_end", "fseq_set_rows_streamed", "fseq_debug_device_bytes", "fseq_debug_packed_columns",
    "fseq_debug_join_path", "fseq_debug_pass2_paths", "fseq_debug_class_columns", "fseq_debug_bipartite_path",
    "fseq_debug_pass2_step", "fseq_debug_chain_launch", "fseq_debug_chain_launch_wg", "fseq_debug_red_plan", "fseq_debug_column_sources", "fseq_debug_red_cls_direct",
    "fseq_write_segments_device", "fseq_random_join_classes_host", "fseq_debug_segments_file", "fseq_debug_random_path",
    "fseq_set_segment_length", "fseq_scan_segment_lengths", "fseq_debug_scan_plan", "fseq_debug_relump_lists",
    "fseq_match_rows", "fseq_debug_match_split",
    "fseq_create_without_rows", "fseq_get_held_out", "fseq_match_held_out", "fseq_debug_held_out_columns", "fseq_debug_row_split_plan",
    "fseq_debug_dp_lists_check", "fseq_debug_dp_on_lists", "fseq_debug_merge_on_lists", "fseq_debug_traceback_parts",
    "fseq_create_without_identity_columns_held", "fseq_match_held_out_restored", "fseq_match_rows_restored", "fseq_get_match_exceptions",
    "fseq_get_segments_restored", "fseq_write_segments_restored", "fseq_debug_restored_bounds",
    "fseq_input_scan_identity", "fseq_input_reduce", "fseq_input_kept_columns", "fseq_input_columns_kept", "fseq_input_end_kept",
    "fseq_set_rows_streamed_without_identity_columns", "fseq_debug_input_kept_range", "fseq_debug_alphabet",
    "fseq_join_score", "fseq_join_score_host", "fseq_debug_join_score_path", "fseq_debug_join_score",
    "fseq_block_graph", "fseq_write_block_graph", "fseq_debug_graph_file",
    "fseq_debug_local_pass",
    "fseq_graph_thread_rows", "fseq_graph_thread_held_out", "fseq_debug_graph_thread",
    "fseq_graph_nearest_rows", "fseq_graph_nearest_held_out", "fseq_debug_graph_nearest_info", "fseq_debug_graph_nearest_plan", "fseq_debug_graph_nearest",
    "fseq_write_block_graph_restored", "fseq_graph_thread_rows_restored", "fseq_graph_thread_held_out_restored",
    "fseq_debug_chain_launch_wg_keys", "fseq_debug_pass2_step_keys",
    "fseq_debug_chain_plan", "fseq_debug_chain_plan_sharded", "fseq_debug_phase_b",
    "fseq_debug_class_tables",
]
# ... of which include/fseq_debug.h declares these (intermediate state for tests, not part of the drop-in boundary)
DEBUG_EXPORTS = ["fseq_debug_dp", "fseq_debug_dp_owned", "fseq_debug_clock", "fseq_debug_ranges", "fseq_debug_block_state", "fseq_debug_column_list", "fseq_debug_rmq", "fseq_debug_dp_schedule", "fseq_debug_set_tuning",
                 "fseq_debug_list_windows", "fseq_debug_device_bytes", "fseq_debug_packed_columns", "fseq_debug_join_path", "fseq_debug_pass2_paths",
                 "fseq_debug_class_columns", "fseq_debug_bipartite_path", "fseq_debug_pass2_step", "fseq_debug_chain_launch", "fseq_debug_chain_launch_wg", "fseq_debug_red_plan", "fseq_debug_column_sources", "fseq_debug_red_cls_direct",
                 "fseq_debug_segments_file", "fseq_debug_random_path", "fseq_debug_scan_plan", "fseq_debug_relump_lists", "fseq_debug_match_split",
                 "fseq_debug_held_out_columns", "fseq_debug_row_split_plan", "fseq_debug_dp_lists_check", "fseq_debug_dp_on_lists",
                 "fseq_debug_merge_on_lists", "fseq_debug_traceback_parts",
                 "fseq_debug_restored_bounds", "fseq_debug_input_kept_range", "fseq_debug_alphabet",
                 "fseq_debug_join_score_path", "fseq_debug_join_score", "fseq_debug_graph_file", "fseq_debug_local_pass",
                 "fseq_debug_graph_thread", "fseq_debug_graph_nearest_info", "fseq_debug_graph_nearest_plan", "fseq_debug_graph_nearest",
                 "fseq_debug_chain_launch_wg_keys", "fseq_debug_pass2_step_keys",
                 "fseq_debug_chain_plan", "fseq_debug_chain_plan_sharded", "fseq_debug_phase_b", "fseq_debug_class_tables"]

FSEQ_E_PEER = 6
P2_RUN_CAP = 8832       # csrc/fseq_chainsort.hpp: the most runs FSEQ_P2_RUN_CAP admits (pass2_paths)
CW_RUN_CAP = 16384      # ... and FSEQ_CHAIN_RUN_CAP (chain_launch_wg)
STAGE_TRACEBACK, STAGE_MERGE, STAGE_SAMPLES = 0, 1, 2
# fseq_progress_fn (include/fseq.h): (user, stage, current_step, step_max)
PROGRESS_FN = C.CFUNCTYPE(None, C.c_void_p, C.c_int, C.c_uint64, C.c_uint64)

JOIN_GREEDY, JOIN_BIPARTITE, JOIN_RANDOM = 0, 1, 2

# fseq_allreduce_fn (include/fseq.h): all-reduce xbuf[offset .. offset + count) over the ranks, op 0 = sum, 1 = max
ALLREDUCE_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_uint64, C.c_uint64, C.c_int)

_lib = None


def load_library():
    """Loads libfseq_hip.so; raises (never falls back) when it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError("%s is missing: run `python __graft_entry__.py build` (hipcc --offload-arch=gfx950); "
                          "there is no CPU fallback for the segmentation path" % LIB_PATH)
    L = C.CDLL(LIB_PATH)
    vp, u64, sz = C.c_void_p, C.c_uint64, C.c_size_t
    L.fseq_abi_version.restype = C.c_uint32
    L.fseq_strerror.restype = C.c_char_p
    L.fseq_strerror.argtypes = [C.c_int]
    L.fseq_create.argtypes = [C.POINTER(Params), C.POINTER(vp)]
    L.fseq_destroy.argtypes = [vp]
    L.fseq_destroy.restype = None
    L.fseq_last_error.restype = C.c_char_p
    L.fseq_last_error.argtypes = [vp]
    L.fseq_set_rows.argtypes = [vp, C.POINTER(vp)]
    L.fseq_set_matrix.argtypes = [vp, vp, sz, sz]
    L.fseq_set_device_columns.argtypes = [vp, vp, sz, C.c_uint32]
    L.fseq_set_device_columns_packed.argtypes = [vp, vp, sz, C.c_uint32, C.c_uint32]
    L.fseq_generate_synthetic.argtypes = [vp, C.POINTER(SynthSpec)]
    L.fseq_get_matrix.argtypes = [vp, u64, u64, vp, sz, sz]
    L.fseq_run_segmentation.argtypes = [vp, C.POINTER(Result)]
    L.fseq_get_traceback.argtypes = [vp, vp]
    L.fseq_get_segments.argtypes = [vp, vp]
    L.fseq_boundary_state.argtypes = [vp, u64, vp, vp]
    L.fseq_short_path_runs.argtypes = [vp, vp, vp]
    L.fseq_join_greedy.argtypes = [vp, vp]
    L.fseq_greedy_match_host.argtypes = [C.c_uint32, C.c_uint32, u64, vp, vp, vp, vp, vp]
    L.fseq_write_founders.argtypes = [vp, C.POINTER(vp), vp, C.c_char_p]
    L.fseq_write_founders_device.argtypes = [vp, vp, C.c_char_p]
    L.fseq_run_segmentation_batch.argtypes = [vp, sz, vp, vp]
    L.fseq_debug_dp_schedule.argtypes = [u64, u64, u64, vp, vp, vp, vp]
    L.fseq_join_bipartite.argtypes = [vp, vp]
    L.fseq_join_random.argtypes = [vp, C.c_uint32, vp]
    L.fseq_bipartite_match_host.argtypes = [C.c_uint32, C.c_uint32, u64, vp, vp, vp, vp, vp, vp]
    L.fseq_random_join_host.argtypes = [C.c_uint32, C.c_uint32, u64, vp, vp, vp, vp, C.c_uint32, vp]
    L.fseq_write_segments.argtypes = [vp, C.POINTER(vp), C.c_int, C.c_char_p]
    L.fseq_debug_dp.argtypes = [vp, vp, vp, vp]
    L.fseq_debug_block_state.argtypes = [vp, u64, vp, vp]
    L.fseq_debug_column_list.argtypes = [vp, u64, vp, vp, vp, vp, vp]
    L.fseq_get_timings.argtypes = [vp, C.POINTER(Timings)]
    L.fseq_debug_rmq.argtypes = [C.c_int, vp, C.c_uint32, vp, vp, C.c_uint32, vp, vp]
    L.fseq_shard_xbuf_words.restype = u64
    L.fseq_shard_xbuf_words.argtypes = [vp, C.c_uint32]
    L.fseq_set_shard.argtypes = [vp, C.c_uint32, C.c_uint32, vp, u64, ALLREDUCE_FN, vp]
    L.fseq_shard_columns.argtypes = [vp, C.POINTER(u64), C.POINTER(u64)]
    L.fseq_shard_owner.argtypes = [vp, u64, C.POINTER(C.c_uint32)]
    L.fseq_rowshard_xbuf_words.restype = u64
    L.fseq_rowshard_xbuf_words.argtypes = [C.c_uint32, C.c_uint32, C.c_uint32]
    L.fseq_rowshard_rows.argtypes = [C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]
    L.fseq_rowshard_pbwt.argtypes = [vp, vp, vp, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.POINTER(C.c_double), C.POINTER(u64)]
    L.fseq_write_segments_host.argtypes = [vp, C.POINTER(vp), C.c_int, vp, vp, C.c_char_p]
    L.fseq_get_join_profile.argtypes = [vp, C.POINTER(JoinProfile)]
    L.fseq_debug_set_tuning.argtypes = [vp, C.c_char_p, C.c_char_p]
    L.fseq_set_progress.argtypes = [vp, PROGRESS_FN, vp]
    L.fseq_step_max.restype = u64
    L.fseq_step_max.argtypes = [vp]
    L.fseq_current_step.restype = u64
    L.fseq_current_step.argtypes = [vp]
    L.fseq_set_memory_budget.argtypes = [vp, u64]
    L.fseq_set_list_memory.argtypes = [vp, u64]
    L.fseq_debug_list_windows.argtypes = [vp, C.POINTER(u64), C.POINTER(u64), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]
    L.fseq_shard_abort.argtypes = [vp, C.c_int]
    L.fseq_debug_dp_owned.argtypes = [vp, C.POINTER(u64), C.POINTER(u64), C.POINTER(C.c_int), C.POINTER(C.c_int)]
    L.fseq_debug_clock.argtypes = [vp, C.POINTER(C.c_double), C.POINTER(C.c_uint32)]
    L.fseq_debug_ranges.argtypes = [C.POINTER(u64), C.POINTER(u64), C.POINTER(C.c_int)]
    L.fseq_match_founders.argtypes = [vp, vp, u64, C.POINTER(MatchSummary)]
    L.fseq_match_founder_rows.argtypes = [vp, C.POINTER(vp), C.c_uint32, u64, C.POINTER(MatchSummary)]
    L.fseq_get_match.argtypes = [vp, vp, vp]
    L.fseq_write_match.argtypes = [vp, C.c_char_p]
    L.fseq_match_rows.argtypes = [vp, vp, C.POINTER(vp), C.c_uint32, C.POINTER(vp), C.c_uint32, u64, C.POINTER(MatchSummary)]
    L.fseq_debug_match_split.argtypes = [vp, C.POINTER(MatchSplitInfo)]
    L.fseq_identity_columns.argtypes = [vp, vp, C.POINTER(IdentitySummary)]
    L.fseq_create_without_identity_columns.argtypes = [vp, C.POINTER(Params), C.POINTER(vp), C.POINTER(IdentitySummary)]
    L.fseq_get_identity_columns.argtypes = [vp, vp, vp]
    L.fseq_write_identity_columns.argtypes = [vp, C.c_char_p]
    L.fseq_write_founders_restored.argtypes = [vp, vp, C.c_char_p]
    L.fseq_match_founders_restored.argtypes = [vp, vp, u64, C.POINTER(MatchSummary)]
    L.fseq_input_begin.argtypes = [vp, vp, C.c_uint32, u64]
    L.fseq_input_chunk_columns.restype = u64
    L.fseq_input_chunk_columns.argtypes = [vp]
    L.fseq_input_scan.argtypes = [vp, u64, u64, C.POINTER(vp)]
    L.fseq_input_columns.argtypes = [vp, u64, u64, C.POINTER(vp)]
    L.fseq_input_end.argtypes = [vp]
    L.fseq_set_rows_streamed.argtypes = [vp, C.POINTER(vp), u64]
    L.fseq_debug_device_bytes.argtypes = [vp, C.POINTER(u64), C.POINTER(u64), C.c_int]
    L.fseq_debug_packed_columns.argtypes = [vp, u64, u64, vp, C.POINTER(u64), C.POINTER(C.c_uint32)]
    L.fseq_debug_join_path.argtypes = [vp, C.POINTER(C.c_int)]
    L.fseq_debug_bipartite_path.argtypes = [vp, C.POINTER(C.c_int)]
    L.fseq_debug_pass2_paths.argtypes = [vp] + [C.POINTER(C.c_uint32)] * 4 + [vp]
    L.fseq_debug_class_tables.argtypes = [vp, vp, C.c_uint32, vp, vp, vp]
    L.fseq_debug_class_columns.argtypes = [vp, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.c_uint32, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.POINTER(u64), vp, u64]
    L.fseq_debug_column_sources.argtypes = [vp, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.c_uint32, C.POINTER(C.c_uint32)]
    L.fseq_debug_red_cls_direct.argtypes = [C.c_uint32, C.c_uint32, C.c_uint32, u64, C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(u64), C.POINTER(u64), C.POINTER(C.c_int)]
    L.fseq_debug_pass2_step.argtypes = [C.c_int, C.c_uint32, C.c_uint32, vp, vp, vp, C.c_uint32, C.c_uint32, vp, vp, vp, vp, C.c_uint32, C.c_uint32, vp, vp, vp]
    L.fseq_debug_chain_launch.argtypes = [C.c_int, C.c_uint32, C.c_uint32, C.c_uint32, u64, vp, vp, vp, C.c_uint32, C.c_uint32, vp, vp, vp, vp, vp, vp, vp]
    L.fseq_debug_chain_launch_wg.argtypes = [C.c_int, C.c_uint32, C.c_uint32, C.c_uint32, u64, vp, vp, vp, C.c_uint32, C.c_uint32, vp, vp, C.c_uint32, C.c_uint32, vp, vp, vp, vp, vp, vp]
    L.fseq_debug_chain_launch_wg_keys.argtypes = L.fseq_debug_chain_launch_wg.argtypes + [vp, vp]
    L.fseq_debug_pass2_step_keys.argtypes = [C.c_int, C.c_uint32, C.c_uint32, vp, vp, vp, C.c_uint32, C.c_uint32, vp, vp, vp, vp, C.c_uint32, C.c_uint32, vp, vp, vp, vp, vp, vp]
    L.fseq_debug_red_plan.argtypes = [C.c_uint32, C.c_uint32, C.c_uint32, C.c_int, C.c_uint32, C.c_uint32, C.c_uint32, vp, vp, C.c_int, C.c_int] + [vp] * 11
    L.fseq_write_segments_device.argtypes = [vp, C.c_int, C.c_char_p]
    L.fseq_random_join_classes_host.argtypes = [C.c_uint32, C.c_uint32, u64, vp, vp, vp, C.c_uint32, vp]
    L.fseq_debug_segments_file.argtypes = [vp] + [C.POINTER(u64)] * 4
    L.fseq_debug_random_path.argtypes = [vp, C.POINTER(C.c_int)]
    L.fseq_set_segment_length.argtypes = [vp, u64]
    L.fseq_scan_segment_lengths.argtypes = [vp, vp, sz, C.POINTER(LengthScanSummary)]
    L.fseq_debug_scan_plan.argtypes = [u64, vp, C.c_uint32, vp, C.POINTER(C.c_uint32), vp, C.POINTER(C.c_uint32)]
    L.fseq_debug_relump_lists.argtypes = [C.c_int, u64, C.c_uint32, C.c_uint32, u64, u64, vp, vp]
    L.fseq_create_without_rows.argtypes = [vp, vp, C.c_uint32, C.POINTER(Params), C.POINTER(vp), C.POINTER(HoldOutSummary)]
    L.fseq_get_held_out.argtypes = [vp, vp, vp]
    L.fseq_match_held_out.argtypes = [vp, vp, C.POINTER(vp), C.c_uint32, u64, C.POINTER(MatchSummary)]
    L.fseq_create_without_identity_columns_held.argtypes = [vp, C.POINTER(Params), C.POINTER(vp), C.POINTER(IdentitySummary)]
    L.fseq_match_held_out_restored.argtypes = [vp, vp, u64, C.POINTER(MatchSummary)]
    L.fseq_match_rows_restored.argtypes = [vp, vp, C.POINTER(vp), C.c_uint32, u64, C.POINTER(MatchSummary)]
    L.fseq_get_match_exceptions.argtypes = [vp, vp, vp, C.POINTER(u64)]
    L.fseq_debug_held_out_columns.argtypes = [vp, u64, u64, vp, C.POINTER(u64), C.POINTER(C.c_uint32)]
    L.fseq_debug_row_split_plan.argtypes = [C.c_uint32, C.c_uint32, vp, C.c_uint32, vp, vp, vp, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]
    L.fseq_debug_dp_lists_check.argtypes = [C.c_uint32, u64, u64, C.c_uint32, vp, vp, C.POINTER(u64), C.POINTER(C.c_uint32)]
    L.fseq_debug_dp_on_lists.argtypes = [vp, C.c_uint32, vp, vp, vp, C.c_uint32, vp, vp, vp, C.POINTER(DpListsInfo)]
    L.fseq_debug_merge_on_lists.argtypes = [vp, C.c_uint32, vp, vp, vp, vp, vp, C.c_uint32, vp, C.c_uint32, vp, C.POINTER(u64), vp, C.POINTER(u64), vp,
                                            C.POINTER(u64), C.POINTER(MergeListsInfo)]
    L.fseq_debug_traceback_parts.argtypes = [C.c_int, u64, u64, vp, vp, vp, vp, C.c_uint32, vp, vp, C.POINTER(u64), vp, vp, C.POINTER(u64)]
    L.fseq_debug_local_pass.argtypes = [C.c_int, C.c_uint32, C.c_uint32, vp, vp, vp, vp]
    L.fseq_get_segments_restored.argtypes = [vp, vp]
    L.fseq_write_segments_restored.argtypes = [vp, C.c_int, C.c_char_p]
    L.fseq_debug_restored_bounds.argtypes = [vp, u64, u64, vp, vp, u64, vp, vp]
    L.fseq_input_scan_identity.argtypes = [vp, u64, u64, C.POINTER(vp)]
    L.fseq_input_reduce.argtypes = [vp, C.POINTER(Params), C.POINTER(IdentitySummary)]
    L.fseq_input_kept_columns.argtypes = [vp, u64, u64, C.POINTER(u64)]
    L.fseq_input_columns_kept.argtypes = [vp, u64, u64, C.POINTER(vp)]
    L.fseq_input_end_kept.argtypes = [vp, C.POINTER(vp)]
    L.fseq_set_rows_streamed_without_identity_columns.argtypes = [vp, C.POINTER(vp), u64, C.POINTER(Params), C.POINTER(vp), C.POINTER(IdentitySummary)]
    L.fseq_debug_alphabet.argtypes = [vp, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), vp]
    L.fseq_debug_input_kept_range.argtypes = [vp, u64, u64, u64, C.POINTER(u64), C.POINTER(u64)]
    L.fseq_join_score.argtypes = [vp, vp, vp, vp, vp, C.POINTER(JoinScoreSummary)]
    L.fseq_join_score_host.argtypes = [C.c_uint32, C.c_uint32, u64, vp, vp, vp, vp, vp, vp, vp, vp, C.POINTER(JoinScoreSummary)]
    L.fseq_debug_join_score_path.argtypes = [vp, C.POINTER(C.c_int)]
    L.fseq_debug_join_score.argtypes = [C.c_int, C.c_uint32, C.c_uint32, C.c_uint32, vp, vp, vp, vp, vp, vp, C.POINTER(JoinScoreSummary)]
    L.fseq_block_graph.argtypes = [vp, vp, vp, vp, C.POINTER(GraphSummary)]
    L.fseq_write_block_graph.argtypes = [vp, C.c_uint32, C.c_int, C.c_char_p]
    L.fseq_debug_graph_file.argtypes = [vp, C.POINTER(GraphFileStats)]
    L.fseq_graph_thread_rows.argtypes = [vp, C.POINTER(vp), C.c_uint32, vp, vp, vp, vp, C.POINTER(GraphThreadSummary)]
    L.fseq_graph_thread_held_out.argtypes = [vp, vp, vp, vp, vp, C.POINTER(GraphThreadSummary)]
    L.fseq_debug_graph_thread.argtypes = [vp, C.POINTER(GraphThreadInfo)]
    L.fseq_graph_nearest_rows.argtypes = [vp, C.POINTER(vp), C.c_uint32, C.c_uint32, vp, vp, vp, vp, vp, vp, C.POINTER(GraphNearestSummary)]
    L.fseq_graph_nearest_held_out.argtypes = [vp, C.c_uint32, vp, vp, vp, vp, vp, vp, C.POINTER(GraphNearestSummary)]
    L.fseq_debug_graph_nearest_info.argtypes = [vp, C.POINTER(GraphNearestInfo)]
    L.fseq_debug_graph_nearest_plan.argtypes = [vp, vp, vp, u64, C.c_uint32, u64, vp, vp, C.POINTER(u64)]
    L.fseq_debug_graph_nearest.argtypes = [C.c_int, vp, u64, C.c_uint32, u64, C.c_uint32, vp, vp, vp, vp, C.c_uint32, C.c_uint32, vp, u64, C.c_uint32,
                                           C.c_uint32, C.c_uint32, u64, vp, vp, vp, C.POINTER(GraphNearestInfo)]
    L.fseq_debug_chain_plan.argtypes = [C.c_uint32, C.c_int, C.c_uint32, C.c_uint32, C.c_int, C.c_uint32, u64, C.c_uint32, C.POINTER(ChainPlan)]
    L.fseq_debug_chain_plan_sharded.argtypes = [C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_int, C.c_uint32, C.c_int, u64, C.c_uint32, C.POINTER(ChainPlan)]
    L.fseq_debug_phase_b.argtypes = [vp, C.POINTER(PhaseBInfo)]
    L.fseq_write_block_graph_restored.argtypes = [vp, C.c_uint32, C.c_int, C.c_char_p]
    L.fseq_graph_thread_rows_restored.argtypes = [vp, C.POINTER(vp), C.c_uint32, vp, vp, vp, vp, C.POINTER(GraphThreadSummary)]
    L.fseq_graph_thread_held_out_restored.argtypes = [vp, vp, vp, vp, vp, C.POINTER(GraphThreadSummary)]
    _lib = L
    return L


def synth_threshold(mu):
    """mu * 2^64 as the generator's integer threshold (same rounding as the C implementations)."""
    if mu <= 0.0:
        return 0
    if mu >= 1.0:
        return 0xFFFFFFFFFFFFFFFF
    return int(mu * 18446744073709551616.0)


def greedy_match_host(m, max_segment_size, lb, rb, a, d):
    """greedy_matcher::match on caller-supplied boundary states (host only, no GPU needed)."""
    L = load_library()
    lb = np.ascontiguousarray(lb, dtype=np.uint64)
    rb = np.ascontiguousarray(rb, dtype=np.uint64)
    a = np.ascontiguousarray(a, dtype=np.uint32)
    d = np.ascontiguousarray(d, dtype=np.uint32)
    perm = np.zeros((len(lb), max_segment_size), dtype=np.uint32)
    rc = L.fseq_greedy_match_host(m, max_segment_size, len(lb), lb.ctypes.data, rb.ctypes.data, a.ctypes.data, d.ctypes.data, perm.ctypes.data)
    if rc != FSEQ_OK:
        raise FseqError(rc, L.fseq_strerror(rc).decode())
    return perm


def debug_ranges():
    """(pushes, pops, built_with_roctx): the phase ranges this process has opened and closed so far."""
    a, b, w = C.c_uint64(), C.c_uint64(), C.c_int()
    load_library().fseq_debug_ranges(C.byref(a), C.byref(b), C.byref(w))
    return a.value, b.value, bool(w.value)


def debug_rmq(keys, beg, end, device=0):
    """rmq.hh as the device routines restate it, on caller keys: (index by the HBM path, index by the LDS path)."""
    L = load_library()
    keys = np.ascontiguousarray(keys, dtype=np.uint32)
    beg = np.ascontiguousarray(beg, dtype=np.uint32)
    end = np.ascontiguousarray(end, dtype=np.uint32)
    a = np.zeros(len(beg), dtype=np.uint32)
    b = np.zeros(len(beg), dtype=np.uint32)
    rc = L.fseq_debug_rmq(device, keys.ctypes.data, len(keys), beg.ctypes.data, end.ctypes.data, len(beg), a.ctypes.data, b.ctypes.data)
    if rc != FSEQ_OK:
        raise FseqError(rc, L.fseq_strerror(rc).decode())
    return a, b


P2_STATS = 23          # csrc/fseq_types.hpp: by runs, by sort, copies, the most runs, 19 words of the run counts' histogram
NOT_WRITTEN = 0xFFFFFFFF


def pass2_step(a0, d0, rank, task_blk, cls, headd, ncls, run_cap=P2_RUN_CAP, workgroups=1, device=0, hand_keys=None, hand_flag=None):
    """One launch of pass 2's streamed chain step (k_chain_snap_grouped) on constructed states: a0 / d0 / rank [nblocks][m],
    task_blk / ncls [ntasks], cls / headd [ntasks][cap].  Returns (snap_a, snap_d) [ntasks][m] (NOT_WRITTEN where the kernel wrote
    nothing) and the kernel's P2_STATS counters.  FseqError(FSEQ_E_ARG) where an input could take the kernel out of bounds.
    hand_keys [nblocks][m] (16 bits) and hand_flag [nblocks]: phase B's hand-over (fseq_debug_pass2_step_keys) -- a block with its flag
    set takes its ranks by position from hand_keys; a fourth value comes back, (groups that took them, groups that gathered)."""
    L = load_library()
    a0 = np.ascontiguousarray(np.atleast_2d(a0), dtype=np.uint32)
    d0 = np.ascontiguousarray(np.atleast_2d(d0), dtype=np.uint32)
    rank = np.ascontiguousarray(np.atleast_2d(rank), dtype=np.uint32)
    task_blk = np.ascontiguousarray(task_blk, dtype=np.uint32)
    ncls = np.ascontiguousarray(ncls, dtype=np.uint32)
    cls = np.ascontiguousarray(np.atleast_2d(cls), dtype=np.uint32)
    headd = np.ascontiguousarray(np.atleast_2d(headd), dtype=np.uint32)
    nblocks, m = a0.shape
    ntasks, cap = cls.shape
    if d0.shape != a0.shape or rank.shape != a0.shape or headd.shape != cls.shape or task_blk.shape != (ntasks,) or ncls.shape != (ntasks,):
        raise FseqError(FSEQ_E_ARG, "pass2_step: shapes disagree")
    snap_a = np.zeros((ntasks, m), dtype=np.uint32)
    snap_d = np.zeros((ntasks, m), dtype=np.uint32)
    stats = np.zeros(P2_STATS, dtype=np.uint32)
    if (hand_keys is None) != (hand_flag is None):
        raise FseqError(FSEQ_E_ARG, "pass2_step: hand_keys and hand_flag go together")
    if hand_keys is not None:
        hand_keys = np.ascontiguousarray(np.atleast_2d(hand_keys), dtype=np.uint16)
        hand_flag = np.ascontiguousarray(hand_flag, dtype=np.uint32)
        if hand_keys.shape != a0.shape or hand_flag.shape != (nblocks,):
            raise FseqError(FSEQ_E_ARG, "pass2_step: hand_keys is [nblocks][m], hand_flag [nblocks]")
        hand_stats = np.zeros(2, dtype=np.uint32)
        rc = L.fseq_debug_pass2_step_keys(device, m, nblocks, a0.ctypes.data, d0.ctypes.data, rank.ctypes.data, cap, ntasks, task_blk.ctypes.data,
                                          cls.ctypes.data, headd.ctypes.data, ncls.ctypes.data, run_cap, workgroups, hand_keys.ctypes.data,
                                          hand_flag.ctypes.data, snap_a.ctypes.data, snap_d.ctypes.data, stats.ctypes.data, hand_stats.ctypes.data)
    else:
        rc = L.fseq_debug_pass2_step(device, m, nblocks, a0.ctypes.data, d0.ctypes.data, rank.ctypes.data, cap, ntasks, task_blk.ctypes.data, cls.ctypes.data,
                                     headd.ctypes.data, ncls.ctypes.data, run_cap, workgroups, snap_a.ctypes.data, snap_d.ctypes.data, stats.ctypes.data)
    if rc != FSEQ_OK:
        raise FseqError(rc, L.fseq_strerror(rc).decode())
    if hand_keys is not None:
        return snap_a, snap_d, stats, hand_stats
    return snap_a, snap_d, stats


def chain_launch(rank, keyd, nkeys, G, cols_per_block, first_chain=0, chains=None, start_a=None, start_d=None, states=True, keys=False, device=0,
                 _wg=None, _hand=None):
    """One chain launch of phase B on streamed rows (k_cm_*) on constructed key blocks rank / keyd [nb_total][m], nkeys[nb_total]:
    the chains first_chain .. first_chain + chains - 1 (default: all behind first_chain) of G blocks, from start_a / start_d
    [chains][m] (None: the identity).  Returns a dict with state_a / state_d [nb_total + 1][m] where states, rank / keyd
    [chains][m] and nkeys [chains] where keys; NOT_WRITTEN where the launch wrote nothing."""
    L = load_library()
    rank = np.ascontiguousarray(np.atleast_2d(rank), dtype=np.uint32)
    keyd = np.ascontiguousarray(np.atleast_2d(keyd), dtype=np.uint32)
    nkeys = np.ascontiguousarray(nkeys, dtype=np.uint32)
    nb_total, m = rank.shape
    if keyd.shape != rank.shape or nkeys.shape != (nb_total,):
        raise FseqError(FSEQ_E_ARG, "chain_launch: shapes disagree")
    if chains is None:
        chains = max(0, (nb_total + G - 1) // G - first_chain) if G else 0
    if (start_a is None) != (start_d is None):
        raise FseqError(FSEQ_E_ARG, "chain_launch: start_a and start_d go together")
    if start_a is not None:
        start_a = np.ascontiguousarray(np.atleast_2d(start_a), dtype=np.uint32)
        start_d = np.ascontiguousarray(np.atleast_2d(start_d), dtype=np.uint32)
        if start_a.shape != (chains, m) or start_d.shape != (chains, m):
            raise FseqError(FSEQ_E_ARG, "chain_launch: start states are [chains][m]")
    out = {}
    if states:
        out["state_a"] = np.zeros((nb_total + 1, m), dtype=np.uint32)
        out["state_d"] = np.zeros((nb_total + 1, m), dtype=np.uint32)
    if keys:
        out["rank"] = np.zeros((chains, m), dtype=np.uint32)
        out["keyd"] = np.zeros((chains, m), dtype=np.uint32)
        out["nkeys"] = np.zeros(chains, dtype=np.uint32)
    ptr = lambda name: out[name].ctypes.data if name in out else None
    head = (device, m, nb_total, G, cols_per_block, rank.ctypes.data, keyd.ctypes.data, nkeys.ctypes.data, first_chain, chains,
            None if start_a is None else start_a.ctypes.data, None if start_a is None else start_d.ctypes.data)
    tail = (ptr("state_a"), ptr("state_d"), ptr("rank"), ptr("keyd"), ptr("nkeys"))
    if _wg is None:
        rc = L.fseq_debug_chain_launch(*head, *tail)
    else:
        stats = np.zeros(CW_STATS, dtype=np.uint32)
        if _hand is None:
            rc = L.fseq_debug_chain_launch_wg(*head, _wg[0], _wg[1], *tail, stats.ctypes.data)
        else:
            hand_keys = np.full((nb_total, m), _hand, dtype=np.uint16)
            hand_flag = np.zeros(nb_total, dtype=np.uint32)
            rc = L.fseq_debug_chain_launch_wg_keys(*head, _wg[0], _wg[1], *tail, stats.ctypes.data, hand_keys.ctypes.data, hand_flag.ctypes.data)
    if rc != FSEQ_OK:
        raise FseqError(rc, L.fseq_strerror(rc).decode())
    if _wg is not None:
        out["stats"] = stats
        if _hand is not None:
            out["hand_keys"], out["hand_flag"] = hand_keys, hand_flag
    return out


CW_STATS = 23          # csrc/fseq_types.hpp: by runs, by sort, from the identity, the most runs, 19 words of the run counts' histogram


def chain_launch_wg(rank, keyd, nkeys, G, cols_per_block, first_chain=0, chains=None, start_a=None, start_d=None, states=True, keys=False, device=0,
                    run_cap=CW_RUN_CAP, workgroups=1):
    """The launch of chain_launch with a chain per workgroup (k_chain_wg): `workgroups` workgroups take the chains by a fixed stride;
    a step goes from the identity, by runs of equal key (at most run_cap of them) or by the sort of its rows.  Returns chain_launch's
    dict plus "stats", the kernel's CW_STATS counters."""
    return chain_launch(rank, keyd, nkeys, G, cols_per_block, first_chain=first_chain, chains=chains, start_a=start_a, start_d=start_d, states=states,
                        keys=keys, device=device, _wg=(run_cap, workgroups))


HAND_FILL = 0xA5C3     # what chain_launch_wg_keys fills the hand-over array with in front of the launch


def chain_launch_wg_keys(rank, keyd, nkeys, G, cols_per_block, first_chain=0, chains=None, start_a=None, start_d=None, states=True, keys=False, device=0,
                         run_cap=CW_RUN_CAP, workgroups=1, fill=HAND_FILL):
    """chain_launch_wg with the hand-over to pass 2 (fseq_debug_chain_launch_wg_keys): the dict also holds "hand_keys" [nb_total][m]
    (16 bits, every word `fill` in front of the launch) and "hand_flag" [nb_total].  Where a flag is set, the block's row of hand_keys
    is rank[b] in the order in front of block b.  Takes m from 65 on."""
    return chain_launch(rank, keyd, nkeys, G, cols_per_block, first_chain=first_chain, chains=chains, start_a=start_a, start_d=start_d, states=states,
                        keys=keys, device=device, _wg=(run_cap, workgroups), _hand=fill)


RED_NONE = 0xFFFFFFFF                       # csrc/fseq_redplan.hpp: a block that is not reduced
RED_FORCE_FULL, RED_FORCE_WIDE = 1, 2       # ... the force marks
RED_USE, RED_DECLINED, RED_NO_BLOCK_LIST = 0, 1, 2      # ... RedVerdict
RED_CONFIGS_MAX = 64                        # include/fseq_debug.h, FSEQ_DEBUG_RED_CONFIGS


def red_cls_direct_host(m, B, bits, cls_ld, config, resident_rows, resident_cls):
    """The direct-or-gather rule of configuration `config` of the reduced column kernel (red_cls_direct, csrc/fseq_redplan.hpp) at
    this geometry, given the workgroups per CU the device reports with either staged-column buffer: (lds_rows, lds_cls, direct).
    No device is touched."""
    a, b, d = C.c_uint64(), C.c_uint64(), C.c_int()
    rc = load_library().fseq_debug_red_cls_direct(m, B, bits, cls_ld, config, resident_rows, resident_cls, C.byref(a), C.byref(b), C.byref(d))
    if rc != FSEQ_OK:
        raise FseqError(rc, "red_cls_direct_host")
    return a.value, b.value, bool(d.value)


def red_plan_host(m, B, bits, direct, cnt, force=None, b_lo=0, b_hi=None, reduced_always=False, no_block_list=False):
    """The plan of phase C on representative rows (plan_reduced, csrc/fseq_redplan.hpp) for the counts cnt[nblocks] (RED_NONE: not
    reduced) and the force marks force[nblocks], as a run of m rows in blocks of B columns at `bits` bits a symbol would make it
    (direct: LDS-resident rows).  No device is touched.  Returns a dict: verdict, full / config_of / config_snap_of [nblocks],
    blocks (the list that goes to the device), bins [(configuration, first, count)], full_at, nfull, listed, max_rows,
    reduced_blocks, rows_mean, and configs, the library's configurations as [(rows, values, T, E, ew, fits)].
    FseqError(FSEQ_E_ARG) where an argument could take an index out of bounds."""
    L = load_library()
    cnt = np.ascontiguousarray(cnt, dtype=np.uint32)
    if cnt.ndim != 1:
        raise FseqError(FSEQ_E_ARG, "red_plan_host: cnt is one count per block")
    nb = len(cnt)
    if force is not None:
        force = np.ascontiguousarray(force, dtype=np.uint8)
        if force.shape != cnt.shape:
            raise FseqError(FSEQ_E_ARG, "red_plan_host: one force mark per block")
    configs = np.zeros((RED_CONFIGS_MAX, 6), dtype=np.uint32)
    full = np.zeros(nb, dtype=np.uint8)
    config_of = np.zeros(nb, dtype=np.int32)
    config_snap_of = np.zeros(nb, dtype=np.int32)
    blocks = np.zeros(3 * nb, dtype=np.uint32)
    bins = np.zeros((RED_CONFIGS_MAX, 3), dtype=np.uint32)
    summary = np.zeros(6, dtype=np.uint32)
    n_configs, n_blocks, n_bins, verdict = C.c_uint32(), C.c_uint32(), C.c_uint32(), C.c_int()
    rc = L.fseq_debug_red_plan(m, B, bits, int(bool(direct)), nb, b_lo, nb if b_hi is None else b_hi, cnt.ctypes.data,
                               None if force is None else force.ctypes.data, int(bool(reduced_always)), int(bool(no_block_list)),
                               configs.ctypes.data, C.addressof(n_configs), C.addressof(verdict), full.ctypes.data, config_of.ctypes.data,
                               config_snap_of.ctypes.data, blocks.ctypes.data, C.addressof(n_blocks), bins.ctypes.data, C.addressof(n_bins),
                               summary.ctypes.data)
    if rc != FSEQ_OK:
        raise FseqError(rc, L.fseq_strerror(rc).decode())
    out = dict(zip(("full_at", "nfull", "listed", "max_rows", "reduced_blocks", "rows_mean"), (int(x) for x in summary)))
    out.update(verdict=verdict.value, full=full, config_of=config_of, config_snap_of=config_snap_of, blocks=blocks[:n_blocks.value],
               bins=[tuple(int(x) for x in row) for row in bins[:n_bins.value]],
               configs=[(int(r), int(v), int(T), int(E), bool(ew), bool(fits)) for r, v, T, E, ew, fits in configs[:n_configs.value]])
    return out


def scan_plan_host(n, lengths):
    """The order of work of a scan over segment lengths (plan_length_scan, csrc/fseq_scanplan.hpp) for n columns: (long_lengths,
    slot, n_short) -- the distinct lengths of the long path (n >= 2L) ascending, for every given length its place among them
    or -1 (the short path), and how many take the short path.  No device is touched."""
    L = load_library()
    lengths = np.ascontiguousarray(lengths, dtype=np.uint64)
    if lengths.ndim != 1:
        raise FseqError(FSEQ_E_ARG, "scan_plan_host: one length per entry")
    long_lengths = np.zeros(max(1, len(lengths)), dtype=np.uint64)
    slot = np.zeros(max(1, len(lengths)), dtype=np.int32)
    n_long, n_short = C.c_uint32(), C.c_uint32()
    rc = L.fseq_debug_scan_plan(int(n), lengths.ctypes.data, len(lengths), long_lengths.ctypes.data, C.byref(n_long), slot.ctypes.data, C.byref(n_short))
    if rc != FSEQ_OK:
        raise FseqError(rc, L.fseq_strerror(rc).decode())
    return long_lengths[:n_long.value].copy(), slot[:len(lengths)].copy(), n_short.value


CHAIN_FIT_ANY = 0xFFFFFFFFFFFFFFFF      # chain_plan_host: a workspace that holds any number of workgroups


def _chain_launches(launches, n):
    return [tuple(int(getattr(launches[i], f)) for f in ("level", "kind", "chains", "blocks", "first_chain", "workgroups")) for i in range(n)]


def _chain_plan_dict(p):
    out = {f: int(getattr(p, f)) for f in ("fan", "fan_round5", "turns", "shard_k", "shard_q", "blocks_per_rank", "n_hyper", "b_lo", "b_hi")}
    out["level_items"] = [int(p.level_items[i]) for i in range(p.n_levels)]
    out["launches"] = _chain_launches(p.launches, p.n_launches)
    return out


def chain_plan_host(m, nblocks, cus, streamed=None, chain_wg=0, chain_fan=0, fit=CHAIN_FIT_ANY, resident=1):
    """The plan of phase B on one GPU (csrc/fseq_chainplan.hpp, fseq_debug_chain_plan) for m rows in nblocks blocks on a device of
    `cus` CUs; streamed: whether the rows take the streamed kernels (None: more than 11,264 rows); chain_wg / chain_fan: the knobs
    FSEQ_CHAIN_WG / FSEQ_CHAIN_FAN; fit, resident: the cap on the workgroups of a launch on k_chain_wg.  No device is touched.
    Returns a dict: fan, fan_round5, turns, level_items, launches [(level, kind, chains, blocks, first_chain, workgroups)]."""
    L = load_library()
    p = ChainPlan()
    rc = L.fseq_debug_chain_plan(m, int(m > 11264 if streamed is None else bool(streamed)), nblocks, cus, chain_wg, chain_fan, fit, resident, C.byref(p))
    if rc != FSEQ_OK:
        raise FseqError(rc, L.fseq_strerror(rc).decode())
    return _chain_plan_dict(p)


def chain_plan_sharded_host(nblocks, world, rank, cus, chain_fan=0, streamed=True, chain_wg=0, fit=CHAIN_FIT_ANY, resident=1):
    """The plan of a sharded rank's phase B (fseq_debug_chain_plan_sharded): chain_plan_host's dict with shard_k, shard_q,
    blocks_per_rank, n_hyper and the rank's blocks [b_lo, b_hi); level_items are the rank's items of the levels 0 .. shard_k."""
    L = load_library()
    p = ChainPlan()
    rc = L.fseq_debug_chain_plan_sharded(nblocks, world, rank, chain_fan, int(bool(streamed)), cus, chain_wg, fit, resident, C.byref(p))
    if rc != FSEQ_OK:
        raise FseqError(rc, L.fseq_strerror(rc).decode())
    return _chain_plan_dict(p)


def row_split_plan_host(m, bits, held):
    """The plan of a split along the rows (row_split_plan, csrc/fseq_rowsplit_plan.hpp) for m rows at `bits` bits a code with the
    rows of `held` set aside: (kept, base, keep, n_slow) -- the rows that stay, ascending, and one descriptor per 32-bit word of a
    kept column (include/fseq_debug.h, fseq_debug_row_split_plan); n_slow words have keep = 0.  FseqError(FSEQ_E_ARG) for a list
    without_rows() refuses.  No device is touched."""
    L = load_library()
    held = np.ascontiguousarray(held, dtype=np.uint32)
    if held.ndim != 1:
        raise FseqError(FSEQ_E_ARG, "row_split_plan_host: one row index per entry")
    m, bits = int(m), int(bits)
    n_kept = max(m - len(held), 0)
    n_words = (n_kept + 32 // bits - 1) // (32 // bits) if bits in (2, 4, 8) else 0
    kept = np.zeros(max(1, n_kept), dtype=np.uint32)
    base = np.zeros(max(1, n_words), dtype=np.uint32)
    keep = np.zeros(max(1, n_words), dtype=np.uint32)
    nw, ns = C.c_uint32(), C.c_uint32()
    rc = L.fseq_debug_row_split_plan(m, bits, held.ctypes.data if len(held) else None, len(held), kept.ctypes.data, base.ctypes.data, keep.ctypes.data,
                                     C.byref(nw), C.byref(ns))
    if rc != FSEQ_OK:
        raise FseqError(rc, L.fseq_strerror(rc).decode())
    return kept[:n_kept].copy(), base[:nw.value].copy(), keep[:nw.value].copy(), ns.value


def restored_bounds_host(kept, n_src, lb, rb):
    """The merged segments [lb[s], rb[s]) of an identity-reduced context, given in its kept columns, in the source's co-ordinates
    (restored_segment_bounds, csrc/fseq_restored_bounds.hpp): (src_lb, src_rb), uint64 arrays.  kept: the source column of every
    kept column; n_src: the source's columns.  FseqError(FSEQ_E_ARG) where kept does not ascend strictly or names a column not
    below n_src, where the segments do not tile the kept columns, and for no segments.  No device is touched."""
    L = load_library()
    kept = np.ascontiguousarray(kept, dtype=np.uint64)
    lb = np.ascontiguousarray(lb, dtype=np.uint64)
    rb = np.ascontiguousarray(rb, dtype=np.uint64)
    if kept.ndim != 1 or lb.ndim != 1 or rb.shape != lb.shape:
        raise FseqError(FSEQ_E_ARG, "restored_bounds_host: one column per entry of kept, one segment per entry of lb and rb")
    S = len(lb)
    src_lb = np.zeros(max(1, S), dtype=np.uint64)
    src_rb = np.zeros(max(1, S), dtype=np.uint64)
    ptr = lambda a: a.ctypes.data if len(a) else None
    rc = L.fseq_debug_restored_bounds(ptr(kept), len(kept), int(n_src), ptr(lb), ptr(rb), S, src_lb.ctypes.data, src_rb.ctypes.data)
    if rc != FSEQ_OK:
        raise FseqError(rc, L.fseq_strerror(rc).decode())
    return src_lb[:S].copy(), src_rb[:S].copy()


def graph_nearest_plan_host(lb, rb, count, bits, budget_bytes=GRAPH_NEAREST_BATCH_BYTES):
    """How graph_nearest_rows() lays out its packed class representatives and cuts the segments into batches (graph_nearest_words
    and graph_nearest_plan, csrc/fseq_graphnearest_plan.hpp, through fseq_debug_graph_nearest_plan; no device): segments
    [lb[s], rb[s]) of count[s] classes at `bits` bits a code.  Returns (words, first): words[s] the representatives' words in
    front of segment s (S + 1 entries), batch b the segments [first[b], first[b + 1])."""
    L = load_library()
    lb = np.ascontiguousarray(lb, dtype=np.uint64)
    rb = np.ascontiguousarray(rb, dtype=np.uint64)
    count = np.ascontiguousarray(count, dtype=np.uint32)
    if lb.ndim != 1 or rb.shape != lb.shape or count.shape != lb.shape:
        raise FseqError(FSEQ_E_ARG, "graph_nearest_plan_host: one entry of lb, rb and count per segment")
    S = len(lb)
    words = np.zeros(S + 1, dtype=np.uint64)
    first = np.zeros(S + 1, dtype=np.uint64)
    nb = C.c_uint64()
    ptr = lambda a: a.ctypes.data if len(a) else None
    rc = L.fseq_debug_graph_nearest_plan(ptr(lb), ptr(rb), ptr(count), S, int(bits), int(budget_bytes), words.ctypes.data, first.ctypes.data, C.byref(nb))
    if rc != FSEQ_OK:
        raise FseqError(rc, L.fseq_strerror(rc).decode())
    return words, first[:nb.value + 1].copy()


def debug_graph_nearest(codes, bits, seg_lb, seg_rb, count, rep, query_codes, qbits, sigma, batch_bytes=None, device=0, want_info=False):
    """The pack and distance kernels of graph_nearest_rows() through the production launcher on caller-supplied tables
    (fseq_debug_graph_nearest; needs no context): codes [m][n] the alignment's codes, packed here at `bits` with pack_columns;
    segments [seg_lb[s], seg_rb[s]) with count[s] classes whose representative rows are rep[s][:count[s]] (rep is [S][X]);
    query_codes [Q][n] packed at qbits; sigma: the alphabet's size (a query code at or above it is a byte outside the alphabet).
    Returns (nodes as CLASS indices, distances, ties), each [S][Q] (with want_info, also fseq_debug_graph_nearest_info's dict).
    FseqError(FSEQ_E_ARG), before a device is touched, for whatever a kernel could form an index from: rep >= m, count > X or 0,
    bounds outside n or out of order, bits / qbits not in {2, 4, 8}, qbits < bits, a code at or above 2^bits or sigma, a query
    code at or above 2^qbits."""
    L = load_library()
    codes = np.ascontiguousarray(codes)
    query_codes = np.ascontiguousarray(query_codes)
    seg_lb = np.ascontiguousarray(seg_lb, dtype=np.uint64)
    seg_rb = np.ascontiguousarray(seg_rb, dtype=np.uint64)
    count = np.ascontiguousarray(count, dtype=np.uint32)
    rep = np.ascontiguousarray(rep, dtype=np.uint32)
    if bits not in (2, 4, 8) or qbits not in (2, 4, 8) or qbits < bits:
        raise FseqError(FSEQ_E_ARG, "debug_graph_nearest: bits and qbits are 2, 4 or 8, and qbits is not below bits")
    if codes.ndim != 2 or query_codes.ndim != 2 or 0 in codes.shape or query_codes.shape[0] == 0 or query_codes.shape[1] != codes.shape[1]:
        raise FseqError(FSEQ_E_ARG, "debug_graph_nearest: codes is [m][n], query_codes [Q][n]")
    if seg_lb.ndim != 1 or len(seg_lb) == 0 or seg_rb.shape != seg_lb.shape or count.shape != seg_lb.shape or rep.ndim != 2 or rep.shape[0] != len(seg_lb) or rep.shape[1] == 0:
        raise FseqError(FSEQ_E_ARG, "debug_graph_nearest: seg_lb, seg_rb and count have S entries, rep is [S][X]")
    if int(codes.max()) >= min(1 << bits, max(int(sigma), 1)) or int(codes.min()) < 0 or int(query_codes.max()) >= (1 << qbits) or int(query_codes.min()) < 0:
        raise FseqError(FSEQ_E_ARG, "debug_graph_nearest: a code at or above 2^bits (or sigma), or a query code at or above 2^qbits")
    (m, n), Q, (S, X) = codes.shape, query_codes.shape[0], rep.shape
    cols, ld = pack_columns(codes.astype(np.uint8), bits)
    qcols, qld = pack_columns(query_codes.astype(np.uint8), qbits)
    out = np.zeros((3, S, Q), dtype=np.uint32)
    info = GraphNearestInfo()
    rc = L.fseq_debug_graph_nearest(int(device), cols.ctypes.data, ld, m, n, bits, seg_lb.ctypes.data, seg_rb.ctypes.data, count.ctypes.data, rep.ctypes.data,
                                    S, X, qcols.ctypes.data, qld, Q, qbits, int(sigma), int(batch_bytes or 0), out[0].ctypes.data, out[1].ctypes.data,
                                    out[2].ctypes.data, C.byref(info))
    if rc != FSEQ_OK:
        raise FseqError(rc, L.fseq_strerror(rc).decode())
    if want_info:
        return out[0], out[1], out[2], {k: getattr(info, k) for k, _ in GraphNearestInfo._fields_ if k != "reserved"}
    return out[0], out[1], out[2]


def input_kept_range_host(kept, c0, ncols):
    """(k0, k1): the entries of the ascending list kept with c0 <= kept[k] < c0 + ncols (input_kept_range,
    csrc/fseq_input_kept_range.hpp, through fseq_debug_input_kept_range; no device)."""
    L = load_library()
    kept = np.ascontiguousarray(kept, dtype=np.uint64)
    k0, k1 = C.c_uint64(), C.c_uint64()
    rc = L.fseq_debug_input_kept_range(kept.ctypes.data if len(kept) else None, len(kept), int(c0), int(ncols), C.byref(k0), C.byref(k1))
    if rc != FSEQ_OK:
        raise FseqError(rc, L.fseq_strerror(rc).decode())
    return k0.value, k1.value


def relump_lists(ent, hdr, k0, L_from, L_to, device=0):
    """One launch of k_relump_lists on constructed lists: ent [ncols][stride][2] {value, count}, hdr [ncols][4] {entries, count of
    value 0, complete, cumulative count}, the lists of the columns k0 .. k0 + ncols - 1 at segment length L_from.  Returns
    (ent, hdr) folded to L_to.  FseqError(FSEQ_E_ARG), before a device is touched, where an input could take the kernel out of
    bounds."""
    L = load_library()
    ent = np.array(ent, dtype=np.uint32, order="C")
    hdr = np.array(hdr, dtype=np.uint32, order="C")
    if ent.ndim != 3 or ent.shape[2] != 2 or hdr.shape != (ent.shape[0], 4):
        raise FseqError(FSEQ_E_ARG, "relump_lists: ent is [ncols][stride][2], hdr [ncols][4]")
    rc = L.fseq_debug_relump_lists(device, int(k0), ent.shape[0], ent.shape[1], int(L_from), int(L_to), ent.ctypes.data, hdr.ctypes.data)
    if rc != FSEQ_OK:
        raise FseqError(rc, L.fseq_strerror(rc).decode())
    return ent, hdr


def _dp_lists(ent, hdr):
    ent = np.ascontiguousarray(ent, dtype=np.uint32)
    hdr = np.ascontiguousarray(hdr, dtype=np.uint32)
    if ent.ndim != 3 or ent.shape[2] != 2 or hdr.shape != (ent.shape[0], 4):
        raise FseqError(FSEQ_E_ARG, "DP lists: ent is [n][stride][2], hdr [n][4]")
    return ent, hdr


def local_pass_packed(d, s, device=0):
    """The packed local pass of phase C's partition step on one workgroup (fseq_debug_local_pass): d, s [threads][E] values below
    2^16 and symbols 0 .. 4 (4: an unused position, value 0), threads a multiple of 64 up to 1024, E one of 11, 12, 15.  Returns
    (dnew [threads][E], tails [threads][4]) as uint32."""
    L = load_library()
    d = np.ascontiguousarray(d, dtype=np.uint32)
    s = np.ascontiguousarray(s, dtype=np.uint32)
    if d.ndim != 2 or d.shape != s.shape:
        raise ValueError("d and s: [threads][rows per thread]")
    dnew = np.zeros(d.shape, dtype=np.uint32)
    tails = np.zeros((d.shape[0], 4), dtype=np.uint32)
    rc = L.fseq_debug_local_pass(int(device), d.shape[0], d.shape[1], d.ctypes.data, s.ctypes.data, dnew.ctypes.data, tails.ctypes.data)
    if rc != FSEQ_OK:
        raise FseqError(rc, L.fseq_strerror(rc).decode())
    return dnew, tails


def dp_lists_check(m, segment_length, ent, hdr):
    """The host's check of lists for SegmentationContext.debug_dp_on_lists (fseq_debug_dp_lists_check; no device): ent
    [n][stride][2] {value, count}, hdr [n][4] {entries, count of value 0, complete, cumulative count}.  Returns None where the DP
    may read them, else (column, rule) of the first list that breaks a rule (column -1: rule 0, the shapes)."""
    L = load_library()
    ent, hdr = _dp_lists(ent, hdr)
    bad, rule = C.c_uint64(), C.c_uint32()
    rc = L.fseq_debug_dp_lists_check(int(m), ent.shape[0], int(segment_length), ent.shape[1], ent.ctypes.data, hdr.ctypes.data, C.byref(bad), C.byref(rule))
    if rc == FSEQ_OK:
        return None
    if rc != FSEQ_E_ARG:
        raise FseqError(rc, L.fseq_strerror(rc).decode())
    return (-1 if bad.value == 2 ** 64 - 1 else bad.value), rule.value


def _dp_arrays(n, segment_length, lb, max_size, size):
    out = [np.ascontiguousarray(a, dtype=np.uint32) for a in (lb, max_size, size)]
    if int(segment_length) < 1 or any(a.shape != (int(n) - int(segment_length) + 1,) for a in out):
        raise FseqError(FSEQ_E_ARG, "DP arrays: lb, max_size and size have n - L + 1 words each")
    return out


def traceback_parts(n, segment_length, lb, max_size, size, part_lo, foreign=None, device=0):
    """The traceback of caller-supplied DP arrays followed part by part, as a sharded run in window mode follows it rank by rank
    (fseq_debug_traceback_parts; one process, no context): part g holds the entries [part_lo[g], part_lo[g + 1]), the last one up
    to n - L + 1, and sees `foreign` (or 0xFFFFFFFF) in every other entry of lb.  Returns (traceback as DPARG_DTYPE, first segment
    first; entries of the chain per part; windows per part).  FseqError(FSEQ_E_ARG), before a device is touched, for part borders
    out of order and for a chain from entry n - L that does not descend to lb == 0 (the message names the entry)."""
    L = load_library()
    lb, max_size, size = _dp_arrays(n, segment_length, lb, max_size, size)
    part_lo = np.ascontiguousarray(part_lo, dtype=np.uint32)
    if foreign is not None:
        foreign = np.ascontiguousarray(foreign, dtype=np.uint32)
        if foreign.shape != lb.shape:
            raise FseqError(FSEQ_E_ARG, "traceback by parts: foreign has n - L + 1 words")
    tb = np.zeros(int(n) // int(segment_length) + 2, dtype=DPARG_DTYPE)
    ents = np.zeros(max(1, len(part_lo)), dtype=np.uint32)
    wins = np.zeros(max(1, len(part_lo)), dtype=np.uint32)
    count, bad = C.c_uint64(), C.c_uint64()
    rc = L.fseq_debug_traceback_parts(device, int(n), int(segment_length), lb.ctypes.data, max_size.ctypes.data, size.ctypes.data,
                                      part_lo.ctypes.data if len(part_lo) else None, len(part_lo), None if foreign is None else foreign.ctypes.data,
                                      tb.ctypes.data, C.byref(count), ents.ctypes.data, wins.ctypes.data, C.byref(bad))
    if rc != FSEQ_OK:
        what = L.fseq_strerror(rc).decode()
        if bad.value != 2 ** 64 - 1:
            what += ": chain entry %d" % bad.value
        raise FseqError(rc, what)
    return tb[:count.value].copy(), ents[:len(part_lo)], wins[:len(part_lo)]


class RowShard(C.Structure):
    _fields_ = [("device", C.c_int32), ("rank", C.c_uint32), ("world", C.c_uint32), ("m", C.c_uint32), ("sigma", C.c_uint32),
                ("bits", C.c_uint32), ("ncols", C.c_uint64), ("d_cols", C.c_void_p), ("ld", C.c_size_t), ("xbuf", C.c_void_p),
                ("xbuf_words", C.c_uint64), ("fn", ALLREDUCE_FN), ("user", C.c_void_p)]


def pack_columns(msa_codes, bits):
    """Row-major codes (m x n, values < 2**bits) -> column-major packed bytes (n x ld, ld a multiple of 16): the layout
    fseq_set_device_columns_packed and fseq_rowshard_pbwt read (row r of a column in byte r * bits / 8)."""
    m, n = msa_codes.shape
    per = 8 // bits
    ld = ((m + per - 1) // per + 15) // 16 * 16
    cols = np.zeros((n, ld * per), dtype=np.uint8)
    cols[:, :m] = msa_codes.T
    out = np.zeros((n, ld), dtype=np.uint8)
    for j in range(per):
        out |= (cols[:, j::per] << (bits * j)).astype(np.uint8)
    return out, ld


def rowshard_xbuf_words(m, bits, world):
    return int(load_library().fseq_rowshard_xbuf_words(m, bits, world))


def rowshard_rows(m, bits, rank, world):
    lo, hi = C.c_uint32(), C.c_uint32()
    rc = load_library().fseq_rowshard_rows(m, bits, rank, world, C.byref(lo), C.byref(hi))
    if rc != FSEQ_OK:
        raise FseqError(rc, load_library().fseq_strerror(rc).decode())
    return lo.value, hi.value


def rowshard_pbwt(d_cols_ptr, ld, m, sigma, bits, ncols, rank, world, xbuf_ptr, xbuf_words, allreduce=None, device=0):
    """fseq_rowshard_pbwt (the north-star row split, include/fseq.h): returns (a, d, pos_lo, pos_hi, ms, exchanges);
    a / d are m long with this rank's positions [pos_lo, pos_hi) filled in.  allreduce(offset, count, op) -> 0."""
    L = load_library()

    def _cb(_user, off, cnt, op):
        try:
            return int(allreduce(int(off), int(cnt), int(op)) or 0)
        except Exception:                           # an exception must not unwind through the C frame
            import traceback
            traceback.print_exc()
            return 1
    cb = ALLREDUCE_FN(_cb) if allreduce is not None else ALLREDUCE_FN()
    args = RowShard(device, rank, world, m, sigma, bits, ncols, d_cols_ptr, ld, xbuf_ptr, xbuf_words, cb, None)
    a = np.zeros(m, dtype=np.uint32)
    d = np.zeros(m, dtype=np.uint32)
    lo, hi, ms, nex = C.c_uint32(), C.c_uint32(), C.c_double(), C.c_uint64()
    rc = L.fseq_rowshard_pbwt(C.byref(args), a.ctypes.data, d.ctypes.data, C.byref(lo), C.byref(hi), C.byref(ms), C.byref(nex))
    if rc != FSEQ_OK:
        raise FseqError(rc, L.fseq_strerror(rc).decode())
    return a, d, lo.value, hi.value, ms.value, nex.value


def dp_schedule(segment_length, n, col_hi):
    """(rounds, cells per round, leading rounds that only need columns < col_hi, pipelined) of the DP schedule."""
    L = load_library()
    a, b, c_, d = C.c_uint32(), C.c_uint32(), C.c_uint32(), C.c_int()
    rc = L.fseq_debug_dp_schedule(segment_length, n, col_hi, C.byref(a), C.byref(b), C.byref(c_), C.byref(d))
    if rc != FSEQ_OK:
        raise FseqError(rc, L.fseq_strerror(rc).decode())
    return a.value, b.value, c_.value, bool(d.value)


def run_batch(contexts):
    """fseq_run_segmentation_batch: all contexts in flight together (one native host thread and stream each).
    Returns the list of per-context return codes; every context's .result is filled in."""
    L = load_library()
    n = len(contexts)
    handles = (C.c_void_p * n)(*[c.h for c in contexts])
    results = (Result * n)()
    rcs = (C.c_int * n)()
    rc = L.fseq_run_segmentation_batch(handles, n, results, rcs)
    if rc != FSEQ_OK:
        raise FseqError(rc, L.fseq_strerror(rc).decode())
    for i, c in enumerate(contexts):
        r = Result()
        C.memmove(C.byref(r), C.byref(results[i]), C.sizeof(Result))
        c.result = r
    return list(rcs)


def bipartite_match_host(m, max_segment_size, lb, rb, a, d):
    """bipartite_matcher::match on caller-supplied boundary states (host only).  Returns (permutations,
    total matching weight between segments s and s+1)."""
    L = load_library()
    lb = np.ascontiguousarray(lb, dtype=np.uint64)
    rb = np.ascontiguousarray(rb, dtype=np.uint64)
    a = np.ascontiguousarray(a, dtype=np.uint32)
    d = np.ascontiguousarray(d, dtype=np.uint32)
    perm = np.zeros((len(lb), max_segment_size), dtype=np.uint32)
    weights = np.zeros(max(1, len(lb) - 1), dtype=np.int64)
    rc = L.fseq_bipartite_match_host(m, max_segment_size, len(lb), lb.ctypes.data, rb.ctypes.data, a.ctypes.data, d.ctypes.data,
                                     perm.ctypes.data, weights.ctypes.data)
    if rc != FSEQ_OK:
        raise FseqError(rc, L.fseq_strerror(rc).decode())
    return perm, weights[:len(lb) - 1]


def random_join_host(m, max_segment_size, lb, rb, a, d, seed):
    """join_context::join_random_order_and_output on caller-supplied boundary states (host only)."""
    L = load_library()
    lb = np.ascontiguousarray(lb, dtype=np.uint64)
    rb = np.ascontiguousarray(rb, dtype=np.uint64)
    a = np.ascontiguousarray(a, dtype=np.uint32)
    d = np.ascontiguousarray(d, dtype=np.uint32)
    perm = np.zeros((len(lb), max_segment_size), dtype=np.uint32)
    rc = L.fseq_random_join_host(m, max_segment_size, len(lb), lb.ctypes.data, rb.ctypes.data, a.ctypes.data, d.ctypes.data, seed, perm.ctypes.data)
    if rc != FSEQ_OK:
        raise FseqError(rc, L.fseq_strerror(rc).decode())
    return perm


def random_join_classes_host(m, max_segment_size, count, rep, size, seed):
    """The random joiner from the runs on, on caller-supplied class tables (host only): count[s] classes of segment s in pBWT
    order, rep / size [segments, max_segment_size] their first rows and row counts.  What join_random runs behind its device front."""
    L = load_library()
    count = np.ascontiguousarray(count, dtype=np.uint32)
    rep = np.ascontiguousarray(rep, dtype=np.uint32)
    size = np.ascontiguousarray(size, dtype=np.uint32)
    assert rep.shape == (len(count), max_segment_size) and size.shape == rep.shape
    perm = np.zeros((len(count), max_segment_size), dtype=np.uint32)
    rc = L.fseq_random_join_classes_host(m, max_segment_size, len(count), count.ctypes.data, rep.ctypes.data, size.ctypes.data, seed, perm.ctypes.data)
    if rc != FSEQ_OK:
        raise FseqError(rc, L.fseq_strerror(rc).decode())
    return perm


def _join_score_result(junctions, breaks, support, sm):
    return {"junctions": junctions, "breaks": breaks, "support": support, "summary": {k: getattr(sm, k) for k, _ in JoinScoreSummary._fields_}}


def join_score_host(m, max_segment_size, lb, rb, a, d, permutations, want_support=False):
    """The junction support of permutations [segments, max_segment_size] on caller-supplied boundary states (host only, no GPU
    needed; fseq_join_score_host): what SegmentationContext.join_score returns."""
    L = load_library()
    lb = np.ascontiguousarray(lb, dtype=np.uint64)
    rb = np.ascontiguousarray(rb, dtype=np.uint64)
    a = np.ascontiguousarray(a, dtype=np.uint32)
    d = np.ascontiguousarray(d, dtype=np.uint32)
    perm = np.ascontiguousarray(permutations, dtype=np.uint32)
    S = len(lb)
    if perm.shape != (S, max_segment_size) or a.size != S * m or d.size != S * m or len(rb) != S:
        raise FseqError(FSEQ_E_ARG, "join_score_host: shapes disagree")
    junctions = np.zeros(max(S - 1, 0), dtype=JOIN_SCORE_DTYPE)
    breaks = np.zeros(max_segment_size, dtype=np.uint32)
    support = np.zeros((max(S - 1, 0), max_segment_size), dtype=np.uint32) if want_support else None
    sm = JoinScoreSummary()
    rc = L.fseq_join_score_host(m, max_segment_size, S, lb.ctypes.data, rb.ctypes.data, a.ctypes.data, d.ctypes.data, perm.ctypes.data,
                                junctions.ctypes.data, breaks.ctypes.data, None if support is None else support.ctypes.data, C.byref(sm))
    if rc != FSEQ_OK:
        raise FseqError(rc, L.fseq_strerror(rc).decode())
    return _join_score_result(junctions, breaks, support, sm)


def debug_join_score(of, perm_cls_left, perm_cls_right, want_support=True, device=0):
    """k_join_score and k_join_score_founders on caller-built class arrays (fseq_debug_join_score): of [S][m] the class of every row
    in every segment, perm_cls_left / perm_cls_right [S - 1][X] the classes of every slot's two rows at every junction,
    JOIN_SCORE_GAP a gap.  Returns what join_score returns (rb is 0).  FseqError(FSEQ_E_ARG), before a device is touched, where an
    input could take a kernel out of bounds or form the empty key."""
    L = load_library()
    of = np.ascontiguousarray(np.atleast_2d(of), dtype=np.uint16)
    cl = np.ascontiguousarray(np.atleast_2d(perm_cls_left), dtype=np.uint16)
    cr = np.ascontiguousarray(np.atleast_2d(perm_cls_right), dtype=np.uint16)
    S, m = of.shape
    if cl.shape != cr.shape or cl.shape[0] != max(S - 1, 0):
        raise FseqError(FSEQ_E_ARG, "debug_join_score: shapes disagree")
    X = cl.shape[1]
    junctions = np.zeros(max(S - 1, 0), dtype=JOIN_SCORE_DTYPE)
    breaks = np.zeros(X, dtype=np.uint32)
    support = np.zeros(cl.shape, dtype=np.uint32) if want_support else None
    sm = JoinScoreSummary()
    rc = L.fseq_debug_join_score(device, m, X, S, of.ctypes.data, cl.ctypes.data, cr.ctypes.data, junctions.ctypes.data, breaks.ctypes.data,
                                 None if support is None else support.ctypes.data, C.byref(sm))
    if rc != FSEQ_OK:
        raise FseqError(rc, L.fseq_strerror(rc).decode())
    return _join_score_result(junctions, breaks, support, sm)


class SegmentationContext:
    """Mirror of segmentation_lp_context / segmentation_sp_context behind the C ABI.

    generate_traceback + update_samples_to_traceback_positions + find_segments_greedy
    (segmentation_lp_context.hh:119-121) are one call here: run().  The result fields mirror
    segmentation_container (reduced_traceback, reduced_pbwt_samples via boundary_state(),
    max_segment_size)."""

    def __init__(self, m, n, segment_length, pbwt_sample_rate=0, block_len=0, list_cap=0, device=0, list_memory=0):
        self.L = load_library()
        self.m, self.n, self.segment_length = int(m), int(n), int(segment_length)
        p = Params(self.m, self.n, self.segment_length, int(pbwt_sample_rate), int(block_len), int(list_cap), int(device))
        h = C.c_void_p()
        rc = self.L.fseq_create(C.byref(p), C.byref(h))
        if rc != FSEQ_OK:
            raise FseqError(rc, self.L.fseq_strerror(rc).decode())
        self.h = h
        self._device = int(device)
        self.result = None
        self._keep = None
        if list_memory:
            self.set_list_memory(list_memory)

    def close(self):
        if getattr(self, "h", None):
            self.L.fseq_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc):
        if rc == FSEQ_OK:
            return
        msg = self.L.fseq_last_error(self.h).decode() or self.L.fseq_strerror(rc).decode()
        if rc == FSEQ_E_NO_REDUCTION:
            raise NoReduction(rc, msg)
        raise FseqError(rc, msg)

    # ---- one alignment over several ranks (fseq_set_shard; the transport lives in founder-sequences_amd/dist.py)
    def set_shard(self, rank, world, xbuf_ptr, xbuf_words, allreduce):
        """allreduce(offset_words, count_words, op) -> 0: all-reduces that slice of the exchange buffer in place.
        Call before the input is set; every rank then holds its own columns only."""
        def _cb(_user, off, cnt, op):
            try:
                return int(allreduce(int(off), int(cnt), int(op)) or 0)
            except Exception:                      # never let an exception cross the C ABI
                import traceback
                traceback.print_exc()
                return 1
        self._shard_cb = ALLREDUCE_FN(_cb)         # keep the thunk alive as long as the context
        self._check(self.L.fseq_set_shard(self.h, rank, world, xbuf_ptr, xbuf_words, self._shard_cb, None))
        self.rank, self.world = rank, world

    def shard_abort(self, code=FSEQ_E_HIP):
        """This rank's host has failed and makes no further calls: the other ranks return FSEQ_E_PEER from their next exchange."""
        self._check(self.L.fseq_shard_abort(self.h, int(code)))

    def set_memory_budget(self, nbytes):
        """Device memory this context may hold in all (ranks that share a card); 0 = whatever is free."""
        self._check(self.L.fseq_set_memory_budget(self.h, int(nbytes)))

    def set_list_memory(self, nbytes):
        """Device memory the per-column lists of a long-path run may occupy (fseq_set_list_memory); 0 = every list held.
        Beyond it the run holds its lists in column windows, with the same results."""
        self._check(self.L.fseq_set_list_memory(self.h, int(nbytes)))

    def list_windows(self):
        """What the last run did with its lists: {bytes_held, columns_per_window, windows, merge_windows}
        (windows == 1: every list held)."""
        b, cols, w, mw = C.c_uint64(), C.c_uint64(), C.c_uint32(), C.c_uint32()
        self._check(self.L.fseq_debug_list_windows(self.h, C.byref(b), C.byref(cols), C.byref(w), C.byref(mw)))
        return {"bytes_held": b.value, "columns_per_window": cols.value, "windows": w.value, "merge_windows": mw.value}

    def set_progress(self, fn):
        """fn(stage, current_step, step_max) at the phase boundaries of run() (None: off); step_max() / current_step()
        may be polled from another thread."""
        self._progress = PROGRESS_FN(lambda _u, stage, cur, mx: fn(stage, cur, mx)) if fn else PROGRESS_FN()
        self._check(self.L.fseq_set_progress(self.h, self._progress, None))

    def step_max(self):
        return int(self.L.fseq_step_max(self.h))

    def current_step(self):
        return int(self.L.fseq_current_step(self.h))

    def shard_xbuf_words(self, world):
        return int(self.L.fseq_shard_xbuf_words(self.h, world))

    def shard_columns(self):
        a, b = C.c_uint64(), C.c_uint64()
        self._check(self.L.fseq_shard_columns(self.h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def shard_owner(self, rb):
        r = C.c_uint32()
        self._check(self.L.fseq_shard_owner(self.h, int(rb), C.byref(r)))
        return r.value

    # ---- input (delegate->sequences(), delegate->alphabet())
    def set_sequences(self, msa, staging_bytes=None):
        """msa: uint8 array [m, n] of raw symbol bytes, any memory order.  staging_bytes: None stages the whole alignment on the
        device (fseq_set_matrix); a number sends it in column chunks through that much device staging (fseq_set_rows_streamed,
        0 = 256 MiB), with the same results."""
        assert msa.dtype == np.uint8 and msa.shape == (self.m, self.n)
        if staging_bytes is None:
            self._check(self.L.fseq_set_matrix(self.h, msa.ctypes.data, msa.strides[0], msa.strides[1]))
            return
        if msa.strides[1] != 1:
            msa = np.ascontiguousarray(msa)
        rows = self._row_pointers(msa)
        self._check(self.L.fseq_set_rows_streamed(self.h, rows, int(staging_bytes)))

    # ---- the input in column chunks of bounded device memory (fseq_input_begin .. fseq_input_end)
    def _row_pointers(self, chunk):
        return (C.c_void_p * self.m)(*[chunk.ctypes.data + r * chunk.strides[0] for r in range(self.m)])

    def _chunk(self, chunk):
        chunk = np.asarray(chunk)
        assert chunk.dtype == np.uint8 and chunk.ndim == 2 and chunk.shape[0] == self.m
        return chunk if chunk.strides[1] == 1 or chunk.shape[1] <= 1 else np.ascontiguousarray(chunk)

    def input_begin(self, alphabet=None, staging_bytes=0):
        """Starts a chunked input.  alphabet: the byte values that may occur (bytes or an array; None: collect it with
        input_scan).  staging_bytes: device memory of the two staging halves together (0 = 256 MiB)."""
        if alphabet is None:
            self._check(self.L.fseq_input_begin(self.h, None, 0, int(staging_bytes)))
            return
        alpha = np.ascontiguousarray(np.frombuffer(bytes(alphabet), dtype=np.uint8) if isinstance(alphabet, (bytes, bytearray)) else np.asarray(alphabet, dtype=np.uint8))
        self._check(self.L.fseq_input_begin(self.h, alpha.ctypes.data, len(alpha), int(staging_bytes)))

    def input_chunk_columns(self):
        """The most columns one input_scan / input_columns call may carry (0 before input_begin)."""
        return int(self.L.fseq_input_chunk_columns(self.h))

    def input_scan(self, c0, chunk):
        """chunk: uint8 [m, w], the columns [c0, c0 + w) of every row; the chunk may be reused when the call returns."""
        chunk = self._chunk(chunk)
        self._check(self.L.fseq_input_scan(self.h, int(c0), chunk.shape[1], self._row_pointers(chunk)))

    def input_columns(self, c0, chunk):
        chunk = self._chunk(chunk)
        self._check(self.L.fseq_input_columns(self.h, int(c0), chunk.shape[1], self._row_pointers(chunk)))

    def input_end(self):
        self._check(self.L.fseq_input_end(self.h))

    # ---- ... with the identity columns dropped on the way (fseq_input_scan_identity .. fseq_input_end_kept)
    def input_scan_identity(self, c0, chunk):
        """input_scan's chunk, finding the identity columns besides the alphabet (also after a supplied alphabet)."""
        chunk = self._chunk(chunk)
        self._check(self.L.fseq_input_scan_identity(self.h, int(c0), chunk.shape[1], self._row_pointers(chunk)))

    def input_reduce(self, segment_length, block_len=0, list_cap=0):
        """After the identity scan has covered every column: makes the kept-column list and the context over the kept columns
        (handed out by input_end_kept).  Returns the summary {n, identity, kept, ms_device}."""
        p = Params(0, 0, int(segment_length), 0, int(block_len), int(list_cap), int(self._device))
        sm = IdentitySummary()
        self._check(self.L.fseq_input_reduce(self.h, C.byref(p), C.byref(sm)))
        self._reduce = (int(segment_length), {k: getattr(sm, k) for k, _ in IdentitySummary._fields_})
        return dict(self._reduce[1])

    def input_kept_columns(self, c0, ncols):
        """How many kept columns lie in [c0, c0 + ncols) (host only, after input_reduce)."""
        count = C.c_uint64()
        self._check(self.L.fseq_input_kept_columns(self.h, int(c0), int(ncols), C.byref(count)))
        return count.value

    def input_columns_kept(self, c0, chunk):
        """The second pass.  chunk: uint8 [m, w], or -- for a chunk without a kept column -- None or the width w alone."""
        if chunk is None or isinstance(chunk, (int, np.integer)):
            w = self.input_chunk_columns() if chunk is None else int(chunk)
            self._check(self.L.fseq_input_columns_kept(self.h, int(c0), min(w, self.n - int(c0)), None))
            return
        chunk = self._chunk(chunk)
        self._check(self.L.fseq_input_columns_kept(self.h, int(c0), chunk.shape[1], self._row_pointers(chunk)))

    def _reduced_context(self, h, segment_length, sm, list_memory=0):
        new = SegmentationContext.__new__(SegmentationContext)
        new.L, new.h = self.L, h
        new.m, new.n, new.segment_length, new._device = self.m, int(sm["kept"]), int(segment_length), self._device
        new.result, new._keep = None, None
        new.source_n = int(sm["n"])
        new.identity_summary = dict(sm)
        if list_memory:
            new.set_list_memory(list_memory)
        return new

    def input_end_kept(self, list_memory=0):
        """Ends the reduced input: the SegmentationContext over the kept columns, as without_identity_columns() returns it."""
        h = C.c_void_p()
        self._check(self.L.fseq_input_end_kept(self.h, C.byref(h)))
        return self._reduced_context(h, self._reduce[0], self._reduce[1], list_memory)

    def set_sequences_without_identity_columns(self, msa, segment_length, staging_bytes=0, block_len=0, list_cap=0, list_memory=0):
        """set_sequences(msa, staging_bytes) followed by without_identity_columns(segment_length, ...) in one call that never
        holds msa's packed form on the device (fseq_set_rows_streamed_without_identity_columns).  msa: uint8 [m, n], or a
        sequence of m uint8 rows of n bytes each (rows that are not one matrix).  Returns the new context."""
        if isinstance(msa, np.ndarray):
            assert msa.dtype == np.uint8 and msa.shape == (self.m, self.n)
            if msa.strides[1] != 1:
                msa = np.ascontiguousarray(msa)
            rows = self._row_pointers(msa)
        else:
            msa = [np.ascontiguousarray(r, dtype=np.uint8) for r in msa]
            assert len(msa) == self.m and all(r.shape == (self.n,) for r in msa)
            rows = (C.c_void_p * self.m)(*[r.ctypes.data for r in msa])
        p = Params(0, 0, int(segment_length), 0, int(block_len), int(list_cap), int(self._device))
        h = C.c_void_p()
        sm = IdentitySummary()
        self._check(self.L.fseq_set_rows_streamed_without_identity_columns(self.h, rows, int(staging_bytes), C.byref(p), C.byref(h), C.byref(sm)))
        return self._reduced_context(h, segment_length, {k: getattr(sm, k) for k, _ in IdentitySummary._fields_}, list_memory)

    def packed_columns(self, c0=0, c1=None):
        """(bytes [c1 - c0, ld], bits): the columns of the resident alignment as they are stored, padding included."""
        c1 = self.n if c1 is None else c1
        ld, bits = C.c_uint64(), C.c_uint32()
        self._check(self.L.fseq_debug_packed_columns(self.h, c0, c1, None, C.byref(ld), C.byref(bits)))
        out = np.zeros((c1 - c0, ld.value), dtype=np.uint8)
        self._check(self.L.fseq_debug_packed_columns(self.h, c0, c1, out.ctypes.data, C.byref(ld), C.byref(bits)))
        return out, bits.value

    def alphabet(self):
        """(sigma, bits, bytes): the codes of the resident input, their width and the byte each of them stands for, in code order."""
        sigma, bits = C.c_uint32(), C.c_uint32()
        table = np.zeros(256, dtype=np.uint8)
        self._check(self.L.fseq_debug_alphabet(self.h, C.byref(sigma), C.byref(bits), table.ctypes.data))
        return sigma.value, bits.value, table[:sigma.value].tobytes()

    def device_bytes(self, reset_peak=False):
        """(now, peak): device bytes this context's buffers hold and the most they have held (since the last reset_peak).
        Accounting of the context's own allocations, not a measurement of the device."""
        now, peak = C.c_uint64(), C.c_uint64()
        self._check(self.L.fseq_debug_device_bytes(self.h, C.byref(now), C.byref(peak), 1 if reset_peak else 0))
        return now.value, peak.value

    def set_device_columns(self, ptr, ld, sigma, keepalive=None):
        self._keep = keepalive
        self._check(self.L.fseq_set_device_columns(self.h, ptr, ld, sigma))

    def set_device_columns_packed(self, ptr, ld_bytes, sigma, bits, keepalive=None):
        self._keep = keepalive
        self._check(self.L.fseq_set_device_columns_packed(self.h, ptr, ld_bytes, sigma, bits))

    def generate_synthetic(self, seed, n_founders, block_len, mu, kind=0):
        s = SynthSpec(seed, n_founders, block_len, synth_threshold(mu), kind)
        self._check(self.L.fseq_generate_synthetic(self.h, C.byref(s)))

    def get_sequences(self, c0=0, c1=None):
        c1 = self.n if c1 is None else c1
        out = np.zeros((self.m, c1 - c0), dtype=np.uint8, order="F")
        self._check(self.L.fseq_get_matrix(self.h, c0, c1, out.ctypes.data, out.strides[0], out.strides[1]))
        return out

    # ---- the path
    def run(self):
        res = Result()
        rc = self.L.fseq_run_segmentation(self.h, C.byref(res))
        self.result = res
        self._check(rc)
        return res

    def set_segment_length(self, segment_length):
        """Another segment length bound on the resident alignment (fseq_set_segment_length): the result and the last match are
        dropped, the next run() gives what a fresh context with that length gives."""
        self._check(self.L.fseq_set_segment_length(self.h, int(segment_length)))
        self.segment_length = int(segment_length)
        self.result = None

    def scan_segment_lengths(self, lengths):
        """The maximum segment size at every given segment length (fseq_scan_segment_lengths): (entries, summary) -- a structured
        array (LENGTH_SCAN_DTYPE), one entry per given length in the given order, and the summary as a dict.  The context holds
        no result afterwards and keeps its own segment length."""
        entries = np.zeros(len(lengths), dtype=LENGTH_SCAN_DTYPE)
        entries["segment_length"] = np.asarray(lengths, dtype=np.uint64)
        sm = LengthScanSummary()
        self._check(self.L.fseq_scan_segment_lengths(self.h, entries.ctypes.data, len(entries), C.byref(sm)))
        self.result = None
        return entries, {k: getattr(sm, k) for k, _ in LengthScanSummary._fields_}

    @property
    def max_segment_size(self):
        return self.result.max_segment_size

    def traceback(self):
        out = np.zeros(self.result.dp_segment_count, dtype=DPARG_DTYPE)
        if len(out):
            self._check(self.L.fseq_get_traceback(self.h, out.ctypes.data))
        return out

    def reduced_traceback(self):
        out = np.zeros(self.result.segment_count, dtype=SEGMENT_DTYPE)
        if len(out):
            self._check(self.L.fseq_get_segments(self.h, out.ctypes.data))
        return out

    def boundary_state(self, i):
        """(input_permutation, input_divergence) of reduced_pbwt_samples[i]."""
        a = np.zeros(self.m, dtype=np.uint32)
        d = np.zeros(self.m, dtype=np.uint32)
        self._check(self.L.fseq_boundary_state(self.h, i, a.ctypes.data, d.ctypes.data))
        return a, d

    def short_path_runs(self):
        k = self.result.max_segment_size
        f = np.zeros(k, dtype=np.uint32)
        r = np.zeros(k, dtype=np.uint32)
        self._check(self.L.fseq_short_path_runs(self.h, f.ctypes.data, r.ctypes.data))
        return f, r

    # ---- joining (join_context / greedy_matcher, host side)
    def join_greedy(self):
        """permutations[s, r]: input row whose segment-s substring is founder r's content."""
        perm = np.zeros((self.result.segment_count, self.result.max_segment_size), dtype=np.uint32)
        self._check(self.L.fseq_join_greedy(self.h, perm.ctypes.data))
        return perm

    def join_bipartite(self):
        perm = np.zeros((self.result.segment_count, self.result.max_segment_size), dtype=np.uint32)
        self._check(self.L.fseq_join_bipartite(self.h, perm.ctypes.data))
        return perm

    def join_random(self, seed=0):
        perm = np.zeros((self.result.segment_count, self.result.max_segment_size), dtype=np.uint32)
        self._check(self.L.fseq_join_random(self.h, seed, perm.ctypes.data))
        return perm

    def write_segments(self, msa, joining, path):
        """--output-segments for the joining method (JOIN_GREEDY / JOIN_BIPARTITE / JOIN_RANDOM)."""
        assert msa.dtype == np.uint8 and msa.flags["C_CONTIGUOUS"] and msa.shape == (self.m, self.n)
        rows = (C.c_void_p * self.m)(*[msa.ctypes.data + r * msa.strides[0] for r in range(self.m)])
        self._check(self.L.fseq_write_segments(self.h, rows, joining, path.encode() if path else None))

    def write_segments_device(self, joining, path):
        """--output-segments from the alignment and the boundary states resident on the device (no host rows, no copy of the
        boundary states): the bytes write_segments writes when given the rows of the alignment the context holds."""
        self._check(self.L.fseq_write_segments_device(self.h, joining, path.encode() if path else None))

    def segments_file_stats(self):
        """The last file write_segments_device or write_segments_restored wrote: {batches, bytes, longest_line, lines} (header included, a line with its newline)."""
        v = [C.c_uint64() for _ in range(4)]
        self._check(self.L.fseq_debug_segments_file(self.h, *[C.byref(x) for x in v]))
        return dict(zip(("batches", "bytes", "longest_line", "lines"), (x.value for x in v)))

    def random_path(self):
        """Which way the last join_random() went: 0 the host joiner, 1 the class tables from the device."""
        path = C.c_int()
        self._check(self.L.fseq_debug_random_path(self.h, C.byref(path)))
        return path.value

    def join_score(self, permutations, want_support=False):
        """What a join is worth (fseq_join_score): for permutations [segments, max_segment_size] -- a joiner's or any other, an entry
        >= m a gap -- {"junctions": a structured array (JOIN_SCORE_DTYPE), one entry per adjacent segment pair; "breaks": per founder
        slot the junctions at which no input row carries its substrings on both sides; "support": [segments - 1, max_segment_size]
        with want_support, else None; "summary": a dict}."""
        S, X = self.result.segment_count, self.result.max_segment_size
        perm = np.ascontiguousarray(permutations, dtype=np.uint32)
        if perm.shape != (S, X):
            raise FseqError(FSEQ_E_ARG, "join_score: permutations are [segments, max_segment_size]")
        junctions = np.zeros(max(S - 1, 0), dtype=JOIN_SCORE_DTYPE)
        breaks = np.zeros(X, dtype=np.uint32)
        support = np.zeros((max(S - 1, 0), X), dtype=np.uint32) if want_support else None
        sm = JoinScoreSummary()
        self._check(self.L.fseq_join_score(self.h, perm.ctypes.data, junctions.ctypes.data, breaks.ctypes.data,
                                           None if support is None else support.ctypes.data, C.byref(sm)))
        return _join_score_result(junctions, breaks, support, sm)

    def join_score_path(self):
        """Which way the last join_score() went: 0 the host form, 1 the device form."""
        path = C.c_int()
        self._check(self.L.fseq_debug_join_score_path(self.h, C.byref(path)))
        return path.value

    def block_graph(self, want_row_nodes=False):
        """The founder block graph of the finished run (fseq_block_graph): {"nodes": a structured array (GRAPH_NODE_DTYPE), one
        entry per class of every merged segment, in id order; "edges": a structured array (GRAPH_EDGE_DTYPE), one entry per pair
        of classes of adjacent segments that some row carries, by junction, then (from, to) ascending; "row_nodes": [segments, m],
        the node of every row in every segment, with want_row_nodes, else None; "summary": a dict}."""
        sm = GraphSummary()
        self._check(self.L.fseq_block_graph(self.h, None, None, None, C.byref(sm)))
        nodes = np.zeros(sm.nodes, dtype=GRAPH_NODE_DTYPE)
        edges = np.zeros(sm.edges, dtype=GRAPH_EDGE_DTYPE)
        row_nodes = np.zeros((sm.segments, self.m), dtype=np.uint32) if want_row_nodes else None
        self._check(self.L.fseq_block_graph(self.h, nodes.ctypes.data, edges.ctypes.data, None if row_nodes is None else row_nodes.ctypes.data, C.byref(sm)))
        return {"nodes": nodes, "edges": edges, "row_nodes": row_nodes,
                "summary": {"segments": sm.segments, "nodes": sm.nodes, "edges": sm.edges, "ms_device": sm.ms_device}}

    def write_block_graph(self, path, paths=False, gap=b"-"):
        """The founder block graph as a GFA 1.0 file, written from the device (fseq_write_block_graph): S lines with the classes'
        substrings without the byte `gap` (None or b"": every byte stays), L lines with the rows two classes share, and with
        paths a P line per input row.  path None or "-": stdout."""
        if gap is not None and len(gap) > 1:
            raise FseqError(FSEQ_E_ARG, "write_block_graph: the gap is one byte, or None")
        self._check(self.L.fseq_write_block_graph(self.h, GRAPH_PATHS if paths else 0, gap[0] if gap else -1, path.encode() if path else None))

    def graph_file_stats(self):
        """The last file write_block_graph wrote, by section: {"nodes" / "links" / "paths": {batches, lines, bytes}} (a line with its
        newline; the header line, 11 bytes, is in no section)."""
        st = GraphFileStats()
        self._check(self.L.fseq_debug_graph_file(self.h, C.byref(st)))
        return {name: {"batches": st.batches[k], "lines": st.lines[k], "bytes": st.bytes[k]} for k, name in enumerate(("nodes", "links", "paths"))}

    # ---- rows that are not the graph's own threaded through it
    def _graph_thread(self, call, n_rows, want_nodes, want_steps):
        S = int(self.result.segment_count) if self.result is not None else 0
        nodes = np.zeros((S, n_rows), dtype=np.uint32) if want_nodes else None
        steps = np.zeros((max(S, 1) - 1, n_rows), dtype=np.uint32) if want_steps else None
        per_row = np.zeros(n_rows, dtype=GRAPH_THREAD_ROW_DTYPE)
        per_segment = np.zeros(S, dtype=GRAPH_THREAD_SEGMENT_DTYPE)
        sm = GraphThreadSummary()
        self._check(call(None if nodes is None else nodes.ctypes.data, None if steps is None else steps.ctypes.data, per_row.ctypes.data,
                         per_segment.ctypes.data if S else None, C.byref(sm)))
        return {"nodes": nodes, "steps": steps, "per_row": per_row, "per_segment": per_segment,
                "summary": {k: getattr(sm, k) for k, _ in GraphThreadSummary._fields_}}

    def graph_thread_rows(self, queries, want_nodes=True, want_steps=True):
        """Thread rows that are NOT the alignment's through the founder block graph of the finished run (fseq_graph_thread_rows):
        queries a C-contiguous uint8 array [n_rows, n] of raw bytes (or a list of bytes objects of length n).  Returns {"nodes":
        [segments, n_rows], the node (block_graph()'s ids) whose substring query q carries in segment s, or GRAPH_NONE; "steps":
        [segments - 1, n_rows], the index into block_graph()["edges"] of the edge between the two nodes of a junction, or
        GRAPH_NONE (both nodes there and no edge: a novel junction); "per_row" (GRAPH_THREAD_ROW_DTYPE); "per_segment"
        (GRAPH_THREAD_SEGMENT_DTYPE); "summary": a dict}.  Without want_nodes / want_steps only the statistics leave the device
        and the entry is None.  The run's results and the last match stay as they were."""
        a = queries
        if not isinstance(a, np.ndarray):
            a = np.array([np.frombuffer(bytes(f), dtype=np.uint8) for f in a], dtype=np.uint8).reshape(len(a), -1)
        a = np.ascontiguousarray(a, dtype=np.uint8)
        if a.ndim != 2 or (a.shape[0] and a.shape[1] != self.n):
            raise ValueError("graph_thread_rows: queries must be rows of n = %d bytes" % self.n)
        rows = (C.c_void_p * max(a.shape[0], 1))(*[a.ctypes.data + r * a.strides[0] for r in range(a.shape[0])])
        return self._graph_thread(lambda *out: self.L.fseq_graph_thread_rows(self.h, rows, a.shape[0], *out), a.shape[0], want_nodes, want_steps)

    def graph_thread_held_out(self, want_nodes=True, want_steps=True):
        """... the held-out rows of a context made by without_rows(), where they lie on the device (fseq_graph_thread_held_out):
        nothing is uploaded; query q is held_out()[1][q]."""
        return self._graph_thread(lambda *out: self.L.fseq_graph_thread_held_out(self.h, *out), int(getattr(self, "n_held", 0)), want_nodes, want_steps)

    def graph_thread_info(self):
        """How the last graph_thread_rows() / graph_thread_held_out() found its nodes (fseq_debug_graph_thread): dict(key_bits,
        table_slots, candidates_verified, candidates_rejected, queries_out_of_alphabet)."""
        info = GraphThreadInfo()
        self._check(self.L.fseq_debug_graph_thread(self.h, C.byref(info)))
        return {k: getattr(info, k) for k, _ in GraphThreadInfo._fields_}

    # ---- the nearest node of every segment, and how far it is
    def _graph_nearest(self, call, n_rows, want):
        S = int(self.result.segment_count) if self.result is not None else 0
        arrays = {k: (np.zeros((S if k != "steps" else max(S, 1) - 1, n_rows), dtype=np.uint32) if on else None) for k, on in want}
        per_row = np.zeros(n_rows, dtype=GRAPH_NEAREST_ROW_DTYPE)
        per_segment = np.zeros(S, dtype=GRAPH_NEAREST_SEGMENT_DTYPE)
        sm = GraphNearestSummary()
        self._check(call(*[None if arrays[k] is None else arrays[k].ctypes.data for k, _ in want], per_row.ctypes.data,
                         per_segment.ctypes.data if S else None, C.byref(sm)))
        arrays.update({"per_row": per_row, "per_segment": per_segment, "summary": {k: getattr(sm, k) for k, _ in GraphNearestSummary._fields_}})
        return arrays

    def graph_nearest_rows(self, queries, max_distance=0, want_nodes=True, want_distances=True, want_ties=True, want_steps=True):
        """For rows that are NOT the alignment's, the NEAREST node of every segment of the founder block graph and how far it is
        (fseq_graph_nearest_rows): queries as graph_thread_rows() takes them.  Returns {"nodes": [segments, n_rows], the node
        (block_graph()'s ids) of segment s with the fewest columns in which its representative row's code differs from query
        q's, the smallest class among equals; "distances": that number; "ties": the classes of the segment that attain it;
        "steps": [segments - 1, n_rows], the index into block_graph()["edges"] of the edge between the two nodes of a junction
        where both distances are at most max_distance and the edge exists, else GRAPH_NONE; "per_row"
        (GRAPH_NEAREST_ROW_DTYPE); "per_segment" (GRAPH_NEAREST_SEGMENT_DTYPE); "summary": a dict}.  An array that is not wanted
        stays on the device and its entry is None.  With max_distance = 0, nodes where the distance is 0, steps and the walk
        statistics are graph_thread_rows()'.  The run's results, the last match and graph_thread_info() stay as they were.  Not
        for identity-reduced or sharded contexts; there is no host form."""
        a = queries
        if not isinstance(a, np.ndarray):
            a = np.array([np.frombuffer(bytes(f), dtype=np.uint8) for f in a], dtype=np.uint8).reshape(len(a), -1)
        a = np.ascontiguousarray(a, dtype=np.uint8)
        if a.ndim != 2 or (a.shape[0] and a.shape[1] != self.n):
            raise ValueError("graph_nearest_rows: queries must be rows of n = %d bytes" % self.n)
        rows = (C.c_void_p * max(a.shape[0], 1))(*[a.ctypes.data + r * a.strides[0] for r in range(a.shape[0])])
        want = (("nodes", want_nodes), ("distances", want_distances), ("ties", want_ties), ("steps", want_steps))
        return self._graph_nearest(lambda *out: self.L.fseq_graph_nearest_rows(self.h, rows, a.shape[0], int(max_distance), *out), a.shape[0], want)

    def graph_nearest_held_out(self, max_distance=0, want_nodes=True, want_distances=True, want_ties=True, want_steps=True):
        """... the held-out rows of a context made by without_rows(), where they lie on the device (fseq_graph_nearest_held_out):
        nothing is uploaded; query q is held_out()[1][q]."""
        want = (("nodes", want_nodes), ("distances", want_distances), ("ties", want_ties), ("steps", want_steps))
        return self._graph_nearest(lambda *out: self.L.fseq_graph_nearest_held_out(self.h, int(max_distance), *out), int(getattr(self, "n_held", 0)), want)

    def graph_nearest_info(self):
        """How the last graph_nearest_rows() / graph_nearest_held_out() packed its words (fseq_debug_graph_nearest_info):
        dict(batches, packed_words, query_words, bits)."""
        info = GraphNearestInfo()
        self._check(self.L.fseq_debug_graph_nearest_info(self.h, C.byref(info)))
        return {k: getattr(info, k) for k, _ in GraphNearestInfo._fields_ if k != "reserved"}

    def write_founders_device(self, permutations, path):
        """--output-founders from the alignment resident on the device (no host rows)."""
        perm = np.ascontiguousarray(permutations, dtype=np.uint32)
        self._check(self.L.fseq_write_founders_device(self.h, perm.ctypes.data, path.encode() if path else None))

    def write_founders(self, msa, permutations, path):
        """msa: the raw input rows as a C-contiguous uint8 array [m, n]."""
        assert msa.dtype == np.uint8 and msa.flags["C_CONTIGUOUS"] and msa.shape == (self.m, self.n)
        rows = (C.c_void_p * self.m)(*[msa.ctypes.data + r * msa.strides[0] for r in range(self.m)])
        perm = np.ascontiguousarray(permutations, dtype=np.uint32)
        self._check(self.L.fseq_write_founders(self.h, rows, perm.ctypes.data, path.encode() if path else None))

    # ---- the founders checked against the input (match-sequences-to-founders, on the device)
    def match_founders(self, permutations=None, founders=None, min_segment_length=0):
        """Thread every input row through the founders greedily (fseq_match_founders / fseq_match_founder_rows).
        permutations: those of a join on this context (the founders write_founders_device would write); or founders: a
        C-contiguous uint8 array [K, n] of raw bytes (or a list of K bytes objects of length n).  Returns the summary as a
        dict; match_pieces() has the pieces."""
        if (permutations is None) == (founders is None):
            raise ValueError("match_founders: give either permutations or founders")
        sm = MatchSummary()
        if permutations is not None:
            perm = np.ascontiguousarray(permutations, dtype=np.uint32)
            self._check(self.L.fseq_match_founders(self.h, perm.ctypes.data, int(min_segment_length), C.byref(sm)))
        else:
            if not isinstance(founders, np.ndarray):
                founders = np.array([np.frombuffer(bytes(f), dtype=np.uint8) for f in founders], dtype=np.uint8).reshape(len(founders), -1)
            founders = np.ascontiguousarray(founders, dtype=np.uint8)
            if founders.ndim != 2 or founders.shape[1] != self.n:
                raise ValueError("match_founders: founders must be K rows of n = %d bytes" % self.n)
            K = founders.shape[0]
            rows = (C.c_void_p * max(K, 1))(*[founders.ctypes.data + r * founders.strides[0] for r in range(K)])
            self._check(self.L.fseq_match_founder_rows(self.h, rows, K, int(min_segment_length), C.byref(sm)))
        self._match = sm
        return {k: getattr(sm, k) for k, _ in MatchSummary._fields_}

    def match_rows(self, queries, permutations=None, founders=None, min_segment_length=0):
        """Thread rows that are NOT the alignment's through the founders (fseq_match_rows): queries a C-contiguous uint8 array
        [n_rows, n] of raw bytes (or a list of bytes objects of length n); permutations or founders as match_founders takes
        them.  Returns the summary dict; the `row` of match_pieces() is the query index; match_split() tells how the walk
        was split along the columns."""
        if (permutations is None) == (founders is None):
            raise ValueError("match_rows: give either permutations or founders")

        def as_rows(a, what):
            if not isinstance(a, np.ndarray):
                a = np.array([np.frombuffer(bytes(f), dtype=np.uint8) for f in a], dtype=np.uint8).reshape(len(a), -1)
            a = np.ascontiguousarray(a, dtype=np.uint8)
            if a.ndim != 2 or a.shape[1] != self.n:
                raise ValueError("match_rows: %s must be rows of n = %d bytes" % (what, self.n))
            return a, (C.c_void_p * max(a.shape[0], 1))(*[a.ctypes.data + r * a.strides[0] for r in range(a.shape[0])])

        q, qrows = as_rows(queries, "queries")
        sm = MatchSummary()
        if permutations is not None:
            perm = np.ascontiguousarray(permutations, dtype=np.uint32)
            self._check(self.L.fseq_match_rows(self.h, perm.ctypes.data, None, 0, qrows, q.shape[0], int(min_segment_length), C.byref(sm)))
        else:
            f, frows = as_rows(founders, "founders")
            self._check(self.L.fseq_match_rows(self.h, None, frows, f.shape[0], qrows, q.shape[0], int(min_segment_length), C.byref(sm)))
        self._match = sm
        return {k: getattr(sm, k) for k, _ in MatchSummary._fields_}

    def match_split(self):
        """How the last match walked (fseq_debug_match_split): dict(segments, overlap, row_groups, flagged_groups,
        rows_not_standing).  After a restored match the segments and the overlap count kept columns."""
        info = MatchSplitInfo()
        self._check(self.L.fseq_debug_match_split(self.h, C.byref(info)))
        return {k: getattr(info, k) for k, _ in MatchSplitInfo._fields_ if k != "reserved"}

    def match_pieces(self):
        """(pieces, sets) of the last match: pieces as MATCH_PIECE_DTYPE records ordered by row, then lb; sets[i] the founder
        set of piece i as set_words uint32 words (founder f at bit f % 32 of word f // 32)."""
        sm = getattr(self, "_match", None)
        n_pieces, words = (sm.pieces, sm.set_words) if sm is not None else (0, 1)
        pieces = np.zeros(n_pieces, dtype=MATCH_PIECE_DTYPE)
        sets = np.zeros((n_pieces, words), dtype=np.uint32)
        self._check(self.L.fseq_get_match(self.h, pieces.ctypes.data, sets.ctypes.data))
        return pieces, sets

    def write_match(self, path):
        """The report of match-sequences-to-founders for the last match (SEQUENCE_INDEX LB RB FOUNDER_INDICES)."""
        self._check(self.L.fseq_write_match(self.h, path.encode() if path else None))

    # ---- rows held out of the resident alignment and matched on the device
    def without_rows(self, held_rows, segment_length, block_len=0, list_cap=0, list_memory=0):
        """A new SegmentationContext over the rows that are not in held_rows (fseq_create_without_rows): the kept rows in this
        context's order, numbered 0 .. kept - 1, and the held-out rows aside on the device for match_held_out().  held_rows:
        distinct row indices, any order.  This context may be closed afterwards, or serve the next fold."""
        held = np.ascontiguousarray(held_rows, dtype=np.uint32).reshape(-1)
        p = Params(0, 0, int(segment_length), 0, int(block_len), int(list_cap), int(self._device))
        h = C.c_void_p()
        sm = HoldOutSummary()
        self._check(self.L.fseq_create_without_rows(self.h, held.ctypes.data if len(held) else None, len(held), C.byref(p), C.byref(h), C.byref(sm)))
        new = SegmentationContext.__new__(SegmentationContext)
        new.L, new.h = self.L, h
        new.m, new.n, new.segment_length, new._device = int(sm.kept), self.n, int(segment_length), self._device
        new.result, new._keep = None, None
        new.source_m = int(sm.m_src)
        new.n_held = int(sm.held)
        new.held_out_summary = {k: getattr(sm, k) for k, _ in HoldOutSummary._fields_ if k != "reserved"}
        if list_memory:
            new.set_list_memory(list_memory)
        return new

    def held_out(self):
        """On a context made by without_rows(): (kept_rows, held_rows) -- the source row of every row of this context, ascending,
        and the held-out rows in the order they were given (the `row` of match_held_out()'s pieces indexes this list)."""
        kept = np.zeros(self.m, dtype=np.uint32)
        held = np.zeros(max(1, getattr(self, "n_held", 0)), dtype=np.uint32)
        self._check(self.L.fseq_get_held_out(self.h, kept.ctypes.data, held.ctypes.data))
        return kept, held[:getattr(self, "n_held", 0)]

    def held_out_columns(self, c0=0, c1=None):
        """... (bytes [c1 - c0, ld_h], bits): the held-out rows as they are stored, padding included (packed_columns()' twin)."""
        c1 = self.n if c1 is None else c1
        ld, bits = C.c_uint64(), C.c_uint32()
        self._check(self.L.fseq_debug_held_out_columns(self.h, c0, c1, None, C.byref(ld), C.byref(bits)))
        out = np.zeros((c1 - c0, ld.value), dtype=np.uint8)
        self._check(self.L.fseq_debug_held_out_columns(self.h, c0, c1, out.ctypes.data, C.byref(ld), C.byref(bits)))
        return out, bits.value

    def match_held_out(self, permutations=None, founders=None, min_segment_length=0):
        """... the held-out rows threaded through the founders (fseq_match_held_out): permutations or founders as match_rows
        takes them; nothing is uploaded.  Returns the summary dict; match_pieces(), write_match() and match_split() serve the
        result."""
        if (permutations is None) == (founders is None):
            raise ValueError("match_held_out: give either permutations or founders")
        sm = MatchSummary()
        if permutations is not None:
            perm = np.ascontiguousarray(permutations, dtype=np.uint32)
            self._check(self.L.fseq_match_held_out(self.h, perm.ctypes.data, None, 0, int(min_segment_length), C.byref(sm)))
        else:
            if not isinstance(founders, np.ndarray):
                founders = np.array([np.frombuffer(bytes(f), dtype=np.uint8) for f in founders], dtype=np.uint8).reshape(len(founders), -1)
            f = np.ascontiguousarray(founders, dtype=np.uint8)
            if f.ndim != 2 or f.shape[1] != self.n:
                raise ValueError("match_held_out: founders must be K rows of n = %d bytes" % self.n)
            frows = (C.c_void_p * max(f.shape[0], 1))(*[f.ctypes.data + r * f.strides[0] for r in range(f.shape[0])])
            self._check(self.L.fseq_match_held_out(self.h, None, frows, f.shape[0], int(min_segment_length), C.byref(sm)))
        self._match = sm
        return {k: getattr(sm, k) for k, _ in MatchSummary._fields_}

    # ---- identity columns (remove-identity-columns / insert-identity-columns, on the device)
    def identity_columns(self):
        """(mask, summary): mask[k] is True iff all rows carry the same symbol in column k (fseq_identity_columns);
        summary = {n, identity, kept, ms_device}.  Needs the alignment only, no run."""
        mask = np.zeros(self.n, dtype=np.uint8)
        sm = IdentitySummary()
        self._check(self.L.fseq_identity_columns(self.h, mask.ctypes.data, C.byref(sm)))
        return mask.astype(bool), {k: getattr(sm, k) for k, _ in IdentitySummary._fields_}

    def without_identity_columns(self, segment_length, block_len=0, list_cap=0, list_memory=0, keep_held_out=False):
        """A new SegmentationContext over the columns that are not identity columns (fseq_create_without_identity_columns);
        its results are in reduced co-ordinates (kept_columns() maps them back).  This context may be closed afterwards.
        keep_held_out: on a context made by without_rows(), carry its held-out rows along
        (fseq_create_without_identity_columns_held): held_out() and match_held_out() (reduced co-ordinates) answer on the new
        context, and match_held_out_restored() matches the full-length held-out rows against the restored founders."""
        p = Params(0, 0, int(segment_length), 0, int(block_len), int(list_cap), int(self._device))
        h = C.c_void_p()
        sm = IdentitySummary()
        create = self.L.fseq_create_without_identity_columns_held if keep_held_out else self.L.fseq_create_without_identity_columns
        self._check(create(self.h, C.byref(p), C.byref(h), C.byref(sm)))
        new = SegmentationContext.__new__(SegmentationContext)
        new.L, new.h = self.L, h
        new.m, new.n, new.segment_length, new._device = self.m, int(sm.kept), int(segment_length), self._device
        new.result, new._keep = None, None
        new.source_n = int(sm.n)
        if keep_held_out:
            new.source_m, new.n_held = self.source_m, self.n_held
        new.identity_summary = {k: getattr(sm, k) for k, _ in IdentitySummary._fields_}
        if list_memory:
            new.set_list_memory(list_memory)
        return new

    def identity_mask(self):
        """On a context made by without_identity_columns(): the mask over the source's columns."""
        mask = np.zeros(getattr(self, "source_n", 0), dtype=np.uint8)
        self._check(self.L.fseq_get_identity_columns(self.h, mask.ctypes.data, None))
        return mask.astype(bool)

    def kept_columns(self):
        """... the source column of every column of this context (ascending)."""
        kept = np.zeros(self.n, dtype=np.uint64)
        self._check(self.L.fseq_get_identity_columns(self.h, None, kept.ctypes.data))
        return kept

    def write_identity_columns(self, path):
        """... the stdout of remove-identity-columns: '0' / '1' per source column, then a newline."""
        self._check(self.L.fseq_write_identity_columns(self.h, path.encode() if path else None))

    def write_founders_restored(self, permutations, path):
        """... --output-founders with the identity columns put back from input row 0 (lines of the source's length)."""
        perm = np.ascontiguousarray(permutations, dtype=np.uint32)
        self._check(self.L.fseq_write_founders_restored(self.h, perm.ctypes.data, path.encode() if path else None))

    def segments_restored(self):
        """... reduced_traceback() with lb / rb in the source's co-ordinates (fseq_get_segments_restored): segment s covers the
        source columns from its first kept column up to the next segment's first kept column, the first from 0, the last to the
        source's n."""
        S = self.result.segment_count if self.result is not None else 0      # (before a run: the library refuses)
        out = np.zeros(max(1, S), dtype=SEGMENT_DTYPE)
        self._check(self.L.fseq_get_segments_restored(self.h, out.ctypes.data))
        return out[:S]

    def write_segments_restored(self, joining, path):
        """... --output-segments in the source's co-ordinates (fseq_write_segments_restored): write_segments_device's file with
        the bounds of segments_restored() and substrings of the source's length, input row 0's byte at the identity columns.
        segments_file_stats() then reports this file."""
        self._check(self.L.fseq_write_segments_restored(self.h, joining, path.encode() if path else None))

    def match_founders_restored(self, permutations, min_segment_length=0):
        """... the source's full-length rows matched against the founders write_founders_restored would write
        (fseq_match_founders_restored): the summary dict of match_founders, pieces in the source's co-ordinates;
        match_pieces() and write_match() then serve this result.  Unsplit unless FSEQ_MATCH_SPLIT is set (set_tuning); the
        segments and FSEQ_MATCH_OVERLAP then count kept columns, and match_split() tells how the walk went."""
        perm = np.ascontiguousarray(permutations, dtype=np.uint32)
        sm = MatchSummary()
        self._check(self.L.fseq_match_founders_restored(self.h, perm.ctypes.data, int(min_segment_length), C.byref(sm)))
        self._match = sm
        return {k: getattr(sm, k) for k, _ in MatchSummary._fields_}

    # ---- query rows against the restored founders (leave-rows-out validation with the identity columns removed)
    def match_held_out_restored(self, permutations, min_segment_length=0):
        """On a context made by without_identity_columns(keep_held_out=True): the full-length held-out rows matched against the
        founders write_founders_restored would write (fseq_match_held_out_restored).  The summary dict of match_founders; the
        pieces are in the source's co-ordinates, their `row` indexes held_out()[1]; match_pieces(), write_match() and
        match_exceptions() serve the result.  The walk is split along the kept columns, by itself as match_rows' is along the
        columns (one segment under 32,768 kept columns) or as FSEQ_MATCH_SPLIT / FSEQ_MATCH_OVERLAP say, both in kept columns;
        the result is the unsplit walk's either way, and match_split() tells how the walk went."""
        perm = np.ascontiguousarray(permutations, dtype=np.uint32)
        sm = MatchSummary()
        self._check(self.L.fseq_match_held_out_restored(self.h, perm.ctypes.data, int(min_segment_length), C.byref(sm)))
        self._match, self._match_rows = sm, self.n_held
        return {k: getattr(sm, k) for k, _ in MatchSummary._fields_}

    def match_rows_restored(self, queries, permutations, min_segment_length=0):
        """On a context made by without_identity_columns(): queries, a C-contiguous uint8 array [n_rows, source_n] of raw
        bytes (or a list of bytes objects of that length), matched against the restored founders (fseq_match_rows_restored).
        Split along the kept columns as match_held_out_restored is."""
        q = queries
        if not isinstance(q, np.ndarray):
            q = np.array([np.frombuffer(bytes(f), dtype=np.uint8) for f in q], dtype=np.uint8).reshape(len(q), -1)
        q = np.ascontiguousarray(q, dtype=np.uint8)
        if q.ndim != 2 or q.shape[1] != getattr(self, "source_n", -1):
            raise ValueError("match_rows_restored: queries must be rows of the source's n = %d bytes" % getattr(self, "source_n", -1))
        qrows = (C.c_void_p * max(q.shape[0], 1))(*[q.ctypes.data + r * q.strides[0] for r in range(q.shape[0])])
        perm = np.ascontiguousarray(permutations, dtype=np.uint32)
        sm = MatchSummary()
        self._check(self.L.fseq_match_rows_restored(self.h, perm.ctypes.data, qrows, q.shape[0], int(min_segment_length), C.byref(sm)))
        self._match, self._match_rows = sm, q.shape[0]
        return {k: getattr(sm, k) for k, _ in MatchSummary._fields_}

    def match_exceptions(self):
        """(offsets, columns) of the last restored match of query rows (fseq_get_match_exceptions): row r differs from row 0
        of the reconstruction in the identity columns columns[offsets[r]:offsets[r + 1]] (source positions, ascending)."""
        total = C.c_uint64()
        self._check(self.L.fseq_get_match_exceptions(self.h, None, None, C.byref(total)))
        offsets = np.zeros(int(getattr(self, "_match_rows", 0)) + 1, dtype=np.uint64)
        columns = np.zeros(total.value, dtype=np.uint32)
        self._check(self.L.fseq_get_match_exceptions(self.h, offsets.ctypes.data, columns.ctypes.data, None))
        return offsets, columns

    # ---- the block graph in the source's co-ordinates
    def write_block_graph_restored(self, path, paths=False, gap=b"-"):
        """On a context made by without_identity_columns() (or set_sequences_without_identity_columns()): write_block_graph's
        file with every S line in the source's co-ordinates (fseq_write_block_graph_restored) -- the label runs over the
        segment's source range of segments_restored(), input row 0's byte at the identity columns, lb / rb are that range.  The
        L and P lines are write_block_graph's; the labels of a P line spell the source's row.  graph_file_stats() then
        reports this file."""
        if gap is not None and len(gap) > 1:
            raise FseqError(FSEQ_E_ARG, "write_block_graph_restored: the gap is one byte, or None")
        self._check(self.L.fseq_write_block_graph_restored(self.h, GRAPH_PATHS if paths else 0, gap[0] if gap else -1, path.encode() if path else None))

    def graph_thread_rows_restored(self, queries, want_nodes=True, want_steps=True):
        """... graph_thread_rows with queries of the source's length, a C-contiguous uint8 array [n_rows, source_n] (or a list
        of bytes objects of that length) (fseq_graph_thread_rows_restored): a query carries a node iff it equals it on the
        segment's kept columns and differs from input row 0 in no identity column of the segment's source range.  Returns what
        graph_thread_rows returns; the column counts are the source's.  The last match and its match_exceptions() stay."""
        a = queries
        if not isinstance(a, np.ndarray):
            a = np.array([np.frombuffer(bytes(f), dtype=np.uint8) for f in a], dtype=np.uint8).reshape(len(a), -1)
        a = np.ascontiguousarray(a, dtype=np.uint8)
        if a.ndim != 2 or (a.shape[0] and a.shape[1] != getattr(self, "source_n", -1)):
            raise ValueError("graph_thread_rows_restored: queries must be rows of the source's n = %d bytes" % getattr(self, "source_n", -1))
        rows = (C.c_void_p * max(a.shape[0], 1))(*[a.ctypes.data + r * a.strides[0] for r in range(a.shape[0])])
        return self._graph_thread(lambda *out: self.L.fseq_graph_thread_rows_restored(self.h, rows, a.shape[0], *out), a.shape[0], want_nodes, want_steps)

    def graph_thread_held_out_restored(self, want_nodes=True, want_steps=True):
        """... the full-length held-out rows of a context made by without_identity_columns(keep_held_out=True), where they lie on
        the device with the exception cells the context was made with (fseq_graph_thread_held_out_restored)."""
        return self._graph_thread(lambda *out: self.L.fseq_graph_thread_held_out_restored(self.h, *out), int(getattr(self, "n_held", 0)), want_nodes, want_steps)

    # ---- debug / parity of intermediate state
    def debug_dp(self):
        k = self.n - self.segment_length + 1
        lb = np.zeros(k, dtype=np.uint32)
        mx = np.zeros(k, dtype=np.uint32)
        sz = np.zeros(k, dtype=np.uint32)
        self._check(self.L.fseq_debug_dp(self.h, lb.ctypes.data, mx.ctypes.data, sz.ctypes.data))
        return lb, mx, sz

    def debug_dp_owned(self):
        """(first, last, owns_final_cell, whole_arrays): the DP entries this rank computed (everything when not sharded)."""
        a, b = C.c_uint64(), C.c_uint64()
        f, w = C.c_int(), C.c_int()
        self._check(self.L.fseq_debug_dp_owned(self.h, C.byref(a), C.byref(b), C.byref(f), C.byref(w)))
        return a.value, b.value, bool(f.value), bool(w.value)

    def debug_clock(self):
        """(GHz, workgroups) of phase C's kernel in the last run -- diagnostic builds (-DFSEQ_CLOCK_STAMPS) only."""
        g, n = C.c_double(), C.c_uint32()
        self._check(self.L.fseq_debug_clock(self.h, C.byref(g), C.byref(n)))
        return g.value, n.value

    def debug_block_state(self, b):
        a = np.zeros(self.m, dtype=np.uint32)
        d = np.zeros(self.m, dtype=np.uint32)
        self._check(self.L.fseq_debug_block_state(self.h, b, a.ctypes.data, d.ctypes.data))
        return a, d

    def debug_column_list(self, col):
        cap = self.m + 2
        v = np.zeros(cap, dtype=np.uint32)
        c = np.zeros(cap, dtype=np.uint32)
        ne, c0, comp = C.c_uint32(), C.c_uint32(), C.c_uint32()
        self._check(self.L.fseq_debug_column_list(self.h, col, v.ctypes.data, c.ctypes.data,
                                                  C.byref(ne), C.byref(c0), C.byref(comp)))
        return v[:ne.value].copy(), c[:ne.value].copy(), c0.value, bool(comp.value)

    def debug_dp_on_lists(self, list_cap, ent, hdr, cuts=()):
        """Phase D alone on constructed lists through the production launchers (fseq_debug_dp_on_lists): ent [n][stride][2] with
        stride = (list_cap + 3) & ~1, hdr [n][4].  cuts empty: the DP as a run chooses it (the speculative sweeps; the serial
        kernel under FSEQ_DP_SERIAL); else resumed launches of the serial kernel cut at those rounds.  Returns (lb, max_size,
        size, info) with info = {unproven, dp_chunks, dp_sweeps, launches}; the context holds no result afterwards."""
        ent, hdr = _dp_lists(ent, hdr)
        if ent.shape[0] != self.n or ent.shape[1] != ((int(list_cap) + 3) & ~1):
            raise FseqError(FSEQ_E_ARG, "DP on lists: ent is [n][(list_cap + 3) & ~1][2]")
        cuts = np.ascontiguousarray(cuts, dtype=np.uint32)
        k = self.n - self.segment_length + 1
        lb, mx, sz = (np.zeros(k, dtype=np.uint32) for _ in range(3))
        info = DpListsInfo()
        self.result = None
        self._check(self.L.fseq_debug_dp_on_lists(self.h, int(list_cap), ent.ctypes.data, hdr.ctypes.data, cuts.ctypes.data if len(cuts) else None,
                                                  len(cuts), lb.ctypes.data, mx.ctypes.data, sz.ctypes.data, C.byref(info)))
        return lb, mx, sz, {k_: getattr(info, k_) for k_, _ in DpListsInfo._fields_}

    def debug_merge_on_lists(self, list_cap, ent, hdr, lb, max_size, size, separate=False, col_splits=()):
        """The traceback and the greedy merge alone on constructed DP arrays and lists, through the functions a run calls
        (fseq_debug_merge_on_lists): ent / hdr as for debug_dp_on_lists, lb / max_size / size n - L + 1 words each.  separate: the
        thresholds come from launches of their own instead of riding with the traceback, they and the merged sizes once per column
        range cut at col_splits and summed on the host.  Returns (traceback, tau, segments, info): DPARG_DTYPE, [count][2] {tau,
        kind} in the traceback's order (empty where none were taken), SEGMENT_DTYPE, {overflow, tau_separate, threshold_launches,
        count_launches}; the context holds no result afterwards."""
        ent, hdr = _dp_lists(ent, hdr)
        if ent.shape[0] != self.n or ent.shape[1] != ((int(list_cap) + 3) & ~1):
            raise FseqError(FSEQ_E_ARG, "merge on lists: ent is [n][(list_cap + 3) & ~1][2]")
        lb, max_size, size = _dp_arrays(self.n, self.segment_length, lb, max_size, size)
        splits = np.ascontiguousarray(col_splits, dtype=np.uint64)
        room = self.n // self.segment_length + 2
        tb = np.zeros(room, dtype=DPARG_DTYPE)
        tau = np.zeros((room, 2), dtype=np.uint32)
        seg = np.zeros(room, dtype=SEGMENT_DTYPE)
        n_tb, n_tau, n_seg = C.c_uint64(), C.c_uint64(), C.c_uint64()
        info = MergeListsInfo()
        self.result = None
        self._check(self.L.fseq_debug_merge_on_lists(self.h, int(list_cap), ent.ctypes.data, hdr.ctypes.data, lb.ctypes.data, max_size.ctypes.data,
                                                     size.ctypes.data, 1 if separate else 0, splits.ctypes.data if len(splits) else None, len(splits),
                                                     tb.ctypes.data, C.byref(n_tb), tau.ctypes.data, C.byref(n_tau), seg.ctypes.data, C.byref(n_seg),
                                                     C.byref(info)))
        return (tb[:n_tb.value].copy(), tau[:n_tau.value].copy(), seg[:n_seg.value].copy(),
                {k_: getattr(info, k_) for k_, _ in MergeListsInfo._fields_})

    def set_tuning(self, name, value="1"):
        """One of the library's FSEQ_* diagnostic knobs for this context (value None = off); the environment is only
        read when a context is created."""
        self._check(self.L.fseq_debug_set_tuning(self.h, name.encode(), None if value is None else str(value).encode()))

    def join_profile(self):
        """Host time of the last join_*() call: {ms_d2h, ms_classes, ms_edges, ms_draw, ms_total, bytes_d2h}."""
        jp = JoinProfile()
        self._check(self.L.fseq_get_join_profile(self.h, C.byref(jp)))
        return {k: getattr(jp, k) for k, _ in JoinProfile._fields_}

    def join_path(self):
        """Which way the last join_greedy() went: 0 the all-host joiner, 1 the LDS device front, 2 the wide device front."""
        path = C.c_int()
        self._check(self.L.fseq_debug_join_path(self.h, C.byref(path)))
        return path.value

    def bipartite_path(self):
        """Which way the last join_bipartite() went: 0 the host joiner, 1 the LDS device form, 2 the wide device form."""
        path = C.c_int()
        self._check(self.L.fseq_debug_bipartite_path(self.h, C.byref(path)))
        return path.value

    def pass2_paths(self):
        """The last run's boundaries through pass 2's streamed chain step: {by_runs, by_sort, copies, max_runs, runs_hist} (all
        zero where the run did not go through that kernel); runs_hist[b]: boundaries of more than 2^(b - 1) and at most 2^b runs."""
        v = [C.c_uint32() for _ in range(4)]
        hist = np.zeros(19, dtype=np.uint32)
        self._check(self.L.fseq_debug_pass2_paths(self.h, *[C.byref(x) for x in v], hist.ctypes.data))
        out = dict(zip(("by_runs", "by_sort", "copies", "max_runs"), (x.value for x in v)))
        out["runs_hist"] = [int(x) for x in hist]
        return out

    def class_tables(self, columns):
        """Pass 2's sweeps of the last run (on representatives) at the given ascending columns, each strictly inside a block:
        (cls, headd, ncls) -- cls[i][r] the class of row r at columns[i], headd[i][:ncls[i]] the divergence in front of every class
        (0xFFFFFFFF behind them)."""
        cols = np.ascontiguousarray(columns, dtype=np.uint64)
        cls = np.empty((len(cols), self.m), dtype=np.uint32)
        headd = np.empty((len(cols), self.m), dtype=np.uint32)
        ncls = np.empty(len(cols), dtype=np.uint32)
        self._check(self.L.fseq_debug_class_tables(self.h, cols.ctypes.data, len(cols), cls.ctypes.data, headd.ctypes.data, ncls.ctypes.data))
        return cls, headd, ncls

    def phase_b(self):
        """What phase B of the last run did (fseq_debug_phase_b): dict(cus, nblocks, fan, resident, fit, hand_armed, stats_kept,
        p2_groups, p2_groups_took_keys, p2_groups_gathered, launches [(level, kind, chains, blocks, first_chain, workgroups)], and
        cw_stats -- by_runs, by_sort, from_identity, max_runs, runs_hist -- or None where k_chain_wg kept no counters)."""
        info = PhaseBInfo()
        self._check(self.L.fseq_debug_phase_b(self.h, C.byref(info)))
        out = {f: int(getattr(info, f)) for f in ("cus", "nblocks", "fan", "resident", "fit", "p2_groups", "p2_groups_took_keys", "p2_groups_gathered")}
        out["hand_armed"], out["stats_kept"] = bool(info.hand_armed), bool(info.stats_kept)
        out["launches"] = _chain_launches(info.launches, info.n_launches)
        s = [int(x) for x in info.cw_stats]
        out["cw_stats"] = dict(by_runs=s[0], by_sort=s[1], from_identity=s[2], max_runs=s[3], runs_hist=s[4:]) if info.stats_kept else None
        return out

    def class_column_sources(self):
        """Where the last run's reduced alignment came from: {from_classes, from_alignment} blocks (phase A's class columns / the
        alignment itself); both zero where the run built none."""
        a, b = C.c_uint32(), C.c_uint32()
        self._check(self.L.fseq_debug_class_columns(self.h, C.byref(a), C.byref(b), 0xFFFFFFFF, None, None, None, None, 0))
        return {"from_classes": a.value, "from_alignment": b.value}

    def column_sources(self, block=None):
        """How the last run's listed blocks came by their columns: {staged, gathered} blocks -- phase A's class columns staged by the
        reduced column kernel itself / the reduced alignment (gathered from the class columns or the alignment) -- and, for a block,
        block_staged; all zero where the run had no reduced alignment to build (LDS-resident rows, no representatives)."""
        a, b, s = C.c_uint32(), C.c_uint32(), C.c_uint32()
        self._check(self.L.fseq_debug_column_sources(self.h, C.byref(a), C.byref(b), 0xFFFFFFFF if block is None else block, C.byref(s)))
        out = {"staged": a.value, "gathered": b.value}
        if block is not None:
            out["block_staged"] = bool(s.value)
        return out

    def class_columns(self, block):
        """Phase A's class columns of a block of the last run: (packed, ldc, nkeys) -- packed[j] the ldc bytes of the block's column j, row
        rho of it the symbol of the block key of rank rho in the alignment's packing -- or (None, ldc, nkeys) where the block has none."""
        have, nkeys, ldc = C.c_uint32(), C.c_uint32(), C.c_uint64()
        self._check(self.L.fseq_debug_class_columns(self.h, None, None, block, C.byref(have), C.byref(nkeys), C.byref(ldc), None, 0))
        if not have.value:
            return None, ldc.value, nkeys.value
        t = self.timings()
        cols = min(t["block_len"], self.n - block * t["block_len"])
        out = np.zeros((cols, ldc.value), dtype=np.uint8)
        self._check(self.L.fseq_debug_class_columns(self.h, None, None, block, C.byref(have), C.byref(nkeys), C.byref(ldc), out.ctypes.data, out.nbytes))
        return out, ldc.value, nkeys.value

    def timings(self):
        t = Timings()
        self._check(self.L.fseq_get_timings(self.h, C.byref(t)))
        return {k: getattr(t, k) for k, _ in Timings._fields_}
