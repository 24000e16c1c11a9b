"""Rows threaded through the founder block graph (include/fseq.h: fseq_graph_thread_rows, fseq_graph_thread_held_out) from the
raw bytes alone: numpy on top of tests/block_graph_model.py, no key, no table and no class table of the library.

Per segment a dict from a node's bytes to its id, a dict from (from, to) to the edge's index, the walks and the statistics by a
plain loop over the segments of every query.  A query byte outside the alignment's alphabet is in no node's bytes, so the dict
finds nothing: no special case.  tests/test_graph_thread_model.py checks the model on the CPU."""
import numpy as np

import block_graph_model as gm

NONE = 0xFFFFFFFF
ROW_DTYPE = np.dtype([("columns_matched", "<u8"), ("longest_walk_columns", "<u8"), ("segments_matched", "<u4"), ("junctions_linked", "<u4"),
                      ("junctions_novel", "<u4"), ("walks", "<u4"), ("longest_walk_segments", "<u4"), ("reserved", "<u4")])
SEGMENT_DTYPE = np.dtype([("matched", "<u4"), ("linked", "<u4"), ("novel", "<u4"), ("reserved", "<u4")])
TABLE_HEADER = b"SEQUENCE_INDEX\tSEGMENTS\tMATCHED\tLINKED\tNOVEL\tWALKS\tLONGEST_WALK\tLONGEST_WALK_COLUMNS\tMATCHED_COLUMNS\n"


def full_mosaic(X, m, S, W, seed, alphabet=b"ACGT"):
    """tests/test_gpu_block_graph.py's generator, draw for draw, which also returns the founders: ([m, S W], [X, S W]) -- S blocks
    of W columns, every block copies all X founders (every row one of them)."""
    rng = np.random.default_rng(seed)
    alpha = np.frombuffer(alphabet, dtype=np.uint8)
    founders = alpha[rng.integers(0, len(alpha), size=(X, S * W))]
    msa = np.empty((m, S * W), dtype=np.uint8)
    for b in range(S):
        pick = rng.permutation(np.concatenate([np.arange(X), rng.integers(0, X, size=m - X)]))
        msa[:, b * W:(b + 1) * W] = founders[pick, b * W:(b + 1) * W]
    return msa, founders


def mosaic_queries(founders, S, W, count, seed):
    """count mosaics of the founders by blocks: every block of a query is one founder's block."""
    rng = np.random.default_rng(seed)
    pick = rng.integers(0, founders.shape[0], size=(count, S))
    out = np.empty((count, S * W), dtype=np.uint8)
    for b in range(S):
        out[:, b * W:(b + 1) * W] = founders[pick[:, b], b * W:(b + 1) * W]
    return out


def thread_model(msa, lb, rb, queries, graph=None):
    """{"nodes" [S, Q], "steps" [S - 1, Q], "per_row", "per_segment", "summary", "graph"} of the queries [Q, n] through the graph
    of msa's segments [lb[s], rb[s])."""
    graph = graph or gm.block_graph_model(msa, lb, rb)
    S, Q = len(lb), len(queries)
    by_bytes = [{} for _ in range(S)]
    for i, nd in enumerate(graph["nodes"]):
        by_bytes[int(nd["segment"])][msa[int(nd["rep_row"]), int(nd["lb"]):int(nd["rb"])].tobytes()] = i
    by_pair = {(int(e["from"]), int(e["to"])): i for i, e in enumerate(graph["edges"])}
    nodes = np.full((S, Q), NONE, dtype=np.uint32)
    steps = np.full((max(S, 1) - 1, Q), NONE, dtype=np.uint32)
    per_row = np.zeros(Q, dtype=ROW_DTYPE)
    per_segment = np.zeros(S, dtype=SEGMENT_DTYPE)
    on_graph = 0
    for q in range(Q):
        for s in range(S):
            nodes[s, q] = by_bytes[s].get(queries[q, int(lb[s]):int(rb[s])].tobytes(), NONE)
        for p in range(S - 1):
            if nodes[p, q] != NONE and nodes[p + 1, q] != NONE:
                steps[p, q] = by_pair.get((int(nodes[p, q]), int(nodes[p + 1, q])), NONE)
        row = per_row[q]
        walk_segments = walk_columns = 0                       # the walk under way
        for s in range(S):
            width = int(rb[s]) - int(lb[s])
            if nodes[s, q] == NONE:
                walk_segments = walk_columns = 0
                continue
            per_segment[s]["matched"] += 1
            row["segments_matched"] += 1
            row["columns_matched"] += width
            if walk_segments and steps[s - 1, q] != NONE:
                walk_segments, walk_columns = walk_segments + 1, walk_columns + width
            else:
                row["walks"] += 1
                walk_segments, walk_columns = 1, width
            row["longest_walk_segments"] = max(int(row["longest_walk_segments"]), walk_segments)
            row["longest_walk_columns"] = max(int(row["longest_walk_columns"]), walk_columns)
        for p in range(S - 1):
            if steps[p, q] != NONE:
                row["junctions_linked"] += 1
                per_segment[p]["linked"] += 1
            elif nodes[p, q] != NONE and nodes[p + 1, q] != NONE:
                row["junctions_novel"] += 1
                per_segment[p]["novel"] += 1
        on_graph += int(row["walks"] == 1 and row["longest_walk_segments"] == S)
    summary = {"rows": Q, "segments": S, "segments_matched": int(per_row["segments_matched"].sum()), "junctions_linked": int(per_row["junctions_linked"].sum()),
               "junctions_novel": int(per_row["junctions_novel"].sum()), "walks": int(per_row["walks"].sum()), "rows_on_graph": on_graph}
    return {"nodes": nodes, "steps": steps, "per_row": per_row, "per_segment": per_segment, "summary": summary, "graph": graph}


def table(threaded):
    """The front end's file (--output-held-out-graph-threads, --output-sequence-graph-threads)."""
    sm = threaded["summary"]
    lines = [TABLE_HEADER]
    for q, r in enumerate(threaded["per_row"]):
        lines.append(b"%d\t%d\t%d\t%d\t%d\t%d\t%d\t%d\t%d\n" % (q, sm["segments"], r["segments_matched"], r["junctions_linked"], r["junctions_novel"], r["walks"],
                                                             r["longest_walk_segments"], r["longest_walk_columns"], r["columns_matched"]))
    lines.append(b"#\tROWS=%d\tSEGMENTS=%d\tSEGMENTS_MATCHED=%d\tJUNCTIONS_LINKED=%d\tJUNCTIONS_NOVEL=%d\tWALKS=%d\tROWS_ON_GRAPH=%d\n" %
                 (sm["rows"], sm["segments"], sm["segments_matched"], sm["junctions_linked"], sm["junctions_novel"], sm["walks"], sm["rows_on_graph"]))
    return b"".join(lines)


# ---- the cases the GPU tests run against the model: name -> (msa, L, queries, what the case is listed for)

MOSAIC = (5, 23, 6, 8, 1)          # X, m, S, W, seed: the oracle's optimum at L = 8 is 5


def substituted(msa, W, row, column):
    """Row `row` with the base at `column` replaced by the first of ACGT that leaves its block's substring no row's."""
    b = column // W
    have = {msa[r, b * W:(b + 1) * W].tobytes() for r in range(msa.shape[0])}
    for base in b"ACGT":
        q = msa[row].copy()
        q[column] = base
        if q[b * W:(b + 1) * W].tobytes() not in have:
            return q
    raise AssertionError("every substitution is some row's substring")


def case(name):
    X, m, S, W, seed = MOSAIC
    msa, founders = full_mosaic(X, m, S, W, seed)
    if name == "mosaic":
        return msa, W, mosaic_queries(founders, S, W, 40, 3), {"novel"}
    if name == "outside":
        # rows 2 and 9 with one cell each set to a byte outside ACGT (the first column of a block, the last of another), row 4 as it is
        q = msa[[2, 9, 4]].copy()
        q[0, 2 * W] = ord("N")
        q[1, 5 * W - 1] = ord("-")
        return msa, W, q, {"unmatched", "outside"}
    if name == "substituted":
        q = np.stack([substituted(msa, W, 7, 3 * W + 5), msa[7], substituted(msa, W, 11, 0), substituted(msa, W, 20, S * W - 1)])
        return msa, W, q, {"unmatched"}
    if name == "mixed":
        # mosaics with a byte outside the alphabet in some and a substitution in others: novel junctions beside unmatched segments
        q = mosaic_queries(founders, S, W, 70, 5)
        q[::7, W + 2] = ord("N")
        q[3::9, 4 * W] = ord("n")
        q = np.concatenate([q, [substituted(msa, W, 1, 2 * W + 1)]])
        return msa, W, q, {"novel", "unmatched", "outside"}
    raise KeyError(name)


CASES = ("mosaic", "outside", "substituted", "mixed")
