"""The nearest node of every segment for rows threaded through the founder block graph (include/fseq.h: fseq_graph_nearest_rows,
fseq_graph_nearest_held_out) from the raw bytes alone: numpy on top of tests/block_graph_model.py and tests/graph_thread_model.py,
no packed word, no popcount and no class table of the library.

Per segment (queries[:, None, lb:rb] != reps[None, :, lb:rb]).sum(-1), argmin (the first minimum is the smallest class) and a tie
count; then graph_thread_model.thread_model's walk loop on the admitted cells.  Raw bytes compare as the codes do: the code table
is injective on the alignment's alphabet, and a query byte outside it equals no byte of the alignment.
tests/test_graph_nearest_model.py checks the model on the CPU."""
import numpy as np

import block_graph_model as gm
import graph_thread_model as tm

NONE = tm.NONE
ROW_DTYPE = np.dtype([("columns_admitted", "<u8"), ("longest_walk_columns", "<u8"), ("mismatches_admitted", "<u8"), ("mismatches", "<u8"),
                      ("segments_admitted", "<u4"), ("segments_exact", "<u4"), ("junctions_linked", "<u4"), ("junctions_novel", "<u4"),
                      ("walks", "<u4"), ("longest_walk_segments", "<u4"), ("max_distance", "<u4"), ("reserved", "<u4")])
SEGMENT_DTYPE = np.dtype([("mismatches", "<u8"), ("admitted", "<u4"), ("exact", "<u4"), ("linked", "<u4"), ("novel", "<u4"), ("max_distance", "<u4"),
                          ("reserved", "<u4")])
SUMMARY = ("rows", "segments", "segments_admitted", "segments_exact", "junctions_linked", "junctions_novel", "walks", "rows_on_graph", "mismatches")
TABLE_HEADER = (b"SEQUENCE_INDEX\tSEGMENTS\tADMITTED\tEXACT\tLINKED\tNOVEL\tWALKS\tLONGEST_WALK\tLONGEST_WALK_COLUMNS\tADMITTED_COLUMNS\t"
                b"MISMATCHES_ADMITTED\tMISMATCHES\tMAX_DISTANCE\n")


def distances(reps, queries):
    """(class, distance, ties), each [Q], of the queries' substrings [Q, W] against a segment's representatives' [X, W]; in slabs
    of queries, so that the comparison's [Q, X, W] array stays small."""
    Q = len(queries)
    arg, dist, ties = np.zeros(Q, dtype=np.uint32), np.zeros(Q, dtype=np.uint32), np.zeros(Q, dtype=np.uint32)
    step = max(1, (1 << 24) // max(1, reps.shape[0] * reps.shape[1]))
    for q0 in range(0, Q, step):
        d = (queries[q0:q0 + step, None, :] != reps[None, :, :]).sum(-1)
        arg[q0:q0 + step] = d.argmin(1)
        dist[q0:q0 + step] = d.min(1)
        ties[q0:q0 + step] = (d == d.min(1)[:, None]).sum(1)
    return arg, dist, ties


def nearest_model(msa, lb, rb, queries, max_distance=0, graph=None):
    """{"nodes", "distances", "ties" [S, Q], "steps" [S - 1, Q], "per_row", "per_segment", "summary", "graph"} of the queries [Q, n]
    against the graph of msa's segments [lb[s], rb[s])."""
    graph = graph or gm.block_graph_model(msa, lb, rb)
    S, Q = len(lb), len(queries)
    noff = np.zeros(S + 1, dtype=np.int64)
    for nd in graph["nodes"]:
        noff[int(nd["segment"]) + 1] += 1
    noff = np.cumsum(noff)
    by_pair = {(int(e["from"]), int(e["to"])): i for i, e in enumerate(graph["edges"])}
    nodes = np.zeros((S, Q), dtype=np.uint32)
    dist = np.zeros((S, Q), dtype=np.uint32)
    ties = np.zeros((S, Q), dtype=np.uint32)
    for s in range(S):
        mine = graph["nodes"][noff[s]:noff[s + 1]]
        assert (mine["segment"] == s).all() and (mine["cls"] == np.arange(len(mine))).all()
        reps = msa[mine["rep_row"].astype(np.int64), int(lb[s]):int(rb[s])]
        arg, dist[s], ties[s] = distances(reps, queries[:, int(lb[s]):int(rb[s])])
        nodes[s] = noff[s] + arg
    admitted = dist <= max_distance
    steps = np.full((max(S, 1) - 1, Q), NONE, dtype=np.uint32)
    per_row = np.zeros(Q, dtype=ROW_DTYPE)
    per_segment = np.zeros(S, dtype=SEGMENT_DTYPE)
    on_graph = 0
    for q in range(Q):
        for p in range(S - 1):
            if admitted[p, q] and admitted[p + 1, q]:
                steps[p, q] = by_pair.get((int(nodes[p, q]), int(nodes[p + 1, q])), NONE)
        row = per_row[q]
        walk_segments = walk_columns = 0                       # the walk under way
        for s in range(S):
            width, d = int(rb[s]) - int(lb[s]), int(dist[s, q])
            row["mismatches"] += d
            row["max_distance"] = max(int(row["max_distance"]), d)
            per_segment[s]["mismatches"] += d
            per_segment[s]["max_distance"] = max(int(per_segment[s]["max_distance"]), d)
            if not admitted[s, q]:
                walk_segments = walk_columns = 0
                continue
            per_segment[s]["admitted"] += 1
            per_segment[s]["exact"] += d == 0
            row["segments_admitted"] += 1
            row["segments_exact"] += d == 0
            row["columns_admitted"] += width
            row["mismatches_admitted"] += d
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
            elif admitted[p, q] and admitted[p + 1, q]:
                row["junctions_novel"] += 1
                per_segment[p]["novel"] += 1
        on_graph += int(row["walks"] == 1 and row["longest_walk_segments"] == S)
    summary = {"rows": Q, "segments": S, "segments_admitted": int(per_row["segments_admitted"].sum()), "segments_exact": int(per_row["segments_exact"].sum()),
               "junctions_linked": int(per_row["junctions_linked"].sum()), "junctions_novel": int(per_row["junctions_novel"].sum()),
               "walks": int(per_row["walks"].sum()), "rows_on_graph": on_graph, "mismatches": int(per_row["mismatches"].sum())}
    return {"nodes": nodes, "distances": dist, "ties": ties, "steps": steps, "per_row": per_row, "per_segment": per_segment, "summary": summary, "graph": graph}


def as_threading(near):
    """What fseq_graph_thread_rows answers, from a model (or a library result) at max_distance = 0: nodes where the distance is 0
    and NONE elsewhere, steps, and the statistics the two share."""
    nodes = np.where(near["distances"] == 0, near["nodes"], np.uint32(NONE)).astype(np.uint32)
    r, g = near["per_row"], near["per_segment"]
    per_row = np.zeros(len(r), dtype=tm.ROW_DTYPE)
    for new, old in (("columns_matched", "columns_admitted"), ("longest_walk_columns",) * 2, ("segments_matched", "segments_admitted"), ("junctions_linked",) * 2,
                     ("junctions_novel",) * 2, ("walks",) * 2, ("longest_walk_segments",) * 2):
        per_row[new] = r[old]
    per_segment = np.zeros(len(g), dtype=tm.SEGMENT_DTYPE)
    for new, old in (("matched", "admitted"), ("linked",) * 2, ("novel",) * 2):
        per_segment[new] = g[old]
    sm = near["summary"]
    summary = {"rows": sm["rows"], "segments": sm["segments"], "segments_matched": sm["segments_admitted"], "junctions_linked": sm["junctions_linked"],
               "junctions_novel": sm["junctions_novel"], "walks": sm["walks"], "rows_on_graph": sm["rows_on_graph"]}
    return {"nodes": nodes, "steps": near["steps"], "per_row": per_row, "per_segment": per_segment, "summary": summary}


def table(near, max_distance):
    """The front end's file (--output-held-out-graph-nearest, --output-sequence-graph-nearest)."""
    sm = near["summary"]
    lines = [TABLE_HEADER]
    for q, r in enumerate(near["per_row"]):
        lines.append(b"%d\t%d\t%d\t%d\t%d\t%d\t%d\t%d\t%d\t%d\t%d\t%d\t%d\n" % (
            q, sm["segments"], r["segments_admitted"], r["segments_exact"], r["junctions_linked"], r["junctions_novel"], r["walks"], r["longest_walk_segments"],
            r["longest_walk_columns"], r["columns_admitted"], r["mismatches_admitted"], r["mismatches"], r["max_distance"]))
    lines.append(b"#\tMAX_DISTANCE_ALLOWED=%d\tROWS=%d\tSEGMENTS=%d\tSEGMENTS_ADMITTED=%d\tSEGMENTS_EXACT=%d\tJUNCTIONS_LINKED=%d\tJUNCTIONS_NOVEL=%d\tWALKS=%d\t"
                 b"ROWS_ON_GRAPH=%d\tMISMATCHES=%d\n" % (max_distance, sm["rows"], sm["segments"], sm["segments_admitted"], sm["segments_exact"], sm["junctions_linked"],
                                                          sm["junctions_novel"], sm["walks"], sm["rows_on_graph"], sm["mismatches"]))
    return b"".join(lines)
