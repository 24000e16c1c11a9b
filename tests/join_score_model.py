"""The junction support of a join (include/fseq.h, fseq_join_score) restated in numpy, from the raw alignment alone: a segment's
classes are the distinct byte strings msa[i, lb:rb]; nothing here looks at a boundary state or at a class table of the library.

    join_score_model(msa, lb, rb, perm)        the score of permutations [S][X] (an entry >= m a gap)
    score_from_labels(labels, left, right)     the same counting on any labels: labels [S][m] a label per row and segment,
                                               left / right [S - 1][X] the labels of every slot's two rows, GAP a gap
    format_join_score(score, rb)               the bytes of the front end's --output-join-score file
    table_home / colliding_keys                the home entry of a key in k_join_score's table (csrc/fseq_joinscore.hpp,
                                               join_score_home), to build keys that collide there

A score is a dict: junctions -- per junction supported, unsupported, gaps, rows_through, weight --, breaks [X], support
[S - 1][X], summary."""
import numpy as np

GAP = -1
FIELDS = ("supported", "unsupported", "gaps", "rows_through", "weight")


def segment_labels(msa, lb, rb):
    """labels[s][i]: the number of row i's substring msa[i, lb_s:rb_s] among the segment's distinct substrings."""
    m = msa.shape[0]
    out = np.zeros((len(lb), m), dtype=np.int64)
    for s, (l, r) in enumerate(zip(lb, rb)):
        sub = np.ascontiguousarray(msa[:, int(l):int(r)])
        rows = sub.view(np.dtype((np.void, sub.shape[1]))).ravel()
        out[s] = np.unique(rows, return_inverse=True)[1].ravel()
    return out


def score_from_labels(labels, left, right):
    labels = np.asarray(labels, dtype=np.int64)
    left = np.asarray(left, dtype=np.int64)
    right = np.asarray(right, dtype=np.int64)
    S, m = labels.shape
    pairs, X = left.shape
    assert pairs == S - 1 and right.shape == left.shape
    base = 1 << 20
    junctions = {f: np.zeros(pairs, dtype=np.uint64) for f in FIELDS}
    support = np.zeros((pairs, X), dtype=np.uint64)
    breaks = np.zeros(X, dtype=np.uint64)
    for p in range(pairs):
        row_pairs, rows = np.unique(labels[p] * base + labels[p + 1], return_counts=True)
        gap = (left[p] == GAP) | (right[p] == GAP)
        slot_pairs = np.where(gap, -1, left[p] * base + right[p])
        at = np.minimum(np.searchsorted(row_pairs, slot_pairs), len(row_pairs) - 1)
        found = ~gap & (row_pairs[at] == slot_pairs)
        sup = np.where(found, rows[at], 0)
        support[p] = sup
        junctions["supported"][p] = np.count_nonzero(found)
        junctions["unsupported"][p] = np.count_nonzero(~gap & ~found)
        junctions["gaps"][p] = np.count_nonzero(gap)
        junctions["weight"][p] = sup.sum()
        junctions["rows_through"][p] = rows[np.unique(at[found])].sum()      # (a pair of classes that several slots share: once)
        breaks += (~gap & ~found)
    summary = {f: int(junctions[f].sum()) for f in FIELDS}
    summary["junctions"] = pairs
    through = junctions["rows_through"]
    summary["min_rows_through"] = int(through.min()) if pairs else m
    summary["min_rows_through_junction"] = int(through.argmin()) if pairs else 0
    summary["max_breaks"] = int(breaks.max()) if X else 0
    return {"junctions": junctions, "breaks": breaks, "support": support, "summary": summary}


def join_score_model(msa, lb, rb, perm):
    m = msa.shape[0]
    perm = np.asarray(perm, dtype=np.int64)
    labels = segment_labels(msa, lb, rb)
    S = len(lb)
    rows = np.minimum(perm, m - 1)
    of_slot = np.where(perm < m, np.take_along_axis(labels, rows, axis=1), GAP)      # [S][X]
    return score_from_labels(labels, of_slot[:S - 1], of_slot[1:])


def same_score(got, want, rb=None):
    """Why a score of the library (join_score, join_score_host, debug_join_score) differs from a model score; None if it does not."""
    for f in FIELDS:
        if not np.array_equal(got["junctions"][f].astype(np.uint64), want["junctions"][f]):
            return "junctions." + f
    if rb is not None and not np.array_equal(got["junctions"]["rb"], np.asarray(rb, dtype=np.uint64)[:len(got["junctions"])]):
        return "junctions.rb"
    if not np.array_equal(got["breaks"].astype(np.uint64), want["breaks"]):
        return "breaks"
    if got["support"] is not None and not np.array_equal(got["support"].astype(np.uint64), want["support"]):
        return "support"
    for k, v in want["summary"].items():
        if got["summary"][k] != v:
            return "summary." + k
    return None


def format_join_score(score, rb):
    sm = score["summary"]
    j = score["junctions"]
    lines = ["# JUNCTIONS=%d\tSUPPORTED=%d\tUNSUPPORTED=%d\tGAPS=%d\tROWS_THROUGH=%d\tWEIGHT=%d\tMIN_ROWS_THROUGH=%d\tMIN_ROWS_THROUGH_JUNCTION=%d\tMAX_BREAKS=%d"
             % (sm["junctions"], sm["supported"], sm["unsupported"], sm["gaps"], sm["rows_through"], sm["weight"], sm["min_rows_through"],
                sm["min_rows_through_junction"], sm["max_breaks"]),
             "JUNCTION\tRB\tSUPPORTED\tUNSUPPORTED\tGAPS\tROWS_THROUGH\tWEIGHT"]
    for p in range(sm["junctions"]):
        lines.append("%d\t%d\t%d\t%d\t%d\t%d\t%d" % (p, int(rb[p]), j["supported"][p], j["unsupported"][p], j["gaps"][p], j["rows_through"][p], j["weight"][p]))
    lines += ["", "FOUNDER\tBREAKS"]
    lines += ["%d\t%d" % (r, b) for r, b in enumerate(score["breaks"])]
    return ("\n".join(lines) + "\n").encode()


def table_log2(X):
    """log2 of the table's capacity: the power of two >= 2 X."""
    lg = 1
    while (1 << lg) < 2 * X:
        lg += 1
    return lg


def table_home(keys, lg):
    return ((np.asarray(keys, dtype=np.uint64) * np.uint64(0x9E3779B1)) & np.uint64(0xFFFFFFFF)) >> np.uint64(32 - lg)


def colliding_keys(X, home, classes=4096):
    """X distinct keys l << 16 | r, l and r below `classes`, whose home entry in the table for X slots is `home`: as (l, r)."""
    lg = table_log2(X)
    l = np.repeat(np.arange(classes, dtype=np.uint64), classes)
    r = np.tile(np.arange(classes, dtype=np.uint64), classes)
    hit = np.flatnonzero(table_home(l << np.uint64(16) | r, lg) == home)[:X]
    assert len(hit) == X, (X, home, len(hit))
    return l[hit].astype(np.int64), r[hit].astype(np.int64)
