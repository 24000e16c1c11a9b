"""The founder block graph in the SOURCE's co-ordinates on an identity-reduced context (include/fseq.h:
fseq_write_block_graph_restored, fseq_graph_thread_rows_restored, fseq_graph_thread_held_out_restored), and the inputs its tests
share.  No new algorithm: the expected file is tests/block_graph_model.py's on the FULL-LENGTH rows with the restored bounds of
tests/segments_restored_cases.py, the expected threading tests/graph_thread_model.py's on the full-length rows and queries.
Nothing here touches the library; tests/test_block_graph_restored_model.py checks it on the CPU."""
import numpy as np

import block_graph_model as gm
import graph_thread_model as tm
import identity_model as im
import segments_restored_cases as rc

GAP = ord("-")


# ---- the model

def kept_of(full):
    """(mask, kept): the identity columns of the full-length rows and the source column of every other one."""
    mask = im.identity_mask(full)
    return mask, np.flatnonzero(~mask)


def restored_graph(full, lb, rb):
    """The graph of the full-length rows whose reduced run has the merged segments [lb[s], rb[s]) (kept columns): (graph, src_lb, src_rb)."""
    mask, kept = kept_of(full)
    src_lb, src_rb = rc.restored_bounds(kept, full.shape[1], lb, rb)
    return gm.block_graph_model(full, src_lb, src_rb), src_lb, src_rb


def expected_gfa(full, lb, rb, paths=False, gap=b"-"):
    return gm.gfa_bytes(full, restored_graph(full, lb, rb)[0], paths, gap)


def expected_threading(full, lb, rb, full_queries):
    graph, src_lb, src_rb = restored_graph(full, lb, rb)
    return tm.thread_model(full, src_lb, src_rb, full_queries, graph)


def exception_cells(full_queries, full):
    """Per query the identity columns in which it differs from row 0, ascending."""
    mask = im.identity_mask(full)
    return [np.flatnonzero(mask & (q != full[0])) for q in full_queries]


# ---- alignments with identity runs at known places

def distinct_columns(founders, alphabet):
    """founders with founder 0's symbol changed (to a letter, not the gap) wherever all founders agree: no column of a mosaic that
    uses every founder in every block is an identity column."""
    letters = [b for b in alphabet if b != GAP]
    for k in np.flatnonzero((founders == founders[0:1]).all(axis=0)):
        founders[0, k] = next(b for b in letters if b != founders[1, k])
    return founders


def mosaic(X, m, S, W, seed, alphabet=b"ACGT"):
    """(rows [m, S W], founders [X, S W]): S blocks of W columns, every block copies all X founders (every row one of them), no
    identity column.  tests/test_gpu_block_graph.py's full_mosaic but for that."""
    rng = np.random.default_rng(seed)
    alpha = np.frombuffer(alphabet, dtype=np.uint8)
    founders = distinct_columns(alpha[rng.integers(0, len(alpha), size=(X, S * W))], alphabet)
    msa = np.empty((m, S * W), dtype=np.uint8)
    for b in range(S):
        pick = rng.permutation(np.concatenate([np.arange(X), rng.integers(0, X, size=m - X)]))
        msa[:, b * W:(b + 1) * W] = founders[pick, b * W:(b + 1) * W]
    return msa, founders


def gapped(W, alphabet, seed, m=41, S=6):
    """tests/test_gpu_block_graph.py's gapped_blocks without identity columns: four founders; founder 0 has no gap; founder 1 is
    all gaps in block 1; founder 2 has a gap in the first and the last column of every strip of 64 columns of every block;
    founder 3 in a third of its columns."""
    rng = np.random.default_rng(seed)
    alpha = np.frombuffer(alphabet, dtype=np.uint8)
    founders = alpha[rng.integers(0, len(alpha), size=(4, S * W))]
    founders[1, W:2 * W] = GAP
    for b in range(S):
        for k in sorted({0, W - 1} | {c for c in (63, 64, 127, 128) if c < W}):
            founders[2, b * W + k] = GAP
    founders[3, rng.random(S * W) < 0.33] = GAP
    founders = distinct_columns(founders, alphabet)
    msa = np.empty((m, S * W), dtype=np.uint8)
    for b in range(S):
        pick = rng.permutation(np.concatenate([np.arange(4), rng.integers(0, 4, size=m - 4)]))
        msa[:, b * W:(b + 1) * W] = founders[pick, b * W:(b + 1) * W]
    return msa, founders


def with_runs(R, runs):
    """R [m, n] with runs of identity columns: runs maps a reduced position p in 0 .. n to the run's bytes, which stand in front of
    R's column p (p = n: behind the last); every row carries them.  Returns (full, kept)."""
    m, n = R.shape
    pieces, kept, at = [], [], 0
    for p in range(n + 1):
        run = runs.get(p, b"")
        if run:
            pieces.append(np.repeat(np.frombuffer(run, dtype=np.uint8)[None, :], m, axis=0))
            at += len(run)
        if p < n:
            pieces.append(R[:, p:p + 1])
            kept.append(at)
            at += 1
    return np.ascontiguousarray(np.concatenate(pieces, axis=1)), np.array(kept, dtype=np.int64)


def run_bytes(length, alphabet, start=0):
    """`length` bytes that walk the alphabet and the gap byte."""
    pool = bytes(alphabet) + b"-"
    return bytes(pool[(start + i * 3 + i // 4) % len(pool)] for i in range(length))


def blocks(S, W):
    return np.arange(S, dtype=np.uint64) * W, (np.arange(S, dtype=np.uint64) + 1) * W


def label_case(W, alphabet=b"ACGT", seed=None, m=41, S=6):
    """gapped(W) with runs planted where the S kernels' strips can go wrong; -> (full, R, kept, L).  The runs, by the block of W
    kept columns whose segment owns them:
      in front of column 0: 63 bytes (the first kept column on lane 63 of segment 0's first strip; identity columns in front of kept[0])
      block 1 (founder 1: gaps alone): two gap bytes behind it -- the label stays empty ('*')
      block 2: one byte behind its first column
      block 3: 64 bytes behind its first column (lane 0 kept, the rest of the strip identity columns)
      block 4: 130 bytes behind its first column (a strip with no kept column)
      behind the last column: two bytes, the second a gap
    Block 0 beyond the front run and block 5 before the end run have none inside: strips of 64 kept columns where W >= 64.
    (W = 1: "behind its first column" is in front of the next block's, which is the same place.)"""
    R, _ = gapped(W, alphabet, W if seed is None else seed, m, S)
    runs = {0: run_bytes(63, alphabet), 2 * W: b"--", 2 * W + 1: run_bytes(1, alphabet, 1), 3 * W + 1: run_bytes(64, alphabet, 2),
            4 * W + 1: run_bytes(130, alphabet, 3), S * W: run_bytes(1, alphabet, 5) + b"-"}
    full, kept = with_runs(R, runs)
    return full, R, kept, W


def reaches(full, lb, rb, gap=b"-"):
    """What an alignment with the merged segments [lb, rb) (kept columns) puts in front of the restored S kernels: a set of names."""
    mask, kept = kept_of(full)
    graph, src_lb, src_rb = restored_graph(full, lb, rb)
    out = set()
    out |= {"range=%d" % int(w) for w in (src_rb - src_lb)}
    if mask[0]:
        out.add("identity in front of kept[0]")
    if mask[-1]:
        out.add("identity behind kept[n-1]")
    runs, at = [], 0
    for p in range(len(mask) + 1):                              # the lengths of the identity runs
        if p < len(mask) and mask[p]:
            at += 1
        elif at:
            runs.append(at)
            at = 0
    out |= {"run=%d" % r for r in runs}
    for s in range(len(lb)):
        for base in range(int(src_lb[s]), int(src_rb[s]), 64):
            strip = mask[base:min(base + 64, int(src_rb[s]))]
            if strip.all():
                out.add("strip without a kept column")
            if len(strip) == 64 and not strip.any():
                out.add("strip of 64 kept columns")
            if not strip[0]:
                out.add("kept column on lane 0")
            if len(strip) == 64 and not strip[63]:
                out.add("kept column on lane 63")
    if gap and (full[0, mask] == gap[0]).any():
        out.add("row 0 is a gap in an identity column")
    labels = [gm.label(full, nd, gap) for nd in graph["nodes"]]
    if any(len(x) == 0 for x in labels):
        out.add("empty label")
    out.add("S=%d" % len(lb))
    out.add("classes=%d" % int(graph["count"].max()))
    return out


# ---- the threading's inputs: rows, and full-length queries with exception cells at known places

THREAD_RUNS = (3, 2, 2, 70, 2, 1, 40)       # in front of each of the 6 blocks of tm.MOSAIC, then behind the last


def thread_rows(alphabet=b"ACGT", S=None, runs=None):
    """(full, R, founders, kept, W): tm.MOSAIC's shape without identity columns of its own, a run in front of every block and
    one behind the last, so that every segment's source range ends in identity columns (and segment 0's begins in them)."""
    X, m, S0, W, seed = tm.MOSAIC
    S = S or S0
    R, founders = mosaic(X, m, S, W, seed, alphabet)
    runs = (runs or THREAD_RUNS)
    runs = tuple(runs[:S]) + (runs[-1],)
    full, kept = with_runs(R, {b * W: run_bytes(runs[b], alphabet, b) for b in range(S + 1)})
    return full, R, founders, kept, W


def expand(reduced_queries, full, kept):
    """Full-length queries without exception cells: row 0's bytes with the kept columns replaced."""
    out = np.repeat(full[0:1], len(reduced_queries), axis=0)
    out[:, kept] = reduced_queries
    return out


def other_byte(b, alphabet=b"ACGT"):
    return next(x for x in alphabet if x != b)


def plant(query, full, cell, byte=None):
    """query with an exception cell at the identity column `cell` (a byte of the alphabet other than row 0's, or `byte`)."""
    assert im.identity_mask(full)[cell]
    q = query.copy()
    q[cell] = other_byte(full[0, cell]) if byte is None else byte
    assert q[cell] != full[0, cell]
    return q


def mosaic_queries(full, founders, kept, S, W, count, seed):
    return expand(tm.mosaic_queries(founders, S, W, count, seed), full, kept)
