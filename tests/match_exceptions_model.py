"""The restored match of QUERY rows (fseq_match_held_out_restored / fseq_match_rows_restored, csrc/fseq_match.hpp) in plain
Python: the loop of match_model.match_row over the merged, ascending sequence of the kept columns and the row's own exception
columns -- identity columns of the reconstruction in which the query differs from row 0, where every restored founder carries
row 0's byte and so none agrees with the query -- with the identity columns in between accounted for in the closed form of
match_restored_model.  An exception column is the ordinary column step with the empty founder set.

The definition stays match_model.match_row(query, identity_model.restore(founders, mask, row0), min_len) on the full-length
data; tests/test_match_exceptions_model.py proves the merged walk equal to it on the cases below, which the GPU test
(tests/test_gpu_held_out_restored.py) plants at its own sizes with the same functions."""
import numpy as np

import match_restored_model as rm

# what a case can be listed for: whole rows (none, every), places in a row (the others), and a property of (case, min_len)
PLACES = ("ends", "run", "around_kept", "uncovered_then_exc", "tile_border", "stage_border", "min_len_gap")
PATTERNS = ("none", "every") + PLACES + ("foreign", "min_len_larger")
STAGE = 64                                                        # columns of the smallest staged chunk of the host rows' upload


def exceptions_of(queries, mask, row0):
    """per query row: the identity columns in which it differs from row 0, ascending"""
    return [np.flatnonzero(mask & (q != row0)) for q in queries]


def match_row_merged(seq, founders, kept, exc, n_src, min_len):
    """seq: the query at the kept columns; founders: K sequences over the kept columns; kept: source positions, ascending;
    exc: the query's exception columns, source positions, ascending (none of them a kept column).
    -> (pieces [(lb, rb, [founder indices])] in source co-ordinates, uncovered cells, short pieces)"""
    K = len(founders)
    out, cur, lb = [], list(range(K)), 0
    uncovered = short = 0

    def gap(g_lo, g_hi):                                          # match_restored_model's closed form over [g_lo, g_hi)
        nonlocal cur, lb, short
        if g_lo >= g_hi:
            return
        if not cur:
            if min_len and g_lo - lb < min_len:
                short += 1
            out.append((lb, g_lo, []))
            lb, cur = g_lo, list(range(K))
        if min_len:
            for _ in range((g_hi - lb - 1) // min_len):
                out.append((lb, lb + min_len, list(cur)))
                lb, cur = lb + min_len, list(range(K))

    def step(pos, agree):                                         # match_model.match_row's step; agree: who carries the symbol
        nonlocal cur, lb, short, uncovered
        recheck = False
        if min_len and min_len <= pos - lb:
            recheck = True
        else:
            dst = [f for f in cur if f in agree]
            if not dst:
                if min_len and pos - lb < min_len:
                    short += 1
                recheck = True
        if recheck:
            out.append((lb, pos, list(cur)))
            lb = pos
            dst = sorted(agree)
            if not dst:
                uncovered += 1
        cur = dst

    g_lo, e = 0, 0
    exc = [int(x) for x in exc]
    for j, c in enumerate(seq):
        pos = int(kept[j])
        while e < len(exc) and exc[e] < pos:                      # the exceptions in front of this kept column
            gap(g_lo, exc[e])
            step(exc[e], set())
            g_lo = exc[e] + 1
            e += 1
        gap(g_lo, pos)
        g_lo = pos + 1
        step(pos, {f for f in range(K) if founders[f][j] == c})
    while e < len(exc):
        gap(g_lo, exc[e])
        step(exc[e], set())
        g_lo = exc[e] + 1
        e += 1
    gap(g_lo, n_src)
    if cur:
        out.append((lb, n_src, list(cur)))
    return out, uncovered, short


# ---- the layouts and the patterns planted in them
A, U, G = 5, 8, 12                                                # kept indices: identity columns on either side; an uncovered cell with a gap behind; a long gap in front


def layout(rng, n_kept, tile, first=70, long_gap=130, last=2, draw=(0, 0, 1, 2, 7)):
    """-> mask over the source columns.  gaps[j] identity columns in front of kept column j (gaps[n_kept]: behind the last):
    `first` in front of the first one (70: the columns 63 and 64, the border of a staged chunk, are identity columns), one on
    either side of kept[A], three behind kept[U], long_gap in front of kept[G], two in front of kept[tile - 1], kept[tile] and
    kept[tile + 1] (the gaps on both sides of the walk's tile border)."""
    assert G < tile - 1 and tile + 1 < n_kept
    gaps = rng.choice(np.array(draw), size=n_kept + 1)
    gaps[0], gaps[n_kept] = first, last
    gaps[A], gaps[A + 1], gaps[U + 1] = max(gaps[A], 1), max(gaps[A + 1], 1), max(gaps[U + 1], 3)
    if long_gap:
        gaps[G] = long_gap
    for j in (tile - 1, tile, tile + 1):
        gaps[j] = max(gaps[j], 2)
    return np.concatenate([np.r_[np.ones(g, dtype=bool), False] for g in gaps[:n_kept]] + [np.ones(gaps[n_kept], dtype=bool)])


def places(mask, tile):
    """pattern -> (exception columns, kept indices whose cell is to be uncovered), for the patterns the layout has room for"""
    kept = np.flatnonzero(~mask)
    n_src = len(mask)
    first, last, long_gap = int(kept[0]), n_src - 1 - int(kept[-1]), int(kept[G] - kept[G - 1] - 1)
    out = {"around_kept": ([kept[A] - 1, kept[A] + 1], []), "uncovered_then_exc": ([kept[U] + 2], [U]),
           "tile_border": ([kept[tile - 1] - 1, kept[tile] - 1, kept[tile + 1] - 1], [])}
    if first and last:
        out["ends"] = ([0, n_src - 1], [])
    if first >= 5:
        out["run"] = ([1, 2, 3], [])
    elif long_gap < 100:
        out["run"] = ([kept[tile] - 2, kept[tile] - 1], [])
    if first > STAGE + 1:
        out["stage_border"] = ([STAGE - 1, STAGE], [])
    if long_gap >= 120:
        out["min_len_gap"] = ([kept[G] - long_gap // 2], [])
        out["run"] = (out.get("run", ([], []))[0] + [kept[G] - 5, kept[G] - 4], [])
    for cols, _ in out.values():
        assert mask[np.array(cols, dtype=np.int64)].all()
    return {k: ([int(c) for c in cols], cells) for k, (cols, cells) in out.items()}


def plant(rng, queries, row0, mask, tile, private, other, foreign=None):
    """Writes the patterns into queries (rows that agree with row 0 in every identity column so far) and returns
    {pattern: [(row, exception columns, uncovered kept indices)]}.  private: a symbol of the alphabet no row of the
    reconstruction has (an exception in an identity column, an uncovered cell in a kept one); other(b): another symbol the
    reconstruction's rows do have.  One query row: every place in that row.  More: row 0 none, row 1 every, the places spread
    over the rows from 2 on and all of them once more in the last row; the other rows get exceptions in 1 % of the identity
    columns.  foreign: a byte outside the alphabet, written into an identity and a kept column of one more row (host rows)."""
    q = len(queries)
    kept = np.flatnonzero(~mask)
    where = {}
    P = places(mask, tile)

    def put(r, name):
        cols, cells = P[name]
        for c in cols:
            queries[r, c] = private if (c + r) % 2 else other(row0[c])
        for j in cells:
            queries[r, kept[j]] = private
        where.setdefault(name, []).append((r, cols, cells))

    used = set()
    if q == 1:
        for name in P:
            put(0, name)
        return where
    where["none"] = [(0, [], [])]
    used.add(0)
    if q >= 3:
        queries[1, mask] = private
        where["every"] = [(1, np.flatnonzero(mask).tolist(), [])]
        used.add(1)
    free = [r for r in range(q) if r not in used]
    for i, name in enumerate(P):
        put(free[i % len(free)], name)
        used.add(free[i % len(free)])
    if q - 1 not in used or len(free) > len(P):
        for name in P:
            put(q - 1, name)
        used.add(q - 1)
    if foreign is not None:
        r = free[len(P) % len(free)]
        cols, cell = [int(kept[A + 2] - 1)] if mask[kept[A + 2] - 1] else [int(kept[A] - 1)], 20
        queries[r, cols[0]] = queries[r, kept[cell]] = foreign
        where["foreign"] = [(r, cols, [cell])]
        used.add(r)
    ident = np.flatnonzero(mask)
    for r in range(q):
        if r not in used:
            hit = ident[rng.random(len(ident)) < 0.01]
            queries[r, hit] = np.where(rng.random(len(hit)) < 0.5, private, [other(b) for b in row0[hit]]).astype(np.uint8)
    return where


def check_planted(queries, row0, mask, where, listed, tile):
    """every pattern the case is listed for is in its rows: the exception columns are exceptions of the row (and, for a whole-row
    pattern, all of them), the uncovered cells carry a symbol row 0's column does not"""
    exc = exceptions_of(queries, mask, row0)
    kept = np.flatnonzero(~mask)
    for name in listed:
        if name == "min_len_larger":
            continue
        assert where.get(name), name
        for r, cols, cells in where[name]:
            got = set(exc[r].tolist())
            assert set(cols) <= got, (name, r)
            if name in ("none", "every"):
                assert len(got) == (0 if name == "none" else int(mask.sum())), name
            if name == "run":
                assert any(c + 1 in got for c in cols)
            if name == "around_kept":
                assert cols[1] - cols[0] == 2 and not mask[cols[0] + 1]
            if name == "uncovered_then_exc":
                assert kept[cells[0]] < cols[0] < kept[cells[0] + 1]
            if name == "stage_border":
                assert cols == [STAGE - 1, STAGE]
            if name == "ends":
                assert cols == [0, len(mask) - 1]
            if name == "tile_border":                                # the last gap of a tile, the gap across the border, the first gap behind it
                assert kept[tile - 2] < cols[0] < kept[tile - 1] < cols[1] < kept[tile] < cols[2] < kept[tile + 1]
            if name == "min_len_gap":                                # room for a close of 50 columns on either side, inside the gap
                assert cols[0] - kept[G - 1] > 51 and kept[G] - cols[0] > 56


def largest_gap(mask):
    kept = np.flatnonzero(~mask)
    return int(np.diff(np.r_[-1, kept, len(mask)]).max() - 1)


# ---- the small cases of the CPU test: name -> layout, query rows and what the case is listed for
SIGMA = 4
ALL_PLACES = PLACES
CASES = {
    "one-row":    dict(q=1, n_kept=70, tile=64, layout={}, listed=ALL_PLACES),
    "rows":       dict(q=14, n_kept=70, tile=64, layout={}, listed=("none", "every", "foreign") + ALL_PLACES),
    "tile-51":    dict(q=3, n_kept=60, tile=51, layout=dict(first=0, last=0), listed=("none", "every", "run", "around_kept", "uncovered_then_exc", "tile_border", "min_len_gap")),
    "short-gaps": dict(q=6, n_kept=70, tile=64, layout=dict(first=3, long_gap=0, last=1), listed=("none", "every", "ends", "run", "around_kept", "uncovered_then_exc", "tile_border", "min_len_larger")),
}


def small_case(name):
    """-> dict(msa: the reconstruction's rows [m, n_src], mask, kept, founders: reduced [K, kept], queries [q, n_src], where)"""
    c = CASES[name]
    rng = np.random.default_rng(sum(name.encode()))
    mask = layout(rng, c["n_kept"], c["tile"], **c["layout"])
    msa, founders, kept = rm.planted_case(rng, 6, len(mask), 4, SIGMA, mask)
    queries = msa[rng.integers(0, 6, size=c["q"])].copy()
    private, foreign = 48 + SIGMA, 0x7E
    where = plant(rng, queries, msa[0], mask, c["tile"], private, lambda b: 48 + (int(b) - 48 + 1) % SIGMA, foreign if "foreign" in c["listed"] else None)
    return dict(msa=msa, mask=mask, kept=kept, founders=founders, queries=queries, where=where)
