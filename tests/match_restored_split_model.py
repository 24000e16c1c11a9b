"""The specification of the restored match walk split along the kept columns (csrc/fseq_match.hpp, k_match_walk_split with
RST / EXC), in numpy over the rows, and the table of cases the CPU test (tests/test_match_restored_split_model.py) proves and
the GPU test (tests/test_gpu_match_restored_split.py) takes every expected count from.

The walk is match_exceptions_model.match_row_merged's: the kept columns at their source positions, the row's own exception
columns between them, the identity columns in between in match_restored_model's closed form.  Here it is cut into segments.

plan          match_split_model.plan over the KEPT columns: G segments with the bounds c_g, cold starts s_g = c_g - overlap, both
              kept indices.  Segment g owns the source positions [P_g, P_{g+1}): P_0 = 0, P_g = kept[c_g], P_G = n_src.
cold_walk     the merged walk from kept index s up to P_{g+1}.  cold (every segment but the first): lb = last = kept[s], all
              founders live, the row's exceptions below kept[s] skipped.  Otherwise from source position 0.  Every close sets
              `last`; a close at source position p is kept (and its uncovered cell / short piece counted) only by the segment that
              owns p.  head is `last` on reaching kept index c_lo, after the exceptions and the gap in front of it; tail is
              `last` behind the gap that ends at P_{g+1}.  Only the last segment emits the piece that ends at n_src.
split_match   all segments' walks; a row STANDS iff head[g] == tail[g - 1] for every g >= 1; a row that does not stand takes its
              pieces from the walk of one segment (the device falls back by groups of 256 rows).

Why a standing row's pieces are the true walk's: after a close at source position p the state is lb = p and a live set that
depends on p and the row alone -- set[p][code] at a kept column, the empty set at an exception column, all founders at any other
identity column (the close behind an uncovered cell, every forced min_len close in a gap) -- and a cold start at kept[s] is the
state of a close there.  From head[g] == tail[g - 1] = x both walks are in the state of a close at x, x lies where walk g - 1 is
the true walk (induction from segment 0), so walk g is the true walk from x on."""
import numpy as np

import identity_model as im
import match_split_model as sm

GROUP = sm.GROUP


def plan(n_kept, G, overlap):
    """match_split_model.plan over the kept columns"""
    return sm.plan(n_kept, G, overlap)


class _Tables:
    def __init__(self, queries_full, founders_kept, mask, row0):
        self.mask = np.asarray(mask, dtype=bool)
        self.kept = np.flatnonzero(~self.mask).astype(np.int64)
        self.n_src, self.n_kept = len(self.mask), len(self.kept)
        q = np.asarray(queries_full, dtype=np.uint8)
        assert q.shape[1] == self.n_src and np.asarray(founders_kept).shape[1] == self.n_kept
        self.cols = sm._Tables(np.ascontiguousarray(q[:, ~self.mask]), founders_kept)          # the sets of the kept columns
        self.m, self.K, self.W, self.full = self.cols.m, self.cols.K, self.cols.W, self.cols.full
        # the exception cells, by source position: rows exc_rows[exc_at[p] : exc_at[p + 1]] differ from row 0 in identity column p
        exc = self.mask[None, :] & (q != np.asarray(row0, dtype=np.uint8)[None, :])
        pos, rows = np.nonzero(exc.T)
        self.exc_rows = rows.astype(np.int64)
        self.exc_at = np.searchsorted(pos, np.arange(self.n_src + 1))
        self.exc_pos = np.unique(pos).astype(np.int64)


def cold_walk(T, min_len, s, c_lo, c_hi, cold):
    """the walk over the kept indices [s, c_hi) and on to P = kept[c_hi] (c_hi = n_kept: n_src), the closes owned from kept index
    c_lo on.  -> dict(rows, lb, rb, sets: the closes kept and, where c_hi = n_kept, the last piece; uncovered, short [m]; head, tail [m])"""
    m, kept, n_src = T.m, T.kept, T.n_src
    p_lo = int(kept[s]) if cold else 0
    p_hi = n_src if c_hi == T.n_kept else int(kept[c_hi])
    live = np.tile(T.full, (m, 1))
    lb = np.full(m, p_lo, dtype=np.int64)
    last = lb.copy()
    head = lb.copy()
    src_next = lb.copy()
    uncovered = np.zeros(m, dtype=np.int64)
    short = np.zeros(m, dtype=np.int64)
    rec = {"rows": [], "lb": [], "rb": [], "sets": []}
    everyone = np.arange(m)
    empty = np.zeros((1, T.W), dtype="<u4")
    mine = not cold

    def emit(rows, rb):
        rec["rows"].append(rows)
        rec["lb"].append(lb[rows].copy())
        rec["rb"].append(np.broadcast_to(np.asarray(rb, dtype=np.int64), rows.shape).copy())
        rec["sets"].append(live[rows].copy())

    def gap(rows, g_hi):                                          # the identity columns [src_next, g_hi) of `rows`
        rows = rows[src_next[rows] < g_hi]
        if not len(rows):
            return
        dead = rows[~live[rows].any(axis=1)]
        if len(dead):                                             # the cell before was uncovered: no founder is left at g_lo either
            g_lo = src_next[dead]
            if mine:
                if min_len:
                    short[dead] += g_lo - lb[dead] < min_len
                emit(dead, g_lo)
            lb[dead] = last[dead] = g_lo
            live[dead] = T.full
        if min_len:
            closes = (g_hi - lb[rows] - 1) // min_len             # closes at lb + i * min_len < g_hi, i = 1 ..
            i = 0
            while True:
                go = rows[closes > i]
                if not len(go):
                    break
                if mine:
                    emit(go, lb[go] + min_len)
                lb[go] += min_len
                last[go] = lb[go]
                live[go] = T.full
                i += 1

    def step(rows, p, M):                                         # match_model.match_rows' step at source position p
        forced = (p - lb[rows] >= min_len) if min_len else np.zeros(len(rows), dtype=bool)
        dst = live[rows] & M
        dead = ~forced & ~dst.any(axis=1)
        if min_len and mine:
            short[rows] += dead
        sel = forced | dead
        re = rows[sel]
        if len(re):
            Mre = np.broadcast_to(M, dst.shape)[sel]
            if mine:
                emit(re, p)
                uncovered[re] += ~Mre.any(axis=1)
            lb[re] = last[re] = p
            dst[sel] = Mre
        live[rows] = dst
        src_next[rows] = p + 1

    def exceptions(lo, hi):                                       # the exception cells at the source positions [lo, hi)
        a, b = np.searchsorted(T.exc_pos, [lo, hi])
        for p in T.exc_pos[a:b].tolist():
            rows = T.exc_rows[T.exc_at[p]:T.exc_at[p + 1]]
            gap(rows, p)
            step(rows, p, empty)

    at = p_lo
    for j in range(s, c_hi):
        p = int(kept[j])
        exceptions(at, p)
        gap(everyone, p)
        if j == c_lo:
            head = last.copy()
            mine = True
        c = T.cols
        step(everyone, p, c.masks[j][c.slot[c.msa[:, j]]])
        at = p + 1
    exceptions(at, p_hi)
    gap(everyone, p_hi)
    if c_hi == T.n_kept:
        rest = np.flatnonzero(live.any(axis=1))
        if len(rest):
            emit(rest, n_src)
    cat = lambda k, dt, shape=(0,): np.concatenate(rec[k]) if rec[k] else np.zeros(shape, dtype=dt)
    return {"rows": cat("rows", np.int64), "lb": cat("lb", np.int64), "rb": cat("rb", np.int64), "sets": cat("sets", "<u4", (0, T.W)),
            "uncovered": uncovered, "short": short, "head": head, "tail": last}


def split_match(queries_full, founders_kept, mask, row0, min_len, G, overlap):
    """-> dict(pieces, sets, uncovered_cells, short_pieces, max_pieces_per_row: as match_model.match_rows on the full-length data;
    stands [m] bool; split: what match_split() reports -- segments, overlap (kept columns), row_groups, flagged_groups,
    rows_not_standing; flagged: the groups)"""
    T = _Tables(queries_full, founders_kept, mask, row0)
    m = T.m
    G, ov, c, s = plan(T.n_kept, G, overlap)
    walks = [cold_walk(T, min_len, s[g], c[g], c[g + 1], g > 0) for g in range(G)]
    stands = np.ones(m, dtype=bool)
    for g in range(1, G):
        stands &= walks[g]["head"] == walks[g - 1]["tail"]
    parts = [sm._only(w, stands) for w in walks]
    unc = sum(int(w["uncovered"][stands].sum()) for w in walks)
    short = sum(int(w["short"][stands].sum()) for w in walks)
    if not stands.all():
        whole = cold_walk(T, min_len, 0, 0, T.n_kept, False)
        parts.append(sm._only(whole, ~stands))
        unc += int(whole["uncovered"][~stands].sum())
        short += int(whole["short"][~stands].sum())
    pieces, sets, most = sm._assemble(m, parts)
    groups = (m + GROUP - 1) // GROUP
    flagged = sorted(set((np.flatnonzero(~stands) // GROUP).tolist()))
    return {"pieces": pieces, "sets": sets, "uncovered_cells": unc, "short_pieces": short, "max_pieces_per_row": most, "stands": stands,
            "split": {"segments": G, "overlap": ov, "row_groups": groups, "flagged_groups": len(flagged), "rows_not_standing": int((~stands).sum())},
            "flagged": flagged}


# ---- inputs.  A case is dict(queries [q, n_src], founders [K, n_kept], mask [n_src], row0 [n_src]): the K founders restored
# (identity_model.restore) are an alignment whose identity columns are exactly `mask`, so the GPU test makes the context of them.
ALPHA = np.frombuffer(b"ACG", dtype=np.uint8)                     # the reconstruction's symbols
PRIVATE = ord("N")                                                # a symbol only query rows have: an exception, an uncovered cell
LONG = 80                                                         # a gap of more than 2 x the largest min_len of the tests (37)
MIN_LENS = (0, 3, 37)


def layout(rng, n_kept, G, overlap, lead=5, trail=90, draw=(0, 0, 1, 2, 7)):
    """-> mask.  gaps[j] identity columns in front of kept column j, gaps[n_kept] behind the last.  Around every bound c_g and
    every cold start s_g: LONG identity columns in front of the kept column and LONG behind it, and two behind kept[c_g - 1]."""
    _, _, c, s = plan(n_kept, G, overlap)
    gaps = rng.choice(np.array(draw), size=n_kept + 1)
    gaps[0], gaps[n_kept] = lead, trail
    for j in c[1:-1] + s[1:]:
        if 0 < j < n_kept:
            gaps[j] = gaps[j + 1] = LONG
    return np.concatenate([np.r_[np.ones(g, dtype=bool), False] for g in gaps[:n_kept]] + [np.ones(gaps[n_kept], dtype=bool)])


def finish(rng, founders, mask, queries_kept, alpha=ALPHA):
    """the full-length case of founders and queries over the kept columns: every kept column gets a second symbol among the
    founders (it is no identity column of the restored founders), row 0 random in the identity columns"""
    founders = np.array(founders, dtype=np.uint8)
    for k in np.flatnonzero((founders == founders[0:1]).all(axis=0)):
        founders[1, k] = alpha[(int(np.flatnonzero(alpha == founders[0, k])[0]) + 1) % len(alpha)]
    row0 = np.empty(len(mask), dtype=np.uint8)
    row0[mask] = alpha[rng.integers(0, len(alpha), size=int(mask.sum()))]
    row0[~mask] = founders[0]
    queries = np.repeat(row0[None, :], len(queries_kept), axis=0)
    queries[:, ~mask] = queries_kept
    assert np.array_equal(im.identity_mask(im.restore(founders, mask, row0)), mask)
    return dict(queries=queries, founders=founders, mask=mask, row0=row0)


def mosaic_rows(rng, founders, q, flips=0.02, alpha=ALPHA):
    """q rows that are mosaics of the founders with a few point changes"""
    K, n = founders.shape
    rows = np.empty((q, n), dtype=np.uint8)
    for r in range(q):
        pos = 0
        while pos < n:
            step = int(rng.integers(1, max(2, n // 3) + 1))
            rows[r, pos:pos + step] = founders[int(rng.integers(K)), pos:pos + step]
            pos += step
    hit = rng.random(rows.shape) < flips
    rows[hit] = alpha[rng.integers(0, len(alpha), size=int(hit.sum()))]
    return rows


def mosaic_case(seed, q, n_kept, K, G, overlap, exceptions=0.01):
    """mosaic queries of K random founders; exceptions in `exceptions` of every row's identity columns but row 0's, which has
    none, and row 1's, which has one in every identity column; uncovered kept cells in column 0 and the last one"""
    rng = np.random.default_rng(seed)
    mask = layout(rng, n_kept, G, overlap)
    founders = ALPHA[rng.integers(0, len(ALPHA), size=(K, n_kept))]
    case = finish(rng, founders, mask, np.zeros((q, n_kept), dtype=np.uint8))
    queries = case["queries"]
    queries[:, ~mask] = mosaic_rows(rng, case["founders"], q)
    kept = np.flatnonzero(~mask)
    queries[0, kept[0]] = queries[q - 1, kept[-1]] = PRIVATE
    hit = mask[None, :] & (rng.random(queries.shape) < exceptions)
    hit[0] = False
    hit[1] = mask
    queries[hit] = PRIVATE
    return case


PLANTED = ("none", "every", "exc c_g-1", "exc c_g+1", "exc s_g-1", "exc s_g+1", "run across P_g", "ends", "uncovered c_g-1",
           "uncovered c_g-1 c_g")


def planted_case(seed, n_kept, K, G, overlap, g=None):
    """Four rows per entry of PLANTED (40 in all; row r carries entry r % 10), each changing between founder 0 and founder 1 every
    50, 43, 61 or 37 kept columns (a close at every change:
    several in every overlap, none within 10 kept columns of a bound or a cold start), with what is planted around the bound c_g
    and the cold start s_g of segment g (default: the middle one), all of which lie between gaps of LONG identity columns (layout):
    exceptions at kept[c_g] -+ 1 and at kept[s_g] -+ 1 (where the cursor's search can be off by one), a run of four across
    P_g = kept[c_g], at source 0 and n_src - 1; an uncovered kept cell at index c_g - 1 with identity columns behind it (its close
    at kept[c_g - 1] + 1 belongs to segment g - 1), and that one followed by another at c_g; a row with no exception, a row with
    one in every identity column."""
    rng = np.random.default_rng(seed)
    Ge, _, c, s = plan(n_kept, G, overlap)
    g = max(1, Ge // 2) if g is None else g
    mask = layout(rng, n_kept, G, overlap)
    founders = ALPHA[rng.integers(0, len(ALPHA), size=(K, n_kept))]
    founders[1] = ALPHA[(np.searchsorted(ALPHA, founders[0]) + 1) % len(ALPHA)]        # founder 1 differs from founder 0 everywhere
    case = finish(rng, founders, mask, np.zeros((4 * len(PLANTED), n_kept), dtype=np.uint8))
    queries, kept, n_src = case["queries"], np.flatnonzero(~mask), len(mask)
    for v, period in enumerate((50, 43, 61, 37)):
        turns = [j for j in range(period, n_kept, period) if min(abs(j - x) for x in c + s) > 10]
        base = case["founders"][0].copy()
        for a, b in zip(turns[0::2], turns[1::2] + [n_kept]):
            base[a:b] = case["founders"][1, a:b]
        queries[v * len(PLANTED):(v + 1) * len(PLANTED), ~mask] = base
    at = {"none": [], "every": np.flatnonzero(mask).tolist(), "exc c_g-1": [kept[c[g]] - 1], "exc c_g+1": [kept[c[g]] + 1],
          "exc s_g-1": [kept[s[g]] - 1], "exc s_g+1": [kept[s[g]] + 1], "run across P_g": [kept[c[g]] + d for d in (-2, -1, 1, 2)],
          "ends": [0, n_src - 1], "uncovered c_g-1": [], "uncovered c_g-1 c_g": []}
    for r in range(len(queries)):
        name = PLANTED[r % len(PLANTED)]
        cols = np.array(at[name], dtype=np.int64)
        assert mask[cols].all(), name
        queries[r, cols] = PRIVATE
        if name.startswith("uncovered"):
            queries[r, kept[c[g] - 1:c[g] + (name == "uncovered c_g-1 c_g")]] = PRIVATE
    assert kept[c[g]] - kept[c[g] - 1] > 1                        # identity columns behind the uncovered cell
    case["where"] = {name: r for r, name in enumerate(PLANTED)}
    return case


def periodic_case(seed, q, n_kept, G, overlap, P=17):
    """match_split_model.periodic_case over the kept columns: rows of all 'A' against P founders of which founder f carries 'C' at
    the kept columns congruent to f mod P; no exceptions.  Every walk closes every P - 1 kept columns in the phase of its start."""
    rng = np.random.default_rng(seed)
    mask = layout(rng, n_kept, G, overlap)
    founders = np.full((P, n_kept), ord("A"), dtype=np.uint8)
    for f in range(P):
        founders[f, f::P] = ord("C")
    return finish(rng, founders, mask, np.full((q, n_kept), ord("A"), dtype=np.uint8))


def mixed_case(seed, n_kept, G, overlap, P=17):
    """600 rows of which only 256 .. 511 are periodic_case's; the others are random over {A, C}, close every few columns and
    carry exceptions in 1 % of their identity columns."""
    case = periodic_case(seed, 600, n_kept, G, overlap, P)
    rng = np.random.default_rng(seed + 1)
    queries, mask = case["queries"], case["mask"]
    other = np.r_[0:256, 512:600]
    sub = queries[other]
    sub[:, ~mask] = np.frombuffer(b"AC", dtype=np.uint8)[rng.integers(0, 2, size=(len(other), n_kept))]
    sub[mask[None, :] & (rng.random(sub.shape) < 0.01)] = PRIVATE
    queries[other] = sub
    return case


def long_piece_case(seed, n_kept, G, overlap):
    """Row 0 is founder 0 over all columns (one piece longer than any segment + overlap); row 2 is row 0 with one exception in the
    middle of the source; row r of the other 38 alternates between the two founders every 5 + r kept columns."""
    rng = np.random.default_rng(seed)
    mask = layout(rng, n_kept, G, overlap)
    founders = np.frombuffer(b"AC", dtype=np.uint8)[:, None].repeat(n_kept, axis=1)
    rows = founders[[0] * 40].copy()
    for r in [1] + list(range(3, 40)):
        rows[r, (np.arange(n_kept) // (5 + r)) % 2 == 1] = ord("C")
    case = finish(rng, founders, mask, rows)
    ident = np.flatnonzero(mask)
    case["queries"][2, ident[len(ident) // 2]] = PRIVATE
    return case


# ---- the cases.  build() -> case; G, overlap (kept columns); expect: "all stand", "none stands", "some" or the list of flagged
# groups, at the min_lens of expect_at (the pieces equal the unsplit walk's at every one of MIN_LENS); why: what it is listed for.
# The mosaics of 40 founders and more are listed as standing at min_len = 0 only: their row 0 has no exception and follows one
# founder for hundreds of columns, so with min_len != 0 nearly all its closes are forced ones in the phase of the walk's start,
# and two walks meet only at a point change that empties both live sets (with 5 founders that is every point change).
# The planted rows are listed at 0 and 37: at min_len = 3 no live set narrows to the one founder a row follows before the next
# forced close, so whether both walks close at a change of founders is left to the four random founders.
CASES = {
    "mosaic K=5": dict(build=lambda: mosaic_case(201, 40, 2000, 5, 5, 300), G=5, overlap=300, expect="all stand", expect_at=MIN_LENS,
                       why="WR = 1; a row without exceptions, a row with one in every identity column; a leading and a trailing gap"),
    "mosaic K=40": dict(build=lambda: mosaic_case(202, 40, 2000, 40, 4, 400), G=4, overlap=400, expect="all stand", expect_at=(0,), why="WR = 2"),
    "mosaic K=70": dict(build=lambda: mosaic_case(203, 257, 2400, 70, 3, 700), G=3, overlap=700, expect="all stand", expect_at=(0,),
                        why="WR = 4; 257 rows: two groups"),
    "mosaic K=200": dict(build=lambda: mosaic_case(204, 40, 2100, 200, 8, 256), G=8, overlap=256, expect="all stand", expect_at=(0,), why="WR = 8"),
    "mosaic K=300": dict(build=lambda: mosaic_case(205, 40, 2000, 300, 2, 512), G=2, overlap=512, expect="all stand", expect_at=(0,),
                         why="live sets in LDS"),
    "planted": dict(build=lambda: planted_case(206, 2000, 6, 5, 300), G=5, overlap=300, expect="all stand", expect_at=(0, 37),
                    why="exceptions at kept[c_g] -+ 1 and kept[s_g] -+ 1, a run across P_g, source 0 and n_src - 1; the uncovered cell at "
                        "c_g - 1 whose close belongs to segment g - 1; gaps of more than 2 min_len in front of and behind kept[c_g] and "
                        "around kept[s_g]"),
    "planted last": dict(build=lambda: planted_case(207, 2000, 6, 4, 256, g=3), G=4, overlap=256, expect="all stand", expect_at=(0, 37),
                         why="the same around the last segment's bound"),
    "periodic": dict(build=lambda: periodic_case(208, 40, 2050, 7, 280), G=7, overlap=280, expect="none stands", expect_at=(0,),
                     why="none stands: every group goes through the G = 1 fall-back of the new instantiations"),
    "mixed groups": dict(build=lambda: mixed_case(209, 2050, 7, 280), G=7, overlap=280, expect=[1], expect_at=(0,),
                         why="600 rows of which exactly group 1 is flagged"),
    "long piece": dict(build=lambda: long_piece_case(210, 2050, 7, 280), G=7, overlap=280, expect=[0], expect_at=(0,),
                       why="a piece longer than any segment + overlap"),
    "G = n_kept": dict(build=lambda: mosaic_case(211, 40, 70, 5, 70, 1, exceptions=0.05), G=70, overlap=1, expect="some", expect_at=(0,),
                       why="G clamped to n_kept: 70 kept columns, G = 70, overlap 1"),
}


def check_expectation(name, got, min_len):
    """the case's listed condition on a split_match result"""
    if min_len not in CASES[name]["expect_at"]:
        return
    expect, stands = CASES[name]["expect"], got["stands"]
    if expect == "all stand":
        assert stands.all(), "%s: %d rows do not stand" % (name, int((~stands).sum()))
    elif expect == "none stands":
        assert not stands.any(), name
    elif expect == "some":
        assert stands.any() and not stands.all(), name
    else:
        assert got["flagged"] == expect, (name, got["flagged"])
