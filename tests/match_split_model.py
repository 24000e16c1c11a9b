"""The specification of the matcher's walk split along the columns (csrc/fseq_match.hpp, k_match_walk_split), in numpy over
the rows, and the table of cases the CPU test (tests/test_match_split_model.py) proves and the GPU test
(tests/test_gpu_match_rows.py) takes every expected count from.

plan          G segments with the bounds c_g = floor(g n / G), G clamped to [1, min(n, 4096)]; the cold start of segment g >= 1
              is s_g = c_g - clamp(overlap, 1, c_g - c_{g-1}), s_0 = 0 (match_split_plan / mt_seg_bound / mt_seg_start).
cold_walk     the loop of match_model.match_rows from column s with lb = s and all founders live up to column c_hi, keeping of the
              closes only those at columns >= c_lo, and `last`, the column of the latest close (s before any): head is `last` on
              reaching c_lo, tail is `last` behind c_hi - 1.
split_match   all segments' walks.  A row STANDS iff head[g] == tail[g - 1] for every g >= 1.  The result takes a standing
              row's pieces from the split walks and every other row's from the unsplit walk (the device falls back by groups of
              256 rows, which is the same pieces if the claim below holds), and reports what fseq_debug_match_split reports.

Why a standing row's pieces are the true walk's: after a close at column k the walk's state is lb = k, live = set[k][code], a
function of k and the row alone (forced closes of min_len != 0 included), and a cold start at s is the state of a close at s.  If
head[g] == tail[g - 1] = x then x >= s_g >= c_{g-1} lies where walk g - 1 is the true walk (induction from segment 0, which is
the true walk), both walks are in the state of a close at x, and walk g is the true walk from x on, so over all of [c_g, c_{g+1})."""
import numpy as np

import match_model as mm

GROUP = 256                     # rows of a workgroup (MT_T)
SPLIT_MAX = 4096                # MT_SPLIT_MAX


def plan(n, G, overlap):
    """-> (G in use, overlap in use (0 where G = 1), bounds c[0 .. G], starts s[0 .. G - 1])"""
    G = max(1, min(int(G), SPLIT_MAX, n))
    c = [g * n // G for g in range(G + 1)]
    s = [0] + [c[g] - max(1, min(int(overlap), c[g] - c[g - 1])) for g in range(1, G)]
    longest = (n + G - 1) // G
    return G, (max(1, min(int(overlap), longest)) if G > 1 else 0), c, s


class _Tables:
    def __init__(self, msa, founders):
        self.msa = np.asarray(msa, dtype=np.uint8)
        founders = np.asarray(founders, dtype=np.uint8)
        self.m, self.n = self.msa.shape
        self.K = K = founders.shape[0]
        self.W = W = (K + 31) // 32
        full = np.zeros(W * 32, dtype=np.uint8)
        full[:K] = 1
        self.full = np.packbits(full, bitorder="little").view("<u4")
        present = np.unique(self.msa)
        self.slot = np.full(256, len(present), dtype=np.int64)
        self.slot[present] = np.arange(len(present))
        eq = np.zeros((self.n, len(present) + 1, W * 32), dtype=np.uint8)
        for i, b in enumerate(present):
            eq[:, i, :K] = (founders == b).T
        self.masks = np.packbits(eq, axis=2, bitorder="little").view("<u4")      # [n, present + 1, W]; the last slot is empty


def cold_walk(T, min_len, s, c_lo, c_hi):
    """-> dict(rows, lb, rb, sets: the closes at columns in [c_lo, c_hi) and, where c_hi = n, the last piece; uncovered, short
    [m]: counted at those closes only; head, tail [m])"""
    m, n = T.m, T.n
    live = np.tile(T.full, (m, 1))
    lb = np.full(m, s, dtype=np.int64)
    last = np.full(m, s, dtype=np.int64)
    head = last.copy()
    uncovered = np.zeros(m, dtype=np.int64)
    short = np.zeros(m, dtype=np.int64)
    rec = {"rows": [], "lb": [], "rb": [], "sets": []}

    def emit(rows, rb):
        rec["rows"].append(rows)
        rec["lb"].append(lb[rows].copy())
        rec["rb"].append(np.full(len(rows), rb, dtype=np.int64))
        rec["sets"].append(live[rows].copy())

    for c in range(s, c_hi):
        if c == c_lo:
            head = last.copy()
        mine = c >= c_lo
        M = T.masks[c][T.slot[T.msa[:, c]]]
        forced = (c - lb >= min_len) if min_len else np.zeros(m, dtype=bool)
        dst = live & M
        dead = ~forced & ~dst.any(axis=1)
        if min_len and mine:
            short += dead
        re = np.flatnonzero(forced | dead)
        if len(re):
            if mine:
                emit(re, c)
                uncovered[re] += ~M[re].any(axis=1)
            lb[re] = c
            last[re] = c
            dst[re] = M[re]
        live = dst
    if c_hi == n:
        rest = np.flatnonzero(live.any(axis=1))
        if len(rest):
            emit(rest, n)
    cat = lambda k, dt, shape=(0,): np.concatenate(rec[k]) if rec[k] else np.zeros(shape, dtype=dt)
    return {"rows": cat("rows", np.int64), "lb": cat("lb", np.int64), "rb": cat("rb", np.int64), "sets": cat("sets", "<u4", (0, T.W)),
            "uncovered": uncovered, "short": short, "head": head, "tail": last}


def _assemble(m, parts):
    """pieces of the walks in `parts` (each restricted to the rows it is taken for) in the device's order: row, then lb, [k, k)
    in front of [k, k + 1)"""
    rows = np.concatenate([p["rows"] for p in parts])
    lbs = np.concatenate([p["lb"] for p in parts])
    rbs = np.concatenate([p["rb"] for p in parts])
    sets = np.concatenate([p["sets"] for p in parts])
    order = np.lexsort((rbs, lbs, rows))
    pieces = np.zeros(len(rows), dtype=[("lb", "<u8"), ("rb", "<u8"), ("row", "<u4"), ("n_founders", "<u4")])
    pieces["lb"], pieces["rb"], pieces["row"] = lbs[order], rbs[order], rows[order]
    sets = np.ascontiguousarray(sets[order], dtype="<u4")
    pieces["n_founders"] = np.unpackbits(sets.view(np.uint8).reshape(len(sets), -1), axis=1).sum(axis=1) if len(sets) else 0
    per_row = np.bincount(rows, minlength=m) if len(rows) else np.zeros(m, dtype=np.int64)
    return pieces, sets, int(per_row.max()) if m else 0


def _only(walk, keep):
    sel = keep[walk["rows"]]
    return {"rows": walk["rows"][sel], "lb": walk["lb"][sel], "rb": walk["rb"][sel], "sets": walk["sets"][sel]}


def split_match(msa, founders, min_len, G, overlap):
    """-> dict(pieces, sets, uncovered_cells, short_pieces, max_pieces_per_row: as match_model.match_rows; stands [m] bool;
    split: what match_split() reports -- segments, overlap, row_groups, flagged_groups, rows_not_standing; flagged: the groups)"""
    T = _Tables(msa, founders)
    m, n = T.m, T.n
    G, ov, c, s = plan(n, G, overlap)
    walks = [cold_walk(T, min_len, s[g], c[g], c[g + 1]) for g in range(G)]
    stands = np.ones(m, dtype=bool)
    for g in range(1, G):
        stands &= walks[g]["head"] == walks[g - 1]["tail"]
    parts = [_only(w, stands) for w in walks]
    unc = sum(int(w["uncovered"][stands].sum()) for w in walks)
    short = sum(int(w["short"][stands].sum()) for w in walks)
    if not stands.all():
        whole = cold_walk(T, min_len, 0, 0, n)
        parts.append(_only(whole, ~stands))
        unc += int(whole["uncovered"][~stands].sum())
        short += int(whole["short"][~stands].sum())
    pieces, sets, most = _assemble(m, parts)
    groups = (m + GROUP - 1) // GROUP
    flagged = sorted(set((np.flatnonzero(~stands) // GROUP).tolist()))
    return {"pieces": pieces, "sets": sets, "uncovered_cells": unc, "short_pieces": short, "max_pieces_per_row": most, "stands": stands,
            "split": {"segments": G, "overlap": ov, "row_groups": groups, "flagged_groups": len(flagged), "rows_not_standing": int((~stands).sum())},
            "flagged": flagged}


# ---- inputs

def periodic_case(m, n, P=17):
    """Rows of all 'A' against P founders of which founder s carries 'B' at the columns congruent to s mod P: every walk closes
    every P - 1 columns in the phase of its start, so two walks whose starts differ by no multiple of P - 1 never share a close."""
    rows = np.full((m, n), ord("A"), dtype=np.uint8)
    founders = np.full((P, n), ord("A"), dtype=np.uint8)
    for f in range(P):
        founders[f, f::P] = ord("B")
    return rows, founders


def mixed_case(seed, n, P=17):
    """600 rows of which only 256 .. 511 are periodic_case's; the others are random over {A, B} and close every few columns."""
    rows, founders = periodic_case(600, n, P)
    rng = np.random.default_rng(seed)
    other = np.r_[0:256, 512:600]
    rows[other] = np.frombuffer(b"AB", dtype=np.uint8)[rng.integers(0, 2, size=(len(other), n))]
    return rows, founders


def long_piece_case(n):
    """Row 0 is founder 0 over all columns (one piece longer than any segment + overlap: no walk behind the first can know its
    lb); row 1 alternates between the two founders every 5 columns."""
    founders = np.frombuffer(b"AC", dtype=np.uint8)[:, None].repeat(n, axis=1)
    rows = founders[[0, 0]].copy()
    rows[1, (np.arange(n) // 5) % 2 == 1] = ord("C")
    return rows, founders


def planted_case(n, G, overlap, sigma=4, K=6, seed=11):
    """Seven rows that follow founder 0, each with a close (a symbol only founder 1 has) or an uncovered cell (a symbol no founder
    has) at one of the columns where the split can go wrong: s_g, c_g - 1, c_g of the middle segment, column 0, column n - 1; and
    two adjacent uncovered cells across c_g."""
    rng = np.random.default_rng(seed)
    alpha = np.arange(48, 48 + sigma, dtype=np.uint8)
    Ge, _, c, s = plan(n, G, overlap)
    g = max(1, Ge // 2) if Ge > 1 else 0
    spots = sorted({0, n - 1, s[g], max(c[g] - 1, 0), min(c[g], n - 1)})
    founders = alpha[rng.integers(0, sigma - 1, size=(K, n))]             # (the last symbol is kept out of the founders)
    founders[1] = alpha[(founders[0] - 48 + 1) % (sigma - 1)]            # founder 1 differs from founder 0 everywhere (sigma >= 3)
    rows = []
    for k in spots:
        r = founders[0].copy()
        r[k] = founders[1, k]
        rows.append(r)                                                    # a close at k
        r = founders[0].copy()
        r[k] = alpha[sigma - 1]
        rows.append(r)                                                    # an uncovered cell at k
    r = founders[0].copy()
    r[max(c[g] - 1, 0)] = alpha[sigma - 1]
    r[min(c[g], n - 1)] = alpha[sigma - 1]
    rows.append(r)
    return np.array(rows, dtype=np.uint8), founders


# ---- the cases.  build() -> (rows, founders); G, overlap, min_lens; expect: "all stand", "none stands", "some" (rows of either
# kind in one run) or the list of flagged groups
CASES = {
    "mosaic K=5": dict(build=lambda: mm.mosaic_case(101, 70, 4000, 5, 4), G=5, overlap=700, min_lens=(0, 37), expect="all stand"),
    "mosaic K=40": dict(build=lambda: mm.mosaic_case(102, 70, 4000, 40, 4), G=5, overlap=700, min_lens=(0, 37), expect="all stand"),
    "mosaic K=70": dict(build=lambda: mm.mosaic_case(103, 300, 6000, 70, 4), G=5, overlap=700, min_lens=(0, 37), expect="all stand"),
    "mosaic K=300": dict(build=lambda: mm.mosaic_case(104, 64, 4096, 300, 16), G=5, overlap=700, min_lens=(0, 37), expect="all stand"),
    "short overlap": dict(build=lambda: mm.mosaic_case(103, 300, 6000, 70, 4), G=8, overlap=256, min_lens=(0,), expect="some"),
    "periodic": dict(build=lambda: periodic_case(40, 4099), G=7, overlap=300, min_lens=(0,), expect="none stands"),
    "periodic aligned": dict(build=lambda: periodic_case(40, 4099), G=2, overlap=2049, min_lens=(0,), expect="all stand"),
    "mixed groups": dict(build=lambda: mixed_case(7, 4099), G=7, overlap=300, min_lens=(0,), expect=[1]),
    "long piece": dict(build=lambda: long_piece_case(4099), G=7, overlap=300, min_lens=(0,), expect=[0]),
}


def check_expectation(name, got):
    """the case's listed condition on a split_match result"""
    expect, stands = CASES[name]["expect"], got["stands"]
    if expect == "all stand":
        assert stands.all(), "%s: %d rows do not stand" % (name, int((~stands).sum()))
    elif expect == "none stands":
        assert not stands.any(), name
    elif expect == "some":
        assert stands.any() and not stands.all(), name
    else:
        assert got["flagged"] == expect, (name, got["flagged"])
