"""The specification of the device matcher (fseq_match_founders / fseq_match_founder_rows), three times:

match_row      the host tool's loop (host/match_founder_sequences.cpp:103-147; tests/test_aux_cli.py restates it as
               _match_oracle), one row at a time in plain Python, with the tool's two error lines counted: uncovered cells
               ("not found in the founders", once per cell) and short pieces ("under the given limit").  This is the definition.
match_rows     the same loop for all rows at once, numpy over the rows and bit sets over the founders: what the GPU tests
               compare with at sizes plain Python cannot walk.  tests/test_match_abi.py pins it to match_row.
match_row_fast min_len = 0 only, one row of a large input: piece by piece (K x window compares) instead of cell by cell.

The CPU test pins match_row to the built host tool, so everything here hangs on the yardstick."""
import numpy as np


def match_row(seq, founders, min_len):
    """-> (pieces [(lb, rb, [founder indices])], uncovered cells, short pieces)"""
    K = len(founders)
    out, uncovered, short = [], 0, 0
    cur = list(range(K))
    lb, count, pos = 0, K, 0
    for c in seq:
        recheck = False
        if min_len and min_len <= pos - lb:
            recheck = True
        else:
            dst = [f for f in cur if founders[f][pos] == c]
            if not dst:
                if min_len and pos - lb < min_len:
                    short += 1
                recheck = True
        if recheck:
            out.append((lb, pos, list(cur)))
            lb = pos
            cur = list(range(K))
            dst = [f for f in cur if founders[f][pos] == c]
            if not dst:
                uncovered += 1
        count, cur = len(dst), dst
        pos += 1
    if count:
        out.append((lb, pos, list(cur)))
    return out, uncovered, short


def sets_to_lists(sets):
    """[P, W] uint32 founder sets -> list of index lists"""
    bits = np.unpackbits(np.ascontiguousarray(sets, dtype="<u4").view(np.uint8).reshape(len(sets), -1), axis=1, bitorder="little")
    return [np.flatnonzero(b).tolist() for b in bits]


def match_rows(msa, founders, min_len):
    """msa [m, n], founders [K, n] uint8 -> dict(pieces: record array (lb, rb, row, n_founders) by row, then lb; sets [P, W]
    uint32; uncovered_cells, short_pieces, max_pieces_per_row)"""
    msa = np.asarray(msa, dtype=np.uint8)
    founders = np.asarray(founders, dtype=np.uint8)
    m, n = msa.shape
    K = founders.shape[0]
    W = (K + 31) // 32
    full = np.zeros(W * 32, dtype=np.uint8)
    full[:K] = 1
    full = np.packbits(full, bitorder="little").view("<u4")
    # sets[c][b]: the founders with byte b at column c, for the bytes the rows have
    present = np.unique(msa)
    slot = np.full(256, len(present), dtype=np.int64)
    slot[present] = np.arange(len(present))
    eq = np.zeros((n, len(present) + 1, W * 32), dtype=np.uint8)
    for i, b in enumerate(present):
        eq[:, i, :K] = (founders == b).T
    masks = np.packbits(eq, axis=2, bitorder="little").view("<u4")          # [n, present + 1, W]; the last slot is empty
    live = np.tile(full, (m, 1))
    lb = np.zeros(m, dtype=np.int64)
    uncovered = np.zeros(m, dtype=np.int64)
    short = np.zeros(m, dtype=np.int64)
    rec_row, rec_lb, rec_rb, rec_set = [], [], [], []

    def emit(rows, rb):
        rec_row.append(rows)
        rec_lb.append(lb[rows].copy())
        rec_rb.append(np.full(len(rows), rb, dtype=np.int64))
        rec_set.append(live[rows].copy())

    for c in range(n):
        M = masks[c][slot[msa[:, c]]]                                        # [m, W]
        forced = (c - lb >= min_len) if min_len else np.zeros(m, dtype=bool)
        dst = live & M
        dead = ~forced & ~dst.any(axis=1)
        if min_len:
            short += dead                                                    # (c - lb < min_len holds for every row that was compared)
        re = np.flatnonzero(forced | dead)
        if len(re):
            emit(re, c)
            lb[re] = c
            dst[re] = M[re]
            uncovered[re] += ~M[re].any(axis=1)
        live = dst
    rest = np.flatnonzero(live.any(axis=1))
    if len(rest):
        emit(rest, n)
    rows = np.concatenate(rec_row) if rec_row else np.zeros(0, dtype=np.int64)
    lbs = np.concatenate(rec_lb) if rec_row else np.zeros(0, dtype=np.int64)
    rbs = np.concatenate(rec_rb) if rec_row else np.zeros(0, dtype=np.int64)
    sets = np.concatenate(rec_set) if rec_row else np.zeros((0, W), dtype="<u4")
    order = np.lexsort((rbs, lbs, rows))                                     # ([0, 0) comes before [0, 1))
    pieces = np.zeros(len(rows), dtype=[("lb", "<u8"), ("rb", "<u8"), ("row", "<u4"), ("n_founders", "<u4")])
    pieces["lb"], pieces["rb"], pieces["row"] = lbs[order], rbs[order], rows[order]
    sets = np.ascontiguousarray(sets[order], dtype="<u4")
    pieces["n_founders"] = np.unpackbits(sets.view(np.uint8).reshape(len(sets), -1), axis=1).sum(axis=1) if len(sets) else 0
    per_row = np.bincount(rows, minlength=m) if len(rows) else np.zeros(m, dtype=np.int64)
    return {"pieces": pieces, "sets": sets, "uncovered_cells": int(uncovered.sum()), "short_pieces": int(short.sum()),
            "max_pieces_per_row": int(per_row.max()) if m else 0}


def match_row_fast(row, founders, window=2048):
    """min_len = 0: -> (pieces [(lb, rb, founder index array)], uncovered cells).  A piece runs to the farthest first mismatch
    of any founder from lb on; an uncovered cell gives a one-column piece with no founder (none in the last column), and one
    in column 0 first closes [0, 0) with every founder."""
    row = np.asarray(row, dtype=np.uint8)
    founders = np.asarray(founders, dtype=np.uint8)
    K, n = founders.shape
    out, uncovered, lb = [], 0, 0
    if not (founders[:, 0] == row[0]).any():
        out.append((0, 0, np.arange(K)))
    while lb < n:
        ends = np.full(K, lb, dtype=np.int64)
        going = np.arange(K)
        at, win = lb, window
        while len(going) and at < n:
            hi = min(n, at + win)
            ne = founders[going, at:hi] != row[at:hi]
            first = np.where(ne.any(axis=1), ne.argmax(axis=1), hi - at)
            ends[going] = at + first
            going = going[first == hi - at]
            at, win = hi, win * 2
        e = int(ends.max())
        if e == lb:
            uncovered += 1
            if lb + 1 < n:
                out.append((lb, lb + 1, np.zeros(0, dtype=np.int64)))
            lb += 1
        else:
            out.append((lb, e, np.flatnonzero(ends == e)))
            lb = e
    return out, uncovered


def mosaic_case(seed, m, n, K, sigma, uncovered=True):
    """Random founders over sigma symbols (printable bytes from '0' on), rows that are mosaics of them with a few point
    changes, one foreign byte in the founders, and -- uncovered -- cells whose symbol no founder has: one in column 0, one
    in the last column, two adjacent ones (where n has the room)."""
    rng = np.random.default_rng(seed)
    alpha = np.arange(48, 48 + sigma, dtype=np.uint8)
    founders = alpha[rng.integers(0, sigma, size=(K, n))]
    msa = np.zeros((m, n), dtype=np.uint8)
    for r in range(m):
        pos = 0
        while pos < n:
            step = int(rng.integers(1, max(2, n // 3) + 1))
            msa[r, pos:pos + step] = founders[int(rng.integers(K)), pos:pos + step]
            pos += step
    flips = rng.random((m, n)) < 0.02
    msa[flips] = alpha[rng.integers(0, sigma, size=int(flips.sum()))]
    for k, b in enumerate(alpha):                         # every symbol occurs in the rows where they have the room: the alphabet
        if not (msa == b).any() and k < m * n:            # (and with it the packing) is sigma's
            msa[(m * n - 1 - k) // n, (m * n - 1 - k) % n] = b
    founders[int(rng.integers(K)), int(rng.integers(n))] = 0x7E      # a byte outside the alphabet: matches nothing
    if uncovered:
        cells = [(0, 0), (m - 1, n - 1)]
        if n >= 5:
            cells += [(m // 2, n // 2), (m // 2, n // 2 + 1)]
        for r, c in cells:                                # no founder keeps the row's symbol at this column
            hit = founders[:, c] == msa[r, c]
            founders[hit, c] = alpha[(int(msa[r, c]) - 48 + 1) % sigma]
    return msa, founders
