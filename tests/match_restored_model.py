"""The gap step of the restored match (fseq_match_founders_restored, csrc/fseq_match.hpp) in plain Python: the loop of
match_model.match_row over the kept columns only, at their source positions, with the identity columns between two kept
columns accounted for in a closed form.  It rests on one property: in an identity column every restored founder carries
row 0's byte (identity_model.restore), as every row does, so a founder set passes such a column unchanged.

tests/test_match_restored_abi.py pins match_row_restored to match_model.match_row on the full-length rows and the
full-length restored founders, so the closed form hangs on the host tool as match_row does."""
import numpy as np

import identity_model as im


def match_row_restored(seq, founders, kept, n_src, min_len):
    """seq: the row at the kept columns; founders: K sequences over the kept columns; kept: the source position of every kept
    column, ascending; n_src: columns of the source.
    -> (pieces [(lb, rb, [founder indices])] in source co-ordinates, uncovered cells, short pieces)"""
    K = len(founders)
    out, uncovered, short = [], 0, 0
    cur = list(range(K))
    lb = 0

    def gap(g_lo, g_hi):
        """the identity columns [g_lo, g_hi)"""
        nonlocal cur, lb, short
        if g_lo >= g_hi:
            return
        if not cur:                                       # the kept cell before was uncovered: no founder is left at g_lo either
            if min_len and g_lo - lb < min_len:
                short += 1
            out.append((lb, g_lo, []))
            lb, cur = g_lo, list(range(K))
        if min_len:
            closes = (g_hi - lb - 1) // min_len           # closes at lb + i * min_len < g_hi, i = 1 ..
            for i in range(closes):
                out.append((lb, lb + min_len, list(cur)))
                lb, cur = lb + min_len, list(range(K))

    g_lo = 0
    for j, c in enumerate(seq):
        pos = int(kept[j])
        gap(g_lo, pos)
        g_lo = pos + 1
        # match_model.match_row's step, pos the source position
        recheck = False
        if min_len and min_len <= pos - lb:
            recheck = True
        else:
            dst = [f for f in cur if founders[f][j] == c]
            if not dst:
                if min_len and pos - lb < min_len:
                    short += 1
                recheck = True
        if recheck:
            out.append((lb, pos, list(cur)))
            lb = pos
            dst = [f for f in range(K) if founders[f][j] == c]
            if not dst:
                uncovered += 1
        cur = dst
    gap(g_lo, n_src)
    if cur:
        out.append((lb, n_src, list(cur)))
    return out, uncovered, short


def planted_case(rng, m, n_src, K, sigma, mask, uncovered_at=()):
    """Rows over sigma symbols ('0' on) that are identity columns exactly where mask says (every other column has a row
    that differs from row 0), K founders over the kept columns that are mosaics of the rows with a few foreign bytes, and
    cells listed in uncovered_at = [(row, kept index)] whose symbol no founder keeps there.
    -> (msa [m, n_src], reduced founders [K, kept], kept columns)"""
    alpha = np.arange(48, 48 + sigma, dtype=np.uint8)
    msa = alpha[rng.integers(0, sigma, size=(m, n_src))]
    msa[:, mask] = msa[0:1, mask]
    kept = np.flatnonzero(~mask)
    for k in kept:
        if (msa[:, k] == msa[0, k]).all():
            msa[int(rng.integers(1, m)), k] = alpha[(int(msa[0, k]) - 48 + 1) % sigma]
    red = im.reduce_rows(msa, mask)
    nk = len(kept)
    founders = np.empty((K, nk), dtype=np.uint8)
    for f in range(K):
        pos = 0
        while pos < nk:
            step = int(rng.integers(1, max(2, nk // 2) + 1))
            founders[f, pos:pos + step] = red[int(rng.integers(m)), pos:pos + step]
            pos += step
    if nk:
        founders[int(rng.integers(K)), int(rng.integers(nk))] = ord("-")     # (a slot without a row prints '-')
    for r, j in uncovered_at:
        hit = founders[:, j] == red[r, j]
        founders[hit, j] = alpha[(int(red[r, j]) - 48 + 1) % sigma]
    return msa, founders, kept
