"""Structured alignments for the segmentation path: inputs whose ORACLE RESULT has a shape that mosaics of a few founders
plus noise never have -- thousands of distinct divergence values, tracebacks of one segment per column, identity stretches
of thousands of columns, recombination exactly on block borders, rows that differ in one column, periodic keys.

Every generator is deterministic (fixed seeds) and returns a C-contiguous uint8 (m, n) array; numpy and the oracle's
generator only, no GPU.  FAMILIES lists, per family, the shape it is run at, the segment-length bound, the block length of
the run that uses the family's own (0: the library's plan) and what the oracle returns for it: tests/test_structured_inputs.py
holds every generator to these figures on the CPU, tests/test_gpu_structured_inputs.py runs them on the device."""
import numpy as np

import fso

SYMS = np.frombuffer(b"ACGT", dtype=np.uint8)


def _random_row(rng, n):
    return SYMS[rng.integers(0, 4, size=n)]


def _next_symbol(x):
    return SYMS[(np.searchsorted(SYMS, x) + 1) & 3]


def staircase(m=5000, n=5400, step=1, c0=200, seed=101):
    """One random row copied m times; row r carries the next symbol in column c0 + r * step only; rows shuffled.  Behind the
    last mutation the rows are pairwise different and every divergence value is another column."""
    assert step >= 1 and c0 + (m - 1) * step < n
    rng = np.random.default_rng(seed)
    msa = np.tile(_random_row(rng, n), (m, 1))
    r = np.arange(m)
    cols = c0 + r * step
    msa[r, cols] = _next_symbol(msa[r, cols])
    return np.ascontiguousarray(msa[rng.permutation(m)])


def staircase_wide():
    return staircase(m=3000, n=9400, step=3, c0=100, seed=102)


def _mosaic(seed, m, n):
    return np.ascontiguousarray(fso.synth_msa(fso.synth_spec(seed, 6, 80, 3e-3), m, n))


def lead_identity(m=70, n=12000, cols=9000, seed=3):
    """A mosaic whose first `cols` columns are row 0's in every row: the first real boundary lies far behind them."""
    msa = _mosaic(seed, m, n)
    msa[:, :cols] = msa[0, :cols]
    return msa


def trail_identity(m=300, n=12000, cols=9000, seed=4):
    """A mosaic whose last `cols` columns are row 0's in every row: the divergences stay thousands of columns behind."""
    msa = _mosaic(seed, m, n)
    msa[:, n - cols:] = msa[0, n - cols:]
    return msa


def counter(m=4096, n=600, period=10):
    """Symbol of (r, j) = bit (j mod period) of r, as A / C.  period = 10: 1,024 distinct rows, four exact copies of each, and
    an order that is reshuffled in every column; period = 13: all 4,096 rows differ (no reduction)."""
    r = np.arange(m)[:, None]
    j = np.arange(n)[None, :] % period
    return np.ascontiguousarray(SYMS[(r >> j) & 1])


def counter_all_distinct():
    return counter(period=13)


def sweep(m=700, n=3000, seed=105):
    """One random row copied m times; column k carries the next symbol in row k mod m only: one row moves per column."""
    rng = np.random.default_rng(seed)
    msa = np.tile(_random_row(rng, n), (m, 1))
    k = np.arange(n)
    msa[k % m, k] = _next_symbol(msa[k % m, k])
    return np.ascontiguousarray(msa)


def uniform_rows(m, n, seed):
    return np.ascontiguousarray(SYMS[np.random.default_rng(seed).integers(0, 4, size=(m, n))])


def every_column_a_segment():
    """16 uniform random rows at L = 1: the optimum cuts behind every column."""
    return uniform_rows(16, 20000, 106)


def every_other_column():
    """40 uniform random rows at L = 2: a segment every two columns."""
    return uniform_rows(40, 17000, 107)


BORDER_B = 50


def border_cuts(n, B=BORDER_B):
    cuts = {0, n} | set(range(0, n, B)) | {b - 1 for b in range(3 * B, n, 3 * B)} | {b + 1 for b in range(2 * B, n, 5 * B)}
    return sorted(cuts)


def border_recombination(m=600, n=3000, K=7, seed=108):
    """K random founders; every row draws its founder again at every multiple of B = 50, one column in front of every third
    and one behind every fifth (from the second) block border: the classes change exactly on, before and behind borders."""
    rng = np.random.default_rng(seed)
    founders = SYMS[rng.integers(0, 4, size=(K, n))]
    msa = np.empty((m, n), dtype=np.uint8)
    cuts = border_cuts(n)
    for lo, hi in zip(cuts[:-1], cuts[1:]):
        msa[:, lo:hi] = founders[rng.integers(0, K, size=m), lo:hi]
    return msa


PERIOD = 37


def periodic(m=512, n=2000):
    """Symbol of (r, j) = a fixed hash of (j + r) mod 37 into ACGT: rows r and r + 37 are equal, and the keys of a block
    repeat with a period that divides no block length.  The hash, (3 x >> 2) & 3, has runs of one and two equal symbols:
    22 of the 37 cyclic shifts differ over ten columns (a random table of 37 symbols makes all 37 differ over any ten
    columns, and the optimum is then the one segment [0, n))."""
    x = np.arange(PERIOD)
    table = SYMS[((3 * x) >> 2) & 3]
    r = np.arange(m)[:, None]
    j = np.arange(n)[None, :]
    return np.ascontiguousarray(table[(j + r) % PERIOD])


def halving_merge():
    """Founders without noise, L = 3: the greedy merge joins half of the traceback's boundaries."""
    return np.ascontiguousarray(fso.synth_msa(fso.synth_spec(10, 4, 1000, 0.0), 200, 17000))


def halving_merge_l1():
    return np.ascontiguousarray(fso.synth_msa(fso.synth_spec(13, 4, 300, 0.0), 40, 17000))


def long_merge(m=48, n=17000, B=12, split=8400, tail=48):
    """A traceback of more than 1,000 segments of which the greedy merge removes more than half.  Noise-free mosaics that
    recombine every B = 12 columns: two founders in [0, split), three in [split, n - tail) -- the optimum of every prefix cuts
    at every stretch (sizes 2 and 3) --, then `tail` columns in which the rows fall into nine classes that any two columns tell
    apart: the maximum segment size of the whole is 9, and the merge joins three stretches of two founders (8 <= 9 < 16) and
    two of three (9 < 27)."""
    msa = np.empty((m, n), dtype=np.uint8)
    msa[:, :split] = fso.synth_msa(fso.synth_spec(10, 2, B, 0.0), m, split)
    msa[:, split:] = fso.synth_msa(fso.synth_spec(11, 3, B, 0.0), m, n, c0=0)[:, split:]
    v = np.arange(m)[:, None] % 9
    j = np.arange(tail)[None, :] % 2
    msa[:, n - tail:] = SYMS[np.where(j == 0, v % 3, v // 3)]
    return msa


# name: (generator, L, block length of the family's own run (0: the library's plan),
#        oracle: status, max_segment_size, traceback length, merged length)
FAMILIES = {
    "staircase": (staircase, 100, 0, (0, 101, 50, 50)),
    "staircase_wide": (staircase_wide, 40, 0, (0, 15, 215, 215)),
    "lead_identity": (lead_identity, 12, 0, (0, 13, 111, 104)),
    "trail_identity": (trail_identity, 12, 0, (0, 26, 159, 156)),
    "counter": (counter, 16, 0, (0, 1024, 1, 1)),
    "counter_all_distinct": (counter_all_distinct, 16, 0, (1, 4096, 1, 0)),
    "sweep": (sweep, 20, 0, (0, 21, 150, 150)),
    "every_column_a_segment": (every_column_a_segment, 1, 0, (0, 4, 20000, 20000)),
    "every_other_column": (every_other_column, 2, 0, (0, 16, 8500, 8500)),
    "border_recombination": (border_recombination, 25, BORDER_B, (0, 28, 60, 60)),
    "periodic": (periodic, 10, 0, (0, 22, 200, 200)),
    "halving_merge": (halving_merge, 3, 0, (0, 4, 33, 17)),
    "halving_merge_l1": (halving_merge_l1, 1, 0, (0, 4, 113, 57)),
    "long_merge": (long_merge, 2, 0, (0, 9, 1414, 591)),
}
