"""Inputs with an exactly known number of representatives R in a block that the DP and pass 2 read, for R on both sides of every
capacity of the reduced column kernel k_columns_red<T, E, 4, PK, EW> (csrc/fseq_reduced.hpp; the configurations are
FSEQ_RED_CONFIGS, csrc/fseq_reduced.hip).  tests/test_reduced_capacity_cases.py holds every case to what is said here on the
CPU, from the oracle alone; tests/test_gpu_reduced_capacities.py runs them.  numpy and the oracle only, no GPU.

Every case is two_halves() at n = 1,300 columns, L = 602, blocks of 100 columns, c = 687:
  * R row types and m - R exact copies of them.  A block that starts in front of column L - 2 is exact (vmin = 1): it has one
    representative per distinct row over [0, k1).  The types are R - 1 distinct rows over [0, 600) and R over [0, 700), so
    blocks 0 to 5 have R - 1 representatives and block 6 = [600, 700), the last exact one, has exactly R.
  * The left parts [0, c) and the right parts [c, n) are R - 1 distinct rows each, and every other cut in [L, n - L] =
    [602, 698] leaves R on one side: the optimum is the one boundary at column 687, inside block 6 and not on its border.
    Pass 2 has one task there, which starts from the reduced stride state phase C dropped at column 672.
  * `pairs` pairs of types agree on [0, c) but for one column below `span` = 80, so the lists of block 6 hold dozens of
    distinct values below the threshold k + 2 - L: 34 to 40 at column 640, 65 to 81 at column 686 -- more than the default
    list capacity of 63, an open list.
  * 10 R <= 7 m: plan_reduced (csrc/fseq_redplan.hpp) sends a block with more representatives than 70 % of the rows to all rows.
    m is the least such row count rounded up to a multiple of 50, so R > 7,884 means m > 11,264: streamed rows.

The expected configurations are written BY HAND from FSEQ_RED_CONFIGS, as thresholds (PHASE_C, PASS_2) and again row by row
in the table; nothing here asks the library.  At blocks of 100 columns every configuration fits the 160 KiB of LDS at every row
count and symbol width of the table (the largest, 1024 x 10 and 1024 x 12, leave 19,816 bytes for each of the two staged
columns; a staged column is at most 11,264 bytes -- 8-bit symbols of 11,264 LDS-resident rows -- or the 11,520 of the
configuration's own rows when the rows stream), so no entry deviates from the first configuration that holds R."""
import numpy as np

import fso

N, L, BLOCK, C = 1300, 602, 100, 687
SPAN = 80
BLOCK_UNDER_TEST = 6
DEFAULT_LIST_CAP = 63
RED_CAP = 11264                         # red_plan's cap: more representatives run on all rows
STREAMED_FROM = 11265                   # rows from which the block order streams

SYMS = {
    2: b"ACGT",
    4: b"ACDEFGHIKLMNPQRS",                                   # 16 letters: 4 bits per stored symbol
    8: b"0123456789ABCDEFGHIJKLMNOPQRSTUVWXYZacgt",           # 40 letters: 8 bits
}

# (most representatives, threads, rows per thread) in the order of FSEQ_RED_CONFIGS: the first line that holds R runs.
# Phase C: the one-wave configurations and those with a list wave, (T - 64) x E rows.
PHASE_C = ((192, 64, 3), (320, 64, 5), (448, 64, 7), (576, 256, 3), (960, 256, 5), (2240, 512, 5), (3136, 512, 7), (4800, 1024, 5),
           (6720, 512, 15), (7680, 1024, 8), (8640, 1024, 9), (9600, 1024, 10), (10560, 1024, 11), (11264, 1024, 12))
# Pass 2's class-table sweeps: the configurations without a list wave, T x E rows.
PASS_2 = ((192, 64, 3), (320, 64, 5), (448, 64, 7), (768, 256, 3), (1280, 256, 5), (2560, 512, 5), (3584, 512, 7), (5120, 1024, 5),
          (7168, 1024, 7), (9216, 1024, 9), (10240, 1024, 10), (11264, 1024, 11))


def rows_of(T, E, list_wave):
    """Rows a configuration holds -- what the library's plan report calls `configuration of N rows`."""
    return (T - 64) * E if list_wave else T * E


def phase_c_of(R):
    """(T, E, rows) of the phase-C configuration for R representatives by the thresholds above (None: all rows).  1024 x 12
    holds 11,520 rows; the plan's cap keeps it to 11,264."""
    for most, T, E in PHASE_C:
        if R <= most:
            return (T, E, rows_of(T, E, T > 64))
    return None


def pass_2_of(R):
    for most, T, E in PASS_2:
        if R <= most:
            return (T, E, rows_of(T, E, False))
    return None


# (R, m, phase C's (T, E), pass 2's (T, E)) -- None for phase C: block 6 runs on all rows beside the reduced blocks 0 to 5; None
# for pass 2: the boundary's state is replayed on all rows from the block's start
TABLE_2_BITS = (
    (192, 300, (64, 3), (64, 3)), (193, 300, (64, 5), (64, 5)),
    (320, 500, (64, 5), (64, 5)), (321, 500, (64, 7), (64, 7)),
    (448, 650, (64, 7), (64, 7)), (449, 650, (256, 3), (256, 3)),
    (576, 850, (256, 3), (256, 3)), (577, 850, (256, 5), (256, 3)),
    (768, 1100, (256, 5), (256, 3)), (769, 1100, (256, 5), (256, 5)),
    (960, 1400, (256, 5), (256, 5)), (961, 1400, (512, 5), (256, 5)),
    (1280, 1850, (512, 5), (256, 5)), (1281, 1850, (512, 5), (512, 5)),
    (2240, 3200, (512, 5), (512, 5)), (2241, 3250, (512, 7), (512, 5)),
    (2560, 3700, (512, 7), (512, 5)), (2561, 3700, (512, 7), (512, 7)),
    (3136, 4500, (512, 7), (512, 7)), (3137, 4500, (1024, 5), (512, 7)),
    (3584, 5150, (1024, 5), (512, 7)), (3585, 5150, (1024, 5), (1024, 5)),
    (4800, 6900, (1024, 5), (1024, 5)), (4801, 6900, (512, 15), (1024, 5)),
    (5120, 7350, (512, 15), (1024, 5)), (5121, 7350, (512, 15), (1024, 7)),
    (6720, 9600, (512, 15), (1024, 7)), (6721, 9650, (1024, 8), (1024, 7)),
    (7168, 10250, (1024, 8), (1024, 7)), (7169, 10250, (1024, 8), (1024, 9)),
    (7680, 11000, (1024, 8), (1024, 9)), (7681, 11000, (1024, 9), (1024, 9)),
    (8640, 12350, (1024, 9), (1024, 9)), (8641, 12350, (1024, 10), (1024, 9)),
    (9216, 13200, (1024, 10), (1024, 9)), (9217, 13200, (1024, 10), (1024, 10)),
    (9600, 13750, (1024, 10), (1024, 10)), (9601, 13750, (1024, 11), (1024, 10)),
    (10240, 14650, (1024, 11), (1024, 10)), (10241, 14650, (1024, 11), (1024, 11)),
    (10560, 15100, (1024, 11), (1024, 11)), (10561, 15100, (1024, 12), (1024, 11)),
    (11264, 16100, (1024, 12), (1024, 11)), (11265, 16100, None, None),
)
TABLE_WIDER_SYMBOLS = (
    (448, 650, (64, 7), (64, 7)), (449, 650, (256, 3), (256, 3)),
    (2240, 3200, (512, 5), (512, 5)), (2241, 3250, (512, 7), (512, 5)),
    (6720, 9600, (512, 15), (1024, 7)), (6721, 9650, (1024, 8), (1024, 7)),
    (8640, 12350, (1024, 9), (1024, 9)), (8641, 12350, (1024, 10), (1024, 9)),
)
# the 70 % edge: 10 R <= 7 m holds at R = 700 and fails at R = 701, where phase C runs block 6 on all rows (blocks 0 to 5 hold
# 700).  Its representatives are still known (701 is below the plan's cap), and pass 2 sweeps them from the block's start
# (long_pass2_reduced, csrc/fseq_path_pass2.hip: a block on all rows dropped no stride states): 256 x 3 holds 701.
TABLE_SHARE = ((700, 1000, (256, 5), (256, 3)), (701, 1000, None, (256, 3)))


class Case:
    """One row of the table.  name: "<bits>b_<R>" ("share_<R>" for the 70 % edge)."""

    def __init__(self, name, bits, R, m, phase_c, pass_2, least_rows=True):
        self.name, self.bits, self.R, self.m, self.phase_c, self.pass_2 = name, bits, R, m, phase_c, pass_2
        self.least_rows = least_rows                 # m is the least row count with 10 R <= 7 m, rounded up to a multiple of 50
        self.pairs = min(R // 3, 400)
        self.seed = 9000 + 7 * R + bits

    @property
    def on_all_rows(self):
        return self.phase_c is None

    def __repr__(self):
        return "Case(%s: R = %d, m = %d)" % (self.name, self.R, self.m)


def _cases():
    out = [Case("2b_%d" % R, 2, R, m, pc, p2) for R, m, pc, p2 in TABLE_2_BITS]
    out += [Case("%db_%d" % (bits, R), bits, R, m, pc, p2) for bits in (4, 8) for R, m, pc, p2 in TABLE_WIDER_SYMBOLS]
    out += [Case("share_%d" % R, 2, R, m, pc, p2, least_rows=False) for R, m, pc, p2 in TABLE_SHARE]
    return out


CASES = {c.name: c for c in _cases()}

# the child processes of the GPU test: a handful of cases each, ~15 million cells of alignment at the most
GROUPS = {
    "2b_192_to_961": ["2b_%d" % R for R in (192, 193, 320, 321, 448, 449, 576, 577, 768, 769, 960, 961)],
    "2b_1280_to_3137": ["2b_%d" % R for R in (1280, 1281, 2240, 2241, 2560, 2561, 3136, 3137)],
    "2b_3584_to_5121": ["2b_%d" % R for R in (3584, 3585, 4800, 4801, 5120, 5121)],
    "2b_6720_to_7681": ["2b_%d" % R for R in (6720, 6721, 7168, 7169, 7680, 7681)],
    "2b_8640_to_9217": ["2b_%d" % R for R in (8640, 8641, 9216, 9217)],
    "2b_9600_to_10241": ["2b_%d" % R for R in (9600, 9601, 10240, 10241)],
    "2b_10560_to_11265": ["2b_%d" % R for R in (10560, 10561, 11264, 11265)],
    "4b_448_to_2241": ["4b_%d" % R for R in (448, 449, 2240, 2241)],
    "4b_6720_to_8641": ["4b_%d" % R for R in (6720, 6721, 8640, 8641)],
    "8b_448_to_2241": ["8b_%d" % R for R in (448, 449, 2240, 2241)],
    "8b_6720_to_8641": ["8b_%d" % R for R in (6720, 6721, 8640, 8641)],
    "share_700_701": ["share_700", "share_701"],
}


def two_halves(R, m, n, c, seed, pairs, span=SPAN, syms=b"ACGT"):
    """R row types over `syms` and m - R exact copies, shuffled.  Returns (rows, types, type of every row).

    The types are pairwise different: columns span .. span + 7 and n - 8 .. n - 1 spell the type's number.  `pairs` pairs of
    types (2 i + 1, 2 i + 2) are equal on [0, c) but for column (7 i) mod span.  The last type is type 0 on [0, c) and
    differs from it in column c: the left parts are R - 1 distinct rows.  The last but one is type 0 on [c, n) and differs
    from it in column c - 1: so are the right parts."""
    assert R >= 8 and 2 * pairs + 2 < R - 2 and R <= 4 ** 8 and span + 8 <= c - 1 and c + 1 <= n - 8 and m >= R
    S = np.frombuffer(syms, dtype=np.uint8)
    q = len(S)
    rng = np.random.default_rng(seed)
    code = rng.integers(0, q, size=(R, n), dtype=np.uint8)
    idx = np.arange(R)
    for j in range(8):
        code[:, span + j] = code[:, n - 1 - j] = (idx >> (2 * j)) & 3
    for i in range(pairs):
        p = (7 * i) % span
        code[2 * i + 2, :c] = code[2 * i + 1, :c]
        code[2 * i + 2, p] = (code[2 * i + 1, p] + 1) % q
    code[R - 1, :c] = code[0, :c]
    code[R - 1, c] = (code[0, c] + 1) % q
    code[R - 2, c:] = code[0, c:]
    code[R - 2, c - 1] = (code[0, c - 1] + 1) % q
    src = np.concatenate([idx, rng.integers(0, R, size=m - R)])
    rng.shuffle(src)
    types = S[code]
    return np.ascontiguousarray(types[src]), types, src


def make(case, with_types=False):
    """The alignment of a case: C-contiguous uint8 (m, n), read-only (with_types: and the R types and every row's type)."""
    rows, types, src = two_halves(case.R, case.m, N, C, case.seed, case.pairs, syms=SYMS[case.bits])
    rows.setflags(write=False)
    return (rows, types, src) if with_types else rows


def expected_list(v, c, k, L):
    """The whole list of column k from the oracle's divergence counts (fso.Pbwt.counts() behind column k): entry 0 lumps the
    values >= k + 2 - L under the value k + 1, the rest are the distinct values below, descending."""
    thr = max(0, k + 2 - L)
    rec = v >= thr
    return np.concatenate([[k + 1], v[~rec][::-1]]), np.concatenate([[c[rec].sum()], c[~rec][::-1]])


def lists_match(ctx, msa, L, every=5, columns=None):
    """The per-column lists a context holds (debug_column_list) against the oracle's pBWT: every `every`-th column and the last
    three, or the given ascending columns.  A list is a prefix of the whole list, cut only behind more than the capacity's
    worth of rows; a complete one carries the count of zeros the DP reads."""
    m, n = msa.shape
    p = fso.Pbwt(msa, debug=False)
    X = ctx.timings()["list_cap_used"]
    last = n if columns is None else max(columns) + 1
    want = None if columns is None else set(columns)
    checked = 0
    for k in range(last):
        p.step()
        if (k % every and k < n - 3) if want is None else k not in want:
            continue
        v, c = p.counts()
        gv, gc, cnt0, complete = ctx.debug_column_list(k)
        ev, ec = expected_list(v, c, k, L)
        assert complete or gc[1:].sum() > X, k
        assert np.array_equal(gv, ev[:len(gv)]) and np.array_equal(gc, ec[:len(gc)]), k
        assert complete == (len(gv) == len(ev)), k
        if complete:
            assert cnt0 == (c[0] if v[0] == 0 else 0), k
        checked += 1
    return checked
