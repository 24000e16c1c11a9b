"""Phase A's trie (csrc/fseq_blocktrie.hpp), the slot loop of phase 1: a class's first row of a group registers its word in
direct[] with the look-up itself (compare-and-swaps issued for a batch of rows, one wait), only rows with another word than
their class's take the pair table, and whole groups of columns are fetched without a test per column.

What can go wrong there and shows nowhere else is looked for on small inputs built with numpy:
  * the word 0xFFFFFFFF -- sixteen times code 3 at 2 bits, eight times code 15 at 4 bits -- is the sentinel of direct[] and can
    never be registered: such a row has to reach the pair table.  (At 8 bits the word needs code 255, and an alignment has at
    most 32 letters here -- test_phase_a_trie_on_lds_resident_rows, kind 2 --, so there is no 8-bit case.)
  * one class, whose one registration a level every other lane reads; only first arrivals (every row registers or goes to the
    pair table in the same level); 2 and 64 classes by the row number (the most lanes on one word of direct[] at once);
  * partial last groups (1 and 15 columns) and a partial last word of rows;
  * one streamed input with class columns, the instantiation the benchmark runs.
Every run is compared with the oracle bit for bit (compare_long), every block boundary state with the oracle's pBWT, and the
traceback with a run that does not use the trie (FSEQ_NO_BLOCKTRIE=1).  The trie's workgroup size follows the row count
(blocktrie_threads: 256 threads up to 3,072 rows, 512 up to 6,144, 1,024 beyond), so "at 1,024 threads" means a row count above
6,144 here: the one-class case of 64 rows runs 256 threads, and the first-arrival case of 5,000 rows runs 512 threads, whose pair
table (4,096 slots) it overflows -- every block is given up and the key-space tree ranks it, which is asserted; 6,400 rows are
added for 1,024 threads, where nothing overflows."""
import importlib

import numpy as np
import pytest

import fso
from test_gpu_class_columns import check_class_columns, unpack
from test_gpu_parity import _block_states_match, compare_long, run_gpu

pytestmark = pytest.mark.gpu

ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)
SIGMA16 = np.frombuffer(b"ABCDEFGHIJKLMNOP", dtype=np.uint8)


@pytest.fixture(scope="module")
def pkg():
    return importlib.import_module("founder-sequences_amd")


@pytest.fixture()
def trie(monkeypatch):
    monkeypatch.setenv("FSEQ_BLOCKTRIE_ALWAYS", "1")
    return monkeypatch


def mosaic(seed, m, n, K, mu, sigma=4, seg=40, switch=0.05):
    """Codes [m, n] below sigma: K random founders, a row follows one and changes it with probability `switch` every `seg`
    columns; a cell mutates with probability mu.  Every code occurs (asserted), so code c is the c-th letter of the alphabet."""
    rng = np.random.default_rng(seed)
    founders = rng.integers(0, sigma, size=(K, n))
    nseg = (n + seg - 1) // seg
    choice = np.repeat(rng.integers(0, K, size=m)[:, None], nseg, axis=1)
    sw = rng.random((m, nseg)) < switch
    choice[sw] = rng.integers(0, K, size=int(sw.sum()))
    cols = np.arange(n)
    codes = founders[choice[:, cols // seg], cols[None, :]]
    flips = rng.random((m, n)) < mu
    codes = np.where(flips, (codes + 1) % sigma, codes)
    return codes.astype(np.uint8)


def letters(codes, sigma=4):
    assert len(np.unique(codes)) == sigma                    # (the library packs the rank of a letter among those that occur)
    return (ACGT if sigma == 4 else SIGMA16)[codes]


def classes(codes, k0, k1):
    """distinct rows of the columns [k0, k1)"""
    return len(np.unique(codes[:, k0:k1], axis=0))


def run_and_check(pkg, monkeypatch, msa, L, B, given_up=0):
    """The run against the oracle, every block boundary state against the oracle's pBWT, the traceback against a run without the trie."""
    ctx, _ = compare_long(pkg, msa, L, block_len=B)
    t = ctx.timings()
    assert t["block_len"] == B and t["phase_a_trie_given_up"] == given_up and (given_up or t["phase_a_given_up"] == 0), t
    _block_states_match(ctx, msa)
    tb = ctx.traceback().copy()
    monkeypatch.setenv("FSEQ_NO_BLOCKTRIE", "1")
    assert np.array_equal(run_gpu(pkg, msa, L, block_len=B).traceback(), tb)
    monkeypatch.delenv("FSEQ_NO_BLOCKTRIE")
    return ctx


# ---------------------------------------------------------------- the sentinel word

# where the group of code sigma - 1 lies in block 1 (blocks of B columns, groups of N = 32 / bits columns from the block's first one):
#   first     the block's first group, the last one phase 1 handles: every class of the block meets it
#   partial   the block's partial last group (B = 33: 1 column, B = 47: 15 columns at 2 bits; 1 and 7 at 4 bits), the first one handled, AND
#             the whole group in front of it -- a partial group of the highest code is not the sentinel word, the whole group behind it
#             is, and its rows come with the ids of a partial group
#   twice     the block's last two groups (B = 48: both whole), the first two handled
PLACEMENTS = {
    "first": (48, lambda B, N: (B, B + N)),
    "partial33": (33, lambda B, N: (2 * B - (B % N) - N, 2 * B)),
    "partial47": (47, lambda B, N: (2 * B - (B % N) - N, 2 * B)),
    "twice": (48, lambda B, N: (2 * B - 2 * N, 2 * B)),
}
ROWS = {"every": lambda m: np.arange(m), "second": lambda m: np.arange(1, m, 2), "one": lambda m: np.array([m // 3])}


def sentinel_case(seed, m, bits, place, rows):
    sigma, N = (4, 16) if bits == 2 else (16, 8)
    B, span = PLACEMENTS[place]
    n = 3 * B + 5                                            # (a last block of 5 columns: one partial group by itself)
    codes = mosaic(seed, m, n, 6, 2e-3, sigma)
    k0, k1 = span(B, N)
    sel = ROWS[rows](m)
    codes[sel, k0:k1] = sigma - 1
    # the input is what it claims: the rows that carry the sentinel word in the group(s), and the classes of those groups
    whole = [(a, a + N) for a in range(B, 2 * B - N + 1, N) if a >= k0 and a + N <= k1]
    assert len(whole) == (2 if place == "twice" else 1), whole
    for a, b in whole:
        full = np.flatnonzero((codes[:, a:b] == sigma - 1).all(axis=1))
        assert np.array_equal(full, sel), (a, b, len(full))
        nother = classes(np.delete(codes, sel, axis=0), a, b) if len(sel) < m else 0
        assert classes(codes, a, b) == nother + 1 and (rows == "every") == (nother == 0)
    return letters(codes, sigma), B, (k0, k1), sel


SENTINEL_CASES = (
    [(2, 1001, p, r) for p in PLACEMENTS for r in ROWS]                              # 256 threads, a partial last word of rows
    + [(2, m, p, "second") for m in (4003, 7001) for p in PLACEMENTS]                # 512 and 1,024 threads
    + [(4, 1001, p, r) for p in PLACEMENTS for r in ROWS]
    + [(4, 7001, p, "second") for p in PLACEMENTS])


@pytest.mark.parametrize("bits,m,place,rows", SENTINEL_CASES)
def test_rows_whose_word_is_the_sentinel(pkg, trie, bits, m, place, rows):
    """A group in which rows carry 0xFFFFFFFF: none of them may register it, all of them are one class of the pair table."""
    msa, B, (k0, k1), sel = sentinel_case(100 + bits, m, bits, place, rows)
    ctx = run_and_check(pkg, trie, msa, 8, B)
    # ... and the device holds the highest code there: the words are the sentinel
    packed, pbits = ctx.packed_columns(k0, k1)
    assert pbits == bits and (unpack(packed, bits, m)[:, sel] == (1 << bits) - 1).all()


# ---------------------------------------------------------------- one class, first arrivals, classes by the row number

@pytest.mark.parametrize("m", [64, 6400])
def test_one_class(pkg, trie, m):
    """All rows equal: one registration a level, and every other lane of every wave reads that word (6,400 rows: 1,024 threads)."""
    row = mosaic(7, 1, 150, 1, 0.0)
    msa = letters(np.repeat(row, m, axis=0))
    for k0 in range(0, 150, 16):
        assert classes(msa, k0, min(150, k0 + 16)) == 1
    run_and_check(pkg, trie, msa, 8, 48)


@pytest.mark.parametrize("m,given_up", [(300, 0), (5000, 3), (6400, 0)])
def test_only_first_arrivals(pkg, trie, m, given_up):
    """All rows distinct inside a block's last group, the first one handled: one row registers, every other one goes to the pair table
    in the same level, and from there on every class is one row that registers.  5,000 rows run 512 threads and overflow their
    4,096 pair slots: every block is given up to the key-space tree (the module's docstring)."""
    n, B = 144, 48
    codes = mosaic(8, m, n, 5, 1e-3)
    r = np.arange(m)
    for b in range(n // B):
        for j in range(16):
            codes[:, (b + 1) * B - 16 + j] = (r >> (2 * (j % 8))) & 3      # (the row number in base 4, twice)
        assert classes(codes, (b + 1) * B - 16, (b + 1) * B) == m
    run_and_check(pkg, trie, letters(codes), 8, B, given_up)


@pytest.mark.parametrize("k", [2, 64])
def test_classes_by_row_number(pkg, trie, k):
    """Row r is founder r % k: with 2 classes by row parity half the lanes of a wave, with 64 one lane in 64 of every thread's rows,
    meet on one word of direct[] in one instruction."""
    m, n, B = 4096, 150, 48
    founders = np.random.default_rng(9).integers(0, 4, size=(k, n)).astype(np.uint8)
    codes = founders[np.arange(m) % k]
    for k0 in range(0, n - 15, 16):
        assert classes(founders, k0, k0 + 16) == k and classes(codes, k0, k0 + 16) == k
    run_and_check(pkg, trie, letters(codes), 8, B)


# ---------------------------------------------------------------- partial last groups

@pytest.mark.parametrize("B", [33, 47])
def test_partial_last_groups_and_a_partial_word_of_rows(pkg, trie, B):
    """1,001 rows: the positions behind the last row in a column's last word follow that word's first row; last groups of 1 and of 15
    columns (and a last block of 5), fetched with a test per column where every other group is fetched whole."""
    m, n = 1001, 3 * B + 5
    codes = mosaic(10 + B, m, n, 8, 2e-3)
    assert m % 16 != 0 and B % 16 in (1, 15)
    for b in range(3):
        assert 1 < classes(codes, (b + 1) * B - B % 16, (b + 1) * B) <= 4 ** (B % 16)
        assert classes(codes, b * B, (b + 1) * B) > 8
    run_and_check(pkg, trie, letters(codes), 8, B)


# ---------------------------------------------------------------- streamed rows, class columns

def test_streamed_rows_with_class_columns(pkg, monkeypatch):
    """12,000 streamed rows in blocks of 47 columns: k_blocktrie<2, 1024, true>.  Half the rows carry the sentinel word in the first
    group of block 1; the class columns of two blocks against numpy's distinct rows in co-lex order."""
    monkeypatch.setenv("FSEQ_REDUCED_ALWAYS", "1")
    m, n, B, L = 12000, 200, 47, 10
    codes = mosaic(11, m, n, 12, 3e-4)
    sel = np.arange(1, m, 2)
    codes[sel, B:B + 16] = 3
    assert np.array_equal(np.flatnonzero((codes[:, B:B + 16] == 3).all(axis=1)), sel)
    assert classes(codes, B, B + 16) == classes(codes[0::2], B, B + 16) + 1
    msa = letters(codes)
    ctx = run_and_check(pkg, monkeypatch, msa, L, B)
    assert ctx.timings()["n_blocks"] == 5
    assert check_class_columns(ctx, every=3) == 2            # blocks 0 and 3
    cls, _, nkeys = ctx.class_columns(1)                      # ... and the block with the sentinel group: its key count
    assert cls is not None and nkeys == classes(codes, B, 2 * B)
