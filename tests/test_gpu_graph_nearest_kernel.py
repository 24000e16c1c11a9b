"""The pack and distance kernels of fseq_graph_nearest_rows (csrc/fseq_graphnearest.hpp) through fseq_debug_graph_nearest: no
context, the production launcher, the caller's segments, class counts and representatives.

The yardstick is numpy on the codes (tests/graph_nearest_model.py's distances(): a comparison, a sum, argmin, a tie count), and the
results must equal it exactly.  The shapes are the smallest at which the kernels can go wrong: segment widths on both sides of a
packed word at every width, a segment above any register cap, rows and queries at different widths with a partial last byte in
every packed column, class counts around a wave, a workgroup and past the threading's cap, query counts around a wave and a tile,
planted ties, and batch budgets that hold everything, one segment and less than one."""
import importlib

import numpy as np
import pytest

import graph_nearest_model as nm

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def pkg():
    return importlib.import_module("founder-sequences_amd")


def model(codes, lb, rb, count, rep, qcodes):
    S, Q = len(lb), len(qcodes)
    out = np.zeros((3, S, Q), dtype=np.uint32)
    for s in range(S):
        reps = codes[np.asarray(rep[s][:count[s]], dtype=np.int64), lb[s]:rb[s]]
        out[0, s], out[1, s], out[2, s] = nm.distances(reps, qcodes[:, lb[s]:rb[s]])
    return out


def tiling(widths):
    rb = np.cumsum(widths)
    return rb - np.asarray(widths), rb


def make(seed, m, widths, counts, Q, sigma, query_sigma=False):
    """Random codes below sigma, segments of the given widths side by side, counts[s] random representative rows a segment, and Q
    queries that are rows with a few codes changed (with query_sigma: some to the code `sigma`)."""
    rng = np.random.default_rng(seed)
    lb, rb = tiling(widths)
    n = int(rb[-1])
    codes = rng.integers(0, sigma, size=(m, n))
    X = max(counts)
    rep = np.zeros((len(widths), X), dtype=np.uint32)
    for s, c in enumerate(counts):
        rep[s, :c] = rng.permutation(m)[:c] if c <= m else rng.integers(0, m, size=c)
    q = codes[rng.integers(0, m, size=Q)].copy()
    hits = rng.random(q.shape) < 0.08
    q[hits] = rng.integers(0, sigma + (1 if query_sigma else 0), size=int(hits.sum()))
    return codes, lb, rb, np.asarray(counts), rep, q


def check(pkg, codes, bits, lb, rb, count, rep, q, qbits, sigma, batch_bytes=None):
    got = pkg.debug_graph_nearest(codes, bits, lb, rb, count, rep, q, qbits, sigma, batch_bytes=batch_bytes, want_info=True)
    want = model(codes, lb, rb, count, rep, q)
    for k, name in enumerate(("classes", "distances", "ties")):
        assert got[k].shape == want[k].shape and np.array_equal(got[k], want[k]), (name, np.argwhere(got[k] != want[k])[:5].tolist())
    assert got[3]["bits"] == qbits
    return got, want


# ---- segment widths on both sides of a packed word; neighbours differ, so a read across a word or a segment border shows

@pytest.mark.parametrize("bits,widths", [(2, [1, 15, 16, 17, 31, 32, 33]), (4, [7, 8, 9]), (8, [3, 4, 5])])
def test_segment_widths(pkg, bits, widths):
    sigma = 1 << bits
    for order in (widths, widths[::-1]):
        codes, lb, rb, count, rep, q = make(bits, 41, order, [6] * len(order), 70, sigma)
        got, want = check(pkg, codes, bits, lb, rb, count, rep, q, bits, sigma)
        per = 32 // bits
        assert got[3]["query_words"] == sum(-(-w // per) for w in order) and got[3]["packed_words"] == 6 * got[3]["query_words"]
        assert (want[1] > 0).any() and (want[1] == 0).any()
    # the same widths one by one, each between two neighbours of other content and at an odd first column
    for w in widths:
        codes, lb, rb, count, rep, q = make(100 + w, 41, [3, w, 2], [4, 5, 3], 20, sigma)
        check(pkg, codes, bits, lb[1:], rb[1:], count[1:], rep[1:], q, bits, sigma)


def test_a_segment_above_the_register_cap(pkg):
    """5,003 columns at 2 bits are 313 words a row: the lanes read their query words again for every class."""
    codes, lb, rb, count, rep, q = make(7, 20, [9, 5003, 17], [3, 5, 4], 67, 4)
    q[3, 9:9 + 5003] = codes[int(rep[1][2]), 9:9 + 5003]                   # an exact copy of class 2's substring
    q[4, 9 + 5002] = (q[3, 9 + 5002] + 1) % 4                                # ... and rows that differ in the segment's last and first column alone
    q[4, 9:9 + 5002] = q[3, 9:9 + 5002]
    q[5, 9:9 + 5003] = q[3, 9:9 + 5003]
    q[5, 9] = (q[3, 9] + 1) % 4
    got, want = check(pkg, codes, 2, lb, rb, count, rep, q, 2, 4)
    assert want[1][1, 3] == 0 and want[1][1, 4] == 1 and want[1][1, 5] == 1 and want[1][1].max() > 1000


# ---- rows and queries at equal and at different widths; m = 41: every packed column ends in a partial byte

@pytest.mark.parametrize("bits,qbits,sigma", [(2, 2, 3), (2, 4, 4), (4, 4, 15), (4, 8, 16), (8, 8, 40)])
def test_width_pairs(pkg, bits, qbits, sigma):
    codes, lb, rb, count, rep, q = make(sigma, 41, [5, 16, 17, 33, 2], [7, 41, 1, 12, 3], 41, sigma, query_sigma=True)
    q[0, :] = sigma                                                          # a query of nothing but bytes outside the alphabet
    got, want = check(pkg, codes, bits, lb, rb, count, rep, q, qbits, sigma)
    assert (q == sigma).sum() > 41 and want[1][:, 0].tolist() == [5, 16, 17, 33, 2] and want[2][:, 0].tolist() == [7, 41, 1, 12, 3] and (want[0][:, 0] == 0).all()


# ---- class counts: a wave, the workgroup's 256 threads of the pack kernel, and past the threading's 4,096

@pytest.mark.parametrize("X", [1, 2, 63, 64, 65, 255, 256, 257, 4097])
def test_class_counts(pkg, X):
    codes, lb, rb, count, rep, q = make(X, min(X + 3, 300), [20, 13], [X, max(1, X // 2)], 37, 4)
    got, want = check(pkg, codes, 2, lb, rb, count, rep, q, 2, 4)
    assert got[3]["packed_words"] == 2 * X + max(1, X // 2)
    if X >= 63:
        assert len(np.unique(want[0][0])) > 10                               # the nearest classes are spread over the table


# ---- query counts: a wave, a tile of 256, packed bytes not filled

@pytest.mark.parametrize("Q", [1, 3, 63, 64, 65, 257])
def test_query_counts(pkg, Q):
    for bits, qbits, sigma in ((2, 2, 4), (2, 4, 4)):
        codes, lb, rb, count, rep, q = make(Q, 23, [8, 33, 16], [5, 9, 2], Q, sigma, query_sigma=qbits > bits)
        check(pkg, codes, bits, lb, rb, count, rep, q, qbits, sigma)


# ---- planted ties

def test_planted_ties(pkg):
    rng = np.random.default_rng(11)
    m, W = 12, 19
    codes = rng.integers(0, 4, size=(m, 2 * W))
    codes[7] = codes[2]                                                      # rows 2 and 7 are one substring twice
    # segment 0: classes 0 .. 3 are the rows 9, 7, 2, 4 -- the duplicates are classes 1 and 2, and class 0's row lies behind theirs
    # segment 1: classes 0 and 1 are the rows 10 and 3: the smaller class is listed second in the rows' memory order
    rep = np.array([[9, 7, 2, 4], [10, 3, 0, 0]], dtype=np.uint32)
    count = np.array([4, 2])
    lb, rb = tiling([W, W])
    q = np.zeros((4, 2 * W), dtype=np.int64)
    q[0] = codes[2]                                                          # distance 0 from both duplicates: class 1, two ties
    q[1] = codes[2]
    q[1, 5] = (q[1, 5] + 1) % 4                                              # distance 1 from both
    # equidistant from the classes 0 and 1 of segment 1: row 10's substring where the two agree, and where they differ half of
    # the columns from each
    differ = np.flatnonzero(codes[10, W:] != codes[3, W:]) + W
    assert len(differ) >= 4
    q[2] = codes[10]
    q[2, differ[len(differ) // 2 * 2:]] = 4                                  # (an odd column out: outside the alphabet, one from both)
    differ = differ[:len(differ) // 2 * 2]
    q[2, differ[::2]] = codes[3, differ[::2]]
    odd = int((q[2, W:] == 4).sum())
    q[3, :] = 4                                                              # nothing but the code sigma
    got, want = check(pkg, codes, 2, lb, rb, count, rep, q, 4, 4)
    classes, dist, ties = got[0], got[1], got[2]
    assert (classes[0, 0], dist[0, 0], ties[0, 0]) == (1, 0, 2) and (classes[0, 1], dist[0, 1], ties[0, 1]) == (1, 1, 2)
    assert (classes[1, 2], dist[1, 2], ties[1, 2]) == (0, len(differ) // 2 + odd, 2)
    assert classes[:, 3].tolist() == [0, 0] and dist[:, 3].tolist() == [W, W] and ties[:, 3].tolist() == [4, 2]


# ---- batches

def test_batches(pkg):
    widths, counts = [5, 40, 16, 17, 90, 1], [3, 9, 2, 7, 4, 6]
    codes, lb, rb, count, rep, q = make(13, 30, widths, counts, 70, 4, query_sigma=True)
    words = [c * -(-w // 8) for w, c in zip(widths, counts)]                 # at 4 bits: 8 codes a word
    whole, want = check(pkg, codes, 2, lb, rb, count, rep, q, 4, 4)
    assert whole[3]["batches"] == 1 and whole[3]["packed_words"] == sum(words)
    for budget, batches in ((4 * sum(words), 1), (4 * max(words), None), (4 * max(words) - 1, None), (4 * min(words), len(widths)), (1, len(widths))):
        got, _ = check(pkg, codes, 2, lb, rb, count, rep, q, 4, 4, batch_bytes=budget)
        assert all(np.array_equal(got[k], whole[k]) for k in range(3))
        first = pkg.graph_nearest_plan_host(lb, rb, count, 4, budget)[1]
        assert got[3]["batches"] == len(first) - 1 and (batches is None or got[3]["batches"] == batches), (budget, got[3])
    assert len(pkg.graph_nearest_plan_host(lb, rb, count, 4, 4 * max(words))[1]) - 1 not in (1, len(widths))     # a budget between the two ends
