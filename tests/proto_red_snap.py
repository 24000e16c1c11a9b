"""Python model of pass 2's sweep form (round 16): the class tables of a block from COLLAPSED divergences.

Claim.  A sweep (tests/proto_reduced.py: the pBWT of a block's representatives, replayed to a boundary column, then the class of
every block key and the divergence in front of every class) uses a divergence v for three things only: its order under max, the
test "inside the block" (v > kblk, kblk the block's first column) and, where that holds, v itself.  The map

    id(v) = 0 if v <= kblk else v - kblk

is monotone, so it commutes with max; "inside" is id >= 1; and v = kblk + id wherever id >= 1.  A pBWT step at column k gives the
first row of every symbol the value k + 1, whose id is k + 1 - kblk: the same step in block-relative columns.  So the sweep may run
on ids from the start -- in 16 bits, a block has at most 4,096 columns -- and a reduced state dropped inside the block is the order
and the ids, two 16-bit arrays.  At the block's first column every divergence is <= kblk: the ids are zeros, whatever the values.

This file states that in numpy over the oracle's pBWT (tests/test_proto_red_snap.py proves it against the sweep on true values, and
tests/test_gpu_class_tables.py holds the kernel to it).  TEST INFRASTRUCTURE (uses oracle/).
"""
import numpy as np

from oracle import fso
import proto_reduced as pr


def collapse(d, kblk):
    """The ids of the divergences d of a state inside (or in front of) the block that starts at column kblk, as 16-bit words."""
    d = np.asarray(d, dtype=np.int64)
    ids = np.where(d > kblk, d - kblk, 0)
    assert ids.max(initial=0) < 65536
    return ids.astype(np.uint16)


def block_case(msa, states, b, B, L, X, vmin=None):
    """Block b of msa (states: the exact (a, d) at every block border): dict with the block's columns [k0, k1), the representatives'
    rows `rows` in start order, their start divergences `d_red`, the packed sub-alignment `sub` (rows x block columns) and
    leaf_of_row (the block key of every row of the alignment, by its rank in the order behind the block)."""
    m, n = msa.shape
    k0, k1 = b * B, min(n, (b + 1) * B)
    a0, d0 = states[b]
    a1, d1 = states[b + 1]
    head = d1 > k0
    head[0] = True
    leaf_of_row = np.zeros(m, dtype=np.int64)
    leaf_of_row[a1] = np.cumsum(head) - 1
    if vmin is None:
        vmin = max(pr.choose_vmin(d0, k0, L, X + X // 4 + 8), 1)
    rows, d_red = pr.reduce_state(a0, d0, a1, d1, vmin)
    return dict(k0=k0, k1=k1, rows=rows, d_red=d_red, sub=np.ascontiguousarray(msa[rows, k0:k1]), leaf_of_row=leaf_of_row, a0=a0, d0=d0)


def tables_true(case, order, d):
    """The class tables from a state of the representatives in true divergences (order: indices into case['rows'])."""
    return pr.class_tables(case["rows"][order], np.asarray(d, dtype=np.int64), case["leaf_of_row"], case["k0"])


def tables_collapsed(case, order, ids):
    """... and from ids: a position starts a class iff its id is at least 1; the divergence in front of the class is kblk + id."""
    ids = np.asarray(ids, dtype=np.int64)
    head = ids >= 1
    assert head[0]                      # (behind at least one column the first position holds that column's value)
    cls_of_entry = np.cumsum(head) - 1
    leaf_of_row = case["leaf_of_row"]
    cls_of_leaf = np.full(int(leaf_of_row.max()) + 1, -1, dtype=np.int64)
    cls_of_leaf[leaf_of_row[case["rows"][order]]] = cls_of_entry
    return cls_of_leaf, (case["k0"] + ids[head]).astype(np.uint32), int(cls_of_entry[-1]) + 1


def sweep_true(case, columns):
    """The tables at the ascending boundary columns (k0 < column <= k1), swept on true values from the block's first column;
    also returns the states passed on the way: {column: (order, d)} for every column in (k0, k1)."""
    k0, k1 = case["k0"], case["k1"]
    p = fso.Pbwt(case["sub"], col0=k0)
    p.set_state(np.arange(len(case["rows"]), dtype=np.uint32), case["d_red"], k0)
    want = set(int(c) for c in columns)
    out, states = {}, {}
    for k in range(k0 + 1, k1 + 1):
        p.step()
        if k < k1:
            states[k] = (p.a, p.d)
        if k in want:
            out[k] = tables_true(case, p.a, p.d)
    return out, states


def sweep_collapsed(case, k_from, order16, ids16, columns):
    """The tables at the ascending boundary columns (k_from < column), swept on ids from the 16-bit state (order16, ids16) at column
    k_from: the pBWT in block-relative columns -- its step at column j hands out j + 1 = the id of column k0 + j + 1."""
    k0 = case["k0"]
    p = fso.Pbwt(case["sub"], col0=0)
    p.set_state(np.asarray(order16, dtype=np.uint32), np.asarray(ids16, dtype=np.uint32), k_from - k0)
    want = set(int(c) for c in columns)
    out = {}
    for k in range(k_from + 1, max(want) + 1):
        p.step()
        if k in want:
            out[k] = tables_collapsed(case, p.a, p.d)
    return out


def start_state16(case):
    """The state a sweep from the block's first column starts from: the representatives in start order, ids all zero (the start
    divergences are not read)."""
    assert (case["d_red"] <= case["k0"]).all()
    return np.arange(len(case["rows"]), dtype=np.uint16), np.zeros(len(case["rows"]), dtype=np.uint16)


def stride_states16(case, states, stride):
    """The reduced states phase C drops: at every multiple of `stride` strictly inside the block, two 16-bit arrays."""
    out = {}
    for q in range(case["k0"] // stride * stride, case["k1"], stride):
        if q <= case["k0"]:
            continue
        order, d = states[q]
        assert order.max() < 65536
        out[q] = (order.astype(np.uint16), collapse(d, case["k0"]))
    return out


def same_tables(x, y):
    return np.array_equal(x[0], y[0]) and np.array_equal(x[1], y[1]) and x[2] == y[2]
