"""CPU proof of pass 2's sweep form (tests/proto_red_snap.py): the class tables from collapsed 16-bit ids are the class tables of the
sweep on true divergences -- from the block's first column and from every reduced stride state."""
import numpy as np
import pytest

from oracle import fso
import proto_red_snap as ps


def _states(msa, B):
    m, n = msa.shape
    p = fso.Pbwt(msa)
    out = []
    for b in range((n + B - 1) // B + 1):
        k = min(b * B, n)
        while p.idx < k:
            p.step()
        out.append((p.a, p.d))
    return out


def _check_block(case, stride):
    """Every boundary column of the block, swept from the nearest state in front of it: (tasks checked, stride states used)."""
    k0, k1 = case["k0"], case["k1"]
    cols = list(range(k0 + 1, k1 + 1))
    truth, states = ps.sweep_true(case, cols)
    starts = {k0: ps.start_state16(case)}
    starts.update(ps.stride_states16(case, states, stride))
    checked = 0
    for q, (order16, ids16) in sorted(starts.items()):
        # (a sweep serves the boundaries up to and including the next state's column: the state on a boundary's own column is not its start)
        upto = min(k1, (q // stride + 1) * stride)
        mine = [k for k in cols if q < k <= upto]
        if not mine:
            continue
        got = ps.sweep_collapsed(case, q, order16, ids16, mine)
        for k in mine:
            assert ps.same_tables(got[k], truth[k]), (k0, q, k)
            checked += 1
    return checked, len(starts) - 1


SHAPES = [
    # m, n, L, B, X, K, Brec, mu, seed, kind
    (60, 600, 10, 50, 4, 3, 100, 5e-3, 5, 0),
    (200, 1200, 15, 100, 15, 6, 150, 3e-3, 31, 0),
    (400, 900, 25, 128, 20, 8, 300, 2e-3, 9, 1),         # sigma = 16
]


@pytest.mark.parametrize("m,n,L,B,X,K,Brec,mu,seed,kind", SHAPES)
@pytest.mark.parametrize("stride", [4, 8, 16])
def test_collapsed_sweeps_equal_true_sweeps(m, n, L, B, X, K, Brec, mu, seed, kind, stride):
    msa = fso.synth_msa(fso.synth_spec(seed, K, Brec, mu, kind), m, n)
    st = _states(msa, B)
    nb = (n + B - 1) // B
    checked = used = 0
    for b in range(nb):
        c, u = _check_block(ps.block_case(msa, st, b, B, L, X), stride)
        checked += c
        used += u
    assert checked == n                                  # every column behind a block's first, the block's end included
    assert used > nb


def _mosaic(seed=3, m=300, n=900):
    return fso.synth_msa(fso.synth_spec(seed, 6, 200, 2e-3), m, n)


def test_a_start_divergence_equal_to_the_first_column_is_outside():
    # the column in front of the block handed out kblk itself: such a value is NOT inside the block (its id is 0), the next one is
    msa = _mosaic()
    B = 100
    st = _states(msa, B)
    case = ps.block_case(msa, st, 4, B, 20, 25)
    k0 = case["k0"]
    assert (case["d_red"] == k0).any()
    assert list(ps.collapse(np.array([0, k0 - 1, k0, k0 + 1, k0 + 7]), k0)) == [0, 0, 0, 1, 7]
    truth, states = ps.sweep_true(case, [k0 + 1, k0 + 2])
    got = ps.sweep_collapsed(case, k0, *ps.start_state16(case), [k0 + 1, k0 + 2])
    assert ps.same_tables(got[k0 + 1], truth[k0 + 1]) and ps.same_tables(got[k0 + 2], truth[k0 + 2])
    # ... and in a stride state: values equal to kblk survive inside the block where rows stay together
    order, d = states[k0 + 8]
    assert (d == k0).any() or (d < k0).any()
    assert ((ps.collapse(d, k0) == 0) == (d <= k0)).all()


@pytest.mark.parametrize("stride", [4, 8, 16, 32])
def test_a_boundary_one_column_behind_a_dropped_state(stride):
    msa = _mosaic(seed=11)
    B = 100
    st = _states(msa, B)
    case = ps.block_case(msa, st, 3, B, 20, 25)
    k0, k1 = case["k0"], case["k1"]
    truth, states = ps.sweep_true(case, range(k0 + 1, k1))
    ss = ps.stride_states16(case, states, stride)
    assert ss
    for q, (order16, ids16) in ss.items():
        if q + 1 < k1:
            got = ps.sweep_collapsed(case, q, order16, ids16, [q + 1])
            assert ps.same_tables(got[q + 1], truth[q + 1]), q
            # the new column's id is q + 1 - k0: the largest in play
            assert int(got[q + 1][1].max()) == q + 1


def test_a_boundary_on_the_blocks_last_column():
    msa = _mosaic(seed=12)
    B = 100
    st = _states(msa, B)
    for b in (2, 8):                                       # (8: the last block)
        case = ps.block_case(msa, st, b, B, 20, 25)
        k0, k1 = case["k0"], case["k1"]
        truth, states = ps.sweep_true(case, [k1 - 1, k1])
        for stride in (8, 16):
            ss = ps.stride_states16(case, states, stride)
            q = max(x for x in ss if x < k1 - 1)
            got = ps.sweep_collapsed(case, q, *ss[q], [k1 - 1, k1])
            assert ps.same_tables(got[k1 - 1], truth[k1 - 1]) and ps.same_tables(got[k1], truth[k1])
        # (the whole block from its first column: ids up to the block length)
        got = ps.sweep_collapsed(case, k0, *ps.start_state16(case), [k1 - 1, k1])
        assert ps.same_tables(got[k1], truth[k1]) and int(got[k1][1].max()) == k1


def test_a_block_whose_representatives_share_one_key():
    # rows that differ in front of the block and agree on all of it: several representatives (their start divergences tell them
    # apart for the lists), one block key, one class at every column
    rng = np.random.default_rng(16)
    m, B = 80, 60
    msa = np.empty((m, 3 * B), dtype=np.uint8, order="F")
    msa[:, :B] = rng.integers(0, 4, size=(m, B)) + ord("A")
    msa[:, B:] = (rng.integers(0, 4, size=(1, 2 * B)) + ord("A"))       # every row the same from the second block on
    st = _states(msa, B)
    case = ps.block_case(msa, st, 1, B, 3 * B, 10, vmin=1)
    assert len(case["rows"]) > 1 and int(case["leaf_of_row"].max()) == 0
    k0, k1 = case["k0"], case["k1"]
    truth, states = ps.sweep_true(case, range(k0 + 1, k1 + 1))
    for stride in (4, 16):
        starts = {k0: ps.start_state16(case)}
        starts.update(ps.stride_states16(case, states, stride))
        for q, s16 in starts.items():
            cols = [k for k in range(q + 1, min(k1, q + stride) + 1)]
            got = ps.sweep_collapsed(case, q, *s16, cols)
            for k in cols:
                assert ps.same_tables(got[k], truth[k])
                assert got[k][2] == 1 and list(got[k][1]) == [k]
