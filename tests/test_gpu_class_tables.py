"""[r16] Pass 2's class-table sweeps in their sweep form (k_columns_red<.., SW>: collapsed 16-bit ids, no value table) and the reduced
stride states as two 16-bit arrays, column by column: fseq_debug_class_tables runs pass 2's own sweep launches at chosen columns
of a finished run, and every table must be the one the oracle's pBWT ON ALL ROWS gives at that column -- a position starts a class
iff its divergence lies inside the block, a row's class is the number of class starts in front of it, the divergence in front of a
class is its first position's.  On the small inputs the model of the sweep form (tests/proto_red_snap.py) is held to the same tables.

Every column of two blocks: every offset 1 .. stride from a dropped state, the columns a state lies on, the block's first column + 1
and its last; FSEQ_RED_SS_STRIDE at 4, 8, 16 and 32; 2, 4 and 8 bits a symbol; a 16-bit reader (1024 x 7) behind a 16-bit writer
(512 x 15), a 32-bit reader (1024 x 5) behind that 16-bit writer and 32-bit readers behind 32-bit writers, each pairing asserted
from the plan (the plan pairs no 32-bit writer with a 16-bit reader: every phase-C configuration for more than 4,800 representatives
holds 16-bit words); streamed rows; a block the plan runs on all rows, which has
no states and is swept from its start; a second input on the same context."""
import importlib

import numpy as np
import pytest

import fso
import proto_red_snap as ps
import reduced_capacity_cases as rc

pytestmark = pytest.mark.gpu

STRIDES = (4, 8, 16, 32)


@pytest.fixture(scope="module")
def pkg():
    return importlib.import_module("founder-sequences_amd")


@pytest.fixture()
def always(monkeypatch):
    monkeypatch.setenv("FSEQ_REDUCED_ALWAYS", "1")
    return monkeypatch


def mosaic(m, n, K, syms, seed, rec=150, mu=2e-3):
    """m rows copied from K random founders over the letters `syms`, switching founder every ~rec columns, a letter in 1 / mu changed."""
    rng = np.random.default_rng(seed)
    S = np.frombuffer(syms, dtype=np.uint8)
    founders = S[rng.integers(0, len(S), size=(K, n))]
    src = np.empty((m, n), dtype=np.int64)
    cur = rng.integers(0, K, size=m)
    for k in range(n):
        sw = rng.random(m) < 1.0 / rec
        cur = np.where(sw, rng.integers(0, K, size=m), cur)
        src[:, k] = cur
    msa = founders[src, np.arange(n)[None, :]]
    mut = rng.random((m, n)) < mu
    msa[mut] = S[rng.integers(0, len(S), size=int(mut.sum()))]
    return np.asfortranarray(msa)


def expected_tables(msa, B, blocks):
    """{column: (class of every row, headd, ncls)} for every column strictly inside the given blocks, from the pBWT on all rows."""
    m, n = msa.shape
    want = {}
    for b in blocks:
        for k in range(b * B + 1, min(n, (b + 1) * B)):
            want[k] = b * B
    p = fso.Pbwt(msa, with_counts=False, debug=False)
    out = {}
    for k in range(1, max(want) + 1):
        p.step()
        if k in want:
            a, d = p.a, p.d
            head = d > want[k]
            head[0] = True
            cls = np.empty(m, dtype=np.uint32)
            cls[a] = np.cumsum(head) - 1
            out[k] = (cls, d[head].astype(np.uint32), int(head.sum()))
    return out


def check_tables(ctx, expect, columns):
    cls, headd, ncls = ctx.class_tables(columns)
    for i, k in enumerate(columns):
        e_cls, e_headd, e_n = expect[k]
        assert int(ncls[i]) == e_n, k
        assert np.array_equal(cls[i], e_cls), k
        assert np.array_equal(headd[i][:e_n], e_headd), k
        assert (headd[i][e_n:] == 0xFFFFFFFF).all(), k


def run(pkg, msa, L, B):
    m, n = msa.shape
    ctx = pkg.SegmentationContext(m, n, L, block_len=B)
    ctx.set_sequences(msa)
    try:
        ctx.run()
    except pkg.NoReduction:
        pass
    assert ctx.timings()["reduced_blocks"] > 0
    return ctx


def block_columns(B, n, blocks):
    return [k for b in blocks for k in range(b * B + 1, min(n, (b + 1) * B))]


# ---- 300 rows x 1,200 columns in blocks of 100 (the one-wave configurations, which have both forms), 2 / 4 / 8 bits a symbol
SMALL = {}


def small_input(bits):
    if bits not in SMALL:
        msa = mosaic(300, 1200, 6, rc.SYMS[bits], 1600 + bits)
        SMALL[bits] = (msa, expected_tables(msa, 100, (3, 11)))
    return SMALL[bits]


@pytest.mark.parametrize("bits", [2, 4, 8])
@pytest.mark.parametrize("stride", STRIDES)
def test_every_column_of_two_blocks(pkg, always, bits, stride):
    always.setenv("FSEQ_RED_SS_STRIDE", str(stride))
    msa, expect = small_input(bits)
    ctx = run(pkg, msa, 15, 100)
    check_tables(ctx, expect, block_columns(100, 1200, (3, 11)))
    # single tasks too: a workgroup of one task, on the column a state lies on and on the one behind it
    q = 300 + 2 * stride
    check_tables(ctx, expect, [q])
    check_tables(ctx, expect, [q + 1])
    check_tables(ctx, expect, [301, 399, 1101, 1199])


def test_the_model_gives_the_same_tables():
    """(no GPU work: the model of the sweep form against the tables on all rows the kernel is held to above)"""
    msa, expect = small_input(2)
    m, n = msa.shape
    B, L, X = 100, 15, 15
    p = fso.Pbwt(msa, with_counts=False, debug=False)
    st = []
    for b in range(n // B + 1):
        while p.idx < b * B:
            p.step()
        st.append((p.a, p.d))
    case = ps.block_case(msa, st, 3, B, L, X)
    _, states = ps.sweep_true(case, [])
    ss = ps.stride_states16(case, states, 8)
    for q, s16 in ss.items():
        cols = [k for k in range(q + 1, min(400, q + 9)) if k in expect]
        got = ps.sweep_collapsed(case, q, *s16, cols)
        for k in cols:
            cls_of_leaf, headd, ncls = got[k]
            assert ncls == expect[k][2] and np.array_equal(headd, expect[k][1])
            assert np.array_equal(cls_of_leaf[case["leaf_of_row"]], expect[k][0])


# ---- blocks of thousands of representatives (tests/reduced_capacity_cases.py): 5,121 take 512 x 15 in phase C and 1024 x 7 in pass 2,
# 16-bit words both; 3,585 take 1024 x 5 in both, 32-bit words both; block 5 holds one representative fewer
BIG = {}


def big_input(name):
    if name not in BIG:
        case = rc.CASES[name]
        msa = np.asfortranarray(rc.make(case))
        BIG[name] = (msa, expected_tables(msa, rc.BLOCK, (5, rc.BLOCK_UNDER_TEST)))
    return BIG[name]


# what the plan makes of blocks 5 and 6 (R - 1 and R representatives): (phase C's (T, E, list wave), the sweeps' (T, E, list wave)).
# 512 x 15 and 1024 x 7 hold 16-bit words, the others 32-bit: block 5 of 2b_5121 is a 16-bit writer read by a 32-bit sweep, block 6 a
# 16-bit writer read by the 16-bit sweep; 2b_3585 is 32-bit on both sides.  (No 32-bit writer meets a 16-bit sweep: a 16-bit sweep
# needs more than 5,120 representatives, and every phase-C configuration for more than 4,800 holds 16-bit words.)
PAIRINGS = {
    "2b_5121": [((512, 15, True), (1024, 5, False)), ((512, 15, True), (1024, 7, False))],
    "2b_3585": [((1024, 5, True), (512, 7, False)), ((1024, 5, True), (1024, 5, False))],
}


def planned(pkg, case):
    """The configurations plan_reduced gives blocks of R - 1 and R representatives at the case's geometry (the run plans with the same
    function on the same counts: tests/test_gpu_reduced_capacities.py pins that)."""
    plan = pkg.red_plan_host(case.m, rc.BLOCK, case.bits, case.m < rc.STREAMED_FROM, [case.R - 1, case.R], reduced_always=True)
    cf = plan["configs"]
    return [(cf[plan["config_of"][b]][2:5], cf[plan["config_snap_of"][b]][2:5]) for b in (0, 1)]


@pytest.mark.parametrize("name,stride", [("2b_5121", s) for s in STRIDES] + [("2b_3585", 8), ("2b_3585", 32)])
def test_blocks_of_thousands_of_representatives(pkg, always, name, stride):
    always.setenv("FSEQ_RED_SS_STRIDE", str(stride))
    assert planned(pkg, rc.CASES[name]) == PAIRINGS[name]       # (if the capacity tables move, this test must move with them)
    msa, expect = big_input(name)
    ctx = run(pkg, msa, rc.L, rc.BLOCK)
    check_tables(ctx, expect, block_columns(rc.BLOCK, rc.N, (5, rc.BLOCK_UNDER_TEST)))


def test_a_block_on_all_rows_is_swept_from_its_start(pkg, always):
    """701 representatives of 1,000 rows: phase C runs block 6 on all rows and drops no state for it; its representatives are known
    and every column is swept from the block's first (up to 99 columns, ids up to the block length)."""
    msa, expect = big_input("share_701")
    ctx = run(pkg, msa, rc.L, rc.BLOCK)
    assert ctx.timings()["reduced_blocks"] == rc.BLOCK_UNDER_TEST          # (blocks 0 to 5 hold 700 representatives: the others run on all rows)
    check_tables(ctx, expect, block_columns(rc.BLOCK, rc.N, (5, rc.BLOCK_UNDER_TEST)))


# ---- streamed rows (12,000: the order does not fit the LDS): the reduced alignment or phase A's class columns, key ranks in the order
@pytest.mark.parametrize("stride", [None, 4, 32])
def test_streamed_rows(pkg, always, stride):
    if stride:
        always.setenv("FSEQ_RED_SS_STRIDE", str(stride))
    if "streamed" not in BIG:
        msa = fso.synth_msa(fso.synth_spec(65, 12, 300, 3e-4, 0), 12000, 1200)
        BIG["streamed"] = (msa, expected_tables(msa, 100, (2, 4)))
    msa, expect = BIG["streamed"]
    ctx = run(pkg, msa, 20, 100)
    check_tables(ctx, expect, block_columns(100, 1200, (2, 4)))


def test_a_second_input_on_the_same_context(pkg, always):
    msa, expect = small_input(2)
    other = mosaic(300, 1200, 5, rc.SYMS[2], 1699)
    ctx = run(pkg, msa, 15, 100)
    check_tables(ctx, expect, block_columns(100, 1200, (3,)))
    ctx.set_sequences(other)
    ctx.run()
    check_tables(ctx, expected_tables(other, 100, (3, 11)), block_columns(100, 1200, (3, 11)))
    ctx.set_sequences(msa)
    ctx.run()
    check_tables(ctx, expect, block_columns(100, 1200, (11,)))


def test_what_the_entry_refuses(pkg, always):
    msa, _ = small_input(2)
    ctx = run(pkg, msa, 15, 100)
    for cols in ([300], [0], [1200], [305, 305], [310, 305]):          # a border, the ends, not ascending
        with pytest.raises(pkg.FseqError) as e:
            ctx.class_tables(cols)
        assert e.value.code == pkg.FSEQ_E_ARG, cols
    always.setenv("FSEQ_NO_REDUCED", "1")
    plain = pkg.SegmentationContext(300, 1200, 15, block_len=100)
    plain.set_sequences(msa)
    plain.run()
    with pytest.raises(pkg.FseqError) as e:
        plain.class_tables([305])
    assert e.value.code == pkg.FSEQ_E_UNSUPPORTED
