"""Phase A's class columns (csrc/fseq_blocktrie.hpp, phase 3) and the reduced alignment gathered from them (k_reduce_msa_lds
on that source, csrc/fseq_reduced.hpp) instead of from a second read of the alignment.

A class column of a block holds, at row rho, the symbol the block key of co-lex rank rho carries in that column; the
representatives' columns of phase C are gathered from them through leaf[i] = rank of representative i's key.  Checked here: the
class columns against numpy's distinct rows of the block, the runs against the oracle and against FSEQ_CLASS_COLUMNS=0 (the
second read), a block the trie gives up (both sources in one run), a context that takes a second input, a memory budget
the buffer does not fit.  Every comparison is integer equality."""
import importlib

import numpy as np
import pytest

import fso
from test_gpu_parity import check_long, compare_long, run_gpu

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def pkg():
    return importlib.import_module("founder-sequences_amd")


@pytest.fixture()
def always(monkeypatch):
    monkeypatch.setenv("FSEQ_REDUCED_ALWAYS", "1")
    return monkeypatch


def unpack(packed, bits, rows):
    """[columns, bytes] packed little-end first -> codes [columns, rows]"""
    per = 8 // bits
    r = np.arange(rows)
    return (packed[:, r // per] >> ((r % per) * bits).astype(np.uint8)) & ((1 << bits) - 1)


def check_class_columns(ctx, every=1):
    """Every block's class columns against the distinct rows of the block in co-lex order (the later column the more significant),
    taken from the alignment as the device holds it."""
    t = ctx.timings()
    B, nbk = t["block_len"], t["n_blocks"]
    packed, bits = ctx.packed_columns()
    codes = unpack(packed, bits, ctx.m)                      # [n, m]
    seen = 0
    for b in range(0, nbk, every):
        k0, k1 = b * B, min(ctx.n, (b + 1) * B)
        cls, ldc, nkeys = ctx.class_columns(b)
        if cls is None:
            continue
        seen += 1
        keys = np.unique(codes[k0:k1][::-1].T, axis=0)       # rows ordered by the last column first
        assert nkeys == len(keys), (b, nkeys, len(keys))
        assert cls.shape == (k1 - k0, ldc)
        got = unpack(cls, bits, nkeys)                       # [columns, nkeys]
        assert np.array_equal(got, keys[:, ::-1].T), b
        # the ranks behind the last key in its packed word are zero
        words = (nkeys * bits + 31) // 32
        tail = unpack(cls[:, :4 * words], bits, words * 32 // bits)[:, nkeys:]
        assert not tail.any(), b
    return seen


CLASS_SHAPES = [
    # m, n, L, K, Brec, mu, seed, kind, block_len
    (12000, 500, 20, 12, 120, 3e-4, 41, 0, 64),
    (12007, 530, 20, 12, 120, 3e-4, 42, 0, 72),              # a partial last word of rows; blocks of 4.5 groups; a last block of 26 columns
    (13000, 400, 20, 12, 300, 3e-4, 69, 1, 100),             # 4-bit symbols: groups of eight columns, eight ranks a word
    (12000, 300, 20, 1, 1000, 0.0, 43, 0, 100),              # one founder, no mutation: one key a block
    (12000, 256, 20, 20, 40, 2e-4, 44, 0, 64),               # every row changes its founder inside a block: a level with thousands of siblings
]


@pytest.mark.parametrize("m,n,L,K,Brec,mu,seed,kind,B", CLASS_SHAPES)
def test_class_columns_are_the_blocks_distinct_keys(pkg, always, m, n, L, K, Brec, mu, seed, kind, B):
    msa = fso.synth_msa(fso.synth_spec(seed, K, Brec, mu, kind), m, n)
    ctx = run_gpu(pkg, msa, L, block_len=B)
    t = ctx.timings()
    assert t["phase_a_trie_given_up"] == 0, t
    assert check_class_columns(ctx) == t["n_blocks"]
    if K == 1:
        assert ctx.class_columns(0)[2] == 1


def test_eight_bit_symbols_take_the_class_columns_too(pkg, always):
    """8-bit symbols are not left to the old path: four ranks a word, three words of a column per thread."""
    m, n, L, B = 12500, 240, 20, 60
    rng = np.random.default_rng(45)
    founders = rng.integers(0, 40, size=(9, n)).astype(np.uint8) + 60
    msa = founders[rng.integers(0, 9, size=m)]
    flips = rng.random((m, n)) < 2e-4
    msa = np.where(flips, (msa + 1).astype(np.uint8), msa).astype(np.uint8)
    ctx, _ = compare_long(pkg, msa, L, check_dp=False, block_len=B)
    t = ctx.timings()
    assert t["phase_a_trie_given_up"] == 0, t
    assert check_class_columns(ctx) == t["n_blocks"]
    s = ctx.class_column_sources()
    assert s["from_classes"] > 0 and s["from_alignment"] == 0, s


def states(ctx):
    return [ctx.boundary_state(i) for i in range(len(ctx.reduced_traceback()))]


def same_result(a, b):
    assert np.array_equal(a.traceback(), b.traceback()) and np.array_equal(a.reduced_traceback(), b.reduced_traceback())
    for (a0, d0), (a1, d1) in zip(states(a), states(b)):
        assert np.array_equal(a0, a1) and np.array_equal(d0, d1)


@pytest.mark.parametrize("m,n,L,K,Brec,mu,seed,kind,B", CLASS_SHAPES[:3])
def test_run_from_class_columns_matches_oracle_and_second_read(pkg, always, m, n, L, K, Brec, mu, seed, kind, B):
    msa = fso.synth_msa(fso.synth_spec(seed, K, Brec, mu, kind), m, n)
    ctx, ref = compare_long(pkg, msa, L, block_len=B)
    t = ctx.timings()
    s = ctx.class_column_sources()
    assert t["reduced_blocks"] > 0 and s["from_classes"] > 0 and s["from_alignment"] == 0, (t, s)
    tb = ctx.traceback().copy()
    st = states(ctx)
    # the second run on the context launches by the plan of the first
    ctx.run()
    assert np.array_equal(ctx.traceback(), tb) and ctx.class_column_sources() == s
    for (a0, d0), (a1, d1) in zip(st, states(ctx)):
        assert np.array_equal(a0, a1) and np.array_equal(d0, d1)
    check_long(ctx, ref, n, L)
    # the second read of the alignment
    always.setenv("FSEQ_CLASS_COLUMNS", "0")
    old = run_gpu(pkg, msa, L, block_len=B)
    so = old.class_column_sources()
    assert so["from_classes"] == 0 and so["from_alignment"] == s["from_classes"], so
    assert old.class_columns(0)[0] is None
    same_result(ctx, old)


def test_blocks_the_trie_gives_up_have_no_class_columns(pkg, always):
    """The input of test_streamed_phase_a_trie_gives_blocks_up: columns 96..191 random, the trie gives the two blocks up and they
    have no class columns.  Those two blocks have more than 12,288 distinct keys, hence (representatives are finer than key
    classes) more representatives than any configuration holds: phase C runs them on all rows and lists them for NEITHER
    source -- the run with both sources is the next test's.  The result is the oracle's, on the first run and by the plan."""
    m = 30000
    rng = np.random.default_rng(71)
    msa = fso.synth_msa(fso.synth_spec(72, 10, 40, 2e-4, 0), m, 288)
    codes = np.unique(msa)
    msa[:, 96:192] = codes[rng.integers(0, len(codes), size=(m, 96))]
    ctx, ref = compare_long(pkg, msa, 8, check_dp=False, block_len=48)
    t = ctx.timings()
    s = ctx.class_column_sources()
    print(t, s)
    assert t["n_blocks"] == 6 and t["phase_a_trie_given_up"] == 2, t
    assert ctx.class_columns(2)[0] is None and ctx.class_columns(3)[0] is None and check_class_columns(ctx) == 4
    # (the two blocks that are reduced took the classes; the two random blocks and the blocks behind them, which inherit their
    # distinct rows, are listed for neither source)
    assert s == {"from_classes": 2, "from_alignment": 0} and t["reduced_blocks"] == 2, (t, s)
    try:
        ctx.run()
    except pkg.NoReduction:
        pass
    check_long(ctx, ref, 288, 8, check_dp=False)
    assert ctx.class_column_sources() == s


def test_both_sources_in_one_run(pkg, always):
    """A block the trie gives up AND the reduced phase C lists: about 9,100 distinct words in the block's last group of columns --
    more new classes than one level's pair table takes (8,192), fewer keys and representatives than a configuration holds
    (11,264).  Its representatives' columns come from the alignment, the other blocks' from the classes, in one run; the
    result is the oracle's, again on the second run (by the plan) and with FSEQ_CLASS_COLUMNS=0."""
    m, n, L, B = 30000, 384, 8, 96
    rng = np.random.default_rng(72)
    msa = fso.synth_msa(fso.synth_spec(74, 1, 4000, 0.0, 0), m, n)
    codes = np.unique(msa)
    assert len(codes) >= 4
    w = rng.integers(0, 9500, size=m)
    for j in range(8):
        msa[:, 184 + j] = codes[(w >> (2 * j)) & 3]
    ctx, ref = compare_long(pkg, msa, L, check_dp=False, block_len=B)
    t = ctx.timings()
    s = ctx.class_column_sources()
    print(t, s)
    assert t["phase_a_trie_given_up"] == 1, t
    assert ctx.class_columns(1)[0] is None and check_class_columns(ctx) == 3
    assert s["from_classes"] > 0 and s["from_alignment"] == 1, s
    try:
        ctx.run()
    except pkg.NoReduction:
        pass
    check_long(ctx, ref, n, L, check_dp=False)
    assert ctx.class_column_sources() == s
    always.setenv("FSEQ_CLASS_COLUMNS", "0")
    old = run_gpu(pkg, msa, L, block_len=B)
    assert old.class_column_sources()["from_classes"] == 0
    same_result(ctx, old)


def test_context_takes_a_second_input(pkg, always):
    """A context's rows, columns and block length are fixed when it is made; what a second input changes is the alphabet -- 4-bit
    symbols behind 2-bit ones: another packing, another class-column stride, groups of eight columns -- and every key.  No class
    column of the first input may be used: the result equals a fresh context's and the oracle's."""
    m, n, L, B = 12007, 530, 20, 72
    msa = fso.synth_msa(fso.synth_spec(42, 12, 120, 3e-4, 0), m, n)
    ctx = run_gpu(pkg, msa, L, block_len=B)
    assert ctx.class_column_sources()["from_classes"] > 0
    ldc0 = ctx.class_columns(0)[1]
    msa2 = fso.synth_msa(fso.synth_spec(46, 9, 200, 4e-4, 1), m, n)
    ref2 = fso.segment_long(msa2, L, keep_dp=False, threads=4)
    ctx.set_sequences(msa2)
    try:
        ctx.run()
    except pkg.NoReduction:
        pass
    check_long(ctx, ref2, n, L, check_dp=False)
    assert ctx.class_columns(0)[1] == 2 * ldc0
    assert check_class_columns(ctx, every=2) > 0
    fresh = run_gpu(pkg, msa2, L, block_len=B)
    assert fresh.class_column_sources() == ctx.class_column_sources()
    same_result(ctx, fresh)


def test_memory_budget_too_small_for_the_class_columns(pkg, always):
    """The class columns fall under fseq_set_memory_budget: where they do not fit, the run reads the alignment a second time as
    before, says so, and leaves no error behind."""
    m, n, L, K, Brec, mu, seed, kind, B = CLASS_SHAPES[0]
    msa = fso.synth_msa(fso.synth_spec(seed, K, Brec, mu, kind), m, n)
    ref = fso.segment_long(msa, L, keep_dp=False, threads=4)
    ctx = pkg.SegmentationContext(m, n, L, block_len=B)
    ctx.set_memory_budget(1 << 20)
    ctx.set_sequences(msa)
    ctx.run()
    check_long(ctx, ref, n, L, check_dp=False)
    s = ctx.class_column_sources()
    assert s["from_classes"] == 0 and s["from_alignment"] > 0, s
    assert ctx.class_columns(0)[0] is None
    assert pkg.load_library().fseq_last_error(ctx.h) == b""
    # ... and with room for them the same context takes them
    ctx.set_memory_budget(0)
    ctx.run()
    assert ctx.class_column_sources()["from_classes"] == s["from_alignment"]
    check_long(ctx, ref, n, L, check_dp=False)


@pytest.mark.parametrize("m,n,L,K,Brec,mu,seed,kind,B", [
    (12000, 2400, 20, 12, 300, 3e-4, 65, 0, 100),
    (13000, 1200, 20, 12, 300, 3e-4, 69, 1, 100),
    (70000, 600, 20, 30, 200, 1e-4, 70, 0, 100),             # a column of more than 16 KB: two LDS-DMA pieces per lane
])
@pytest.mark.parametrize("gather", [False, True])
def test_second_read_kernels_stay_covered(pkg, always, m, n, L, K, Brec, mu, seed, kind, B, gather):
    """FSEQ_CLASS_COLUMNS=0: the kernels that build the reduced alignment from the alignment itself -- what the blocks the trie gives
    up take, by LDS (one and two pieces a lane) or, FSEQ_REDUCED_MSA_GATHER, by gathers from memory -- on every listed block."""
    always.setenv("FSEQ_CLASS_COLUMNS", "0")
    if gather:
        always.setenv("FSEQ_REDUCED_MSA_GATHER", "1")
    msa = fso.synth_msa(fso.synth_spec(seed, K, Brec, mu, kind), m, n)
    ctx, _ = compare_long(pkg, msa, L, check_dp=False, block_len=B)
    s = ctx.class_column_sources()
    assert ctx.timings()["reduced_blocks"] > 0 and s["from_classes"] == 0 and s["from_alignment"] > 0, s
