"""[r10] The reduced column kernel stages phase A's class columns itself (csrc/fseq_kernels.hpp `red_cls`, RedArgs::cls_have): the
ids of a block's order are the key ranks leaf[i], the staged column is the class column, and neither the gather kernel nor the
reduced alignment is needed for that block.

Every case runs one input in three modes -- staged (the default), FSEQ_CLASS_GATHER=1 (the class columns gathered into the
reduced alignment: the form before) and FSEQ_CLASS_COLUMNS=0 (the reduced alignment from a second read of the alignment) --
and compares traceback, segments, max_segment_size, every boundary state and the per-column lists of the sampled columns with
the CPU oracle and between the modes.  `column_sources()` (fseq_debug_column_sources) says which blocks were staged, so a
case cannot pass on the old path.  Every comparison is integer equality."""
import importlib
import re

import numpy as np
import pytest

import fso
import proto_reduced as pr
from test_gpu_parity import check_long

pytestmark = pytest.mark.gpu

MODES = {"staged": {}, "gather": {"FSEQ_CLASS_GATHER": "1"}, "second_read": {"FSEQ_CLASS_COLUMNS": "0"}}


@pytest.fixture(scope="module")
def pkg():
    return importlib.import_module("founder-sequences_amd")


def make_ctx(pkg, m, n, L, B, knobs=(), debug=False):
    ctx = pkg.SegmentationContext(m, n, L, block_len=B)
    ctx.set_tuning("FSEQ_REDUCED_ALWAYS", "1")
    if debug:
        ctx.set_tuning("FSEQ_DEBUG", "1")
    for k, v in dict(knobs).items():
        ctx.set_tuning(k, v)
    return ctx


def run_ctx(pkg, ctx):
    try:
        ctx.run()
    except pkg.NoReduction:
        pass
    return ctx


def run_mode(pkg, msa, L, B, mode):
    m, n = msa.shape
    ctx = make_ctx(pkg, m, n, L, B, MODES[mode])
    ctx.set_sequences(msa)
    return run_ctx(pkg, ctx)


def sample_columns(n, B):
    """every 7th column, the first two and the last of every block, the last columns of the alignment"""
    return sorted({k for k in range(n) if k % 7 == 0 or k % B in (0, 1, B - 1) or k > n - 5})


def oracle_lists(msa, L, cols):
    """What fseq_debug_column_list holds of the sampled columns, from the pBWT of all rows: (values, counts) with entry 0 the
    lump of the values >= k + 2 - L and the distinct values below it descending, and the count of zeros."""
    p = fso.Pbwt(msa, debug=False)
    want = set(cols)
    out = {}
    for k in range(msa.shape[1]):
        p.step()
        if k in want:
            v, c = p.counts()
            thr = max(0, k + 2 - L)
            rec = v >= thr
            out[k] = (np.concatenate([[k + 1], v[~rec][::-1]]), np.concatenate([[c[rec].sum()], c[~rec][::-1]]), int(c[0]) if v[0] == 0 else 0)
    return out


def lists_of(ctx, cols):
    return {k: ctx.debug_column_list(k) for k in cols}


def check_lists(ctx, got, want):
    cap = ctx.timings()["list_cap_used"]
    for k, (gv, gc, cnt0, complete) in got.items():
        ev, ec, z = want[k]
        assert complete or gc[1:].sum() > cap, k
        assert np.array_equal(gv, ev[:len(gv)]) and np.array_equal(gc, ec[:len(gc)]), k
        assert complete == (len(gv) == len(ev)), k
        if complete:
            assert cnt0 == z, k


def same_lists(a, b):
    for k in a:
        x, y = a[k], b[k]
        assert np.array_equal(x[0], y[0]) and np.array_equal(x[1], y[1]) and x[2:] == y[2:], k


def states(ctx):
    return [ctx.boundary_state(i) for i in range(len(ctx.reduced_traceback()))]


def same_result(a, b):
    assert a.result.max_segment_size == b.result.max_segment_size
    assert np.array_equal(a.traceback(), b.traceback()) and np.array_equal(a.reduced_traceback(), b.reduced_traceback())
    for (a0, d0), (a1, d1) in zip(states(a), states(b)):
        assert np.array_equal(a0, a1) and np.array_equal(d0, d1)


def three_modes(pkg, msa, L, B, ref=None, staged_all=False):
    """The input in the three modes against the oracle and each other; returns the staged context."""
    m, n = msa.shape
    if ref is None:
        ref = fso.segment_long(msa, L, keep_dp=False, threads=4)
    cols = sample_columns(n, B)
    want = oracle_lists(msa, L, cols)
    out = {}
    for mode in MODES:
        ctx = run_mode(pkg, msa, L, B, mode)
        check_long(ctx, ref, n, L, check_dp=False)
        got = lists_of(ctx, cols)
        check_lists(ctx, got, want)
        out[mode] = (ctx, got)
    for mode in ("gather", "second_read"):
        same_result(out["staged"][0], out[mode][0])
        same_lists(out["staged"][1], out[mode][1])
        s = out[mode][0].column_sources()
        assert s["staged"] == 0 and s["gathered"] > 0, (mode, s)
    s, g = out["staged"][0].column_sources(), out["gather"][0].column_sources()
    assert s["staged"] > 0 and s["staged"] + s["gathered"] == g["gathered"], (s, g)
    if staged_all:
        assert s["gathered"] == 0, s
    # where the columns came from keeps its meaning: staged or gathered, a block with class columns counts as from_classes
    assert out["staged"][0].class_column_sources() == out["gather"][0].class_column_sources()
    assert out["second_read"][0].class_column_sources()["from_classes"] == 0
    return out["staged"][0], ref


def keys_shared_by_representatives(msa, L, B, b):
    """CPU, from the input: in block b several representatives carry one block key.  The representatives of the block are the rows
    that start a class at vmin in the state behind it (proto_reduced.reduce_state); vmin <= thr0 = k0 + 2 - L whatever the list
    capacity, and a smaller vmin only splits classes further, so the repeat at vmin = thr0 is a repeat at the run's vmin."""
    m, n = msa.shape
    k0, k1 = b * B, min(n, (b + 1) * B)
    thr0 = k0 + 2 - L
    assert thr0 >= 1
    p = fso.Pbwt(msa, debug=False)
    for _ in range(k0):
        p.step()
    a0, d0 = p.a.copy(), p.d.copy()
    for _ in range(k0, k1):
        p.step()
    a_red, _ = pr.reduce_state(a0, d0, p.a.copy(), p.d.copy(), thr0)
    _, leaf_of_row = np.unique(msa[:, k0:k1], axis=0, return_inverse=True)
    leaves = np.asarray(leaf_of_row).reshape(-1)[a_red]
    return len(a_red), len(np.unique(leaves))


# m, n, L, K, Brec, mu, seed, kind (0: 2-bit, 1: 4-bit symbols), B.  Mutation rates that leave 1,400 to 4,200 representatives a block: 512 x 7
# and larger, whose LDS holds one or two workgroups a CU with either staged-column buffer.  A block of up to 2,240 representatives runs on
# 512 x 5 -- three workgroups a CU in 54,272 bytes each, two with 4 KB more -- or on a 64- or 256-thread configuration: gathered.
SHAPES = [
    (11265, 1000, 20, 12, 120, 2e-3, 141, 0, 100),           # the first streamed row count
    (12007, 1030, 25, 12, 120, 1.5e-3, 142, 0, 100),         # a partial last word of rows, a last block of 30 columns (and ~750 representatives)
    (13000, 1000, 20, 12, 300, 2e-3, 169, 1, 100),           # 4-bit symbols: the carried second digit on key ranks
]


@pytest.mark.parametrize("m,n,L,K,Brec,mu,seed,kind,B", SHAPES)
def test_staged_class_columns_match_oracle_and_both_gathers(pkg, m, n, L, K, Brec, mu, seed, kind, B):
    msa = fso.synth_msa(fso.synth_spec(seed, K, Brec, mu, kind), m, n)
    # (b): representatives that share a block key, from the input alone
    reps, keys = keys_shared_by_representatives(msa, L, B, 3)
    assert keys < reps <= 11264, (reps, keys)
    ctx, ref = three_modes(pkg, msa, L, B, staged_all=(seed == 169))
    t = ctx.timings()
    print(ctx.column_sources(), t["reduced_rows_mean"])
    assert t["reduced_blocks"] > 0 and t["phase_a_trie_given_up"] == 0, t
    bits = 4 if kind else 2
    odd = [b for b in range(t["n_blocks"]) if (-(-ctx.class_columns(b)[2] * bits // 8)) % 16]
    assert odd, "no block whose keys end inside a 16-byte piece"
    # the second run goes by the remembered plan
    tb, st, s = ctx.traceback().copy(), states(ctx), ctx.column_sources()
    run_ctx(pkg, ctx)
    assert np.array_equal(ctx.traceback(), tb) and ctx.column_sources() == s
    for (a0, d0), (a1, d1) in zip(st, states(ctx)):
        assert np.array_equal(a0, a1) and np.array_equal(d0, d1)
    check_long(ctx, ref, n, L, check_dp=False)


def test_eight_bit_symbols_and_a_configuration_that_must_gather(pkg):
    """8-bit symbols: a class column is 12,288 bytes, so two staged-column buffers of that width are 22 KB more than the 1 KB
    buffers of a configuration of a few hundred rows -- whose LDS is a few KB and bounds how many of its workgroups a CU holds.
    Its resident count would drop: its blocks must be gathered (the direct-or-gather rule, red_cls_direct), and the result is
    still the oracle's.  The input has nine founders and a few mutations: a few hundred representatives a block."""
    m, n, L, B = 12500, 1000, 20, 100
    rng = np.random.default_rng(145)
    founders = rng.integers(0, 40, size=(9, n)).astype(np.uint8) + 60
    msa = founders[rng.integers(0, 9, size=m)]
    flips = rng.random((m, n)) < 2e-4
    msa = np.ascontiguousarray(np.where(flips, (msa + 1).astype(np.uint8), msa).astype(np.uint8))
    # CPU: every block has at most 1,024 representatives' worth of distinct rows in reach of its lists -- the configurations of
    # 64 and 256 threads (192 to 1,280 rows), not the 512- and 1024-thread ones whose LDS leaves one or two workgroups a CU anyway
    ref = fso.segment_long(msa, L, keep_dp=False, threads=4)
    cols = sample_columns(n, B)
    want = oracle_lists(msa, L, cols)
    ctxs = {}
    for mode in MODES:
        ctx = run_mode(pkg, msa, L, B, mode)
        check_long(ctx, ref, n, L, check_dp=False)
        got = lists_of(ctx, cols)
        check_lists(ctx, got, want)
        ctxs[mode] = (ctx, got)
    ctx = ctxs["staged"][0]
    t, s = ctx.timings(), ctx.column_sources()
    print(t["reduced_rows_mean"], s)
    assert t["reduced_blocks"] > 0 and t["reduced_rows_mean"] <= 1024, t
    assert s["staged"] == 0 and s["gathered"] > 0, s
    assert ctx.class_column_sources()["from_classes"] == s["gathered"]
    for mode in ("gather", "second_read"):
        same_result(ctx, ctxs[mode][0])
        same_lists(ctxs["staged"][1], ctxs[mode][1])


def test_a_staged_block_with_one_key(pkg):
    """Block 3 is one constant column after the other -- one key, a class column of which sixteen bytes are staged -- behind twenty
    columns that spell one of 2,000 patterns: its ~2,000 representatives (rows that differ in reach of its lists) all carry
    leaf 0, and they put it on a configuration that stages."""
    m, n, L, K, Brec, mu, seed, kind, B = SHAPES[0]
    msa = fso.synth_msa(fso.synth_spec(seed, K, Brec, mu, kind), m, n)
    codes = np.unique(msa)
    rng = np.random.default_rng(147)
    pat = codes[rng.integers(0, len(codes), size=(2000, 20))]
    msa[:, 280:300] = pat[rng.integers(0, 2000, size=m)]
    msa[:, 300:400] = codes[0]
    reps, keys = keys_shared_by_representatives(msa, L, B, 3)
    assert keys == 1 and 1500 <= reps <= 2240, (reps, keys)
    ctx, _ = three_modes(pkg, msa, L, B)
    assert ctx.class_columns(3)[2] == 1
    assert ctx.column_sources(3)["block_staged"]


def eight_bit_rows_with_copies(R, m, n, seed):
    """R rows of random bytes among forty codes, pairwise different within three columns, and m - R exact copies, shuffled"""
    rng = np.random.default_rng(seed)
    base = rng.integers(0, 40, size=(R, n)).astype(np.uint8) + 60
    idx = np.arange(R)
    for j in range(3):
        base[:, j] = 60 + (idx // 40 ** j) % 40
    src = np.concatenate([idx, rng.integers(0, R, size=m - R)])
    rng.shuffle(src)
    return np.ascontiguousarray(base[src])


def test_eight_bit_symbols_staged_on_a_large_configuration(pkg):
    """4,200 representatives a block of 8-bit symbols: 1024 x 5, one workgroup per CU with either buffer (12 KB class columns,
    4,200 of their bytes staged: one byte gather per row as before)."""
    m, n, L, B = 11300, 1000, 20, 100
    msa = eight_bit_rows_with_copies(4200, m, n, 148)
    ctx, _ = three_modes(pkg, msa, L, B, staged_all=True)
    assert ctx.class_columns(2)[2] == 4200


def boundary_kinds(rbs, B, stride=32):
    """pass 2's sweeps by where they start: at the block's first column (ids are translated there), at a reduced stride state
    (ids are key ranks already), and the boundaries on a block border (a copy)."""
    kinds = {"start": 0, "stride": 0, "border": 0}
    for rb in (int(x) for x in rbs):
        if rb % B == 0:
            kinds["border"] += 1
            continue
        start = (rb - 1) // stride * stride
        kinds["start" if start <= rb // B * B else "stride"] += 1
    return kinds


def test_pass_2_sweeps_from_the_block_start_and_from_stride_states(pkg):
    """The boundaries are the oracle's (they do not depend on the block length): the block length is chosen on the CPU, among
    90 to 110 columns, so that boundaries fall in the first columns of a block (the sweep starts at the block's first column
    and translates the ids), behind a reduced stride state inside a block (the ids are key ranks already) and on a block
    border."""
    m, n, L = 12000, 1500, 20
    msa = fso.synth_msa(fso.synth_spec(144, 12, 120, 2e-3, 0), m, n)
    ref = fso.segment_long(msa, L, keep_dp=False, threads=4)
    rbs = [rb for rb in ref["reduced"]["rb"] if rb < n]
    B = next((B for B in range(90, 111) if min(boundary_kinds(rbs, B).values()) >= 1 and boundary_kinds(rbs, B)["start"] >= 3 and boundary_kinds(rbs, B)["stride"] >= 3), None)
    assert B is not None, [boundary_kinds(rbs, B) for B in range(90, 111)]
    print(B, boundary_kinds(rbs, B))
    three_modes(pkg, msa, L, B, ref=ref)


def both_sources_input():
    """test_both_sources_in_one_run's (tests/test_gpu_class_columns.py): about 9,100 distinct words in block 1's last group of
    columns -- the trie gives the block up, the reduced phase C lists it."""
    m, n = 30000, 384
    rng = np.random.default_rng(72)
    msa = fso.synth_msa(fso.synth_spec(74, 1, 4000, 0.0, 0), m, n)
    codes = np.unique(msa)
    assert len(codes) >= 4
    w = rng.integers(0, 9500, size=m)
    for j in range(8):
        msa[:, 184 + j] = codes[(w >> (2 * j)) & 3]
    return msa


def test_blocks_without_class_columns_beside_blocks_that_stage_them(pkg):
    msa = both_sources_input()
    L, B = 8, 96
    ctx, ref = three_modes(pkg, msa, L, B)
    t, s = ctx.timings(), ctx.column_sources(1)
    print(t["phase_a_trie_given_up"], s, ctx.class_column_sources())
    assert t["phase_a_trie_given_up"] == 1 and ctx.class_columns(1)[0] is None
    assert s["staged"] > 0 and s["gathered"] >= 1 and not s["block_staged"], s
    # (block 2's representatives differ in block 1's random columns: thousands, on a configuration that stages)
    assert ctx.column_sources(2)["block_staged"]
    assert ctx.class_column_sources()["from_alignment"] == 1
    tb, st = ctx.traceback().copy(), states(ctx)
    run_ctx(pkg, ctx)                                        # by the remembered plan
    assert ctx.column_sources(1) == s and np.array_equal(ctx.traceback(), tb)
    for (a0, d0), (a1, d1) in zip(st, states(ctx)):
        assert np.array_equal(a0, a1) and np.array_equal(d0, d1)
    check_long(ctx, ref, msa.shape[1], L, check_dp=False)


def test_second_input_with_another_symbol_width(pkg):
    """4-bit symbols behind 2-bit ones on one context: another packing, another class-column pitch and staged width; nothing of the
    first input's plan or columns may be used."""
    m, n, L, B = 12007, 1000, 20, 100
    msa = fso.synth_msa(fso.synth_spec(142, 12, 120, 2e-3, 0), m, n)
    ctx = make_ctx(pkg, m, n, L, B)
    ctx.set_sequences(msa)
    run_ctx(pkg, ctx)
    check_long(ctx, fso.segment_long(msa, L, keep_dp=False, threads=4), n, L, check_dp=False)
    s0, ldc0 = ctx.column_sources(), ctx.class_columns(0)[1]
    assert s0["staged"] > 0, s0
    msa2 = fso.synth_msa(fso.synth_spec(146, 9, 200, 2e-3, 1), m, n)
    ref2 = fso.segment_long(msa2, L, keep_dp=False, threads=4)
    ctx.set_sequences(msa2)
    run_ctx(pkg, ctx)
    check_long(ctx, ref2, n, L, check_dp=False)
    assert ctx.class_columns(0)[1] == 2 * ldc0
    cols = sample_columns(n, B)
    check_lists(ctx, lists_of(ctx, cols), oracle_lists(msa2, L, cols))
    fresh = run_mode(pkg, msa2, L, B, "staged")
    assert fresh.column_sources() == ctx.column_sources() and ctx.column_sources()["staged"] > 0
    same_result(ctx, fresh)


def test_peak_memory_falls_by_the_reduced_alignment(pkg):
    """Everything staged: no reduced alignment is allocated.  Its size in the gather mode is n columns of ceil16(the most
    representatives of a block * bits / 8) bytes; the most representatives is at least the most distinct rows a block has over
    the columns from its first threshold on (CPU, from the input: vmin <= k0 + 2 - L, and representatives are classes of rows
    equal from vmin - 1 to the block's end)."""
    m, n, L, K, Brec, mu, seed, kind, B = SHAPES[2]          # (4-bit symbols; every block has more than 2,240 representatives)
    msa = fso.synth_msa(fso.synth_spec(seed, K, Brec, mu, kind), m, n)
    most = max(len(np.unique(msa[:, max(b * B + 1 - L, 0):min(n, (b + 1) * B)], axis=0)) for b in range(2, (n + B - 1) // B))
    red_msa_bytes = n * ((-(-most * 4 // 8) + 15) // 16 * 16)
    peaks = {}
    for mode in ("staged", "gather"):
        ctx = make_ctx(pkg, m, n, L, B, MODES[mode])
        ctx.device_bytes(reset_peak=True)
        ctx.set_sequences(msa)
        run_ctx(pkg, ctx)
        run_ctx(pkg, ctx)
        peaks[mode] = ctx.device_bytes()[1]
        s = ctx.column_sources()
        assert (s["gathered"] == 0) == (mode == "staged"), (mode, s)
        del ctx
    print(peaks, red_msa_bytes, most)
    assert peaks["staged"] + red_msa_bytes <= peaks["gather"], (peaks, red_msa_bytes)


def test_slim_configuration_keeps_two_workgroups_with_class_sized_buffers(pkg, capfd):
    """BASELINE C4's geometry (blocks of 814 columns, 2-bit symbols) on streamed rows: 5,600 representatives a block run on the
    slim configuration (512 x 15), its staged-column buffers sized for a class column (3 KB each, 2 KB more than its rows
    need), and the library's plan report -- the occupancy query of tests/test_gpu_columns_slim.py -- still says two workgroups
    per CU.  The blocks are staged, and the lists are those of the gather."""
    from test_gpu_columns_slim import distinct_rows_with_copies
    m, n, L, B = 11400, 1640, 820, 814
    msa = distinct_rows_with_copies(R=5600, m=m, n=n, seed=711)
    ctx = make_ctx(pkg, m, n, L, B, debug=True)
    ctx.set_sequences(msa)
    capfd.readouterr()
    run_ctx(pkg, ctx)
    err = capfd.readouterr().err
    plans = re.findall(r"configuration of (\d+) rows: (\d+) blocks, (\d+) representatives on average \((\d+) threads x (\d+) rows, (\d+) distinct values, (\d+) bytes of LDS, (\d+) workgroups per CU\); columns: ([^(]*)\(", err)
    slim = [p for p in plans if (p[3], p[4]) == ("512", "15")]
    assert slim, err[-3000:]
    print(slim)
    for p in slim:
        assert int(p[7]) == 2 and int(p[6]) <= 80 * 1024 and "class columns, staged" in p[8], p
    s = ctx.column_sources()
    assert s["staged"] > 0 and s["gathered"] == 0, s
    old = run_mode(pkg, msa, L, B, "gather")
    same_result(ctx, old)
    cols = [k for k in sample_columns(n, B) if k < L - 2]
    same_lists(lists_of(ctx, cols), lists_of(old, cols))
