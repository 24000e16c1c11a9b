"""A list budget (fseq_set_list_memory): the long path holds the per-column lists of one window of column blocks at a time,
runs the DP rounds each window feeds, and takes the merge thresholds in a second pass over the windows -- with the same
results, bit for bit, as the run that holds every list.  Every windowed run here asserts windows >= 3
(fseq_debug_list_windows), so none of these passes by fitting in one window."""
import importlib

import numpy as np
import pytest

import fso
from test_gpu_parity import _free_hbm_bytes, check_full_size_properties, compare_long, depth_blocks, run_gpu

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def pkg():
    return importlib.import_module("founder-sequences_amd")


def same_results(a, b, dp=True):
    """Two runs of one input agree on the DP arrays, the traceback, the merged segments and every boundary state."""
    assert a.result.max_segment_size == b.result.max_segment_size
    assert a.result.dp_segment_count == b.result.dp_segment_count and a.result.segment_count == b.result.segment_count
    if dp:
        n, L = a.n, a.segment_length
        written = np.ones(n - L + 1, dtype=bool)
        written[n - 2 * L + 1:n - L] = False                     # (entries no cell writes)
        for x, y in zip(a.debug_dp(), b.debug_dp()):
            assert np.array_equal(x[written], y[written])
    ta, tb_ = a.traceback(), b.traceback()
    for f in ("lb", "rb", "segment_max_size", "segment_size"):
        assert np.array_equal(ta[f], tb_[f]), f
    ra, rb = a.reduced_traceback(), b.reduced_traceback()
    for f in ("lb", "rb", "segment_size"):
        assert np.array_equal(ra[f], rb[f]), f
    for i in range(len(ra)):
        xa, xd = a.boundary_state(i)
        ya, yd = b.boundary_state(i)
        assert np.array_equal(xa, ya) and np.array_equal(xd, yd), i


def depth_replay_without_lists(ctx, m, n, L, blocks, cells_per_block=100, seed=1):
    """test_gpu_parity.check_depth_against_oracle without its list checks (a windowed run keeps no list behind): the oracle's
    pBWT runs each block from the GPU's boundary state of the block; the merged boundaries inside it, the state it ends in and
    sampled DP cells (evaluated again on the oracle's counts over the GPU's DP array) must agree."""
    lb, mx, sz = ctx.debug_dp()
    B, nblocks = ctx.timings()["block_len"], ctx.timings()["n_blocks"]
    k_dp = n - L + 1
    mx = mx.copy()
    mx[n - 2 * L + 1:n - L] = 0xFFFFFFFF
    dp = np.zeros(k_dp, dtype=fso.DP_DTYPE)
    dp["lb"], dp["rb"], dp["segment_max_size"], dp["segment_size"] = lb, np.arange(k_dp, dtype=np.uint64) + L, mx, sz
    rmq = fso.Rmq(mx, debug=False)
    for i in range(63, k_dp, 64):
        rmq.update(i)
    red = ctx.reduced_traceback()
    rb_index = {int(rb): i for i, rb in enumerate(red["rb"])}
    lo_cells, hi_cells = min(2 * L, n - L) - 1, n - L
    rng = np.random.default_rng(seed)
    checked = dict(blocks=0, boundaries=0, cells=0)
    for b in sorted(set(int(x) for x in blocks)):
        assert 0 <= b < nblocks
        c0, c1 = b * B, min(n, (b + 1) * B)
        p = fso.Pbwt(ctx.get_sequences(c0, c1), debug=False, col0=c0)
        a, d = ctx.debug_block_state(b)
        p.set_state(a, d, c0)
        lo, hi = max(c0, lo_cells), min(c1, hi_cells)
        cells = set(rng.choice(np.arange(lo, hi), size=min(cells_per_block, hi - lo), replace=False).tolist()) if hi > lo else set()
        for k in range(c0, c1):
            p.step()
            if k + 1 in rb_index:
                ga, gd = ctx.boundary_state(rb_index[k + 1])
                assert np.array_equal(ga, p.a) and np.array_equal(gd, p.d), ("boundary", b, k + 1)
                checked["boundaries"] += 1
            if k in cells:
                v, c = p.counts()
                got = fso.dp_step(v, c, dp, rmq.h, m, L, 0, k, (0, k + 1, m, m), debug=False)
                tt = k + 1 - L
                assert got == (int(lb[tt]), k + 1, int(mx[tt]), int(sz[tt])), ("cell", b, k, got)
                checked["cells"] += 1
        a, d = ctx.debug_block_state(b + 1)
        assert np.array_equal(a, p.a) and np.array_equal(d, p.d), ("block end", b)
        checked["blocks"] += 1
    return checked


def windowed_against_oracle(pkg, msa, L, parts=5, **kw):
    """The run that holds every list, then a budget of about 1 / parts of its list memory: oracle parity and equality."""
    full = run_gpu(pkg, msa, L, **kw)
    lw = full.list_windows()
    assert lw["windows"] == 1 and lw["merge_windows"] == 0 and lw["columns_per_window"] == msa.shape[1]
    budget = lw["bytes_held"] // parts
    ctx, _ref = compare_long(pkg, msa, L, list_memory=budget, **kw)
    w = ctx.list_windows()
    assert w["windows"] >= 3 and 0 < w["bytes_held"] <= budget, w
    if ctx.result.max_segment_size < msa.shape[0] and ctx.result.dp_segment_count > 1:
        assert w["merge_windows"] >= 1, w
    same_results(ctx, full)
    return ctx, full


SHAPES = [
    # m, n, L, K, Brec, mu, seed, kind, block_len
    (300, 5000, 10, 8, 200, 2e-3, 28, 0, 16),            # LDS-resident rows, classic DP schedule
    (2504, 4000, 50, 16, 2000, 1e-4, 0x5EED0002, 0, 200),  # C2 / C3 rows
    (1000, 12000, 100, 10, 300, 1e-3, 23, 0, 256),       # pipelined DP schedule (L >= 96): the drain round with the last window
    (12000, 3000, 10, 12, 200, 3e-4, 46, 0, 12),         # streamed rows, 250 blocks
    (600, 1500, 20, 8, 300, 2e-3, 25, 1, 64),            # sigma = 16
    (64, 4000, 6, 5, 90, 5e-3, 29, 0, 4),                # 1000 blocks of 4 columns
]


@pytest.mark.parametrize("m,n,L,K,Brec,mu,seed,kind,B", SHAPES)
def test_windowed_lists_match_oracle(pkg, m, n, L, K, Brec, mu, seed, kind, B):
    msa = fso.synth_msa(fso.synth_spec(seed, K, Brec, mu, kind), m, n)
    windowed_against_oracle(pkg, msa, L, block_len=B)


def test_windowed_retries_grow_the_capacity(pkg):
    """list_cap = 2: the DP (or a threshold) finds a list too short inside some window; the attempt runs again at a larger
    capacity, in smaller windows."""
    m, n, L, K, Brec, mu, seed, kind, B = SHAPES[0]
    msa = fso.synth_msa(fso.synth_spec(seed, K, Brec, mu, kind), m, n)
    ctx, _ = windowed_against_oracle(pkg, msa, L, block_len=B, list_cap=2)
    assert ctx.timings()["retries"] >= 1


@pytest.mark.parametrize("knobs", [
    {"FSEQ_REDUCED_ALWAYS": "1", "FSEQ_REDUCED_MARGIN": "0"},   # reduced blocks whose lists are flagged: run again on all rows
    {"FSEQ_NO_REDUCED": "1"},                                   # every block on all rows, with its stride states
    {"FSEQ_DP_SERIAL": "1"},
])
@pytest.mark.parametrize("shape", [0, 3])
def test_windowed_lists_with_knobs(pkg, monkeypatch, knobs, shape):
    for k, v in knobs.items():
        monkeypatch.setenv(k, v)
    m, n, L, K, Brec, mu, seed, kind, B = SHAPES[shape]
    msa = fso.synth_msa(fso.synth_spec(seed, K, Brec, mu, kind), m, n)
    windowed_against_oracle(pkg, msa, L, block_len=B)


def test_config_c3_windowed_equals_unbounded(pkg):
    """BASELINE C3 at full size (m = 2,504, n = 10^6, L = 100): a windowed run equals the run that holds every list in the DP
    arrays, the traceback, the merged segments and every boundary state; a second run on the same context is identical."""
    c = fso.CONFIGS["C3"]
    m, n, L = c["m"], c["n"], c["L"]
    full = pkg.SegmentationContext(m, n, L)
    full.generate_synthetic(c["seed"], c["K"], c["B"], c["mu"], c["kind"])
    full.run()
    budget = full.list_windows()["bytes_held"] // 6
    win = pkg.SegmentationContext(m, n, L, list_memory=budget)
    win.generate_synthetic(c["seed"], c["K"], c["B"], c["mu"], c["kind"])
    win.run()
    w = win.list_windows()
    assert w["windows"] >= 3 and w["bytes_held"] <= budget and w["merge_windows"] >= 3, w
    same_results(win, full)
    win.run()
    assert win.list_windows() == w
    same_results(win, full)
    # only the lists of the window last held are there: never stale ring contents
    with pytest.raises(pkg.FseqError) as ei:
        win.debug_column_list(0)
    assert ei.value.code == 1
    win.debug_column_list(n - 1)
    win.close()
    full.close()


def test_lists_beyond_the_device_run_in_windows(pkg):
    """test_gpu_oom's shape: m = 20,000, n = 2.5 M, list_cap = m would be 400 GB of lists.  With an 8 GB budget it runs, and
    equals the run at the default list capacity (whose lists fit)."""
    m, n, L = 20_000, 2_500_000, 100
    budget = 8 << 30
    ctx = pkg.SegmentationContext(m, n, L, list_cap=m, list_memory=budget)
    ctx.generate_synthetic(7, 8, 1000, 1e-4, 0)
    ctx.run()
    w = ctx.list_windows()
    assert w["windows"] >= 3 and w["bytes_held"] <= budget, w
    assert ctx.timings()["list_cap_used"] == m
    ref = pkg.SegmentationContext(m, n, L)
    ref.generate_synthetic(7, 8, 1000, 1e-4, 0)
    ref.run()
    assert ref.list_windows()["windows"] == 1
    same_results(ctx, ref)
    ref.close()
    ctx.close()


def test_config_c4_shape_more_diverse_in_windows(pkg):
    """C4's shape with four times the bench's mutation rate (K = 64, mu = 2e-4): 192 GB of lists, refused with FSEQ_E_OOM
    without a budget (profiles/r05_diversity_C4.txt).  With a 32 GB budget it completes; the size-independent properties,
    the DP on a column prefix against the oracle, and a depth replay of a few blocks against the oracle (no list checks:
    the lists are gone)."""
    if _free_hbm_bytes() < 200e9:
        pytest.skip("less than 200 GB of HBM free")
    c = fso.CONFIGS["C4"]
    m, n, L = c["m"], c["n"], c["L"]
    budget = 32 << 30
    ctx = pkg.SegmentationContext(m, n, L, list_memory=budget)
    ctx.generate_synthetic(c["seed"], 64, c["B"], 2e-4, c["kind"])
    res = ctx.run()
    w = ctx.list_windows()
    assert w["windows"] >= 3 and w["bytes_held"] <= budget, w
    check_full_size_properties(pkg, ctx, res, m, n, L, 2400)
    got = depth_replay_without_lists(ctx, m, n, L, depth_blocks(ctx.timings(), n)[:4], cells_per_block=100)
    assert got["blocks"] >= 3 and got["cells"] >= 300, got
    ctx.close()


def test_budget_below_one_window_fails_with_oom_and_the_context_stays_usable(pkg):
    m, n, L, K, Brec, mu, seed, kind, B = SHAPES[0]
    msa = fso.synth_msa(fso.synth_spec(seed, K, Brec, mu, kind), m, n)
    ctx = pkg.SegmentationContext(m, n, L, block_len=B, list_memory=4096)
    ctx.set_sequences(msa)
    with pytest.raises(pkg.FseqError) as ei:
        ctx.run()
    assert ei.value.code == pkg.FSEQ_E_OOM
    assert "list memory budget of 4096 bytes holds no window" in str(ei.value) and "needs" in str(ei.value)
    full = run_gpu(pkg, msa, L, block_len=B)
    ctx.set_list_memory(full.list_windows()["bytes_held"] // 4)
    ctx.run()
    assert ctx.list_windows()["windows"] >= 3
    same_results(ctx, full)
    # 0: every list held again, on the same context
    ctx.set_list_memory(0)
    ctx.run()
    assert ctx.list_windows()["windows"] == 1
    same_results(ctx, full)
    v, cnt, _c0, _complete = ctx.debug_column_list(0)
    fv, fcnt, _, _ = full.debug_column_list(0)
    assert np.array_equal(v, fv) and np.array_equal(cnt, fcnt)


def test_budget_on_a_sharded_context_is_unsupported(pkg):
    import torch
    m, n, L = 300, 5000, 10
    a = pkg.SegmentationContext(m, n, L)
    words = int(a.L.fseq_shard_xbuf_words(a.h, 2))
    xbuf = torch.zeros(words + 64, dtype=torch.int32, device="cuda:0")
    a.set_shard(0, 2, xbuf.data_ptr(), xbuf.numel(), lambda off, cnt, op: 0)
    with pytest.raises(pkg.FseqError) as ei:
        a.set_list_memory(1 << 30)
    assert ei.value.code == 5                                       # FSEQ_E_UNSUPPORTED
    b = pkg.SegmentationContext(m, n, L, list_memory=1 << 30)
    with pytest.raises(pkg.FseqError) as ei:
        b.set_shard(0, 2, xbuf.data_ptr(), xbuf.numel(), lambda off, cnt, op: 0)
    assert ei.value.code == 5
    a.close()
    b.close()


def test_column_list_not_held_is_an_argument_error(pkg):
    m, n, L, K, Brec, mu, seed, kind, B = SHAPES[0]
    msa = fso.synth_msa(fso.synth_spec(seed, K, Brec, mu, kind), m, n)
    ctx, full = windowed_against_oracle(pkg, msa, L, block_len=B)
    held = []
    for col in range(0, n, 97):
        try:
            v, cnt, c0, comp = ctx.debug_column_list(col)
        except pkg.FseqError as e:
            assert e.code == 1
            continue
        held.append(col)
        fv, fcnt, fc0, fcomp = full.debug_column_list(col)
        assert np.array_equal(v, fv) and np.array_equal(cnt, fcnt) and c0 == fc0 and comp == fcomp, col
    assert held and len(held) < len(range(0, n, 97)) // 2
