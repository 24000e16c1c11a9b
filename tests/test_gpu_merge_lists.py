"""The traceback and the greedy merge on the card, kernel by kernel, on constructed DP arrays and column lists
(tests/merge_list_cases.py: the model, the generators and the tables; tests/test_merge_list_cases.py checks on the CPU that every
case reaches what it is listed for).  fseq_debug_merge_on_lists runs follow_traceback and the merge half of
long_traceback_and_merge as an unsharded run calls them -- the thresholds riding with the traceback (k_seg_tau_tb) or taken by
launches of their own, whole or once per column range (k_seg_tau, k_seg_count under the ownership rule) --, and
fseq_debug_traceback_parts follows the traceback part by part as a sharded run in window mode does (k_tb_windows(vlo, vhi),
k_tb_chain_part, k_tb_emit(vlo)).  The traceback, the thresholds, the merged segments and the entries per part are the model's,
bit for bit; there is no tolerance anywhere.

Two things the issue lists cannot be reached through a merge and are covered by their nearest neighbours (the summary of the
change says so too): a complete list without an excess has tau = 0 only where max_size[n - L] >= m, and then no merge runs -- the
thresholds that ride with the traceback show it (max_ge_m, and every traceback case); and a merged size counted where current_lb
lies below every value of a list would be the list's whole sum, m on a complete list (never a join) and undecided on a cut one --
count_strips counts every entry but the last of lists that end in current_lb exactly."""
import importlib

import numpy as np
import pytest

import merge_list_cases as M

pytestmark = pytest.mark.gpu

E_ARG, E_HIP, E_UNSUPPORTED = 1, 3, 5


@pytest.fixture(scope="module")
def pkg():
    return importlib.import_module("founder-sequences_amd")


# one context per shape, reused across the cases of that shape (the tables keep equal shapes together); its rows are a generated
# alignment the traceback and the merge never read
_held = {"shape": None, "ctx": None}


def context(pkg, m, n, L, fresh=False):
    if _held["shape"] != (m, n, L) or fresh:
        if _held["ctx"] is not None:
            _held["ctx"].close()
        ctx = pkg.SegmentationContext(m, n, L)
        ctx.generate_synthetic(0x5EED, 8, 500, 1e-3)
        _held.update(shape=(m, n, L), ctx=ctx)
    return _held["ctx"]


def guarded(pkg, what, call):
    try:
        return call()
    except pkg.FseqError as e:
        if e.code == E_HIP:
            pytest.exit("%s: %s -- nothing more is started on a device that has faulted" % (what, e), returncode=3)
        raise


def same(what, label, got, want):
    assert got.dtype == want.dtype and len(got) == len(want), "%s: %s has %d entries, the model %d" % (what, label, len(got), len(want))
    if got.tobytes() != want.tobytes():
        bad = [i for i in range(len(got)) if got[i].tobytes() != want[i].tobytes()]
        raise AssertionError("%s: %s differs at %d of %d entries, first at %d: device %s, model %s" % (what, label, len(bad), len(got), bad[0], got[bad[0]], want[bad[0]]))


def as_device(pkg, tb):
    return tb.astype(pkg.DPARG_DTYPE)


# ---- the traceback, whole
def run_traceback(pkg, ctx, what, n, L, arrays, open_every=0):
    lb, mx, sz = arrays
    ent, hdr = M.lump_lists(M.TB_M, n, 2, open_every)
    want_tb = M.traceback(n, L, lb, mx, sz)
    want_tau = M.thresholds(want_tb, ent, hdr)
    tb, tau, seg, info = guarded(pkg, what, lambda: ctx.debug_merge_on_lists(2, ent, hdr, lb, mx, sz))
    print(what, "S", len(tb), "tau", len(tau), info)
    same(what, "the traceback", tb, as_device(pkg, want_tb))
    same(what, "the thresholds that rode with it", tau, want_tau)
    assert len(seg) == 0 and info == dict(overflow=0, tau_separate=0, threshold_launches=0, count_launches=0), (what, info)
    return want_tb


@pytest.mark.parametrize("name", list(M.TB_CASES))
def test_traceback(pkg, name):
    """The clean chain on a fresh context (every_entry: S > 4,096, the second copy runs), then the same with every off-chain entry of
    lb redrawn: the result must not change."""
    c = M.TB_CASES[name]
    n, L = c["n"], c["L"]
    ctx = context(pkg, M.TB_M, n, L, fresh=True)
    open_every = 3 if name == "every_entry" else 0
    clean = run_traceback(pkg, ctx, name + " clean", n, L, M.tb_arrays(name, False), open_every)
    assert len(clean) == len(c["chain"])
    run_traceback(pkg, ctx, name + " garbage", n, L, M.tb_arrays(name, True), open_every)
    # thresholds from launches of their own are not taken where no merge runs
    lb, mx, sz = M.tb_arrays(name, True)
    ent, hdr = M.lump_lists(M.TB_M, n, 2)
    tb, tau, seg, info = guarded(pkg, name, lambda: ctx.debug_merge_on_lists(2, ent, hdr, lb, mx, sz, separate=True))
    same(name + " separate", "the traceback", tb, as_device(pkg, clean))
    assert len(tau) == 0 and len(seg) == 0 and info == dict(overflow=0, tau_separate=1, threshold_launches=0, count_launches=0), info


def test_traceback_on_a_reused_context(pkg):
    """One context, S = 5,000, 100, 116, 117, 4,097, 100, 117: the first copy fetches the count of the call before + 16 entries and
    thresholds, a second copy the rest.  Every third column's list is cut, so a threshold names its column."""
    n, L = M.REUSE_N, M.REUSE_L
    ctx = context(pkg, M.TB_M, n, L, fresh=True)
    for i, S in enumerate(M.REUSE_S):
        arrays = M.chain_arrays(n, L, tuple(M.reuse_chain(i)), bool(i % 2), 700 + i)
        tb = run_traceback(pkg, ctx, "reuse call %d, S = %d" % (i, S), n, L, arrays, open_every=3)
        assert len(tb) == S


# ---- the traceback, by parts
@pytest.mark.parametrize("name", list(M.TB_CASES))
def test_traceback_parts(pkg, name):
    c = M.TB_CASES[name]
    n, L, chain = c["n"], c["L"], c["chain"]
    dp_size = n - L + 1
    pointers = M.foreign_pointers(n, L, len(name))
    for dirty in (False, True):
        lb, mx, sz = M.tb_arrays(name, dirty)
        want = as_device(pkg, M.traceback(n, L, lb, mx, sz))
        for layout, part_lo in M.part_layouts(name).items():
            for foreign in (None, pointers):
                what = "%s %s parts=%s%s foreign=%s" % (name, layout, part_lo[:4], "..." if len(part_lo) > 4 else "", "NULL" if foreign is None else "pointers")
                tb, ents, wins = guarded(pkg, what, lambda: pkg.traceback_parts(n, L, lb, mx, sz, part_lo, foreign))
                want_ents, want_wins = M.part_profile(chain, part_lo, dp_size)
                print(what, "entries", ents.tolist(), "windows", wins.tolist())
                same(what, "the traceback", tb, want)
                assert ents.tolist() == want_ents.tolist(), (what, ents.tolist(), want_ents.tolist())
                assert wins.tolist() == want_wins.tolist(), (what, wins.tolist(), want_wins.tolist())


# ---- the merge
def run_merge(pkg, name, separate, splits=()):
    G, lb, mx, sz = M.mg_case(name)
    want_tb, want_tau, want_seg, want_overflow, _ = M.mg_expected(name)
    S = len(want_tb)
    ctx = context(pkg, G.m, G.n, G.L)
    what = "%s separate=%d splits=%s" % (name, separate, list(splits))
    tb, tau, seg, info = guarded(pkg, what, lambda: ctx.debug_merge_on_lists(G.X, G.ent, G.hdr, lb, mx, sz, separate=separate, col_splits=splits))
    print(what, "S", len(tb), "tau", len(tau), "segments", len(seg), info)
    same(what, "the traceback", tb, as_device(pkg, want_tb))
    merges = G.max_seg < G.m and S > 1
    if not separate or merges:
        same(what, "the thresholds", tau, want_tau)
    else:
        assert len(tau) == 0, what
    assert info["overflow"] == int(want_overflow) and info["tau_separate"] == int(separate), (what, info)
    same(what, "the merged segments", seg, want_seg.astype(pkg.SEGMENT_DTYPE))
    ranges = len(splits) + 1
    asked = merges and not want_overflow and any(int(s["segment_size"]) < 100000 for s in want_seg)   # (a size that is a count, not an entry's own)
    assert info["threshold_launches"] == (ranges if separate and merges else 0), (what, info)
    assert info["count_launches"] == (ranges if separate and asked else 0), (what, info)
    return tb, tau, seg, info


@pytest.mark.parametrize("separate", [False, True])
@pytest.mark.parametrize("name", list(M.MG_CASES))
def test_merge(pkg, name, separate):
    """The thresholds both ways: riding with the traceback (k_seg_tau_tb), and from launches of their own (k_seg_tau, the merged
    sizes from k_seg_count) over all columns as one range."""
    if name == "large_S" and not separate:
        context(pkg, M.MG_M, M.mg_case(name)[0].n, M.MG_L, fresh=True)              # S > 4,096 on a fresh context: the second copy of the thresholds
    run_merge(pkg, name, separate)


@pytest.mark.parametrize("name", list(M.MG_CASES))
def test_merge_over_column_ranges(pkg, name):
    """Thresholds and counts once per column range, summed on the host: a boundary column equal to a split, one below a split, a
    range without a boundary, eight ranges.  The result is the unsplit run's (both are the model's)."""
    whole = run_merge(pkg, name, True)
    for layout, splits in M.split_layouts(name).items():
        got = run_merge(pkg, name, True, splits)
        for a, b in zip(whole[:3], got[:3]):
            assert a.tobytes() == b.tobytes(), (name, layout)


# ---- the entry itself
def test_refusals(pkg):
    G, lb, mx, sz = M.mg_case("tau_edges")
    chain = M.chain_of(G.n, G.L, lb)

    def refused(call, code=E_ARG, says=None):
        with pytest.raises(pkg.FseqError) as e:
            call()
        assert e.value.code == code, e.value
        assert says is None or says in str(e.value), e.value

    ctx = pkg.SegmentationContext(G.m, G.n, G.L)
    refused(lambda: ctx.debug_merge_on_lists(G.X, G.ent, G.hdr, lb, mx, sz))                       # no input set
    ctx.generate_synthetic(1, 4, 100, 0.0)
    bad = G.hdr.copy()
    bad[G.rbs[2] - 1, 0] = G.ent.shape[1] + 1
    refused(lambda: ctx.debug_merge_on_lists(G.X, G.ent, bad, lb, mx, sz), says="rule 1")           # a list a kernel could index out of
    for t in (chain[0], chain[2], chain[-1]):
        for v in (t + 1, G.L - 1, M.NONE):
            wrong = lb.copy()
            wrong[t] = v
            refused(lambda: ctx.debug_merge_on_lists(G.X, G.ent, G.hdr, wrong, mx, sz), says="chain entry %d" % t)
    off = lb.copy()
    off[chain[1] + 1] = M.NONE                                                                       # off the chain: anything goes
    ctx.debug_merge_on_lists(G.X, G.ent, G.hdr, off, mx, sz)
    refused(lambda: ctx.debug_merge_on_lists(G.X, G.ent, G.hdr, lb, mx, sz, separate=False, col_splits=[50]))
    for splits in ([0], [G.n], [50, 50], [70, 30]):
        refused(lambda: ctx.debug_merge_on_lists(G.X, G.ent, G.hdr, lb, mx, sz, separate=True, col_splits=splits))
    refused(lambda: ctx.debug_merge_on_lists(G.X + 2, G.ent, G.hdr, lb, mx, sz))                     # the stride is the capacity's
    L_ = pkg.load_library()
    assert L_.fseq_debug_merge_on_lists(ctx.h, G.X, G.ent.ctypes.data, G.hdr.ctypes.data, lb.ctypes.data, mx.ctypes.data, sz.ctypes.data, 2, None, 0,
                                        None, None, None, None, None, None, None) == E_ARG            # an unknown flag
    ctx.set_list_memory(1 << 20)
    refused(lambda: ctx.debug_merge_on_lists(G.X, G.ent, G.hdr, lb, mx, sz), E_UNSUPPORTED)
    ctx.close()


def test_run_after_the_debug_entry_equals_a_fresh_contexts(pkg):
    """The entry leaves no result on the context and nothing a following run would see."""
    G, lb, mx, sz = M.mg_case("alternating")

    def outcome(ctx):
        res = ctx.run()
        return (res.max_segment_size, ctx.traceback().tobytes(), ctx.reduced_traceback().tobytes(), [a.tobytes() for a in ctx.debug_dp()])

    fresh = pkg.SegmentationContext(G.m, G.n, G.L)
    fresh.generate_synthetic(0x5EED, 8, 500, 1e-3)
    want = outcome(fresh)
    fresh.close()
    used = pkg.SegmentationContext(G.m, G.n, G.L)
    used.generate_synthetic(0x5EED, 8, 500, 1e-3)
    assert outcome(used) == want                                                                     # a result to lose
    used.debug_merge_on_lists(G.X, G.ent, G.hdr, lb, mx, sz)
    with pytest.raises(pkg.FseqError) as e:                                                          # no result is held
        used.debug_dp()
    assert e.value.code == E_ARG
    room = np.zeros(G.n, dtype=pkg.DPARG_DTYPE)
    assert pkg.load_library().fseq_get_traceback(used.h, room.ctypes.data) == E_ARG and not room.view(np.uint8).any()
    assert outcome(used) == want
    used.debug_merge_on_lists(G.X, G.ent, G.hdr, lb, mx, sz, separate=True, col_splits=[40, 41])
    assert outcome(used) == want
    used.close()
    virgin = pkg.SegmentationContext(G.m, G.n, G.L)                                                  # and on a context that has never run
    virgin.generate_synthetic(0x5EED, 8, 500, 1e-3)
    virgin.debug_merge_on_lists(G.X, G.ent, G.hdr, lb, mx, sz)
    assert outcome(virgin) == want
    virgin.close()


def test_release_held_context():
    if _held["ctx"] is not None:
        _held["ctx"].close()
        _held.update(shape=None, ctx=None)
