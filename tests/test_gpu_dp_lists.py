"""Phase D on the card, kernel by kernel, on constructed column lists (tests/dp_list_cases.py: the model, the generators and the
table; tests/test_dp_list_cases.py checks on the CPU that every case asks what it is listed for).  fseq_debug_dp_on_lists runs the
production launchers on the lists: k_dp whole, k_dp resumed at the case's cut rounds, and the speculative sweeps under the library's
own plan and under forced ones.  LB, M and SZ over the entries a cell writes and the "a list was too short" word are the model's,
bit for bit; there is no tolerance anywhere."""
import importlib

import numpy as np
import pytest

import dp_list_cases as D

pytestmark = pytest.mark.gpu

E_ARG, E_HIP, E_UNSUPPORTED = 1, 3, 5
KNOBS = ("FSEQ_DP_SERIAL", "FSEQ_DP_SPEC_ROUNDS", "FSEQ_DP_SPEC_WIN", "FSEQ_DP_SPEC_MAX_SWEEPS")


@pytest.fixture(scope="module")
def pkg():
    return importlib.import_module("founder-sequences_amd")


# one context per shape, reused across the cases and modes of that shape (the table keeps equal shapes together); its rows are a
# generated alignment the DP never reads
_held = {"shape": None, "ctx": None, "knobs": {}}


def context(pkg, m, n, L, knobs):
    if _held["shape"] != (m, n, L):
        if _held["ctx"] is not None:
            _held["ctx"].close()
        ctx = pkg.SegmentationContext(m, n, L)
        ctx.generate_synthetic(0x5EED, 8, 500, 1e-3)
        _held.update(shape=(m, n, L), ctx=ctx, knobs={})
    ctx = _held["ctx"]
    for name in KNOBS:
        want = knobs.get(name)
        if _held["knobs"].get(name) != want:
            ctx.set_tuning(name, want)
            _held["knobs"][name] = want
    return ctx


def default_cuts(S):
    """Cut rounds for a case that lists none: after the first round, a launch of one round a third of the way in, the final cell alone."""
    third = S["nreg"] // 3
    return tuple(sorted({r for r in (1, third, third + 1, S["nrounds"] - 1) if 0 < r < S["nrounds"]}))


def run_and_compare(pkg, name, knobs, cuts=()):
    c = D.CASES[name]
    m, n, L = c["m"], c["n"], c["L"]
    X, ent, hdr = D.device_lists(name)
    ctx = context(pkg, m, n, L, knobs)
    try:
        lb, mx, sz, info = ctx.debug_dp_on_lists(X, ent, hdr, cuts)
    except pkg.FseqError as e:
        if e.code == E_HIP:
            pytest.exit("%s knobs=%s cuts=%s: %s -- nothing more is started on a device that has faulted" % (name, knobs, list(cuts), e), returncode=3)
        raise
    what = "%s knobs=%s cuts=%s info=%s" % (name, knobs, list(cuts), info)
    assert info["unproven"] == D.expect_unproven(name), what
    if D.compared_by_arrays(name):
        LB, M, SZ = D.reference(name)
        w = D.written_entries(n, L)
        for label, got, want in (("M", mx, M), ("LB", lb, LB), ("SZ", sz, SZ)):
            bad = np.nonzero(got[w] != want[w])[0]
            assert not len(bad), "%s: %s differs at %d entries, first at entry %d: device %d, model %d" % (
                what, label, len(bad), int(w[bad[0]]), int(got[w[bad[0]]]), int(want[w[bad[0]]]))
    return info


@pytest.mark.parametrize("name", list(D.CASES))
def test_serial_whole(pkg, name):
    info = run_and_compare(pkg, name, {"FSEQ_DP_SERIAL": "1"})
    assert info["dp_chunks"] == 0 and info["launches"] == 1


@pytest.mark.parametrize("name", list(D.CASES))
def test_resumed_at_cut_rounds(pkg, name):
    c = D.CASES[name]
    cuts = c["cuts"] or default_cuts(D.schedule(c["L"], c["n"]))
    info = run_and_compare(pkg, name, {"FSEQ_DP_SERIAL": "1"}, cuts)
    assert info["launches"] == len(cuts) + 1


@pytest.mark.parametrize("name", list(D.CASES))
def test_speculative_own_plan(pkg, name):
    """The DP as a run chooses it: the speculative sweeps wherever the library's plan has three chunks, else the serial kernel."""
    info = run_and_compare(pkg, name, {})
    assert (info["dp_chunks"] >= 3 and info["launches"] == 0) or (info["dp_chunks"] == 0 and info["launches"] == 1), info


@pytest.mark.parametrize("name,plan", [(n, p) for n in D.CASES for p in D.CASES[n]["plans"]])
def test_speculative_forced_plans(pkg, name, plan):
    rounds, win, sweeps = plan
    knobs = {}
    if rounds:
        knobs["FSEQ_DP_SPEC_ROUNDS"] = str(rounds)
    if win:
        knobs["FSEQ_DP_SPEC_WIN"] = str(win)
    if sweeps:
        knobs["FSEQ_DP_SPEC_MAX_SWEEPS"] = str(sweeps)
    info = run_and_compare(pkg, name, knobs)
    assert info["dp_chunks"] >= 2, info
    if rounds:
        S = D.schedule(D.CASES[name]["L"], D.CASES[name]["n"])
        assert info["dp_chunks"] == (S["nreg"] + rounds - 1) // rounds, info
    if sweeps:
        # (the budget ran out: the serial kernel took over behind the first dirty chunk, a resumed launch -- or the sweeps were done within it)
        assert info["dp_sweeps"] >= 1000 + sweeps or info["dp_sweeps"] <= sweeps, info


def test_run_after_the_debug_entry_equals_a_fresh_contexts(pkg):
    """The entry leaves no result on the context and nothing a following run would see."""
    name = "spec_classic"
    c = D.CASES[name]
    m, n, L = c["m"], c["n"], c["L"]
    X, ent, hdr = D.device_lists(name)

    def outcome(ctx):
        res = ctx.run()
        return (res.max_segment_size, ctx.traceback().tobytes(), ctx.reduced_traceback().tobytes(), [a.tobytes() for a in ctx.debug_dp()],
                [x.tobytes() for i in range(min(3, res.segment_count)) for x in ctx.boundary_state(i)])

    fresh = pkg.SegmentationContext(m, n, L)
    fresh.generate_synthetic(0x5EED, 8, 500, 1e-3)
    want = outcome(fresh)
    fresh.close()
    used = pkg.SegmentationContext(m, n, L)
    used.generate_synthetic(0x5EED, 8, 500, 1e-3)
    first = outcome(used)                              # a result to lose
    assert first == want
    used.debug_dp_on_lists(X, ent, hdr)
    with pytest.raises(pkg.FseqError) as e:            # no result is held
        used.debug_dp()
    assert e.value.code == E_ARG
    with pytest.raises(pkg.FseqError):
        used.debug_column_list(L)
    assert outcome(used) == want
    used.debug_dp_on_lists(X, ent, hdr, (1, 2))
    assert outcome(used) == want
    used.close()
    # and before any run, on a context that has never run
    virgin = pkg.SegmentationContext(m, n, L)
    virgin.generate_synthetic(0x5EED, 8, 500, 1e-3)
    virgin.debug_dp_on_lists(X, ent, hdr)
    assert outcome(virgin) == want
    virgin.close()


def test_refusals(pkg):
    name = "strips_33"
    c = D.CASES[name]
    m, n, L = c["m"], c["n"], c["L"]
    X, ent, hdr = D.device_lists(name)
    S = D.schedule(L, n)

    def refused(call, code=E_ARG):
        with pytest.raises(pkg.FseqError) as e:
            call()
        assert e.value.code == code, e.value

    ctx = pkg.SegmentationContext(m, n, L)
    refused(lambda: ctx.debug_dp_on_lists(X, ent, hdr))                               # no input set
    ctx.generate_synthetic(1, 4, 100, 0.0)
    bad = hdr.copy()
    bad[L + 5, 0] = ent.shape[1] + 1
    refused(lambda: ctx.debug_dp_on_lists(X, ent, bad))                               # a list the kernel could index out of
    for cuts in ((0,), (S["nrounds"],), (5, 5), (7, 3)):
        refused(lambda: ctx.debug_dp_on_lists(X, ent, hdr, cuts))
    refused(lambda: ctx.debug_dp_on_lists(X + 2, ent, hdr))                           # the stride is the capacity's
    ctx.set_list_memory(1 << 20)
    refused(lambda: ctx.debug_dp_on_lists(X, ent, hdr), E_UNSUPPORTED)
    ctx.close()
    short = pkg.SegmentationContext(m, 2 * L - 1, L)
    short.generate_synthetic(1, 4, 100, 0.0)
    refused(lambda: short.debug_dp_on_lists(X, ent[:2 * L - 1], hdr[:2 * L - 1]))
    short.close()
