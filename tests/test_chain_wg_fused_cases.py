"""CPU: every case of tests/chain_wg_fused_cases.py has the property it is listed for, on its inputs alone -- where its runs lie against
the chunks of the kernel's waves, which waves have no positions, that the spikes at the chunk borders decide a head's divergence,
how many runs it has against the cap.  tests/test_gpu_chain_wg_fused.py runs the same cases through k_chain_wg."""
import numpy as np
import pytest

import chain_step_cases as cs
import chain_wg_cases as cw
import chain_wg_fused_cases as cf

BY = {c["id"]: c for c in cf.FUSED_CASES}


def starts_of(B):
    return cs.run_starts(B["a"], B["rank"][0])


def chunks(m):
    ch = cw.chunk(m)
    return [(min(m, w * ch), min(m, (w + 1) * ch)) for w in range(cw.NW)]


@pytest.mark.parametrize("case", cf.FUSED_CASES, ids=[c["id"] for c in cf.FUSED_CASES])
def test_every_step_takes_the_listed_form(case):
    B = cf.build_fused(case)
    assert np.array_equal(B["rank"][0][B["a"]], B["kp"]) and B["rank"].max() < B["nkeys"][0]
    sa, sd = cw.launch_args(case, B)
    steps, stats = cw.walk(B["rank"], B["keyd"], B["nkeys"], 1, cs.COLS, 0, 1, sa, sd, False, case["run_cap"])
    assert [[s[1] for s in ch] for ch in steps] == [list(case["paths"])]
    if case["runs"] is not None:
        assert [s[2] for s in steps[0]] == list(case["runs"])
    assert stats[:3].sum() == 1


def test_the_table_holds_the_five_kinds():
    names = {c["name"] for c in cf.FUSED_CASES}
    assert {"span", "edges", "carry-spikes", "cap-crossing", "cap+1-crossing"} <= names and any(n.startswith("small-") for n in names)
    assert sorted({c["m"] for c in cf.FUSED_CASES}) == [65, 700, 11265, 12288] and cf.SMALL_M == (700, 65)


@pytest.mark.parametrize("m", [11265, 12288])
def test_runs_that_span_whole_chunks(m):
    B = cf.build_fused(BY["%d-span" % m])
    st = starts_of(B)
    ch = cw.chunk(m)
    assert np.all(np.diff(st) == 3 * ch + 5)
    # chunks without a start: everything such a wave sees is carry-in
    bare = [w for w, (lo, hi) in enumerate(chunks(m)) if lo < hi and not np.any((st >= lo) & (st < hi))]
    assert len(bare) >= 8
    # ... two or more of them in a row inside one run
    assert any(w + 1 in bare for w in bare)
    # the extreme: chain_wg_cases' one-key cases, one run over every chunk
    assert ("one",) in [c["blocks"][0] for c in cw.WG_CASES if c["m"] == m]


@pytest.mark.parametrize("m", [11265, 12288])
def test_starts_at_a_chunks_first_and_last_position(m):
    B = cf.build_fused(BY["%d-edges" % m])
    st = set(starts_of(B).tolist())
    for lo, hi in chunks(m):
        if lo < hi:
            assert lo in st
            if hi - lo == cw.chunk(m):
                assert hi - 1 in st
    assert len(st) >= 2 * 14


def test_waves_with_empty_chunks():
    assert cw.chunk(700) == 64 and cw.chunk(65) == 64
    assert [w for w, (lo, hi) in enumerate(chunks(700)) if lo == hi] == [11, 12, 13, 14, 15]
    c65 = chunks(65)
    assert c65[0] == (0, 64) and c65[1] == (64, 65) and all(lo == hi for lo, hi in c65[2:])
    for m in cf.SMALL_M:
        assert m < cs.M_MIN
        forms = {BY["%d-%s" % (m, n)]["paths"][0] for n in ("small-runs", "small-one", "small-heads", "small-sort")}
        assert forms == {"runs", "sort"}
        B = cf.build_fused(BY["%d-small-runs" % m])
        assert len(starts_of(B)) == min(m // 3, 40)
    # a run across the border of the only two chunks of 65 rows with a position: one key
    assert len(starts_of(cf.build_fused(BY["65-small-one"]))) == 1


@pytest.mark.parametrize("m", [11265, 12288])
def test_the_spikes_at_the_chunk_borders_bite(m):
    """Inside the run across every chunk border: a spike at the chunk's last position, at the next chunk's first, or both.  The run
    is the one whole run in the range of the head behind it, so the head's divergence IS the spike: with either spike dropped from
    the run's maximum (what a lost open run, or a lost carry-in, does) the model's output differs."""
    case = BY["%d-carry-spikes" % m]
    B = cf.build_fused(case)
    st = starts_of(B)
    cuts, borders = cf.border_cuts(m)
    assert np.array_equal(st, cuts) and len(borders) >= 14
    a1, d1 = cs.chain_step(B["a"], B["d"], B["rank"][0], B["keyd"][0])
    kinds = set()
    for c, b in enumerate(borders.tolist(), start=1):
        j = int(np.searchsorted(st, b, side="right")) - 1              # the run across the border
        assert st[j] < b - 1 and b + 1 < st[j + 1] and j >= 1 and B["kp"][st[j + 1]] == B["kp"][st[j] - 1] != B["kp"][b]
        spiked = [p for p in (b - 1, b) if B["d"][p] >= cf.SPIKE]
        kinds.add(tuple(p - b for p in spiked))
        top = max(spiked, key=lambda p: B["d"][p])
        # the head behind the run takes the run's maximum: the higher spike
        head_new = int(np.flatnonzero(a1 == B["a"][st[j + 1]])[0])
        assert d1[head_new] == B["d"][top] and B["d"][top] > np.delete(B["d"][st[j]:st[j + 1] + 1], top - st[j]).max()
        dropped = B["d"].copy()
        dropped[top] = 0
        _, d1x = cs.chain_step(B["a"], dropped, B["rank"][0], B["keyd"][0])
        assert d1x[head_new] != d1[head_new]
    assert kinds == {(-1,), (0,), (-1, 0)}


def test_the_cap_with_its_last_run_across_a_border():
    m, ch = 12288, cw.chunk(12288)
    for name, R in (("cap-crossing", 100), ("cap+1-crossing", 101)):
        case = BY["%d-%s" % (m, name)]
        assert case["run_cap"] == 100
        st = starts_of(cf.build_fused(case))
        assert len(st) == R
        lo, hi = st[99], (st[100] if R == 101 else m)
        assert lo < 10 * ch < hi and (hi - 1) // ch - lo // ch >= 3     # run 99 of the cap's 100: across chunk borders, whole chunks inside it
    assert BY["%d-cap-crossing" % m]["paths"] == ("runs",) and BY["%d-cap+1-crossing" % m]["paths"] == ("sort",)
