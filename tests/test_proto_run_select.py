"""The bitmap select of the run steps (tests/run_select_cases.py states it in numpy as csrc/fseq_chainsort.hpp computes it) against the
search it replaces: for every new position, the run is np.searchsorted(off, p, "right") - 1 and the position is a head where
off[run] == p.  And, from the inputs alone, that the cases of tests/test_gpu_run_select.py ask for what they are listed for.  No GPU."""
import numpy as np
import pytest

import chain_step_cases as cs
import chain_wg_cases as cw
import run_select_cases as rs


@pytest.mark.parametrize("name", sorted(rs.LAYOUTS))
def test_select_equals_the_search(name):
    off, m = rs.layout(rs.LAYOUTS[name])
    bits, pre = rs.build_select(off, m)
    p = np.arange(m)
    run, head = rs.select(bits, pre, p)
    want = np.searchsorted(off, p, "right") - 1
    assert np.array_equal(run, want)
    assert np.array_equal(head, off[want] == p)
    # what the kernels hold: 16 bits a word's count of starts in front, at most 2^18 rows
    assert pre.max() < (1 << 16) and len(off) <= cw.CW_RUN_CAP and m <= rs.SEL_ROWS


def test_the_layouts_are_the_ones_listed():
    L = {k: rs.layout(v) for k, v in rs.LAYOUTS.items()}
    assert len(L["R1"][0]) == 1
    off, m = L["every-position-a-head"]
    assert len(off) == m and m % 64 != 0
    off, m = L["starts-0-31-32-63"]
    assert set(off % 64) == {0, 31, 32, 63} and m % 64 != 0
    for name in ("a-whole-word-of-starts", "every-position-a-head"):
        off, m = L[name]
        assert np.bincount(off >> 6).max() == 64
    off, m = L["a-word-of-64-starts"]
    assert np.all(np.diff(off[1:65]) == 1) and (off[1] >> 6) != (off[64] >> 6)         # 64 consecutive starts over two words
    off, m = L["long-runs"]
    lens = np.diff(np.r_[off, m])
    assert lens.max() > 128 and len(np.setdiff1d(np.arange((m + 63) // 64), off >> 6)) > 0     # (words with no start)
    assert len(L["most-runs"][0]) == cw.CW_RUN_CAP and L["most-runs"][1] == rs.SEL_ROWS


def runs_of(kp):
    return len(np.flatnonzero(np.r_[True, kp[1:] != kp[:-1]]))


@pytest.mark.parametrize("case", rs.PASS2_CASES, ids=[c["id"] for c in rs.PASS2_CASES])
def test_pass2_cases_ask_for_what_they_are_listed_for(case):
    B = rs.build_pass2(case)
    m = case["m"]
    for b, how in enumerate(case["blocks"]):
        kp = B["kp"][b]
        R = runs_of(kp)
        key = B["cls"][b][B["rank"][b]]
        assert np.array_equal(key[B["a0"][b]], kp)                        # (the task's classes by position are the case's)
        assert np.array_equal(B["hand_keys"][b], B["rank"][b][B["a0"][b]]) and B["hand_keys"][b].max() < (1 << 16)
        if case["runs"] is not None:
            assert R == case["runs"]
        assert cs.pass2_path(m, int(B["ncls"][b]), R, case["run_cap"]) == case["path"]
        # a block handed over starts (block x m) 16-bit words into the array: 16-byte aligned only where that is a multiple of 8
        if how == "handed" and m % 8 != 0 and b == 1:
            assert (b * m * 2) % 16 == 2 * (m % 8)
        if how == "handed":
            assert not B["rank_given"][b].any() and R > 1 or case["runs"] == 1
    st = np.flatnonzero(np.r_[True, B["kp"][0][1:] != B["kp"][0][:-1]])
    if case["keys"][0] == "edges":
        c = rs.chunk(m)
        assert set(st % 8) == set(range(8)) and {63, 64, 65} <= set(st)
        assert all({b - 1, b, b + 1} <= set(st) for b in range(c, m, c)) and len(range(c, m, c)) >= 14
        assert set(range(2048, 2057)) <= set(st) and 2048 % rs.PIECE == 0          # eight runs of one position in one lane's piece
        if m == 11265:
            assert c == 768 and (rs.NW - 1) * c >= m and m % rs.PIECE == 1 and m - 1 in st   # wave 15 idle; the last piece holds one position
    if case["keys"][0] == "new-positions":
        assert {0, 31, 32, 63} == set(rs.sorted_run_starts(B["kp"][0])[:-1] % 64)
        assert np.diff(np.r_[st, m]).max() > 128
    if case["keys"][0] == "far-pair":
        kp, d0 = B["kp"][0], B["d0"][0]
        at = np.flatnonzero(kp == 9)
        second = at[5]
        assert len(at) == 10 and second - at[4] > 128 and np.all(np.diff(at[:5]) == 1) and np.all(np.diff(at[5:]) == 1)
        # the head of the second run takes the maximum of d0 behind the first run up to itself: a spike between, above its own d0
        between = d0[at[4] + 1:second + 1]
        assert between.max() > d0[second] and between.max() > 0
    assert {11265, 11272, 12288, 12289} == {c["m"] for c in rs.PASS2_CASES}


def test_pass2_cases_cover_both_caps_on_both_sides():
    by = {(c["run_cap"], c["runs"]): c["path"] for c in rs.PASS2_CASES if c["runs"] is not None}
    assert by[(8832, 8832)] == "runs" and by[(8832, 8833)] == "p4" and by[(100, 100)] == "runs" and by[(100, 101)] == "p4"
    assert by[(8832, 1)] == "runs"
    assert any(c["blocks"] == ("handed", "handed") and c["m"] == 11265 for c in rs.PASS2_CASES)
    assert any(set(c["blocks"]) == {"handed", "gathered"} and c["m"] == 11265 for c in rs.PASS2_CASES)


@pytest.mark.parametrize("case", rs.CW_CASES, ids=[c["id"] for c in rs.CW_CASES])
def test_chain_wg_cases_take_the_run_path(case):
    B = cw.build_wg(case)
    sa, sd = cw.launch_args(case, B)
    steps, stats = cw.walk(B["rank"], B["keyd"], B["nkeys"], case["G"], cs.COLS, case["first"], case["chains"], sa, sd, case["keys"], case["run_cap"])
    assert [s[1] for ch in steps for s in ch] == list(case["paths"]) == ["runs"]
    if case["runs"] is not None:
        assert [s[2] for ch in steps for s in ch] == case["runs"]
    assert {rs.SEL_ROWS, rs.SEL_ROWS + 1} <= {c["m"] for c in rs.CW_CASES}
