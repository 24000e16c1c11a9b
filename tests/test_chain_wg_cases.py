"""CPU: every case of tests/chain_wg_cases.py has the property it is listed for, on its inputs alone -- the form every step takes,
its run count, the bits of its keys, where its runs lie, how many whole runs a head's range holds.  tests/test_gpu_chain_wg.py
runs the same cases through k_chain_wg."""
import numpy as np
import pytest

import chain_step_cases as cs
import chain_wg_cases as cw

BY = {c["id"]: c for c in cw.WG_CASES}


def steps_of(case, B=None):
    B = B or cw.build_wg(case)
    sa, sd = cw.launch_args(case, B)
    return cw.walk(B["rank"], B["keyd"], B["nkeys"], case["G"], cs.COLS, case["first"], case["chains"], sa, sd, case["keys"], case["run_cap"])


def whole_runs_between(a, key):
    """For every run but the first of its key: the whole runs between the previous run of its key and itself."""
    k = np.asarray(key)[np.asarray(a)]
    starts = cs.run_starts(a, key)
    rk = k[starts]
    last, out = {}, []
    for j, v in enumerate(rk.tolist()):
        if v in last:
            out.append(j - last[v] - 1)
        last[v] = j
    return np.array(out, dtype=np.int64), starts


@pytest.mark.parametrize("case", [c for c in cw.WG_CASES if c["m"] < 100000], ids=[c["id"] for c in cw.WG_CASES if c["m"] < 100000])
def test_every_step_takes_the_listed_form(case):
    steps, stats = steps_of(case)
    flat = [s for chain in steps for s in chain]
    assert [s[1] for s in flat] == list(case["paths"])
    if case["runs"] is not None:
        assert [s[2] for s in flat] == list(case["runs"])
    assert stats[0] + stats[1] + stats[2] == len(flat)
    assert len(steps) == case["chains"] and case["workgroups"] >= 1


def test_the_sizes_and_the_cap():
    ms = sorted({c["m"] for c in cw.WG_CASES})
    assert ms == [11265, 12288, 524289] and 11265 % 64 and 12288 % 1024 == 0
    for m in (11265, 12288):
        assert BY["%d-cap" % m]["runs"] == [BY["%d-cap" % m]["run_cap"]] and BY["%d-cap" % m]["paths"] == ("runs",)
        assert BY["%d-cap+1" % m]["runs"] == [BY["%d-cap+1" % m]["run_cap"] + 1] and BY["%d-cap+1" % m]["paths"] == ("sort",)
        assert BY["%d-cap0" % m]["run_cap"] == 0
        _, stats = steps_of(BY["%d-cap0" % m])
        assert stats[1] == 1 and stats[3] == 0 and not stats[4:].any()       # (the knob at 0: no run is counted)
        assert BY["%d-all-heads" % m]["runs"] == [m] and m <= cw.CW_RUN_CAP
        B = cw.build_wg(BY["%d-all-heads" % m])
        assert B["nkeys"][0] == m
        assert cw.build_wg(BY["%d-one-key" % m])["nkeys"][0] == 1
    assert all(c["run_cap"] <= cw.CW_RUN_CAP for c in cw.WG_CASES)


def test_key_and_position_bits():
    """20 position bits: 12 key bits share the word, 13 do not -- with the same 6,000 runs, far below the cap."""
    m = 524289
    assert cs.bits_of(m - 1) == 20 and cs.bits_of(4096 - 1) == 12 and cs.bits_of(4097 - 1) == 13
    assert cw.step_path(m, 4096, 6000, cw.CW_RUN_CAP, False) == "runs" and cw.step_path(m, 4097, 6000, cw.CW_RUN_CAP, False) == "sort"
    for name, nk in (("bits-32", 4096), ("bits-33", 4097)):
        c = BY["%d-%s" % (m, name)]
        assert c["blocks"] == (("runs", 6000, nk),) and c["runs"] == [6000] and c["run_cap"] == cw.CW_RUN_CAP
    # (the streamed regime ends below 2^20 rows, and the cap is below 2^15: no smaller m has such a step of few runs)
    assert cw.CW_RUN_CAP < 4097 * 4 and cs.M_MAX < (1 << 20)


@pytest.mark.parametrize("m", [11265, 12288])
def test_where_the_runs_lie(m):
    # every border of a 64-group and of a wave's chunk inside a run
    case = BY["%d-borders" % m]
    B = cw.build_wg(case)
    k = B["rank"][0][B["a"]]
    inner = np.arange(64, m, 64)
    assert np.all(k[inner] == k[inner - 1])
    ch = cw.chunk(m)
    assert ch % 64 == 0 and 0 < ch < m and k[ch] == k[ch - 1]
    # the whole runs a head's range holds
    for name, lo, hi in (("one-between", 1, 1), ("many-between", 2, 2), ("far-between", 3999, 3999), ("alternate", 1, 1)):
        case = BY["%d-%s" % (m, name)]
        B = cw.build_wg(case)
        gaps, starts = whole_runs_between(B["a"], B["rank"][0])
        assert len(gaps) and gaps.min() == lo and gaps.max() == hi, name
        if name == "alternate":
            assert np.all(np.diff(np.r_[starts, m]) == 1)
        if name == "far-between":
            # blocks of 64 runs between: the levels of the table over them
            assert (3999 // 64 - 1).bit_length() - 1 == 5
    # runs are maximal: no head's range without a whole run, in any case
    for case in cw.WG_CASES:
        if case["m"] != m or case["own_start"] is False:
            continue
        B = cw.build_wg(case)
        seq_a, _ = cs.sequential_states(B["a"], B["d"], B["rank"], B["keyd"])
        for b in range(len(B["nkeys"])):
            gaps, _ = whole_runs_between(seq_a[b], B["rank"][b])
            assert not len(gaps) or gaps.min() >= 1


def test_chains_and_workgroups():
    for m in (11265, 12288):
        for wg in (1, 3):
            assert BY["%d-five-chains-wg%d" % (m, wg)]["chains"] == 5 and BY["%d-five-chains-wg%d" % (m, wg)]["workgroups"] == wg
            assert BY["%d-five-chains-G2-wg%d" % (m, wg)]["chains"] == 5
        assert BY["%d-expand-G2-first1" % m]["first"] == 1
        assert BY["%d-ident-G1" % m]["G"] == 1 and BY["%d-ident-G3" % m]["G"] == 3 and BY["%d-ident-G3" % m]["keys"]
        # an expansion leaves the state behind a chain's last block alone unless that is the last of all
        case = BY["%d-expand-G2" % m]
        B = cw.build_wg(case)
        sa, sd = cw.launch_args(case, B)
        want = cs.chain(B["rank"], B["keyd"], B["nkeys"], 2, cs.COLS, 0, 3, sa, sd)
        assert np.all(want["state_a"][[0, 1, 2, 3, 4, 5]] != cs.NOT_WRITTEN)     # (every state is some chain's to write in a whole launch)
        case = BY["%d-expand-G2-first1" % m]
        sa, sd = cw.launch_args(case, B)
        want = cs.chain(B["rank"], B["keyd"], B["nkeys"], 2, cs.COLS, 1, 2, sa, sd)
        assert np.all(want["state_a"][[0, 1]] == cs.NOT_WRITTEN) and np.all(want["state_a"][[2, 3, 4, 5]] != cs.NOT_WRITTEN)
        # chain 1 alone steps through block 2 only: the state behind block 3 (in front of block 4) stays unwritten
        case = BY["%d-expand-G2-chain1-alone" % m]
        assert case["first"] == 1 and case["chains"] == 1 and case["blocks"] == BY["%d-expand-G2" % m]["blocks"]
        B1 = cw.build_wg(case)
        sa, sd = cw.launch_args(case, B1)
        want = cs.chain(B1["rank"], B1["keyd"], B1["nkeys"], 2, cs.COLS, 1, 1, sa, sd)
        assert np.all(want["state_a"][[0, 1, 4, 5]] == cs.NOT_WRITTEN) and np.all(want["state_a"][[2, 3]] != cs.NOT_WRITTEN)
        assert [[s[0] for s in ch] for ch in steps_of(case, B1)[0]] == [[2]]


def test_the_spread_kernels_cases_through_the_forms():
    """chain_step_cases.CHAIN_CASES, which the GPU test forces through k_chain_wg, hold all three forms -- a step that sorts because
    its key and position bits exceed a word among them."""
    seen = set()
    for case in cs.CHAIN_CASES:
        if case["m"] > 70000:
            continue
        nk = [n for n in case["nkeys"] if not isinstance(n, tuple)]
        if not case["own_start"]:
            seen.add("ident")
        if any(not cw.counts_runs(case["m"], n, cw.CW_RUN_CAP) for n in nk):
            seen.add("wide")
        if any(n <= 2 for n in nk):
            seen.add("runs")
    assert seen == {"ident", "wide", "runs"}
