"""CPU checks of tests/merge_list_cases.py, the tables tests/test_gpu_merge_lists.py runs on the device: the model of the traceback
and the greedy merge on the oracle's DP array and complete lists of real alignments is the oracle's own traceback and reduced
traceback, field for field; every case passes the host validator of the lists and reaches what it is listed for, computed from the
model alone (the strip a threshold falls in, the doubling rounds, whether the second copy runs, the parts a chain passes); the chain
check runs under the host sanitizers as a program of its own; and both debug entries refuse, without a device, what they must."""
import importlib
import os
import subprocess

import numpy as np
import pytest

import merge_list_cases as M
import fso
import proto_length_scan as P
import segment_length_cases as SL

E_ARG = 1


@pytest.fixture(scope="module")
def pkg():
    build = importlib.import_module("founder-sequences_amd.build")
    build.build()
    return importlib.import_module("founder-sequences_amd")


# ---- the model is the oracle's
@pytest.mark.parametrize("L", [1, 2, 7, 20])
def test_model_on_the_oracles_dp_is_the_oracles_traceback_and_merge(pkg, L):
    case = SL.small_long(L)
    msa = SL.make(case)
    m, n = msa.shape
    ref = fso.segment_long(msa, L, keep_dp=True)
    dp = ref["dp"]
    counts = P.column_counts(msa)
    lists = [P.column_list(v, c, k, L, P.UNCUT) for k, (v, c) in enumerate(counts)]
    stride = max(len(e) for e, _ in lists)
    ent = np.zeros((n, stride, 2), dtype=np.uint32)
    hdr = np.zeros((n, 4), dtype=np.uint32)
    for k, (e, h) in enumerate(lists):
        ent[k, :len(e)] = e
        hdr[k] = h
    assert pkg.dp_lists_check(m, L, ent, hdr) is None
    lb = dp["lb"].astype(np.uint32)
    tb = M.traceback(n, L, lb, dp["segment_max_size"], dp["segment_size"])
    want = ref["traceback"]
    assert len(tb) == len(want) >= 3
    for f in ("lb", "rb", "segment_max_size", "segment_size"):
        assert np.array_equal(tb[f], want[f]), f
    seg, overflow, at = M.merge(m, tb, ent, hdr)
    red = ref["reduced"]
    assert not overflow and at is None and len(seg) == len(red) >= 2 and (len(seg) < len(tb) or L == 1)
    assert np.array_equal(seg["lb"], red["lb"]) and np.array_equal(seg["rb"], red["rb"]) and np.array_equal(seg["segment_size"], red["segment_size"])
    # the thresholds say what the counts say: a boundary joins at current_lb iff kind != NEVER and current_lb >= tau
    tau = M.thresholds(tb, ent, hdr)
    max_seg = int(tb[-1]["segment_max_size"])
    for j in range(1, len(tb)):
        values = M.multiset(ent, hdr, int(tb[j]["rb"]) - 1)
        for cur in {0, int(tb[j - 1]["rb"]), int(tau[j, 0]) if tau[j, 1] != M.TAU_NEVER else 0, max(0, int(tau[j, 0]) - 1) if tau[j, 1] != M.TAU_NEVER else 0}:
            fits = tau[j, 1] != M.TAU_NEVER and cur >= tau[j, 0]
            assert fits == (int((values > cur).sum()) <= max_seg), (j, cur, tau[j])


# ---- the traceback cases
@pytest.mark.parametrize("name", list(M.TB_CASES))
def test_traceback_case_reaches_what_it_is_listed_for(pkg, name):
    c = M.TB_CASES[name]
    n, L, chain = c["n"], c["L"], c["chain"]
    dp_size = n - L + 1
    assert n >= 2 * L and chain[0] == dp_size - 1
    ent, hdr = M.lump_lists(M.TB_M, n, 2)
    assert pkg.dp_lists_check(M.TB_M, L, ent, hdr) is None
    for dirty in (False, True):
        lb, mx, sz = M.tb_arrays(name, dirty)
        assert M.chain_of(n, L, lb) == chain and mx[n - L] == M.TB_M                # garbage leaves the chain alone; no merge runs
        tb = M.traceback(n, L, lb, mx, sz)
        assert len(tb) == len(chain) and tb[0]["lb"] == 0 and tb[-1]["rb"] == n
    dirty_lb = M.tb_arrays(name, True)[0]
    off = np.ones(dp_size, dtype=bool)
    off[chain] = False
    g = dirty_lb[off].astype(np.int64)
    t = np.arange(dp_size)[off]
    if off.sum() > 1000:
        # every kind of word stands off the chain: 0, below L, upwards, beyond the array, all ones, valid-looking pointers
        assert (g == 0).any() and (g == M.NONE).any() and ((g >= t + L) & (g < dp_size + L)).any() and ((g > dp_size + L) & (g < M.NONE)).any()
        assert ((g >= L) & (g <= t)).sum() > dp_size // 8 and (L == 1 or ((g > 0) & (g < L)).any())
    prof = M.window_profile(chain)
    want = c["listed_for"]
    if "S" in want:
        assert len(chain) == want["S"]
    if "windows" in want:
        assert [w for w, _, _ in prof] == want["windows"]
    if "full_window" in want:
        # a window that holds ceil(W / L) chain entries, entered at its top entry: the doubling needs every round it has
        assert any(cnt == want["full_window"] == -(-M.W // L) and top for _, cnt, top in prof), prof
        assert M.doubling_rounds(L) == want["rounds"] and 2 ** want["rounds"] >= want["full_window"] > 2 ** (want["rounds"] - 2)
    if "second_copy" in want:
        assert len(chain) > M.FIRST_COPY
    if "successor_at_base" in want:
        for key, below in (("successor_at_base", 0), ("successor_below_base", 1)):
            i = chain.index(want[key])
            assert (want[key] + below) % M.W == 0 and i > 0 and chain[i - 1] // M.W == (want[key] + below) // M.W
        assert chain[-1] == 0
    if "two_in_a_window" in want:
        pairs = [(a, b) for a, b in zip(chain, chain[1:]) if a // M.W == b // M.W]
        assert len(pairs) == want["two_in_a_window"] and all(a % M.W == L and b % M.W == 0 for a, b in pairs)
        assert M.doubling_rounds(L) == (2 if L <= M.W else 1)        # W / L + 2 = 3, or 2
    if name == "one_segment_W_plus_1":
        assert dp_size == M.W + 1 and prof == [(1, 1, False)]
    if name == "ends_in_window_2_of_4":
        assert (dp_size + M.W - 1) // M.W == 4 and chain[-1] // M.W == 2
    if name == "skipped_windows":
        assert (dp_size + M.W - 1) // M.W == 7


def test_traceback_table_covers_the_listed_shapes():
    names = set(M.TB_CASES)
    assert {"one_segment_100", "one_segment_W_plus_1", "every_entry", "borders", "ends_in_window_2_of_4", "skipped_windows"} <= names
    assert {"min_stride_L%d_%d" % (L, d) for L in (2, 3, 7) for d in (2 * M.W - 1, 2 * M.W, 2 * M.W + 1)} <= names
    assert {"large_L%d" % L for L in (8191, 8192, 8193)} <= names
    assert all(M.TB_CASES["large_L%d" % L]["n"] == 6 * L + 37 for L in (8191, 8192, 8193))
    assert M.TB_CASES["every_entry"]["n"] == 3 * M.W + 5 and M.TB_CASES["skipped_windows"]["n"] - 5 + 1 == 6 * M.W + 3
    # the reuse sequence: far below, at, and one above the count of the call before + 16; above the first copy of a fresh context
    assert M.REUSE_S[:5] == (5000, 100, 116, 117, 4097) and M.REUSE_S[0] > M.FIRST_COPY
    guess = [M.FIRST_COPY] + [s + M.GUESS_SLACK for s in M.REUSE_S[:-1]]
    rel = [s - g for s, g in zip(M.REUSE_S, guess)]
    assert 0 in rel and 1 in rel and min(rel) < -4000 and max(rel) > 3000
    for i, S in enumerate(M.REUSE_S):
        ch = M.reuse_chain(i)
        assert len(ch) == S and ch[0] == M.REUSE_N - M.REUSE_L and ch[-1] >= 0
        M.lb_of_chain(M.REUSE_N, M.REUSE_L, ch)


def test_part_layouts_cover_the_listed_placements():
    seen = set()
    counts = set()
    for name, c in M.TB_CASES.items():
        dp_size = c["n"] - c["L"] + 1
        for layout, part_lo in M.part_layouts(name).items():
            assert part_lo[0] == 0 and all(a < b for a, b in zip(part_lo, part_lo[1:])) and part_lo[-1] < dp_size and len(part_lo) <= 64
            counts.add(len(part_lo))
            ents, wins = M.part_profile(c["chain"], part_lo, dp_size)
            assert ents.sum() == len(c["chain"]) and (wins <= ents).all()
            seen |= M.part_features(c["chain"], part_lo, dp_size)
    assert counts == {1, 2, 3, 8}
    assert seen == {"window_border", "mid_window", "shared_window", "jumps_over_a_part", "leaves_to_vlo_minus_1", "stays_at_vlo", "ends_in_a_middle_part"}
    f = M.foreign_pointers(1000, 3, 1).astype(np.int64)
    t = np.arange(len(f))
    assert ((f == 0) | ((f >= 3) & (f <= t))).all() and (f > 0).sum() > 900


# ---- the merge cases
@pytest.mark.parametrize("name", list(M.MG_CASES))
def test_merge_case_reaches_what_it_is_listed_for(pkg, name):
    G, lb, mx, sz = M.mg_case(name)
    assert G.m == M.MG_M and G.L == M.MG_L and pkg.dp_lists_check(G.m, G.L, G.ent, G.hdr) is None
    tb, tau, seg, overflow, at = M.mg_expected(name)
    S = len(tb)
    assert [int(x) for x in tb["rb"]] == G.rbs and int(tb[-1]["segment_max_size"]) == G.max_seg
    steps, lbs = M.walk_steps(name)
    want = M.MG_CASES[name]["listed_for"]
    if G.max_seg < G.m:
        # the walk over the thresholds is the walk over the counts
        assert overflow == ("?" in steps) and (at is None or steps.index("?") == at - 1)
        if not overflow:
            assert steps.count("C") + 1 == len(seg) and seg[0]["lb"] == 0 and seg[-1]["rb"] == G.n
            assert all(a["rb"] == b["lb"] for a, b in zip(seg, seg[1:]))
    cols = [rb - 1 for rb in G.rbs]
    if "strips" in want:
        got = {(int(G.hdr[k, 0]), M.excess_entry(G.ent, G.hdr, k, G.max_seg)) for k in cols[1:]}
        lengths = (1, 2, 63, 64, 65, 127, 128, 129, 200)
        for nent in lengths:
            for p in (0, 1, 63, 64, 65, 128, nent - 1):
                if p < nent:
                    assert (nent, p) in got, (nent, p)
            assert nent == 1 or (nent, None) in got
        # the strip of 64 entries the threshold falls in, and the carry in front of it: exactly max_seg at entries 63 and 64
        assert {p // 64 for _, p in got if p is not None} == {0, 1, 2, 3}
        for k in cols[1:]:
            p = M.excess_entry(G.ent, G.hdr, k, G.max_seg)
            if p:
                assert int(G.ent[k, :p, 1].sum()) == G.max_seg
        assert {63, 64} <= {p - 1 for _, p in got if p}
        kinds = {int(x) for x in tau[1:, 1]}
        assert kinds == {M.TAU_EXACT, M.TAU_OPEN, M.TAU_NEVER} and not overflow
        assert any(G.hdr[k, 2] for k in cols[1:-1]) and any(not G.hdr[k, 2] for k in cols[1:-1])
    if "segments" in want:
        assert len(seg) == want["segments"]
    if "joins" in want:
        assert steps.count("J") == want["joins"]
    if "cuts" in want:
        assert steps.count("C") == want["cuts"] == S - 1
    if "alternating" in want:
        assert steps == "CJ" * ((S - 1) // 2)
    if "tau_eq_lb" in want:
        eq = [j for j in range(1, S) if tau[j, 1] == M.TAU_EXACT and tau[j, 0] == lbs[j - 1] and lbs[j - 1] > 0]
        assert len(eq) >= want["tau_eq_lb"] and all(steps[j - 1] == "J" for j in eq)
        plus = [j for j in range(1, S) if tau[j, 1] == M.TAU_EXACT and tau[j, 0] == lbs[j - 1] + 1]
        assert len(plus) >= want["tau_eq_lb_plus_1"] and all(steps[j - 1] == "C" for j in plus)
        # a segment between two cuts keeps the DP's size; a list value equal to current_lb is not counted; a count of exactly max_seg joins
        on = set(int(x) for x in sz[[rb - G.L for rb in G.rbs]])
        assert sum(1 for s in seg[1:-1] if int(s["segment_size"]) in on) >= want["keeps_dp_size"]
        assert sum(1 for j in eq if lbs[j - 1] in G.ent[cols[j], :G.hdr[cols[j], 0], 0]) >= want["value_eq_lb"]
        assert sum(1 for s in seg if s["segment_size"] == G.max_seg) >= want["count_eq_max_seg"]
    if "count_stops" in want:
        # the joins' lists hold current_lb exactly, at the listed entries; their counts are the merged sizes
        stops = []
        for j in range(1, S):
            if steps[j - 1] == "J":
                k = cols[j]
                at_entry = np.nonzero(G.ent[k, :G.hdr[k, 0], 0] == lbs[j - 1])[0]
                assert len(at_entry) == 1
                stops.append((int(at_entry[0]), int(G.hdr[k, 0])))
                s = seg[[int(x) for x in seg["rb"]].index(G.rbs[j])]
                assert int(s["segment_size"]) == int(G.ent[k, :at_entry[0], 1].sum())
        assert tuple(stops) == want["count_stops"]
        assert {a // 64 for a, _ in stops} == {0, 1, 2} and any(a + 1 == ne for a, ne in stops)
    if "open_decided" in want:
        dec = [j for j in range(1, S) if tau[j, 1] == M.TAU_OPEN and steps[j - 1] == "J"]
        assert len(dec) >= want["open_decided"] and not overflow
    if "overflow" in want:
        assert int(overflow) == want["overflow"]
    if "undecided_at" in want:
        assert at == {"first": 1, "middle": at, "last": S - 1}[want["undecided_at"]] and 1 <= at <= S - 1
        assert want["undecided_at"] != "middle" or 1 < at < S - 1
        assert tau[at, 1] == M.TAU_OPEN and len(seg) == 0
    if "no_merge" in want:
        assert G.max_seg >= G.m and len(seg) == 0 and (tau == 0).all()
    if "S" in want:
        assert S == want["S"] > M.FIRST_COPY and 10 < len(seg) < S and not overflow
        assert {"J", "C"} == set(steps) and any(tau[j, 0] == lbs[j - 1] and lbs[j - 1] > 0 for j in range(1, S))
    lay = M.split_layouts(name)
    mid = cols[len(cols) // 2]
    assert lay["at_boundary"] == [mid] and lay["one_above_boundary"] == [mid + 1] and len(lay["eight"]) == 7
    a, b = (lay["empty_range"] + [G.n])[:2]
    assert not any(a <= k < b for k in cols)
    for s in lay.values():
        assert all(0 < x < G.n for x in s) and all(x < y for x, y in zip(s, s[1:]))


def test_merge_table_covers_the_listed_walks():
    keys = set()
    for c in M.MG_CASES.values():
        keys |= set(c["listed_for"])
    assert keys >= {"strips", "segments", "cuts", "alternating", "tau_eq_lb", "tau_eq_lb_plus_1", "keeps_dp_size", "value_eq_lb", "count_stops", "open_decided",
                    "overflow", "undecided_at", "no_merge", "S"}
    assert {M.MG_CASES[n]["listed_for"].get("undecided_at") for n in M.MG_CASES} >= {"first", "middle", "last"}


# ---- the chain check, and the entries' refusals
def test_chain_check_under_the_sanitizers(tmp_path):
    """The header is host-only: tests/tb_chain_sanitized.cpp includes it alone and runs good chains over garbage and every broken
    entry on arrays of exactly n - L + 1 words, as a program of its own under AddressSanitizer and UndefinedBehaviorSanitizer
    (nothing loaded into Python runs under either)."""
    here = os.path.dirname(os.path.abspath(__file__))
    exe = str(tmp_path / "tb_chain_sanitized")
    subprocess.run(["g++", "-std=c++17", "-g", "-O1", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", os.path.join(os.path.dirname(here), "founder-sequences_amd", "csrc"), os.path.join(here, "tb_chain_sanitized.cpp"), "-o", exe], check=True)
    p = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120)
    assert p.returncode == 0 and p.stdout.strip() == "ok", p.stderr[-3000:]


def test_traceback_parts_refuses_without_a_device(pkg):
    name = "borders"
    c = M.TB_CASES[name]
    n, L, chain = c["n"], c["L"], c["chain"]
    lb, mx, sz = M.tb_arrays(name, True)
    dp_size = n - L + 1

    def refused(call, entry=None):
        with pytest.raises(pkg.FseqError) as e:
            call()
        assert e.value.code == E_ARG, e.value
        if entry is not None:
            assert "chain entry %d" % entry in str(e.value), e.value

    # (device 1 << 20: were a refusal to come after the device is chosen, the code would not be FSEQ_E_ARG)
    parts = lambda lb_, part_lo, **kw: pkg.traceback_parts(n, L, lb_, mx, sz, part_lo, device=1 << 20, **kw)
    refused(lambda: parts(lb, []))
    refused(lambda: parts(lb, list(range(65))))                                      # more than 64 parts
    refused(lambda: parts(lb, [1, 5]))                                               # the first part begins at 0
    refused(lambda: parts(lb, [0, 5, 5]))
    refused(lambda: parts(lb, [0, 9, 5]))
    refused(lambda: parts(lb, [0, dp_size]))                                         # a part behind the array
    refused(lambda: pkg.traceback_parts(n, L, lb[:-1], mx, sz, [0], device=1 << 20))
    refused(lambda: pkg.traceback_parts(n, L, lb, mx, sz, [0], foreign=lb[:-1], device=1 << 20))
    refused(lambda: pkg.traceback_parts(2 * L - 1, L, lb[:L], mx[:L], sz[:L], [0], device=1 << 20))   # n < 2L
    for t in (chain[0], chain[3], chain[-1]):
        for v in (t + 1, L - 1, M.NONE, t + L):
            bad = lb.copy()
            bad[t] = v
            refused(lambda: parts(bad, [0]), entry=t)
    L_ = pkg.load_library()
    assert L_.fseq_debug_traceback_parts(0, n, L, None, mx.ctypes.data, sz.ctypes.data, None, 1, None, None, None, None, None, None) == E_ARG


def test_merge_on_lists_refuses_no_context(pkg):
    G, lb, mx, sz = M.mg_case("tau_edges")
    L_ = pkg.load_library()
    assert L_.fseq_debug_merge_on_lists(None, G.X, G.ent.ctypes.data, G.hdr.ctypes.data, lb.ctypes.data, mx.ctypes.data, sz.ctypes.data, 0, None, 0,
                                        None, None, None, None, None, None, None) == E_ARG
    # (a context is made on a device: its refusals are with the GPU tests)
