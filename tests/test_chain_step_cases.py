"""The model and the case tables of tests/chain_step_cases.py, on the CPU: the vectorised chain step equals the per-position
models of tests/proto_pass2_runs.py; every case of the tables meets the conditions it is listed for -- its run count, its class
count and bit widths, the path the kernel's own expressions give it, and a non-empty set of ranges for every range-maximum
branch it names -- so that no GPU test passes because its input never asked the question; and the two debug entries refuse,
before they touch a device, everything a kernel would form an index from."""
import ctypes as C
import importlib

import numpy as np
import pytest

import chain_step_cases as cs
import proto_pass2_runs as pp


# ---------------------------------------------------------------------------------------------- the model
@pytest.mark.parametrize("m,D", [(1, 1), (2, 1), (2, 2), (65, 1), (65, 65), (700, 3), (700, 64), (3000, 2), (3000, 513), (3000, 3000)])
def test_vectorised_step_equals_the_per_position_models(m, D):
    rng = np.random.default_rng(m * 7 + D)
    for trial in range(4):
        a0 = cs.make_perm(cs.PERMS[trial % 3], m, rng)
        d0 = cs.make_d0(cs.D0_FAMILIES[(trial + D) % 5], m, rng)
        key = rng.permutation(m) if D == m else rng.integers(0, D, size=m)
        headd = rng.integers(0, cs.D_LIMIT, size=D)
        a1, d1 = cs.chain_step(a0, d0, key, headd)
        wa, wd = pp.chain_step_sorted(a0, d0, key, headd)
        assert np.array_equal(a1, wa) and np.array_equal(d1, wd)
        assert np.array_equal(cs.run_starts(a0, key), pp.run_starts(a0, key))
        for cap in (0, 1, m):
            ra, rd, R, _ = pp.chain_step_runs(a0, d0, key, headd, cap)
            assert np.array_equal(a1, ra) and np.array_equal(d1, rd) and R == len(cs.run_starts(a0, key))


def test_stretches_step_equals_the_run_model():
    rng = np.random.default_rng(3)
    m = 2500
    a0 = cs.make_perm("random", m, rng)
    key = cs.key_by_row(a0, cs.keys_stretches(m, 40, rng))
    d0 = cs.make_d0("spikes", m, rng)
    headd = rng.integers(0, cs.D_LIMIT, size=40)
    a1, d1 = cs.chain_step(a0, d0, key, headd)
    ra, rd, R, by_runs = pp.chain_step_runs(a0, d0, key, headd, m)
    assert by_runs and R < m // 10 and np.array_equal(a1, ra) and np.array_equal(d1, rd)


def test_range_categories_count_every_non_first_position_once():
    rng = np.random.default_rng(4)
    m = 5000
    a0 = cs.make_perm("random", m, rng)
    key = rng.integers(0, 300, size=m)
    cats = cs.range_categories(a0, cs.make_d0("random", m, rng), key)
    gaps = sum(v for k, v in cats.items() if isinstance(k, tuple) and k[1] > 0) + cats.get(("gap", 0, "lo"), 0)
    assert cats["prefix"] + cats["suffix"] + cats["scan"] + cats["adjacent"] + gaps == m - len(np.unique(key))
    # the three in-block branches by hand on one block: d0 = 5 1 9 1 1 7 ..., ranges [1, 2] (prefix grows), [3, 5] (suffix), [3, 4] (scan)
    d0 = np.zeros(64, dtype=np.int64)
    d0[:6] = (5, 1, 9, 1, 1, 7)
    one = lambda lo, hi: cs.range_categories(np.arange(64), d0, np.where(np.isin(np.arange(64), (lo - 1, hi)), 0, np.arange(64) + 1))
    assert (one(1, 2)["prefix"], one(3, 5)["suffix"], one(3, 4)["scan"]) == (1, 1, 1)
    assert one(4, 63)["suffix"] == 1                                      # (hi ends the block)


@pytest.mark.parametrize("G", [1, 2, 3, 5])
def test_chain_model_expansions_equal_the_sequential_steps(G):
    """Chains started from the sequential model's states reproduce it, whatever G; a launch of some chains leaves the state
    behind its last chain unwritten; composite keys of a chain = the ranks of its rows by (the blocks' keys in turn)."""
    rng = np.random.default_rng(G)
    m, nb = 400, 5
    rank = rng.integers(0, 6, size=(nb, m))
    keyd = np.array([rng.integers(0, (b + 1) * cs.COLS + 1, size=m) for b in range(nb)])
    a, d = cs.make_perm("random", m, rng), cs.make_d0("random", m, rng)
    sa, sd = cs.sequential_states(a, d, rank, keyd)
    nch = (nb + G - 1) // G
    out = cs.chain(rank, keyd, None, G, cs.COLS, 0, nch, sa[::G][:nch], sd[::G][:nch])
    assert np.array_equal(out["state_a"], sa) and np.array_equal(out["state_d"], sd)
    if nch > 1:
        out = cs.chain(rank, keyd, None, G, cs.COLS, 0, nch - 1, sa[::G][:nch - 1], sd[::G][:nch - 1])
        b_cut = (nch - 1) * G
        assert np.array_equal(out["state_a"][:b_cut], sa[:b_cut]) and np.all(out["state_a"][b_cut:] == cs.NOT_WRITTEN)
    # composite keys: from the identity, d = the chain's first column; a position starts a key iff it is position 0 or d exceeds that column
    comp = cs.chain(rank, keyd, None, G, cs.COLS, 1 if nch > 1 else 0, 1, states=False, keys=True)
    b0 = G if nch > 1 else 0
    a, d = np.arange(m), np.full(m, b0 * cs.COLS)
    for b in range(b0, min(nb, b0 + G)):
        a, d = pp.chain_step_sorted(a, d, rank[b], keyd[b])
    starts = [p for p in range(m) if p == 0 or d[p] > b0 * cs.COLS]
    assert comp["nkeys"][0] == len(starts) and list(comp["keyd"][0][:len(starts)]) == [d[p] for p in starts]
    assert np.all(comp["keyd"][0][len(starts):] == cs.NOT_WRITTEN)
    assert list(comp["rank"][0][a]) == [sum(1 for q in starts if q <= p) - 1 for p in range(m)]


# ---------------------------------------------------------------------------------------------- the tables
def test_tables_have_the_rows_the_kernels_need():
    ids = [c["id"] for c in cs.PASS2_CASES]
    assert len(set(ids)) == len(ids) and len({c["id"] for c in cs.CHAIN_CASES}) == len(cs.CHAIN_CASES)
    ms = {c["m"] for c in cs.PASS2_CASES}
    assert ms == {11265, 11328, 12288, 12289, 65536, 65537, 262144, 262145}
    for m in ms:
        assert {c["path"] for c in cs.PASS2_CASES if c["m"] == m} >= ({"p4", "wide"} if m == 262145 else {"runs", "p4"})
    assert {c["d0"] for c in cs.PASS2_CASES if c["path"] == "wide"} == set(cs.D0_FAMILIES)
    assert {c["m"] for c in cs.CHAIN_CASES} == {11265, 12288, 12289, 65537, 300000}
    assert all(cs.M_MIN <= c["m"] <= cs.M_MAX for c in cs.PASS2_CASES + cs.CHAIN_CASES)


@pytest.mark.parametrize("case", cs.PASS2_CASES, ids=[c["id"] for c in cs.PASS2_CASES])
def test_pass2_case_meets_its_conditions(case):
    B = cs.build_pass2(case)
    m, D = B["m"], B["D"]
    assert sorted(B["a0"]) == list(range(m)) and B["d0"].max() < cs.D_LIMIT and B["d0"].min() >= 0
    assert B["rank"].max() < B["cap"] <= cs.P2_CLS_CAP and B["cls"].max() < D <= B["cap"]
    key = B["cls"][B["rank"]]
    # (stretches: as many classes as stretches at the most, of the D the task's table names)
    assert np.array_equal(key, B["key"]) and (len(np.unique(key)) == D or ("stretches" in case["keys"][0] and 2 <= len(np.unique(key)) < D))
    R = len(cs.run_starts(B["a0"], key))
    if case["runs"] is not None:
        assert R == case["runs"]
    assert cs.pass2_path(m, D, R, case["run_cap"]) == case["path"], (R, D)
    if case["passes"] is not None:
        assert cs.digit_passes(D) == case["passes"]
    if case["path"] == "wide":
        assert cs.bits_of(D - 1) + cs.bits_of(m - 1) > 32 and not cs.pass2_counts_runs(m, case["run_cap"])
    # (a task by runs takes a range maximum for the heads of its runs only: its categories are theirs)
    cats = cs.range_categories(B["a0"], B["d0"], key, heads_only=case["path"] == "runs")
    for name in case["cats"]:
        assert cats.get(name, 0) > 0, (name, cats)
    if case["keys"][0].startswith("planted"):
        assert max(case["keys"][2]) == cs.top_level(m)
        for k in range(cs.top_level(m) + 1):
            assert cats[("gap", k, "lo")] > 0 and cats[("gap", k, "hi")] > 0, k


def test_pass2_edges_of_the_table():
    by = {c["id"]: c for c in cs.PASS2_CASES}
    # the run path's LDS arrays exactly full, and one run more
    assert by["11265-R8832-random-random"]["runs"] == cs.P2_RUN_CAP and by["11265-R8832-random-random"]["path"] == "runs"
    assert by["11265-R8833-random-random"]["runs"] == cs.P2_RUN_CAP + 1 and by["11265-R8833-random-random"]["path"] == "p4"
    # a wave's chunk of the sort is 768 positions at the fewest streamed rows: the last wave's is empty
    per = ((11265 + 15) // 16 + 63) & ~63
    assert per == 768 and 15 * per > 11265
    # one-word pairs end between 8,192 and 8,193 classes at 19 position bits, and hold 11,264 classes at 18
    assert cs.pass2_path(262145, 8192, 262145, cs.P2_RUN_CAP) == "p4" and cs.pass2_path(262145, 8193, 262145, cs.P2_RUN_CAP) == "wide"
    assert cs.pass2_path(262144, 11264, 262144, cs.P2_RUN_CAP) == "p4" and cs.pass2_counts_runs(262144, 1) and not cs.pass2_counts_runs(262145, 1)
    assert (cs.top_level(11265), cs.top_level(65536), cs.top_level(65537), cs.top_level(262144), cs.top_level(262145)) == (7, 9, 9, 11, 11)
    assert cs.top_level(300000) == 12


def test_grouped_case_meets_its_conditions():
    Gc = cs.build_grouped()
    m, cap = Gc["m"], Gc["cap"]
    assert list(Gc["task_blk"]) == [0, 1, 1, 1, 1, 1, 2] and Gc["rank"].max() < cap
    for t, want in enumerate(Gc["paths"]):
        D = int(Gc["ncls"][t])
        if want in ("copy", "skip"):
            assert D == (0 if want == "copy" else cs.NOT_WRITTEN)
            continue
        assert Gc["cls"][t].max() < D <= cap
        b = Gc["task_blk"][t]
        key = Gc["cls"][t][Gc["rank"][b]]
        R = len(cs.run_starts(Gc["a0"][b], key))
        assert cs.pass2_path(m, D, R, cs.P2_RUN_CAP) == want, (t, R)
    _, _, stats = cs.pass2_model(Gc["a0"], Gc["d0"], Gc["rank"], Gc["task_blk"], Gc["cls"], Gc["headd"], Gc["ncls"], cs.P2_RUN_CAP)
    assert list(stats[:4]) == [3, 2, 1, m] and stats[4:].sum() == 5


def _working(case):
    """(chains of the launch that step through a block at all, the blocks stepped per chain)."""
    per_chain = cs.stepped_blocks(len(case["nkeys"]), case["G"], case["first"], case["chains"], case["keys"])
    return sum(1 for blocks in per_chain if blocks), per_chain


@pytest.mark.parametrize("case", cs.CHAIN_CASES, ids=[c["id"] for c in cs.CHAIN_CASES])
def test_chain_case_meets_its_conditions(case):
    """Everything a case is listed for is held over the blocks its launch STEPS through -- a block whose chain only copies its start
    state asks the sort and the range maximum nothing."""
    B = cs.build_chain(case)
    m, nb, G = B["m"], len(B["nkeys"]), case["G"]
    for b in range(nb):
        assert len(np.unique(B["rank"][b])) == B["nkeys"][b] == B["rank"][b].max() + 1
    assert case["first"] + case["chains"] <= (nb + G - 1) // G and sorted(B["a"]) == list(range(m))
    if "expand" in case["name"] and G > 1:
        assert nb % G != 0
    working, per_chain = _working(case)
    stepped = [b for blocks in per_chain for b in blocks]
    assert stepped == list(case["steps"]) and stepped
    # every chain of the launch works in the part and row kernels, but in the expansion of chains of one block
    assert working == (1 if case["name"] == "expand-G1" else case["chains"])
    passes = [cs.digit_passes(int(B["nkeys"][b])) for b in stepped]
    widths = [cs.cm_pair_is_one_word(m, int(B["nkeys"][b])) for b in stepped]
    if case["nkeys"][:5] == (1, 2, 512, 513, m) and case["name"] != "expand-G1":
        # blocks of one and of two passes in the SAME step of the launch, and both sides of 512 | 513 keys among the stepped
        first_step = {cs.digit_passes(int(B["nkeys"][blocks[0]])) for blocks in per_chain}
        assert first_step == {1, 2} and set(passes) == {1, 2}
        assert {int(B["nkeys"][b]) for b in stepped} & {512, 513} and [cs.digit_passes(n) for n in (1, 2, 512, 513)] == [1, 1, 1, 2]
    if "+" in case["name"]:
        # the chain counts: that many chains at work, and workgroups of the rounded grid without a chain where 8 does not divide them
        assert working == case["chains"] and (set(passes) == {1, 2} or case["chains"] == 1)
        idle_rows = (case["chains"] + 7) // 8 * 8 - case["chains"]
        assert idle_rows == {9: 7, 8: 0, 7: 1, 3: 5, 1: 7}[case["chains"]]
    if case["name"] == "one-launch":
        assert widths == [True, False] and [int(B["nkeys"][b]) for b in stepped] == [32768, 32769]
    if case["name"].startswith("apart"):
        assert widths == [case["nkeys"][0] == 32768]
    if case["name"] == "planted":
        levels = case["nkeys"][0][2]
        assert stepped[0] == 0 and case["own_start"]                      # (block 0 is stepped, from the start state the pairs were planted in)
        cats = cs.range_categories(B["a"], B["d"], B["rank"][0])
        assert max(levels) == cs.top_level(m)
        for k in levels:
            assert cats[("gap", k, "lo")] > 0 and cats[("gap", k, "hi")] > 0, k
        assert cats["adjacent"] > 0 and cats["prefix"] + cats["suffix"] + cats["scan"] > 0
    elif m == 300000:
        assert not any(widths) and passes == ([2, 3, 3] if len(stepped) == 3 else [2, 3])
        assert [int(B["nkeys"][b]) for b in stepped] == ([262144, 262145, m] if len(stepped) == 3 else [262144, m])
        # the ranges of the first stepped block, from the state its chain starts in: inside a block, neighbours, the table
        a0, d0 = (B["a"], B["d"]) if case["own_start"] else (np.arange(m), np.zeros(m, dtype=np.int64))
        cats = cs.range_categories(a0, d0, B["rank"][0])
        assert cats["prefix"] + cats["suffix"] + cats["scan"] > 0 and cats["adjacent"] > 0 and cats[("gap", 0, "lo")] > 0


def test_chain_table_covers_the_chain_counts_and_both_outputs():
    for keys in (False, True):
        assert {_working(c)[0] for c in cs.CHAIN_CASES if c["keys"] == keys and "+" in c["name"]} >= {1, 7, 8, 9}
    assert {(c["states"], c["keys"]) for c in cs.CHAIN_CASES} == {(True, False), (False, True), (True, True)}
    for m in (11265, 12288, 12289):
        assert {(c["start"], c["perm"]) for c in cs.CHAIN_CASES if c["m"] == m and c["name"] == "start"} == {(f, p) for f in cs.D0_FAMILIES for p in ("identity", "reversal")}
    assert {c["G"] for c in cs.CHAIN_CASES} == {1, 2, 3}
    # three radix passes: the fewest keys that need them, stepped, in a composition and in a chain of three
    three = [c for c in cs.CHAIN_CASES if 1 in c["steps"] and len(c["nkeys"]) > 1 and c["nkeys"][1] == 262145]
    assert {c["G"] for c in three} == {1, 3}


# ---------------------------------------------------------------------------------------------- the entries' refusals
@pytest.fixture(scope="module")
def pkg():
    build = importlib.import_module("founder-sequences_amd.build")
    build.build()
    return importlib.import_module("founder-sequences_amd")


def _u32(x):
    return np.ascontiguousarray(x, dtype=np.uint32)


def _pass2_args(m=11265, cap=64, nblocks=2, ntasks=3):
    rng = np.random.default_rng(0)
    return dict(m=m, nblocks=nblocks, a0=_u32([rng.permutation(m) for _ in range(nblocks)]), d0=_u32(np.zeros((nblocks, m))),
                rank=_u32(rng.integers(0, cap, size=(nblocks, m))), cap=cap, ntasks=ntasks, task_blk=_u32([0, 0, 1][:ntasks]),
                cls=_u32(np.tile(np.arange(cap) % 8, (ntasks, 1))), headd=_u32(np.zeros((ntasks, cap))), ncls=_u32([8, 0, 0xFFFFFFFF][:ntasks]),
                run_cap=8832, workgroups=1)


def _call_pass2(pkg, A):
    L = pkg.load_library()
    m, nt = A["m"], A["ntasks"]
    sa, sd, st = _u32(np.zeros((nt, max(m, 1)))), _u32(np.zeros((nt, max(m, 1)))), _u32(np.zeros(pkg.P2_STATS))
    p = lambda x: x.ctypes.data
    return L.fseq_debug_pass2_step(0, m, A["nblocks"], p(A["a0"]), p(A["d0"]), p(A["rank"]), A["cap"], nt, p(A["task_blk"]), p(A["cls"]), p(A["headd"]),
                                   p(A["ncls"]), A["run_cap"], A["workgroups"], p(sa), p(sd), p(st))


def _edit(A, name, index, value):
    A[name] = A[name].copy()
    A[name][index] = value


PASS2_REFUSALS = {
    "m below the streamed rows": lambda A: A.update(m=11264),
    "m above the build's rows": lambda A: A.update(m=589825),
    "a0 not a permutation (a row twice)": lambda A: _edit(A, "a0", (1, 5), A["a0"][1, 6]),
    "a0 out of range": lambda A: _edit(A, "a0", (0, 0), 11265),
    "rank at cap": lambda A: _edit(A, "rank", (1, 11264), 64),
    "cap above the class table": lambda A: A.update(cap=11265),
    "cap zero": lambda A: A.update(cap=0),
    "ncls above cap": lambda A: _edit(A, "ncls", 0, 65),
    "a class at ncls, in an entry no rank names": lambda A: (_edit(A, "rank", (slice(None), slice(None)), np.minimum(A["rank"], 62)), _edit(A, "cls", (0, 63), 8)),
    "run_cap above the LDS arrays": lambda A: A.update(run_cap=8833),
    "task of no block": lambda A: _edit(A, "task_blk", 2, 2),
    "a block's tasks apart": lambda A: _edit(A, "task_blk", slice(None), [0, 1, 0]),
    "no workgroup": lambda A: A.update(workgroups=0),
    "no task": lambda A: A.update(ntasks=0),
}


def test_pass2_entry_accepts_the_base_arguments(pkg):
    assert _call_pass2(pkg, _pass2_args()) != pkg.FSEQ_E_ARG              # (no device here: FSEQ_E_HIP from the runtime, behind the checks)


@pytest.mark.parametrize("rule", PASS2_REFUSALS, ids=lambda r: r.replace(" ", "-"))
def test_pass2_entry_refuses(pkg, rule):
    A = _pass2_args()
    PASS2_REFUSALS[rule](A)
    assert _call_pass2(pkg, A) == pkg.FSEQ_E_ARG


def _chain_args(m=11265, nb=5):
    rng = np.random.default_rng(1)
    return dict(m=m, nb=nb, G=2, rank=_u32(rng.integers(0, 9, size=(nb, m))), keyd=_u32(np.zeros((nb, m))), nkeys=_u32([9] * nb), first=1, chains=2,
                start_a=_u32([rng.permutation(m) for _ in range(2)]), start_d=_u32(np.zeros((2, m))), states=True, keys=True)


def _call_chain(pkg, A):
    L = pkg.load_library()
    m, nb, ch = max(A["m"], 1), A["nb"], max(A["chains"], 1)
    sa, sd = _u32(np.zeros((nb + 1, m))), _u32(np.zeros((nb + 1, m)))
    kr, kd, kn = _u32(np.zeros((ch, m))), _u32(np.zeros((ch, m))), _u32(np.zeros(ch))
    p = lambda x, on=True: x.ctypes.data if on and x is not None else None
    return L.fseq_debug_chain_launch(0, A["m"], nb, A["G"], 1000, p(A["rank"]), p(A["keyd"]), p(A["nkeys"]), A["first"], A["chains"], p(A["start_a"]),
                                     p(A["start_d"]), p(sa, A["states"]), p(sd, A["states"]), p(kr, A["keys"]), p(kd, A["keys"]), p(kn, A["keys"]))


CHAIN_REFUSALS = {
    "m below the streamed rows": lambda A: A.update(m=11264),
    "m above the build's rows": lambda A: A.update(m=589825),
    "nkeys zero": lambda A: _edit(A, "nkeys", 4, 0),
    "nkeys above m": lambda A: _edit(A, "nkeys", 0, 11266),
    "rank at nkeys": lambda A: _edit(A, "rank", (4, 11264), 9),
    "G zero": lambda A: A.update(G=0),
    "chains past the level's": lambda A: A.update(first=2, chains=2),
    "first chain past the level's": lambda A: A.update(first=3, chains=1),
    "no chain": lambda A: A.update(chains=0),
    "start state not a permutation": lambda A: _edit(A, "start_a", (1, 0), A["start_a"][1, 1]),
    "start state out of range": lambda A: _edit(A, "start_a", (0, 11264), 11265),
    "start_a without start_d": lambda A: A.update(start_d=None),
    "no output wanted": lambda A: A.update(states=False, keys=False),
    "no key block": lambda A: A.update(nb=0),
}


def test_chain_entry_accepts_the_base_arguments(pkg):
    assert _call_chain(pkg, _chain_args()) != pkg.FSEQ_E_ARG


@pytest.mark.parametrize("rule", CHAIN_REFUSALS, ids=lambda r: r.replace(" ", "-"))
def test_chain_entry_refuses(pkg, rule):
    A = _chain_args()
    CHAIN_REFUSALS[rule](A)
    assert _call_chain(pkg, A) == pkg.FSEQ_E_ARG


def test_python_wrappers_raise_the_refusal(pkg):
    A = _pass2_args()
    _edit(A, "rank", (0, 0), 64)
    with pytest.raises(pkg.FseqError) as e:
        pkg.pass2_step(A["a0"], A["d0"], A["rank"], A["task_blk"], A["cls"], A["headd"], A["ncls"])
    assert e.value.code == pkg.FSEQ_E_ARG
    B = _chain_args()
    with pytest.raises(pkg.FseqError) as e:
        pkg.chain_launch(B["rank"], B["keyd"], B["nkeys"], 0, 1000)
    assert e.value.code == pkg.FSEQ_E_ARG
    for half in (dict(start_a=B["start_a"]), dict(start_d=B["start_d"])):
        with pytest.raises(pkg.FseqError) as e:
            pkg.chain_launch(B["rank"], B["keyd"], B["nkeys"], 2, 1000, first_chain=1, chains=2, **half)
        assert e.value.code == pkg.FSEQ_E_ARG
