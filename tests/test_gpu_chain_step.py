"""The streamed chain step's kernels (csrc/fseq_chainsort.hpp) on constructed states, kernel by kernel, against the numpy model
of tests/chain_step_cases.py: every output word, integers, no tolerance.  Pass 2's k_chain_snap_grouped through
fseq_debug_pass2_step -- by runs, by one-word pairs (pass2_step<true>) and by two-word pairs (pass2_step<false>, which no whole
run of the suite reaches), the path asserted from the kernel's counters -- and phase B's k_cm_* through
fseq_debug_chain_launch, the launcher phase B itself uses -- one, two and three radix passes (the third: more than 2^18 keys),
one- and two-word pairs, expansion and composition.  tests/test_chain_step_cases.py checks on the CPU that every case asks what
it is listed for."""
import importlib

import numpy as np
import pytest

import chain_step_cases as cs

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def pkg():
    return importlib.import_module("founder-sequences_amd")


def same(got, want):
    return got.shape == np.shape(want) and np.array_equal(got, want)


@pytest.mark.parametrize("case", cs.PASS2_CASES, ids=[c["id"] for c in cs.PASS2_CASES])
def test_pass2_step_equals_the_model(pkg, case):
    B = cs.build_pass2(case)
    args = ([B["a0"]], [B["d0"]], [B["rank"]], [0], [B["cls"]], [B["headd"]], [B["D"]])
    want_a, want_d, want_stats = cs.pass2_model(*args, B["run_cap"])
    snap_a, snap_d, stats = pkg.pass2_step(*args, run_cap=B["run_cap"])
    assert same(snap_a, want_a)
    assert same(snap_d, want_d)
    assert same(stats, want_stats), (list(stats), list(want_stats))
    # the path the table names, from the kernel's own counters
    assert (int(stats[0]), int(stats[1]), int(stats[2])) == ((1, 0, 0) if case["path"] == "runs" else (0, 1, 0))
    if case["runs"] is not None and cs.pass2_counts_runs(case["m"], case["run_cap"]):
        assert stats[3] == case["runs"]
    if not cs.pass2_counts_runs(case["m"], case["run_cap"]):
        assert stats[3] == 0 and not stats[4:].any()                      # (2^18 rows and more, or the knob at 0: no run is counted)


@pytest.mark.parametrize("workgroups", [1, 3])
def test_pass2_groups_of_one_launch(pkg, workgroups):
    """Three blocks, seven tasks; one workgroup takes every group in turn (and rebuilds the ranks and the records for each), three
    take one each.  A block's tasks by runs, by sort, a border copy and a task that is not this kernel's, in one group."""
    Gc = cs.build_grouped()
    args = (Gc["a0"], Gc["d0"], Gc["rank"], Gc["task_blk"], Gc["cls"], Gc["headd"], Gc["ncls"])
    want_a, want_d, want_stats = cs.pass2_model(*args, cs.P2_RUN_CAP)
    snap_a, snap_d, stats = pkg.pass2_step(*args, workgroups=workgroups)
    assert same(snap_a, want_a) and same(snap_d, want_d)
    skipped = Gc["paths"].index("skip")
    assert np.all(snap_a[skipped] == cs.NOT_WRITTEN) and np.all(snap_d[skipped] == cs.NOT_WRITTEN)
    copied = Gc["paths"].index("copy")
    assert np.array_equal(snap_a[copied], Gc["a0"][1]) and np.array_equal(snap_d[copied], Gc["d0"][1])
    assert same(stats, want_stats), (list(stats), list(want_stats))
    assert (int(stats[0]), int(stats[1]), int(stats[2])) == (3, 2, 1) and stats[4:].sum() == 5


@pytest.mark.parametrize("case", cs.CHAIN_CASES, ids=[c["id"] for c in cs.CHAIN_CASES])
def test_chain_launch_equals_the_model(pkg, case):
    B = cs.build_chain(case)
    m, nb, G, first, chains = B["m"], len(B["nkeys"]), case["G"], case["first"], case["chains"]
    start_a = start_d = seq_a = None
    if case["own_start"]:
        # every chain of the launch starts from the sequential model's state in front of its first block
        seq_a, seq_d = cs.sequential_states(B["a"], B["d"], B["rank"], B["keyd"])
        start_a = [seq_a[(first + c) * G] for c in range(chains)]
        start_d = [seq_d[(first + c) * G] for c in range(chains)]
    want = cs.chain(B["rank"], B["keyd"], B["nkeys"], G, cs.COLS, first, chains, start_a, start_d, states=case["states"], keys=case["keys"])
    got = pkg.chain_launch(B["rank"], B["keyd"], B["nkeys"], G, cs.COLS, first_chain=first, chains=chains, start_a=start_a, start_d=start_d,
                           states=case["states"], keys=case["keys"])
    assert sorted(got) == sorted(want)
    for name in sorted(want):
        assert same(got[name], want[name]), name
    if case["states"] and seq_a is not None:
        # expansion: the states of the launch's chains are the sequential model's; a chain whose last block is not the last of all
        # leaves no trace of a step through it -- the state behind it is the next chain's to write, or nobody's in this launch
        lo, hi = first * G, min(nb, (first + chains) * G)
        written = list(range(lo, hi)) + ([nb] if hi == nb else [])
        for b in range(nb + 1):
            if b in written:
                assert np.array_equal(got["state_a"][b], seq_a[b]) and np.array_equal(got["state_d"][b], seq_d[b]), b
            else:
                assert np.all(got["state_a"][b] == cs.NOT_WRITTEN) and np.all(got["state_d"][b] == cs.NOT_WRITTEN), b
    if case["keys"]:
        for c in range(chains):
            n = int(got["nkeys"][c])
            assert 1 <= n <= m and got["rank"][c].max() == n - 1 and np.all(got["keyd"][c][n:] == cs.NOT_WRITTEN)
