"""Pass 2 on streamed rows behind the reduced phase C, boundaries moved as runs of equal class (pass2_runs in
csrc/fseq_chainsort.hpp) beside the sort of all rows (pass2_step), and the records of a block's boundary state built once for
the block's boundaries.

A block's boundary state is a pBWT order, so the rows of one class at a boundary inside the block lie in a few runs of
consecutive positions; a boundary with at most FSEQ_P2_RUN_CAP runs is moved run by run, any other by the radix sort.  Every
boundary state is compared with the oracle (compare_long / check_long of test_gpu_parity); ctx.pass2_paths() tells which way
the boundaries went.  FSEQ_REDUCED_ALWAYS, a short segment length (blocks hold several boundaries) and at least 12,000 rows
(streamed) throughout."""
import importlib

import numpy as np
import pytest

import fso
from test_gpu_parity import check_long, compare_long, run_gpu

pytestmark = pytest.mark.gpu

FEW = dict(m=12037, n=2400, L=8, K=3, Brec=4000, mu=3e-4, seed=301, B=100)     # m: no multiple of 64 or 1,024; no recombination


@pytest.fixture(scope="module")
def pkg():
    return importlib.import_module("founder-sequences_amd")


@pytest.fixture()
def always(monkeypatch):
    monkeypatch.setenv("FSEQ_REDUCED_ALWAYS", "1")
    return monkeypatch


@pytest.fixture(scope="module")
def few():
    """Three founders and their mutants, no recombination: long runs, about two a class.  (alignment, oracle)"""
    c = FEW
    msa = fso.synth_msa(fso.synth_spec(c["seed"], c["K"], c["Brec"], c["mu"], 0), c["m"], c["n"])
    return msa, fso.segment_long(msa, c["L"], keep_dp=False, threads=4)


def inner_boundaries(ctx):
    rb = ctx.reduced_traceback()["rb"].astype(np.int64)
    return int(np.sum(rb % ctx.timings()["block_len"] != 0))


def run_checked(pkg, msa, ref, L, B):
    ctx = run_gpu(pkg, msa, L, block_len=B)
    check_long(ctx, ref, msa.shape[1], L, check_dp=False)
    return ctx


def test_few_founders_all_boundaries_by_runs(pkg, always, few):
    """Range maxima between runs of one 64-block, m not a multiple of 64; every inner boundary on the run path."""
    msa, ref = few
    ctx = run_checked(pkg, msa, ref, FEW["L"], FEW["B"])
    t = ctx.timings()
    p = ctx.pass2_paths()
    print(p)
    assert p["by_runs"] > 0 and p["by_sort"] == 0 and 0 < p["max_runs"] <= pkg.P2_RUN_CAP, p
    assert sum(p["runs_hist"]) == p["by_runs"] and max(b for b, c in enumerate(p["runs_hist"]) if c) == int(p["max_runs"] - 1).bit_length(), p
    if t["reduced_blocks"] == t["n_blocks"]:
        assert p["by_runs"] == inner_boundaries(ctx), p
        assert p["copies"] == len(ctx.reduced_traceback()) - p["by_runs"], p


def test_one_founder_one_run(pkg, always):
    """One founder and hardly a mutation: one or two classes at a boundary, one run at most of them."""
    m, n, L, B = 12000, 1600, 8, 100
    msa = fso.synth_msa(fso.synth_spec(302, 1, 200, 1e-6, 0), m, n)
    ctx, _ = compare_long(pkg, msa, L, check_dp=False, block_len=B)
    p = ctx.pass2_paths()
    print(p)
    assert p["by_runs"] > 0 and p["by_sort"] == 0, p
    assert p["max_runs"] <= 16, p


def test_founders_boundary_inside_blocks_takes_both_paths(pkg, always):
    """Recombination every 150 columns against blocks of 100: behind a founders' boundary inside a block nearly every position
    starts a run (more than the cap: the radix sort), in front of it the runs are few."""
    m, n, L, B = 16000, 2400, 8, 100
    msa = fso.synth_msa(fso.synth_spec(303, 20, 150, 2e-4, 0), m, n)
    ctx, _ = compare_long(pkg, msa, L, check_dp=False, block_len=B)
    p = ctx.pass2_paths()
    print(p)
    assert p["by_runs"] > 0 and p["by_sort"] > 0, p
    assert p["by_runs"] + p["by_sort"] == inner_boundaries(ctx), p
    assert p["max_runs"] > pkg.P2_RUN_CAP, p


def test_cap_edges(pkg, always, few):
    """The largest run count R of the run: at a cap of R every boundary still goes by runs, at R - 1 the largest ones sort
    their rows, at 0 all do; the states are the oracle's each time."""
    msa, ref = few
    R = run_gpu(pkg, msa, FEW["L"], block_len=FEW["B"]).pass2_paths()["max_runs"]
    assert 1 < R <= pkg.P2_RUN_CAP
    paths = {}
    for cap in (R, R - 1, 0):
        always.setenv("FSEQ_P2_RUN_CAP", str(cap))
        paths[cap] = run_checked(pkg, msa, ref, FEW["L"], FEW["B"]).pass2_paths()
    print(R, paths)
    total = paths[R]["by_runs"]
    assert total > 0 and paths[R]["by_sort"] == 0 and paths[R]["max_runs"] == R
    assert paths[R - 1]["by_sort"] >= 1 and paths[R - 1]["by_runs"] + paths[R - 1]["by_sort"] == total
    assert paths[R - 1]["max_runs"] == R
    assert paths[0]["by_runs"] == 0 and paths[0]["by_sort"] == total


def test_set_tuning_reaches_the_cap(pkg, always, few):
    msa, ref = few
    ctx = pkg.SegmentationContext(FEW["m"], FEW["n"], FEW["L"], block_len=FEW["B"])
    ctx.set_tuning("FSEQ_P2_RUN_CAP", 0)
    ctx.set_sequences(msa)
    ctx.run()
    p = ctx.pass2_paths()
    assert p["by_runs"] == 0 and p["by_sort"] > 0, p
    check_long(ctx, ref, FEW["n"], FEW["L"], check_dp=False)


def test_more_than_2_18_rows_sort_their_rows(pkg, always):
    """270,000 rows: a class and a position do not share a descriptor word, every boundary takes the radix sort."""
    m, n, L, B = 270000, 400, 8, 100
    msa = fso.synth_msa(fso.synth_spec(304, 4, 200, 1e-4, 0), m, n)
    ctx, _ = compare_long(pkg, msa, L, check_dp=False, block_len=B)
    assert ctx.timings()["reduced_blocks"] > 0
    p = ctx.pass2_paths()
    print(p)
    assert p["by_runs"] == 0 and p["by_sort"] == inner_boundaries(ctx) > 0 and p["max_runs"] == 0, p


def test_context_reused_on_another_input(pkg, always, few):
    """The records of a block belong to the input they were built from: a second, different input on the same context."""
    msa, ref = few
    ctx = run_checked(pkg, msa, ref, FEW["L"], FEW["B"])
    msa2 = fso.synth_msa(fso.synth_spec(305, 7, 200, 6e-4, 0), FEW["m"], FEW["n"])
    ref2 = fso.segment_long(msa2, FEW["L"], keep_dp=False, threads=4)
    ctx.set_sequences(msa2)
    try:
        ctx.run()
    except pkg.NoReduction:
        pass
    check_long(ctx, ref2, FEW["n"], FEW["L"], check_dp=False)
    assert ctx.pass2_paths()["by_runs"] > 0
