"""Pass 2 on streamed rows behind the reduced phase C (k_chain_snap_grouped, csrc/fseq_chainsort.hpp): a block's boundaries on one
workgroup, the block's ranks gathered once, the class table in LDS, one record gather per row.

Shapes with a short segment length, so that blocks hold several boundaries each.  Reached here: the sort in one digit pass
(every block at most 512 representatives, so at most 512 classes) and in two (blocks of more than 512), boundaries on a
block border (copies of the border state), and blocks that run on all rows beside reduced ones (their boundaries go to
k_colblock_stream).  Every boundary state is compared with the oracle where it is affordable; at m = 100,000 the run
through the representatives is compared with the run on all rows (FSEQ_NO_REDUCED), which computes the same states
without them."""
import importlib

import numpy as np
import pytest

import fso
from test_gpu_parity import compare_long, run_gpu

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def pkg():
    return importlib.import_module("founder-sequences_amd")


@pytest.fixture()
def always(monkeypatch):
    monkeypatch.setenv("FSEQ_REDUCED_ALWAYS", "1")
    return monkeypatch


def boundaries_per_block(ctx):
    t = ctx.timings()
    rb = ctx.reduced_traceback()["rb"].astype(np.int64)
    inner = rb[rb % t["block_len"] != 0]
    return len(rb), len(inner) - len(np.unique(inner // t["block_len"])), int(np.sum(rb % t["block_len"] == 0))


@pytest.mark.parametrize("m,n,L,K,Brec,mu,seed,B,two_pass", [
    (12000, 2400, 8, 12, 300, 3e-4, 201, 100, False),       # few founders: at most 512 classes, one digit pass
    (20000, 1600, 6, 24, 200, 2e-4, 202, 64, None),
    (16000, 1500, 8, 900, 200, 1e-4, 203, 100, True),       # hundreds of founders: blocks of more than 512 representatives
])
def test_streamed_pass2_matches_oracle(pkg, always, m, n, L, K, Brec, mu, seed, B, two_pass):
    msa = fso.synth_msa(fso.synth_spec(seed, K, Brec, mu, 0), m, n)
    ctx, _ = compare_long(pkg, msa, L, check_dp=False, block_len=B)
    t = ctx.timings()
    assert t["reduced_blocks"] > 0
    nb, repeats, _ = boundaries_per_block(ctx)
    assert repeats > 0, "no block holds two boundaries"
    if two_pass:
        assert t["reduced_rows_mean"] > 512, t
    elif two_pass is not None:
        assert t["reduced_rows_mean"] <= 512, t


def test_streamed_pass2_border_copies_and_blocks_on_all_rows(pkg, always):
    """Boundaries on block borders, and blocks with more representatives than FSEQ_REDUCED_CAP (their boundaries from the
    block's start on all rows) beside the reduced blocks."""
    m, n, L, K, Brec, mu, seed, B = 16000, 3000, 4, 20, 150, 5e-4, 204, 50
    msa = fso.synth_msa(fso.synth_spec(seed, K, Brec, mu, 0), m, n)
    mean = run_gpu(pkg, msa, L, block_len=B).timings()["reduced_rows_mean"]
    always.setenv("FSEQ_REDUCED_CAP", str(mean))
    ctx, _ = compare_long(pkg, msa, L, check_dp=False, block_len=B)
    t = ctx.timings()
    assert 0 < t["reduced_blocks"] < t["n_blocks"], t
    _, repeats, borders = boundaries_per_block(ctx)
    assert repeats > 0 and borders > 0, (repeats, borders)


def test_streamed_pass2_at_100k_rows_matches_the_run_on_all_rows(pkg, monkeypatch):
    """C4's row count with a short alignment: the library's own choice (the representatives) against FSEQ_NO_REDUCED, every
    boundary state."""
    m, n, L = 100000, 4000, 40
    msa = fso.synth_msa(fso.synth_spec(0x5EED0004, 64, 600, 5e-5, 0), m, n)
    ctx = run_gpu(pkg, msa, L, block_len=200)
    assert ctx.timings()["reduced_blocks"] > 0
    assert boundaries_per_block(ctx)[1] > 0
    monkeypatch.setenv("FSEQ_NO_REDUCED", "1")
    ref = run_gpu(pkg, msa, L, block_len=200)
    assert ref.timings()["reduced_blocks"] == 0
    assert np.array_equal(ctx.reduced_traceback(), ref.reduced_traceback())
    for i in range(len(ctx.reduced_traceback())):
        a, d = ctx.boundary_state(i)
        ra, rd = ref.boundary_state(i)
        assert np.array_equal(a, ra) and np.array_equal(d, rd), i
