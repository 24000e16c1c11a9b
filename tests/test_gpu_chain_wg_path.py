"""One whole run on streamed rows with phase B's chains on a workgroup each (k_chain_wg: FSEQ_CHAIN_WG=1, every streamed launch of
phase B) and on the spread kernels alone (FSEQ_CHAIN_WG=2): segments, traceback and every boundary state equal, and equal to the
oracle's.  A founder mosaic of just over 11,264 rows; 60 blocks in chains of four, so that phase B has two levels below its top
chain -- compositions from the identity and expansions from the states of the level above, by runs and by the sort of the rows."""
import importlib
import re

import numpy as np
import pytest

import fso
from helpers import founder_mosaic
from test_gpu_parity import check_long

pytestmark = pytest.mark.gpu

M, N, L, B, FAN = 11300, 3000, 20, 50, 4


@pytest.fixture(scope="module")
def pkg():
    return importlib.import_module("founder-sequences_amd")


@pytest.fixture(scope="module")
def mosaic():
    msa = founder_mosaic(12, M, N, brec=100, seed=1401)
    return msa, fso.segment_long(msa, L, keep_dp=False, threads=4)


def run_with(pkg, msa, knob):
    ctx = pkg.SegmentationContext(M, N, L, block_len=B)
    ctx.set_tuning("FSEQ_CHAIN_FAN", FAN)
    ctx.set_tuning("FSEQ_CHAIN_WG", knob)
    ctx.set_tuning("FSEQ_DEBUG", 1)
    ctx.set_sequences(msa)
    try:
        ctx.run()
    except pkg.NoReduction:
        pass
    return ctx


def test_both_forms_of_phase_b_equal_the_oracle(pkg, mosaic, capfd):
    msa, ref = mosaic
    capfd.readouterr()
    wg = run_with(pkg, msa, 1)
    note = capfd.readouterr().err
    spread = run_with(pkg, msa, 2)
    note_spread = capfd.readouterr().err
    assert wg.timings()["n_blocks"] == N // B
    for ctx in (wg, spread):
        check_long(ctx, ref, N, L, check_dp=False)
    for f in ("lb", "rb", "segment_max_size", "segment_size"):
        assert np.array_equal(wg.traceback()[f], spread.traceback()[f]), f
    # which kernels ran, from the library's own notes: the counters of k_chain_wg, kept on request
    found = re.search(r"phase B chain steps on a workgroup of their own: (\d+) by runs, (\d+) by the sort of the rows, (\d+) from the identity", note)
    assert found, note
    by_runs, by_sort, ident = (int(x) for x in found.groups())
    # 60 blocks in chains of 4: 15 composites, those in chains of 4: 4 composites, which the top chain takes.  Up: every block of a
    # level once, 60 + 15 steps, the first of each of the 15 + 4 chains from the identity.  The top chain: 4 steps, the first from the
    # identity.  Down: all but the last block of every chain, and the last of all: 15 - 4 + 1 and 60 - 15 + 1 steps.
    assert ident == 15 + 4 + 1 and by_runs > 0
    assert by_runs + by_sort + ident == (60 + 15) + 4 + (15 - 4 + 1) + (60 - 15 + 1)
    assert "on a workgroup of their own" not in note_spread
