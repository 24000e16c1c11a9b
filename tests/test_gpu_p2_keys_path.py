"""One whole run on streamed rows with phase B's keys handed to pass 2 (FSEQ_P2_KEYS unset) and without (FSEQ_P2_KEYS=2, every group of
pass 2 gathers its own): both equal the oracle and each other in every boundary state.  The shape of tests/test_gpu_chain_wg_path.py:
11,300 rows, 60 blocks of 50 columns in chains of four, phase B's chains on a workgroup each (FSEQ_CHAIN_WG=1).  Then the same
context takes another input, and another segment length: a flag left over from the run before would be a silent wrong answer."""
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


def context(pkg, keys):
    ctx = pkg.SegmentationContext(M, N, L, block_len=B)
    ctx.set_tuning("FSEQ_CHAIN_FAN", FAN)
    ctx.set_tuning("FSEQ_CHAIN_WG", 1)
    ctx.set_tuning("FSEQ_DEBUG", 1)
    if keys is not None:
        ctx.set_tuning("FSEQ_P2_KEYS", keys)
    return ctx


def run(pkg, ctx, msa=None):
    if msa is not None:
        ctx.set_sequences(msa)
    try:
        ctx.run()
    except pkg.NoReduction:
        pass
    return ctx


def groups_of(note):
    """(groups pass 2's chain steps ran, groups that took handed-over keys, groups that gathered) from the library's notes."""
    ran = re.findall(r"pass 2 chain steps: (\d+) groups on", note)
    took = re.findall(r"pass 2 chain steps: (\d+) groups took the keys phase B handed over, (\d+) gathered their own", note)
    assert ran and took, note
    return int(ran[-1]), int(took[-1][0]), int(took[-1][1])


def states(ctx):
    return [ctx.boundary_state(i) for i in range(len(ctx.reduced_traceback()))]


def test_handed_keys_and_gathered_keys_equal_the_oracle(pkg, capfd):
    msa = founder_mosaic(12, M, N, brec=100, seed=1401)
    ref = fso.segment_long(msa, L, keep_dp=False, threads=4)
    capfd.readouterr()
    handed = run(pkg, context(pkg, None), msa)
    note = capfd.readouterr().err
    gathered = run(pkg, context(pkg, 2), msa)
    note2 = capfd.readouterr().err
    for ctx in (handed, gathered):
        check_long(ctx, ref, N, L, check_dp=False)
    for (a, d), (a2, d2) in zip(states(handed), states(gathered)):
        assert np.array_equal(a, a2) and np.array_equal(d, d2)
    # the level-0 expansion steps through all but the last block of its 15 chains, and the last of all: 60 - 15 + 1 blocks
    ran, took, own = groups_of(note)
    assert 0 < took <= 60 - 15 + 1 and took + own == ran
    ran2, took2, own2 = groups_of(note2)
    assert took2 == 0 and own2 == ran2 == ran

    # the same context, another input: the flags of the run before must not be taken for this one's
    msa_b = founder_mosaic(12, M, N, brec=100, seed=1402)
    ref_b = fso.segment_long(msa_b, L, keep_dp=False, threads=4)
    assert not np.array_equal(ref_b["reduced"]["rb"], ref["reduced"]["rb"])
    run(pkg, handed, msa_b)
    check_long(handed, ref_b, N, L, check_dp=False)
    ran, took, own = groups_of(capfd.readouterr().err)
    assert took > 0 and took + own == ran
    # ... and another segment length on the resident alignment
    L2 = 33
    ref_c = fso.segment_long(msa_b, L2, keep_dp=False, threads=4)
    handed.set_segment_length(L2)
    run(pkg, handed)
    check_long(handed, ref_c, N, L2, check_dp=False)
    ran, took, own = groups_of(capfd.readouterr().err)
    assert took + own == ran
