"""Pass 2's streamed chain step (k_chain_snap_grouped, csrc/fseq_chainsort.hpp) with the keys phase B hands over: for a block whose
flag is set the kernel reads the block's ranks in the order of its boundary state from the handed-over array and gathers none.  One
launch of chain_step_cases.build_grouped -- three blocks; tasks on the run path, on the radix path, a border copy and a skipped task --
with keys handed over for some blocks and not for others: every output word equals the same call without any handed-over keys and
the numpy model's.  Integers, no tolerance."""
import importlib

import numpy as np
import pytest

import chain_step_cases as cs

pytestmark = pytest.mark.gpu

GARBAGE = 0xFFFF            # no rank of any block (cap is 1,207): what lies behind a clear flag


@pytest.fixture(scope="module")
def pkg():
    return importlib.import_module("founder-sequences_amd")


@pytest.fixture(scope="module")
def grouped(pkg):
    """The launch, the model's outputs, and the outputs of the call without handed-over keys (once for the module)."""
    G = cs.build_grouped()
    args = (G["a0"], G["d0"], G["rank"], G["task_blk"], G["cls"], G["headd"], G["ncls"])
    model = cs.pass2_model(*args, cs.P2_RUN_CAP)
    plain = pkg.pass2_step(*args, workgroups=2)
    for got, want in zip(plain, model):
        assert np.array_equal(got, want)
    assert set(G["paths"]) == {"runs", "p4", "copy", "skip"}
    return G, args, model


def keys_of(G, flags, wrong_behind_clear=True):
    hk = np.stack([G["rank"][b][G["a0"][b]] for b in range(len(flags))]).astype(np.uint16)
    for b, f in enumerate(flags):
        if not f and wrong_behind_clear:
            hk[b] = GARBAGE
    return hk


@pytest.mark.parametrize("flags", [(1, 1, 1), (0, 1, 0), (1, 0, 1), (0, 0, 1), (0, 0, 0)], ids=lambda f: "".join(map(str, f)))
@pytest.mark.parametrize("workgroups", [1, 3])
def test_handed_keys_change_nothing(pkg, grouped, flags, workgroups):
    G, args, model = grouped
    # block 1 holds tasks of every kind; blocks 0 and 2 one task each, by runs and by the sort of the rows
    assert [G["paths"][t] for t in np.flatnonzero(G["task_blk"] == 1)] == ["runs", "p4", "copy", "skip", "runs"]
    sa, sd, stats, hand = pkg.pass2_step(*args, workgroups=workgroups, hand_keys=keys_of(G, flags), hand_flag=np.array(flags))
    for got, want, name in zip((sa, sd, stats), model, ("snap_a", "snap_d", "stats")):
        assert np.array_equal(got, want), name
    # a group a block: the groups that took handed-over keys are the blocks with a set flag
    assert tuple(hand) == (sum(flags), 3 - sum(flags))


def test_a_wrong_array_behind_a_clear_flag_is_not_read(pkg, grouped):
    """Every flag clear, every handed-over word wrong -- in range (so that reading it would change the classes, not fault) and out of
    range alike: the outputs are the model's."""
    G, args, model = grouped
    for wrong in (np.zeros_like(G["a0"], dtype=np.uint16), np.full(G["a0"].shape, GARBAGE, dtype=np.uint16),
                  keys_of(G, (1, 1, 1))[::-1].copy()):
        sa, sd, stats, hand = pkg.pass2_step(*args, workgroups=2, hand_keys=wrong, hand_flag=np.zeros(3, dtype=np.uint32))
        for got, want in zip((sa, sd, stats), model):
            assert np.array_equal(got, want)
        assert tuple(hand) == (0, 3)


def test_a_wrong_array_behind_a_set_flag_is_read(pkg, grouped):
    """The test bites: block 0's keys swapped for block 2's behind a SET flag change block 0's task (a handed-over array is used
    where its flag says so) -- and nothing else."""
    G, args, model = grouped
    hk = keys_of(G, (1, 1, 1))
    hk[0] = hk[2]
    sa, sd, stats, hand = pkg.pass2_step(*args, workgroups=2, hand_keys=hk, hand_flag=np.array([1, 0, 0]))
    t0 = np.flatnonzero(G["task_blk"] == 0)
    assert not np.array_equal(sa[t0], model[0][t0])
    rest = np.flatnonzero(G["task_blk"] != 0)
    assert np.array_equal(sa[rest], model[0][rest]) and np.array_equal(sd[rest], model[1][rest])


def test_refusals(pkg, grouped):
    G, args, _ = grouped
    with pytest.raises(pkg.FseqError):                                       # a key that is no rank of the block behind a set flag
        pkg.pass2_step(*args, hand_keys=np.full(G["a0"].shape, GARBAGE, dtype=np.uint16), hand_flag=np.array([0, 1, 0]))
    with pytest.raises(pkg.FseqError):                                       # one without the other
        pkg.pass2_step(*args, hand_keys=keys_of(G, (1, 1, 1)))
