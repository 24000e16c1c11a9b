"""fseq_set_segment_length on the card: a context that has run at one segment length, set to another, gives bit for bit what a
fresh context created with that length gives on the same rows -- the result, the traceback, the segments, every boundary state
and the permutations of all three joiners."""
import functools
import importlib

import numpy as np
import pytest

import proto_length_scan as P

pytestmark = pytest.mark.gpu

E_ARG, E_UNSUPPORTED = 1, 5


@pytest.fixture(scope="module")
def pkg():
    return importlib.import_module("founder-sequences_amd")


@functools.lru_cache(maxsize=None)
def rows(kind):
    if kind == "lds":
        return P.case_msa("lds_resident")
    if kind == "streamed":
        return P.mosaic(8, 11265, 4000, seed=31, mu=0.0005)
    # identity columns: every fourth column of a mosaic set to one symbol
    msa = P.mosaic(6, 80, 3200, seed=41, mu=0.001)
    msa[:, ::4] = ord("A")
    return msa


def run(pkg, ctx):
    try:
        return ctx.run()
    except pkg.NoReduction:
        return ctx.result


def everything(pkg, ctx):
    res = run(pkg, ctx)
    out = [res.max_segment_size, res.short_path, res.dp_segment_count, res.segment_count]
    if res.short_path:
        return out + [x.tobytes() for x in ctx.short_path_runs()]
    red = ctx.reduced_traceback()
    out += [ctx.traceback().tobytes(), red.tobytes()]
    out += [tuple(x.tobytes() for x in ctx.boundary_state(i)) for i in range(len(red))]
    if res.max_segment_size < ctx.m:
        out += [ctx.join_greedy().tobytes(), ctx.join_bipartite().tobytes(), ctx.join_random(seed=5).tobytes()]
    return out


def fresh(pkg, msa, L):
    ctx = pkg.SegmentationContext(msa.shape[0], msa.shape[1], L)
    ctx.set_sequences(msa)
    return ctx


@functools.lru_cache(maxsize=None)
def fresh_everything(kind, L):
    pkg = importlib.import_module("founder-sequences_amd")
    ctx = fresh(pkg, rows(kind), L)
    out = everything(pkg, ctx)
    ctx.close()
    return out


@pytest.mark.parametrize("kind,lengths", [("lds", (20, 97)), ("lds", (200, 5)), ("lds", (20, 2000, 7)), ("streamed", (64, 200))])
def test_another_length_equals_a_fresh_context(pkg, kind, lengths):
    """L2 > L1; L2 < L1 (200 -> 5: the DP arrays grow); long -> short -> long; streamed rows."""
    msa = rows(kind)
    ctx = fresh(pkg, msa, lengths[0])
    assert everything(pkg, ctx) == fresh_everything(kind, lengths[0])
    for L in lengths[1:]:
        ctx.set_segment_length(L)
        out = np.zeros(4, dtype=pkg.SEGMENT_DTYPE)
        assert ctx.L.fseq_get_segments(ctx.h, out.ctypes.data) == E_ARG      # no result until the next run
        assert everything(pkg, ctx) == fresh_everything(kind, L), L
    ctx.close()


def test_context_without_identity_columns(pkg, tmp_path):
    msa = rows("identity")
    src = fresh(pkg, msa, 30)
    a = src.without_identity_columns(30)
    b = src.without_identity_columns(12)
    src.close()
    assert a.n == b.n < msa.shape[1]
    run(pkg, a)
    a.set_segment_length(12)
    assert everything(pkg, a) == everything(pkg, b)
    # the identity relation is kept: the restored founders are those of the context made at that length
    pa, pb = tmp_path / "a.txt", tmp_path / "b.txt"
    a.write_founders_restored(a.join_greedy(), str(pa))
    b.write_founders_restored(b.join_greedy(), str(pb))
    assert pa.read_bytes() == pb.read_bytes() and len(pa.read_bytes().split(b"\n")[0]) == msa.shape[1]
    a.close()
    b.close()


def test_refusals_change_nothing(pkg):
    msa = rows("lds")
    ctx = fresh(pkg, msa, 20)
    before = everything(pkg, ctx)
    with pytest.raises(pkg.FseqError) as e:
        ctx.set_segment_length(0)
    assert e.value.code == E_ARG and ctx.segment_length == 20
    assert ctx.reduced_traceback().tobytes() == before[5]          # the result is still there
    assert ctx.L.fseq_set_segment_length(None, 5) == E_ARG
    ctx.close()
    # a chunked input under way
    c2 = pkg.SegmentationContext(msa.shape[0], msa.shape[1], 20)
    c2.input_begin(staging_bytes=1 << 22)
    with pytest.raises(pkg.FseqError) as e:
        c2.set_segment_length(30)
    assert e.value.code == E_ARG
    c2.close()


def test_device_bytes_settle_under_cycling(pkg):
    """L1, L2, L1, L2 with a run at each: no more device bytes after the fourth than after the second (the DP arrays and the
    traceback buffer have grown to the smaller length's sizes and stay)."""
    msa = rows("lds")
    ctx = fresh(pkg, msa, 200)
    held = []
    for L in (200, 5, 200, 5):
        ctx.set_segment_length(L)
        run(pkg, ctx)
        held.append(ctx.device_bytes()[0])
    assert held[3] <= held[1] and held[2] <= held[1]
    ctx.close()


def test_match_founders_after_another_length(pkg):
    msa = rows("lds")
    ctx = fresh(pkg, msa, 20)
    run(pkg, ctx)
    ctx.match_founders(permutations=ctx.join_greedy())
    ctx.set_segment_length(56)
    with pytest.raises(pkg.FseqError):
        ctx.match_pieces()                                         # the last match went with the result
    run(pkg, ctx)
    got = ctx.match_founders(permutations=ctx.join_greedy())
    ref = fresh(pkg, msa, 56)
    run(pkg, ref)
    want = ref.match_founders(permutations=ref.join_greedy())
    drop = lambda s: {k: v for k, v in s.items() if k != "ms_device"}
    assert drop(got) == drop(want)
    assert ctx.match_pieces()[0].tobytes() == ref.match_pieces()[0].tobytes()
    ctx.close()
    ref.close()
