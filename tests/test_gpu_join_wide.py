"""The wide device front of fseq_join_greedy (fseq_joinprep.hpp: k_join_classes_wide, k_join_edges_wide, k_join_scan).

Above 181 classes a segment the pair's counter matrix no longer fits LDS: the wide front walks it in strips of consecutive
left classes (32,768 counters a strip), counts the edges in a first pass, scans the counts into offsets and writes the
edges in a second pass.  FSEQ_JOIN_WIDE forces it at any max_segment_size; by itself it runs above 181 classes from 16 MiB
of boundary states on, which none of these shapes reaches.  Founder mosaics (helpers.founder_mosaic) give exact X; the
references come from the oracle's boundary states through greedy_oracle.greedy_match, not from the device.  Every case
asserts the path that ran (join_path()), the permutations against the reference, and the same permutations from a second
context that goes through the all-host joiner (FSEQ_JOIN_HOST)."""
import functools
import importlib

import numpy as np
import pytest

import greedy_oracle as go
from helpers import founder_mosaic_segments
from test_join import mosaic_segmentation as _mosaic_segmentation

pytestmark = pytest.mark.gpu

JW_CELLS = 32768                                               # fseq_joinprep.hpp: counters of a strip
HOST, LDS, WIDE = 0, 1, 2                                      # fseq_debug_join_path


@pytest.fixture(scope="module")
def pkg():
    return importlib.import_module("founder-sequences_amd")


@functools.lru_cache(maxsize=None)
def mosaic_segmentation(X, m, n, copies, seed=None):
    """(alignment, the oracle's segmentation), computed once per shape and left unchanged by every test."""
    return _mosaic_segmentation(X, m, n, copies, seed=seed)


def run_device(pkg, msa, res, tuning=None, L=20):
    m, n = msa.shape
    ctx = pkg.SegmentationContext(m, n, L)
    if tuning:
        ctx.set_tuning(tuning)
    ctx.set_sequences(np.ascontiguousarray(msa))
    r = ctx.run()
    assert r.max_segment_size == res["max_segment_size"]
    red = ctx.reduced_traceback()
    for f in ("lb", "rb", "segment_size"):
        assert np.array_equal(red[f], res["reduced"][f]), f
    return ctx


def reference(m, res):
    red, X = res["reduced"], res["max_segment_size"]
    segs = [(int(x["lb"]), int(x["rb"])) for x in red]
    return np.array(go.greedy_match(m, X, segs, res["a"], res["d"]), dtype=np.uint32).reshape(len(segs), X)


def check_wide(pkg, msa, res):
    """The forced wide front gives the reference through path 2, a second context with FSEQ_JOIN_HOST the same through
    path 0.  Returns (the wide context, the permutations)."""
    want = reference(msa.shape[0], res)
    ctx = run_device(pkg, msa, res, "FSEQ_JOIN_WIDE")
    got = ctx.join_greedy()
    assert ctx.join_path() == WIDE
    assert got.shape == want.shape and np.array_equal(got, want), np.argwhere(got != want)[:5].tolist()
    hctx = run_device(pkg, msa, res, "FSEQ_JOIN_HOST")
    host = hctx.join_greedy()
    assert hctx.join_path() == HOST
    assert np.array_equal(host, want)
    return ctx, got


def strips(res):
    """Most strips a pair of this segmentation needs: ceil(LC / floor(JW_CELLS / RC))."""
    sz = res["reduced"]["segment_size"].astype(np.int64)
    return max([1] + [-(-int(lc) // (JW_CELLS // int(rc))) for lc, rc in zip(sz[:-1], sz[1:])])


@pytest.mark.parametrize("X,m,n", [(2, 200, 3300), (64, 200, 3300), (181, 400, 8000)])
def test_one_strip_on_the_lds_fronts_ground(pkg, X, m, n):
    """Forced wide where the LDS front runs by itself: one strip a pair, and the results of the same input with no tuning,
    which goes through path 1."""
    msa, res = mosaic_segmentation(X, m, n, None)
    assert strips(res) == 1
    _, got = check_wide(pkg, msa, res)
    ctx = run_device(pkg, msa, res)
    plain = ctx.join_greedy()
    assert ctx.join_path() == LDS
    assert np.array_equal(plain, got)


@pytest.mark.parametrize("X,m,n", [(182, 400, 8000), (301, 400, 4000)])
def test_the_strip_border(pkg, X, m, n):
    """182 x 182 = 33,124 counters: the first X whose full pairs need two strips."""
    msa, res = mosaic_segmentation(X, m, n, None)
    assert strips(res) >= 2
    check_wide(pkg, msa, res)


@pytest.mark.parametrize("X,m,n,most", [(600, 1200, 3300, 11), (1157, 2400, 3300, 42)])
def test_many_strips_and_unequal_class_counts(pkg, X, m, n, most):
    """X = 1,157 is BASELINE C4's: 28 left classes a strip at a full right segment, up to 42 strips a pair.  The mosaic's blocks use
    subsets of the founders, so adjacent segments have different class counts."""
    msa, res = mosaic_segmentation(X, m, n, None)
    sz = res["reduced"]["segment_size"]
    assert (sz < X).any() and (sz == X).any() and (sz[:-1] != sz[1:]).any()
    assert strips(res) == most
    check_wide(pkg, msa, res)


def test_ties(pkg):
    """Every class of a segment equally large: the edge order is all that separates the host's choices."""
    msa, res = mosaic_segmentation(300, 600, 3300, 2)
    check_wide(pkg, msa, res)


@pytest.mark.parametrize("S", [1, 2, 65])
def test_no_pair_one_pair_many(pkg, S):
    """One segment: no edge kernel is launched and the scan runs over no pair."""
    msa, res = founder_mosaic_segments(300, 600, S)
    assert len(res["reduced"]) == S
    check_wide(pkg, msa, res)


def test_row_ids_above_16_bits_on_streamed_boundary_states(pkg):
    """m = 70,000 (no multiple of 64 or 1,024): the boundary states come from the streamed pass 2, a strip's rows span many
    rounds of the workgroup, representatives need more than 16 bits."""
    m = 70000
    msa, res = mosaic_segmentation(300, m, 2000, None, seed=5)
    assert len(res["reduced"]) > 10
    _, got = check_wide(pkg, msa, res)
    assert got.max() > 0xFFFF


def test_the_front_by_itself_stays_off_below_its_threshold(pkg):
    """128 KB of boundary states above the LDS limit: no tuning, the all-host joiner."""
    msa, res = mosaic_segmentation(301, 400, 4000, None)
    ctx = run_device(pkg, msa, res)
    got = ctx.join_greedy()
    assert ctx.join_path() == HOST
    assert np.array_equal(got, reference(400, res))


def test_founders_through_the_device_writer(pkg, tmp_path):
    msa, res = mosaic_segmentation(600, 1200, 3300, None)
    ctx, perm = check_wide(pkg, msa, res)
    a, b = str(tmp_path / "h.txt"), str(tmp_path / "d.txt")
    ctx.write_founders(np.ascontiguousarray(msa), perm, a)
    ctx.write_founders_device(perm, b)
    assert open(a, "rb").read() == open(b, "rb").read()


def test_join_path_before_a_join(pkg):
    msa, res = mosaic_segmentation(64, 200, 3300, None)
    ctx = run_device(pkg, msa, res, "FSEQ_JOIN_WIDE")
    with pytest.raises(pkg.FseqError) as err:
        ctx.join_path()
    assert err.value.code == pkg.FSEQ_E_ARG
    ctx.join_greedy()
    assert ctx.join_path() == WIDE
