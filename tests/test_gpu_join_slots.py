"""The device joiners at every slot count up to their LDS limit.

fseq_join_greedy (class tables and co-occurrence edges, fseq_joinprep.hpp) and fseq_join_bipartite (texts, Kuhn-Munkres
and chaining, fseq_joinbip.hpp) lay out their LDS by X = max_segment_size: k_bip_match's lanes own columns j, j + 64 and
j + 128, both X x X matrices grow to ~130 KB at X = 181 (JP_MAX_CLASSES), and above that both joiners go to the host.
Founder mosaics (helpers.founder_mosaic) give exact X and steerable segment counts.  The references come from the oracle's
boundary states, not the device's: greedy_oracle.greedy_match, and the host bipartite joiner (fseq_join.hpp, checked against
scipy's optimum in test_join.py), which the device must equal entry for entry.  join_profile()'s bytes_d2h tells which path
ran, because the device paths also fall back to the host on their own (implausible class tables, failed allocations)."""
import hashlib
import importlib

import numpy as np
import pytest

import fso
import greedy_oracle as go
from helpers import founder_mosaic, founder_mosaic_segments
from test_join import mosaic_segmentation

pytestmark = pytest.mark.gpu

JP_MAX_CLASSES = 181                                           # fseq_joinprep.hpp


@pytest.fixture(scope="module")
def pkg():
    return importlib.import_module("founder-sequences_amd")


def joined_path(ctx, kind, S, m, X):
    """'device' or 'host' from the bytes the last join copied to the host."""
    b = ctx.join_profile()["bytes_d2h"]
    if b == S * m * 8:
        return "host"
    if kind == "bipartite" and b == S * X * 4 + S * 4:
        return "device"
    fixed = S * (2 * X + 3) * 4
    if kind == "greedy" and b >= fixed and (b - fixed) % 8 == 0:
        return "device"
    return "unknown (%d bytes)" % b


def run_device(pkg, msa, res, L=20, host=False):
    m, n = msa.shape
    ctx = pkg.SegmentationContext(m, n, L)
    if host:
        ctx.set_tuning("FSEQ_JOIN_HOST")
    ctx.set_sequences(np.ascontiguousarray(msa))
    r = ctx.run()
    assert r.max_segment_size == res["max_segment_size"]
    red = ctx.reduced_traceback()
    for f in ("lb", "rb", "segment_size"):
        assert np.array_equal(red[f], res["reduced"][f]), f
    return ctx


def references(pkg, m, res):
    red, X = res["reduced"], res["max_segment_size"]
    segs = [(int(x["lb"]), int(x["rb"])) for x in red]
    greedy = np.array(go.greedy_match(m, X, segs, res["a"], res["d"]), dtype=np.uint32).reshape(len(segs), X)
    bip, _ = pkg.bipartite_match_host(m, X, red["lb"], red["rb"], res["a"], res["d"])
    return greedy, bip


def check_joins(pkg, msa, res, want_path, host_too=False):
    """Both joiners of a device run equal the references, through the path named; with host_too, a second context with
    FSEQ_JOIN_HOST gives the same permutations through the host.  Returns the device context and the bipartite result."""
    m = msa.shape[0]
    X, S = res["max_segment_size"], len(res["reduced"])
    greedy, bip = references(pkg, m, res)
    ctx = run_device(pkg, msa, res)
    for kind, join, want in (("greedy", ctx.join_greedy, greedy), ("bipartite", ctx.join_bipartite, bip)):
        got = join()
        assert joined_path(ctx, kind, S, m, X) == want_path, kind
        assert got.shape == want.shape and np.array_equal(got, want), (kind, np.argwhere(got != want)[:5].tolist())
    if host_too:
        hctx = run_device(pkg, msa, res, host=True)
        for kind, join, want in (("greedy", hctx.join_greedy, greedy), ("bipartite", hctx.join_bipartite, bip)):
            got = join()
            assert joined_path(hctx, kind, S, m, X) == "host", kind
            assert np.array_equal(got, want), kind
    return ctx, bip


# X around k_bip_match's strip edges (64, 128) and up to the LDS limit: (X, m, n)
SLOT_CASES = [(2, 200, 3300), (63, 200, 3300), (64, 200, 3300), (65, 200, 3300), (127, 300, 5000), (128, 300, 5000),
              (129, 300, 5000), (180, 400, 8000), (181, 400, 8000)]


@pytest.mark.parametrize("X,m,n", SLOT_CASES)
def test_device_joiners_at_slot_count(pkg, X, m, n):
    msa, res = mosaic_segmentation(X, m, n, None)
    if X > 2:
        assert (res["reduced"]["segment_size"] < X).any() and (res["reduced"]["segment_size"] == X).any()
    check_joins(pkg, msa, res, "device", host_too=True)


@pytest.mark.parametrize("X,m,n", [(182, 400, 8000), (301, 400, 4000)])
def test_host_fallback_above_the_lds_limit(pkg, X, m, n):
    msa, res = mosaic_segmentation(X, m, n, None)
    check_joins(pkg, msa, res, "host")


@pytest.mark.parametrize("X,m", [(65, 200), (181, 400)])
@pytest.mark.parametrize("S", [1, 2, 32, 33, 34, 65])
def test_chain_tiles(pkg, X, m, S):
    """k_bip_chain stages the matchings in tiles of 32 segments: one segment (no pair: k_bip_match and k_join_edges are
    not launched), one pair, a full tile, a tile and one or two segments behind it, two full tiles and one."""
    msa, res = founder_mosaic_segments(X, m, S)
    check_joins(pkg, msa, res, "device")


@pytest.mark.parametrize("X,m,n,copies", [(64, 192, 3300, 3), (130, 260, 3300, 2), (181, 362, 3300, 2)])
def test_tie_heavy_inputs(pkg, X, m, n, copies):
    """Every class of a segment equally large: the texts' size order and the matching's choice among the many optimal
    matchings must break ties as the host does."""
    msa, res = mosaic_segmentation(X, m, n, copies)
    check_joins(pkg, msa, res, "device")


@pytest.mark.parametrize("m,n", [(12000, 2500), (70000, 2000)])
def test_many_rows_at_the_lds_limit(pkg, m, n):
    """X = 181 on streamed rows (m > 11,264: the boundary states come from the streamed pass 2) and with row ids above
    16 bits; neither m is a multiple of 64."""
    msa, res = mosaic_segmentation(JP_MAX_CLASSES, m, n, None, seed=5)
    assert len(res["reduced"]) > 10
    check_joins(pkg, msa, res, "device")


def test_device_matchings_are_optimal_at_the_lds_limit(pkg):
    """Independent of the host joiner: the device permutations' realised weights against scipy's optimum."""
    import join_oracle as jo
    from collections import Counter
    m = 400
    msa, res = mosaic_segmentation(JP_MAX_CLASSES, m, 8000, None)
    red, X = res["reduced"], res["max_segment_size"]
    ctx = run_device(pkg, msa, res)
    perm = ctx.join_bipartite()
    assert joined_path(ctx, "bipartite", len(red), m, X) == "device"
    for s in (1, 2, len(red) // 2, len(red) - 1):
        sl, cl = [], []
        for t in (s - 1, s):
            c = jo.classes(m, int(red["lb"][t]), res["a"][t], res["d"][t])
            slots = jo.slot_classes(perm[t], c)
            assert Counter((len(c[i]), k) for i, k in Counter(slots).items()) == jo.bipartite_copy_multiset(m, X, c)
            sl.append(slots)
            cl.append(c)
        best, base = jo.optimal_weight(sl[0], cl[0], sl[1], cl[1])
        assert sum(int(base[l, r]) for l, r in zip(sl[0], sl[1])) == best, s


def test_device_founders_writer_at_the_lds_limit(pkg, tmp_path):
    m = 400
    msa, res = mosaic_segmentation(JP_MAX_CLASSES, m, 8000, None)
    ctx, bip = check_joins(pkg, msa, res, "device")
    a, b = str(tmp_path / "h.txt"), str(tmp_path / "d.txt")
    ctx.write_founders(np.ascontiguousarray(msa), bip, a)
    ctx.write_founders_device(bip, b)
    assert open(a, "rb").read() == open(b, "rb").read()


def _sha(path):
    h = hashlib.sha256()
    with open(path, "rb") as f:
        for chunk in iter(lambda: f.read(1 << 24), b""):
            h.update(chunk)
    return h.hexdigest()


def test_device_founders_writer_in_two_batches(pkg, tmp_path):
    """X = 181 lines of 1.5 M columns are more than 256 MiB: k_founders runs in two batches."""
    X, m, n = JP_MAX_CLASSES, 200, 1_500_000
    assert X * (n + 1) > (256 << 20)
    msa = founder_mosaic(X, m, n, brec=1000, seed=3)
    ctx = pkg.SegmentationContext(m, n, 20)
    ctx.set_sequences(msa)
    res = ctx.run()
    assert res.max_segment_size == X
    perm = ctx.join_bipartite()
    assert joined_path(ctx, "bipartite", res.segment_count, m, X) == "device"
    assert perm.max() < m                                      # (the host writer indexes its rows with them)
    a, b = str(tmp_path / "h.txt"), str(tmp_path / "d.txt")
    ctx.write_founders(msa, perm, a)
    ctx.write_founders_device(perm, b)
    assert _sha(a) == _sha(b)


def test_config_c5_full_size_joiners(pkg):
    """BASELINE C5 at full size (m = 10,000 x n = 1,000,000, X = 159): every boundary state on the host; the device
    bipartite permutations equal the host joiner's on them, and the device greedy equals the FSEQ_JOIN_HOST form."""
    c = fso.CONFIGS["C5"]
    m, n, L = c["m"], c["n"], c["L"]
    ctx = pkg.SegmentationContext(m, n, L)
    ctx.generate_synthetic(c["seed"], c["K"], c["B"], c["mu"], c["kind"])
    r = ctx.run()
    X, S = int(r.max_segment_size), int(r.segment_count)
    assert X == 159 and S > 8000
    red = ctx.reduced_traceback()
    perm_bip = ctx.join_bipartite()
    assert joined_path(ctx, "bipartite", S, m, X) == "device"
    perm_greedy = ctx.join_greedy()
    assert joined_path(ctx, "greedy", S, m, X) == "device"
    A = np.empty((S, m), dtype=np.uint32)
    D = np.empty((S, m), dtype=np.uint32)
    for i in range(S):
        A[i], D[i] = ctx.boundary_state(i)
    host_bip, _ = pkg.bipartite_match_host(m, X, red["lb"], red["rb"], A, D)
    del A, D
    assert np.array_equal(perm_bip, host_bip), np.argwhere(perm_bip != host_bip)[:5].tolist()
    ctx.set_tuning("FSEQ_JOIN_HOST")                           # (drops the result: the same input segmented again)
    ctx.run()
    assert np.array_equal(ctx.reduced_traceback(), red)
    host_greedy = ctx.join_greedy()
    assert joined_path(ctx, "greedy", S, m, X) == "host"
    assert np.array_equal(perm_greedy, host_greedy)
