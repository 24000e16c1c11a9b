"""The wide device form of fseq_join_bipartite (fseq_joinbipw.hpp: k_bip_minrow_wide, k_bip_texts_wide, k_bip_match_wide,
k_bip_chain_wide behind k_join_classes_wide).

Above 181 texts a segment the pair's X x X weight matrix no longer fits LDS: the wide form keeps it in a slab of device
memory per persistent workgroup and the potentials, the matching and the per-column state in LDS, and restates the host's
Kuhn-Munkres in the host's order of arithmetic.  FSEQ_JOIN_BIP_WIDE forces it at any max_segment_size up to 4,096; by itself
it is not reached by any of these shapes.  Founder mosaics (helpers.founder_mosaic) give exact X.  The reference of every
case is the host joiner (bipartite_match_host) on the *oracle's* boundary states, never a device result.  Every case asserts
the path that ran (bipartite_path()), the permutations against the reference entry for entry, and the same from a second
context that goes through the host joiner (FSEQ_JOIN_HOST)."""
import functools
import importlib
import os
import subprocess

import numpy as np
import pytest

import fso
from helpers import founder_mosaic_segments
from test_join import check_bipartite_host
from test_gpu_join_wide import mosaic_segmentation           # (the shapes of that file: one oracle run serves both)

pytestmark = pytest.mark.gpu

HOST, LDS, WIDE = 0, 1, 2                                      # fseq_debug_bipartite_path


@pytest.fixture(scope="module")
def pkg():
    return importlib.import_module("founder-sequences_amd")


@functools.lru_cache(maxsize=None)
def mosaic_segments(X, m, S):
    return founder_mosaic_segments(X, m, S)


def reference(pkg, m, res):
    red = res["reduced"]
    perm, _ = pkg.bipartite_match_host(m, res["max_segment_size"], red["lb"], red["rb"], res["a"], res["d"])
    return perm


def run_device(pkg, msa, res, tuning=(), L=20):
    m, n = msa.shape
    ctx = pkg.SegmentationContext(m, n, L)
    for name, value in tuning:
        ctx.set_tuning(name, value)
    ctx.set_sequences(np.ascontiguousarray(msa))
    r = ctx.run()
    assert r.max_segment_size == res["max_segment_size"]
    red = ctx.reduced_traceback()
    for f in ("lb", "rb", "segment_size"):
        assert np.array_equal(red[f], res["reduced"][f]), f
    return ctx


def join(pkg, msa, res, tuning, path, want):
    ctx = run_device(pkg, msa, res, tuning)
    got = ctx.join_bipartite()
    assert ctx.bipartite_path() == path
    assert got.shape == want.shape and np.array_equal(got, want), np.argwhere(got != want)[:5].tolist()
    return ctx, got


def check_wide(pkg, msa, res, slabs=None):
    """The forced wide form gives the reference through path 2, a second context with FSEQ_JOIN_HOST the same through
    path 0.  Returns (the wide context, the permutations)."""
    want = reference(pkg, msa.shape[0], res)
    tuning = [("FSEQ_JOIN_BIP_WIDE", "1")] + ([("FSEQ_JOIN_BIP_SLABS", str(slabs))] if slabs else [])
    ctx, got = join(pkg, msa, res, tuning, WIDE, want)
    join(pkg, msa, res, [("FSEQ_JOIN_HOST", "1")], HOST, want)
    return ctx, got


@pytest.mark.parametrize("X,m,n", [(2, 200, 3300), (64, 200, 3300), (181, 400, 8000)])
def test_forced_wide_on_the_lds_forms_ground(pkg, X, m, n):
    """Forced wide where the LDS form runs by itself, and the results of the same input with no tuning (path 1)."""
    msa, res = mosaic_segmentation(X, m, n, None)
    _, got = check_wide(pkg, msa, res)
    join(pkg, msa, res, [], LDS, got)


@pytest.mark.parametrize("X,m,n", [(182, 400, 8000), (301, 400, 4000)])
def test_the_border(pkg, X, m, n):
    """The first X the LDS form does not take, and one with more columns than the workgroup has threads."""
    msa, res = mosaic_segmentation(X, m, n, None)
    check_wide(pkg, msa, res)


@pytest.mark.parametrize("X,m,n", [(600, 1200, 3300), (1157, 2400, 3300)])
def test_more_columns_than_threads_and_unequal_text_counts(pkg, X, m, n):
    """X = 1,157 is BASELINE C4's slot count: five columns a thread.  The mosaic's blocks use subsets of the founders, so
    the sorted texts, the placeholders and the full case all occur, and adjacent segments have different counts."""
    msa, res = mosaic_segmentation(X, m, n, None)
    sz = res["reduced"]["segment_size"]
    assert (sz < X).any() and (sz == X).any() and (sz[:-1] != sz[1:]).any()
    _, got = check_wide(pkg, msa, res)
    if X == 600:
        # scipy's optimum and the copy multisets, on three sampled pairs
        S = len(res["reduced"])
        assert np.array_equal(got, check_bipartite_host(pkg, m, X, res, pairs=(1, S // 2, S - 1)))


def test_ties(pkg):
    """Every class of a segment equally large: only the scan order separates the optimal matchings."""
    msa, res = mosaic_segmentation(300, 600, 3300, 2)
    check_wide(pkg, msa, res)


@pytest.mark.parametrize("S,slabs", [(1, None), (2, None), (65, None), (65, 3)])
def test_no_pair_one_pair_many(pkg, S, slabs):
    """One segment: no solver launch.  65 segments on three slabs: a workgroup solves more than 20 pairs on one slab."""
    msa, res = mosaic_segments(300, 600, S)
    assert len(res["reduced"]) == S
    check_wide(pkg, msa, res, slabs)


@functools.lru_cache(maxsize=None)
def rows_sorted_by_first_block():
    """The 70,000-row mosaic with its rows in the order of their first block: the classes of the first segment are runs of
    consecutive rows, so the last ones have no row below 2^16 (the segmentation does not depend on the rows' order)."""
    msa, res = mosaic_segmentation(300, 70000, 2000, None, seed=5)
    srt = np.ascontiguousarray(msa[np.lexsort(msa[:, :100].T[::-1])])
    out = fso.segment_long(srt, 20)
    assert out["status"] == 0 and out["max_segment_size"] == 300
    assert np.array_equal(out["reduced"]["lb"], res["reduced"]["lb"])
    return srt, out


@pytest.mark.parametrize("sort_rows", [False, True])
def test_row_ids_above_16_bits_on_streamed_boundary_states(pkg, sort_rows):
    """m = 70,000 (no multiple of 64 or 256): the boundary states come from the streamed pass 2 and the class tables see row
    ids above 16 bits.  A permutation entry of this joiner is the *smallest* row of a class (the text's first_sequence_index),
    and the mosaic spreads every class over all rows: the host joiner's own largest entry on it is 2,674.  With the rows sorted
    by their first block the smallest rows of the first segment's last classes are above 2^16 (largest entry 69,752)."""
    msa, res = rows_sorted_by_first_block() if sort_rows else mosaic_segmentation(300, 70000, 2000, None, seed=5)
    assert len(res["reduced"]) > 10 and msa.shape[0] - 1 > 0xFFFF
    _, got = check_wide(pkg, msa, res)
    if sort_rows:
        assert got.max() > 0xFFFF


def test_by_itself_below_the_threshold(pkg):
    """128 KB of boundary states above the LDS limit: no tuning, the host joiner."""
    msa, res = mosaic_segmentation(301, 400, 4000, None)
    join(pkg, msa, res, [], HOST, reference(pkg, 400, res))


def test_join_host_wins(pkg):
    msa, res = mosaic_segmentation(301, 400, 4000, None)
    join(pkg, msa, res, [("FSEQ_JOIN_BIP_WIDE", "1"), ("FSEQ_JOIN_HOST", "1")], HOST, reference(pkg, 400, res))


def test_bipartite_path_before_a_join_and_after_a_new_input(pkg):
    msa, res = mosaic_segmentation(64, 200, 3300, None)
    ctx = run_device(pkg, msa, res, [("FSEQ_JOIN_BIP_WIDE", "1")])
    with pytest.raises(pkg.FseqError) as err:
        ctx.bipartite_path()
    assert err.value.code == pkg.FSEQ_E_ARG
    ctx.join_bipartite()
    assert ctx.bipartite_path() == WIDE
    ctx.set_sequences(np.ascontiguousarray(msa))
    with pytest.raises(pkg.FseqError) as err:
        ctx.bipartite_path()
    assert err.value.code == pkg.FSEQ_E_ARG
    ctx.run()
    ctx.join_bipartite()
    assert ctx.bipartite_path() == WIDE


def test_the_cli_in_child_processes(tmp_path):
    """founder_sequences --segment-joining=bipartite-matching with FSEQ_JOIN_BIP_WIDE and with FSEQ_JOIN_HOST in the
    environment: the same founders and the same segments file, byte for byte."""
    cli = importlib.import_module("founder-sequences_amd.build").build_cli()
    msa, res = mosaic_segmentation(301, 400, 4000, None)
    fa = tmp_path / "in.fa"
    with open(fa, "wb") as f:
        for i in range(msa.shape[0]):
            f.write(b">s%d\n" % i + bytes(msa[i]) + b"\n")
    out = {}
    for knob in ("FSEQ_JOIN_BIP_WIDE", "FSEQ_JOIN_HOST"):
        env = {k: v for k, v in os.environ.items() if not k.startswith("FSEQ_JOIN")}
        env[knob] = "1"
        env["FSEQ_DEBUG"] = "1"                                # (the wide form names itself on stderr)
        founders, segments = tmp_path / (knob + ".founders"), tmp_path / (knob + ".segments")
        r = subprocess.run([cli, "-i", str(fa), "-f", "FASTA", "-s", "20", "--segment-joining=bipartite-matching",
                            "--output-founders", str(founders), "--output-segments", str(segments)], capture_output=True, timeout=300, env=env)
        assert r.returncode == 0, r.stderr
        assert (b"bipartite join, wide form" in r.stderr) == (knob == "FSEQ_JOIN_BIP_WIDE")
        out[knob] = (founders.read_bytes(), segments.read_bytes())
    lines = out["FSEQ_JOIN_HOST"][0].split(b"\n")
    assert len(lines) - 1 == 301 and all(len(x) == 4000 for x in lines[:-1])
    assert out["FSEQ_JOIN_BIP_WIDE"][0] == out["FSEQ_JOIN_HOST"][0]
    assert out["FSEQ_JOIN_BIP_WIDE"][1] == out["FSEQ_JOIN_HOST"][1]
