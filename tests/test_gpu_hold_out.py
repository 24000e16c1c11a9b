"""Rows held out of a resident alignment on the device (fseq_create_without_rows, fseq_match_held_out): the split kernel against
the numpy statement of tests/hold_out_model.py byte for byte, the sub-context against a fresh upload of the kept rows, the match
against fseq_match_rows on the held-out rows' raw bytes and against tests/match_split_model.py, refusals and lifetime, and the
front end against a run on the shorter list file."""
import importlib
import os
import subprocess

import numpy as np
import pytest

import hold_out_model as hm
import match_model as mm
import match_split_model as sm
from helpers import founder_mosaic
from test_gpu_identity import borrowed_packed, results_of
from test_gpu_match_rows import assert_equals_models

pytestmark = pytest.mark.gpu

BITS = hm.BITS
STAGE_CHUNKS = 512                                                # RS_STAGE_CHUNKS of csrc/fseq_rowsplit_plan.hpp: 16-byte chunks of source a workgroup stages
STRIP_BYTES = 16 * STAGE_CHUNKS                                   # a column of more bytes is taken in strips: 32,768 rows at 2 bits, 8,192 at 8
SIGMAS = [2, 4, 16, 40]
ROWS = [2, 3, 4, 5, 15, 16, 17, 63, 64, 65, 255, 256, 257, 4095, 4096, 4097, 16385]
COLUMNS = [1, 2, 63, 64, 65, 1003]


def tile_columns(m, bits, n_kept):
    """columns a workgroup of k_rows_split takes at a time where the column is one strip (row_split_strips)"""
    src_chunks = ((m * bits + 7) // 8 + 15) // 16
    out_chunks = ((n_kept * bits + 7) // 8 + 15) // 16
    return max(1, min(STAGE_CHUNKS // (src_chunks + 1), STAGE_CHUNKS // out_chunks))


TILE_M, TILE_SIGMA = 255, 4                                       # 64 bytes a column: 4 chunks, tiles of 102 columns with one row held out
TILE = tile_columns(TILE_M, 2, TILE_M - 1)
# (m, sigma, n): every m, every sigma and every n once at least; the strip-mined rows at 2 and at 8 bits with few columns
CASES = [(m, SIGMAS[i % 4], COLUMNS[i % 6]) for i, m in enumerate(ROWS)]
CASES += [(TILE_M, TILE_SIGMA, TILE - 1), (TILE_M, TILE_SIGMA, TILE), (TILE_M, TILE_SIGMA, TILE + 1)]
CASES += [(4 * STRIP_BYTES + 1, 4, 5), (STRIP_BYTES + 1, 40, 3), (3 * STRIP_BYTES + 77, 40, 2)]


@pytest.fixture(scope="module")
def pkg():
    return importlib.import_module("founder-sequences_amd")


@pytest.fixture(scope="module")
def build():
    return importlib.import_module("founder-sequences_amd.build")


def codes_for(m, sigma, n, seed):
    """codes < sigma in which every code occurs where the cells allow: the upload then packs at BITS[sigma]"""
    codes = np.random.default_rng(seed).integers(0, sigma, size=(m, n), dtype=np.uint8)
    flat = codes.reshape(-1)
    flat[:min(sigma, flat.size)] = np.arange(min(sigma, flat.size))
    return codes


def all_patterns(m, bits, seed):
    out = dict(hm.patterns(m, bits))
    out.update(hm.random_patterns(m, seed))
    if m > STRIP_BYTES:                                           # strips: a run longer than a stage of source between two kept rows
        out["run_stage"] = np.arange(5, min(m - 2, 5 + STRIP_BYTES * (8 // bits) + 40), dtype=np.uint32)
    return {k: v for k, v in out.items() if 1 <= len(v) < m}


def check_split(pkg, src, codes, bits, tag):
    m, n = codes.shape
    for name, held in all_patterns(m, bits, m).items():
        sub = src.without_rows(held, 5)
        want_k, want_h = hm.split(codes, held, bits)
        got_k, bits_k = sub.packed_columns()
        got_h, bits_h = sub.held_out_columns()
        assert bits_k == bits_h == bits and sub.m == m - len(held) and sub.n == n and sub.source_m == m
        assert sub.held_out_summary["held"] == len(held) and sub.held_out_summary["kept"] == sub.m
        assert got_k.shape == want_k.shape and np.array_equal(got_k, want_k), (tag, name, "kept")
        assert got_h.shape == want_h.shape and np.array_equal(got_h, want_h), (tag, name, "held")
        kept, back = sub.held_out()
        assert np.array_equal(kept, hm.kept_rows(m, held)) and np.array_equal(back, held)
        sub.close()


def test_the_cases_cover_what_they_claim():
    assert {m for m, _, _ in CASES} >= set(ROWS) and {s for _, s, _ in CASES} == set(SIGMAS)
    assert {n for _, _, n in CASES} >= set(COLUMNS) | {TILE - 1, TILE, TILE + 1} and TILE == 102
    assert all(m * n <= 40_000_000 for m, _, n in CASES)
    strips = [(m, BITS[s]) for m, s, n in CASES if (m * BITS[s] + 7) // 8 > STRIP_BYTES]
    assert {b for _, b in strips} == {2, 8} and all(n <= 5 for m, s, n in CASES if (m * BITS[s] + 7) // 8 > STRIP_BYTES)
    assert (STRIP_BYTES + 1, 8) in strips and (4 * STRIP_BYTES + 1, 2) in strips


@pytest.mark.parametrize("m,sigma,n", CASES, ids=lambda v: str(v))
def test_split_differential(pkg, m, sigma, n):
    """packed_columns() of the new context and held_out_columns() equal the model byte for byte, padding included, at every held
    pattern that exists at this m."""
    codes = codes_for(m, sigma, n, m + n)
    bits = BITS[sigma] if m * n >= sigma else None
    src = pkg.SegmentationContext(m, n, 5)
    src.set_sequences((48 + codes).astype(np.uint8))
    _, src_bits = src.packed_columns(0, 0)
    assert bits in (None, src_bits)
    if bits is None:                                              # (fewer cells than symbols: the codes are the ranks of what is there)
        _, codes = np.unique(codes, return_inverse=True)
        codes = codes.reshape(m, n).astype(np.uint8)
    check_split(pkg, src, codes, src_bits, "uploaded")
    src.close()


@pytest.mark.parametrize("m,sigma,n", [(17, 2, 65), (255, 16, 64), (4097, 40, 3), (STRIP_BYTES + 1, 40, 3), (4 * STRIP_BYTES + 1, 4, 2)], ids=lambda v: str(v))
def test_split_of_a_borrowed_source_with_garbage_in_its_padding(pkg, m, sigma, n):
    """A borrowed packed source with ld 48 bytes larger and 0xFF in every padding byte and padding field: none of it reaches an
    output field or the outputs' own padding."""
    codes = codes_for(m, sigma, n, 3 * m)
    src = borrowed_packed(pkg, codes, sigma, pad=48, garbage=True)
    check_split(pkg, src, codes, BITS[sigma], "borrowed")
    src.close()


@pytest.mark.parametrize("m,sigma,n", [(65, 4, 1003), (4096, 16, 64)], ids=lambda v: str(v))
def test_split_of_a_streamed_source(pkg, m, sigma, n):
    codes = codes_for(m, sigma, n, 5 * m)
    src = pkg.SegmentationContext(m, n, 5)
    src.set_sequences((48 + codes).astype(np.uint8), staging_bytes=2 * 16 * m + 4096)
    check_split(pkg, src, codes, BITS[sigma], "streamed")
    src.close()


# ---- the sub-context is an ordinary one

def mosaic_with_held(seed, m, n, n_held):
    """A founder mosaic over ACGT with a fifth symbol that occurs in held-out rows only: five codes at 4 bits in the sub-context,
    four at 2 bits in a fresh upload of the kept rows."""
    msa = founder_mosaic(6, m, n, brec=250, seed=seed)
    rng = np.random.default_rng(seed)
    held = rng.permutation(m)[:n_held].astype(np.uint32)
    for r in held[::2]:
        msa[r, rng.integers(0, n, size=5)] = ord("N")
    return np.ascontiguousarray(msa), held


def files_of(ctx, res, tmp_path, tag):
    f, e = str(tmp_path / ("F_" + tag)), str(tmp_path / ("E_" + tag))
    ctx.write_founders_device(res["bipartite"], f)
    ctx.write_segments_device(1, e)
    return open(f, "rb").read(), open(e, "rb").read()


@pytest.mark.parametrize("list_memory", [0, 1 << 20])
def test_same_results_as_a_fresh_upload(pkg, tmp_path, list_memory):
    m, n, L = 60, 3000, 20
    msa, held = mosaic_with_held(7, m, n, 9)
    kept = hm.kept_rows(m, held)
    assert ord("N") in msa[held] and ord("N") not in msa[kept]
    src = pkg.SegmentationContext(m, n, L)
    src.set_sequences(msa)
    sub = src.without_rows(held, L, list_memory=list_memory)
    src.close()                                                   # the source goes at once: run, join and match without it
    fresh = pkg.SegmentationContext(len(kept), n, L, list_memory=list_memory)
    fresh.set_sequences(msa[kept])
    assert sub.packed_columns()[1] == 4 and fresh.packed_columns()[1] == 2
    assert np.array_equal(sub.get_sequences(), msa[kept])
    for length in (L, 35):
        if length != L:
            sub.set_segment_length(length)
            fresh.set_segment_length(length)
        a, b = results_of(sub), results_of(fresh)
        assert a["max"] == b["max"] < len(kept)
        for f in ("traceback", "segments", "greedy", "bipartite", "random"):
            assert np.array_equal(a[f], b[f]), (f, length)
        for (a1, d1), (a2, d2) in zip(a["states"], b["states"]):
            assert np.array_equal(a1, a2) and np.array_equal(d1, d2)
        assert files_of(sub, a, tmp_path, "sub") == files_of(fresh, b, tmp_path, "fresh")
    now, peak = sub.device_bytes()
    ld_k, ld_h = sub.packed_columns(0, 0)[0].shape[1], sub.held_out_columns(0, 0)[0].shape[1]
    assert (ld_k, ld_h) == (32, 16) and now >= (ld_k + ld_h) * n + 32 and peak >= now
    fresh.close()
    sub.close()


# ---- the match

def founders_of(ctx, perm, rows):
    """the founders file's rows for these permutations"""
    segments = ctx.reduced_traceback()
    founders = np.full((perm.shape[1], rows.shape[1]), ord("-"), dtype=np.uint8)
    for s, seg in enumerate(segments):
        ok = perm[s] < len(rows)
        founders[ok, int(seg["lb"]):int(seg["rb"])] = rows[perm[s][ok], int(seg["lb"]):int(seg["rb"])]
    return founders


def match_result(ctx, summary, tmp_path, tag):
    pieces, sets = ctx.match_pieces()
    path = str(tmp_path / ("match_" + tag))
    ctx.write_match(path)
    return {k: v for k, v in summary.items() if k != "ms_device"}, pieces, sets, open(path, "rb").read()


@pytest.mark.parametrize("n_held", [1, 255, 256, 257])
def test_match_held_out_is_match_rows_on_the_raw_bytes(pkg, tmp_path, n_held):
    """By permutations and by K founder rows, min_segment_length 0 and 7: summary, pieces, founder sets and the report of
    match_rows(msa[held]) on the same context.  The held list is in a shuffled order, and `row` follows it."""
    m, n, L = n_held + 40, 2000, 20
    msa, held = mosaic_with_held(n_held, m, n, n_held)
    kept = hm.kept_rows(m, held)
    assert n_held < 3 or not np.array_equal(held, np.sort(held))
    src = pkg.SegmentationContext(m, n, L)
    src.set_sequences(msa)
    sub = src.without_rows(held, L)
    src.close()
    sub.run()
    perm = sub.join_greedy()
    founders = founders_of(sub, perm, msa[kept])
    for min_len in (0, 7):
        for how in ("permutations", "rows"):
            kw = {"permutations": perm} if how == "permutations" else {"founders": founders}
            want = match_result(sub, sub.match_rows(msa[held], min_segment_length=min_len, **kw), tmp_path, "rows")
            got = match_result(sub, sub.match_held_out(min_segment_length=min_len, **kw), tmp_path, "held")
            assert got[0] == want[0], (min_len, how)
            assert np.array_equal(got[1], want[1]) and np.array_equal(got[2], want[2]) and got[3] == want[3]
            assert len(np.unique(got[1]["row"])) == n_held        # (every held-out row has a piece: `row` indexes the list)
    sub.close()


@pytest.mark.parametrize("case", ["mosaic", "planted", "periodic"])
def test_match_held_out_under_a_forced_split_is_the_model(pkg, tmp_path, case):
    """FSEQ_MATCH_SPLIT / FSEQ_MATCH_OVERLAP forced on the sub-context: the pieces and what match_split() reports are those of
    tests/match_split_model.py -- a shape where every row stands (the model's mosaic of five founders) and two where the group falls
    back and is walked again unsplit (planted_case, whose rows follow one founder over all columns, and periodic_case)."""
    n, G, overlap = 4099, 7, 300
    if case == "mosaic":
        n, G, overlap = 4000, 5, 700
        queries, founders = mm.mosaic_case(101, 70, n, 5, 4)
    elif case == "planted":
        queries, founders = sm.planted_case(n, G, overlap, sigma=4, K=6, seed=5)
    else:
        queries, founders = sm.periodic_case(40, n)
    symbols = np.unique(np.concatenate([queries.reshape(-1), founders.reshape(-1)]))
    symbols = symbols[symbols != 0x7E]                            # (the founders' foreign byte stays outside the alphabet)
    rng = np.random.default_rng(9)
    others = symbols[rng.integers(0, len(symbols), size=(5, n))]
    others[0, :len(symbols)] = symbols
    order = rng.permutation(len(queries) + 5)
    msa = np.ascontiguousarray(np.vstack([others, queries])[np.argsort(order)])      # source row order[i] is row i of the stack
    held = order[5:].astype(np.uint32)
    assert np.array_equal(msa[held], queries)
    src = pkg.SegmentationContext(len(msa), n, 50)
    src.set_sequences(msa)
    sub = src.without_rows(held, 50)
    src.close()
    with pytest.raises(pkg.FseqError):                            # nothing matched yet
        sub.match_split()
    sub.set_tuning("FSEQ_MATCH_SPLIT", G)
    sub.set_tuning("FSEQ_MATCH_OVERLAP", overlap)
    for min_len in (0, 7):
        want = sm.split_match(queries, founders, min_len, G, overlap)
        if case == "mosaic":
            assert want["stands"].all() and want["split"]["flagged_groups"] == 0
        else:
            assert not want["stands"].any() and want["split"]["flagged_groups"] == 1
        s = sub.match_held_out(founders=founders, min_segment_length=min_len)
        assert_equals_models(sub, s, want, len(founders), want["split"], tmp_path)
    sub.close()


# ---- refusals and lifetime

def test_three_folds_of_one_source(pkg):
    m, n, L = 45, 2000, 20
    msa = founder_mosaic(5, m, n, brec=200, seed=12)
    src = pkg.SegmentationContext(m, n, L)
    src.set_sequences(msa)
    for fold in range(3):
        held = np.arange(fold, m, 3, dtype=np.uint32)
        kept = hm.kept_rows(m, held)
        sub = src.without_rows(held, L)
        fresh = pkg.SegmentationContext(len(kept), n, L)
        fresh.set_sequences(msa[kept])
        a, b = results_of(sub), results_of(fresh)
        assert a["max"] == b["max"]
        for f in ("traceback", "segments", "greedy", "bipartite", "random"):
            assert np.array_equal(a[f], b[f]), (fold, f)
        s = sub.match_held_out(permutations=a["greedy"])
        assert s["n_founders"] == a["max"] and len(np.unique(sub.match_pieces()[0]["row"])) == len(held)
        sub.close()
        fresh.close()
    assert src.run().max_segment_size >= 5                        # the source is as it was
    src.close()


def test_refusals(pkg):
    import ctypes as C
    m, n, L = 30, 1500, 20
    msa = founder_mosaic(4, m, n, brec=150, seed=2)
    src = pkg.SegmentationContext(m, n, L)
    with pytest.raises(pkg.FseqError) as e:                       # no alignment resident
        src.without_rows([1], L)
    assert e.value.code == pkg.FSEQ_E_ARG
    src.set_sequences(msa)
    for bad in ([], list(range(m)), [3, 3], [m], [0, 0xFFFFFFFF]):
        with pytest.raises(pkg.FseqError) as e:
            src.without_rows(bad, L)
        assert e.value.code == pkg.FSEQ_E_ARG and "without rows" in str(e.value), bad
    h = C.c_void_p(1)
    held = (C.c_uint32 * 1)(1)
    for p in (pkg.Params(5, 0, L, 0, 0, 0, 0), pkg.Params(0, n + 1, L, 0, 0, 0, 0), pkg.Params(0, 0, 0, 0, 0, 0, 0), pkg.Params(0, 0, L, 0, 0, 0, 1 + src._device)):
        assert src.L.fseq_create_without_rows(src.h, held, 1, C.byref(p), C.byref(h), None) == pkg.FSEQ_E_ARG and h.value is None
    with pytest.raises(pkg.FseqError) as e:                       # a plain context holds nothing out
        src.match_held_out(founders=msa[:2])
    assert e.value.code == pkg.FSEQ_E_ARG
    with pytest.raises(pkg.FseqError):
        src.held_out()
    with pytest.raises(pkg.FseqError):
        src.held_out_columns()
    reduced = src.without_identity_columns(L)                     # an identity-reduced source is refused
    with pytest.raises(pkg.FseqError) as e:
        reduced.without_rows([1], L)
    assert e.value.code == pkg.FSEQ_E_UNSUPPORTED
    reduced.close()
    sub = src.without_rows([4, 2], L)
    with pytest.raises(pkg.FseqError) as e:                       # it takes no other input
        sub.set_sequences(msa[:m - 2])
    assert e.value.code == pkg.FSEQ_E_ARG
    with pytest.raises(pkg.FseqError) as e:                       # permutations need a run
        sub.match_held_out(permutations=np.zeros((1, 4), dtype=np.uint32))
    assert e.value.code == pkg.FSEQ_E_ARG
    # the other way round works: the sub-context as the source of without_identity_columns gives a plain context over its rows
    kept = hm.kept_rows(m, [4, 2])
    plain = sub.without_identity_columns(L)
    mask, _ = sub.identity_columns()
    assert np.array_equal(plain.get_sequences(), msa[kept][:, ~mask])
    with pytest.raises(pkg.FseqError) as e:
        plain.match_held_out(founders=msa[:2, :plain.n])
    assert e.value.code == pkg.FSEQ_E_ARG
    plain.close()
    sub.close()
    src.close()


def test_a_sharded_source_refuses(pkg):
    from test_gpu_shard import run_world
    m, n, L = 40, 6000, 20
    msa = founder_mosaic(6, m, n, brec=100, seed=4)
    for c in run_world(pkg, 2, lambda c: c.set_sequences(msa), m, n, L):
        with pytest.raises(pkg.FseqError) as e:
            c.without_rows([1, 2], L)
        assert e.value.code == pkg.FSEQ_E_UNSUPPORTED


# ---- the front end, in child processes

def test_front_end_against_a_run_on_the_shorter_list(build, tmp_path):
    """--hold-out=3,10:12 -o -e --output-held-out-matches: the founders and segments files of a run on the list file without those
    four lines, and the report of the in-tree match_founder_sequences on the written founders and the four sequences in that order."""
    cli = build.build_cli()
    tools = dict(zip(build.AUX_TOOLS, build.build_aux()))
    m, n, L = 20, 3000, 20
    msa = founder_mosaic(5, m, n, brec=200, seed=21)
    src = tmp_path / "in"
    src.mkdir()
    names = []
    for i, row in enumerate(msa):
        (src / ("s%02d" % i)).write_bytes(row.tobytes())
        names.append(str(src / ("s%02d" % i)))
    held = hm.parse_hold_out("3,10:12", m)
    (tmp_path / "all.txt").write_text("\n".join(names) + "\n")
    (tmp_path / "kept.txt").write_text("\n".join(nm for i, nm in enumerate(names) if i not in held) + "\n")
    (tmp_path / "held.txt").write_text("\n".join(names[i] for i in held) + "\n")
    common = ["--segment-length-bound", str(L), "--match-min-segment-length", "7"]
    r = subprocess.run([cli, "--input", str(tmp_path / "all.txt"), "--hold-out=3,10:12", "--output-founders=" + str(tmp_path / "F"), "--output-segments=" + str(tmp_path / "E"),
                        "--output-held-out-matches=" + str(tmp_path / "M")] + common, capture_output=True, timeout=120)
    assert r.returncode == 0 and b"Held 4 of 20 sequences out of the segmentation." in r.stderr, r.stderr
    r = subprocess.run([cli, "--input", str(tmp_path / "kept.txt"), "--output-founders=" + str(tmp_path / "F2"), "--output-segments=" + str(tmp_path / "E2")] + common,
                       capture_output=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert (tmp_path / "F").read_bytes() == (tmp_path / "F2").read_bytes() and (tmp_path / "E").read_bytes() == (tmp_path / "E2").read_bytes()
    assert len((tmp_path / "F").read_bytes().splitlines()) >= 2
    r = subprocess.run([tools["match_founder_sequences"], "--sequences", str(tmp_path / "held.txt"), "--founders", str(tmp_path / "F"), "--founders-format", "text",
                        "--min-segment-length", "7", "--single-threaded"], capture_output=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert (tmp_path / "M").read_bytes() == r.stdout and r.stdout.count(b"\n") > 4
