"""Query rows matched against the restored founders on the device (fseq_create_without_identity_columns_held,
fseq_match_held_out_restored, fseq_match_rows_restored, fseq_get_match_exceptions) against the definition:
match_model.match_rows(full-length queries, identity_model.restore(founders, mask, row 0), min_len).  Integer work: every
comparison is exact.  tests/test_match_exceptions_model.py proves the merged walk the kernel follows equal to the same definition
on the patterns planted here (tests/match_exceptions_model.py)."""
import importlib
import subprocess

import numpy as np
import pytest

import identity_model as im
import match_exceptions_model as xm
import match_model as mm
from helpers import founder_mosaic
from test_gpu_match import assert_equals_model, founders_of, tile_cols
from test_gpu_match_restored import doctored, report_of

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def pkg():
    return importlib.import_module("founder-sequences_amd")


@pytest.fixture(scope="module")
def build():
    return importlib.import_module("founder-sequences_amd.build")


MIN_LENS = [0, 1, 3, 50]
L = 5
FOREIGN = 0x7E
# name: alphabet of the reconstruction's rows, the symbol only query rows have (the source alignment's alphabet is both: its
# packing is `bits`), rows of the reconstruction, query rows, founders of the mosaic over the kept columns, set words of the
# live-set form (1, 2, 4, 8 register words; more: LDS).  130 kept columns: two tiles of the walk, three where the LDS form's tile
# is 51 columns.  Query rows 1 .. 257: part of a workgroup of the walk, one, and one row more.
CASES = {
    "b2-w1-q1":    dict(alphabet=b"ACG",   private=ord("N"), bits=2, m=37,  q=1,   X=6,   words=(1, 1)),
    "b2-w1-q255":  dict(alphabet=b"ACG",   private=ord("N"), bits=2, m=37,  q=255, X=6,   words=(1, 1)),
    "b4-w2-q256":  dict(alphabet=b"ACGT-", private=ord("N"), bits=4, m=100, q=256, X=40,  words=(2, 2)),
    "b2-w1-q257":  dict(alphabet=b"ACG",   private=ord("N"), bits=2, m=37,  q=257, X=6,   words=(1, 1)),
    "b8-w4-q64":   dict(alphabet=bytes(range(48, 88)), private=ord("Z"), bits=8, m=300, q=64, X=100, words=(3, 4)),
    "b2-w8-q65":   dict(alphabet=b"ACG",   private=ord("N"), bits=2, m=300, q=65,  X=200, words=(5, 8)),
    "b4-lds-q63":  dict(alphabet=b"ACGT-", private=ord("N"), bits=4, m=330, q=63,  X=280, words=(9, 64)),
}
N_KEPT = 130


def make_case(name):
    """-> dict(source [m + q, n_src], held: the query rows' indices in it, rows: the reconstruction's rows, queries, mask, where, tile)"""
    c = CASES[name]
    rng = np.random.default_rng(sum(name.encode()))
    alpha = np.frombuffer(c["alphabet"], dtype=np.uint8)
    tile = tile_cols(c["X"], len(alpha) + 1)
    mask = xm.layout(rng, N_KEPT, tile, draw=(0, 0, 1, 2, 7, 30, 60, 90))
    red = founder_mosaic(c["X"], c["m"], N_KEPT, brec=50, seed=c["m"] + c["X"], alphabet=c["alphabet"])
    for k in np.flatnonzero((red == red[0:1]).all(axis=0)):       # (a kept column is one in which the rows differ)
        red[1, k] = alpha[(int(np.flatnonzero(alpha == red[0, k])[0]) + 1) % len(alpha)]
    rows = np.empty((c["m"], len(mask)), dtype=np.uint8)
    rows[:, ~mask] = red
    rows[:, mask] = alpha[rng.integers(0, len(alpha), size=int(mask.sum()))][None, :]
    queries = rows[rng.integers(0, c["m"], size=c["q"])].copy()
    other = lambda b: alpha[(int(np.flatnonzero(alpha == b)[0]) + 1) % len(alpha)]
    where = xm.plant(rng, queries, rows[0], mask, tile, c["private"], other)
    m = c["m"] + c["q"]
    held = rng.permutation(m)[:c["q"]].astype(np.uint32)          # (in no order: row i of the queries is source row held[i])
    source = np.empty((m, len(mask)), dtype=np.uint8)
    source[held] = queries
    source[np.setdiff1d(np.arange(m), held)] = rows
    return dict(source=np.ascontiguousarray(source), held=held, rows=rows, queries=queries, mask=mask, where=where, tile=tile)


def test_the_cases_cover_what_they_claim():
    """(no GPU work) every pattern, the axes, the sizes"""
    assert {c["bits"] for c in CASES.values()} == {2, 4, 8} and {c["q"] for c in CASES.values()} == {1, 63, 64, 65, 255, 256, 257}
    assert [c["words"][1] for c in CASES.values()].count(1) >= 1 and {c["words"][1] for c in CASES.values()} == {1, 2, 4, 8, 64}
    tiles = set()
    for name, c in CASES.items():
        d = make_case(name)
        mask, n_src = d["mask"], len(d["mask"])
        assert 2000 <= n_src <= 6000 and d["source"].shape[0] <= 400, (name, n_src)
        assert np.array_equal(im.identity_mask(d["rows"]), mask) and int((~mask).sum()) == N_KEPT
        assert len(np.unique(d["source"])) == len(c["alphabet"]) + 1 and c["private"] not in d["rows"]
        listed = xm.PLACES if c["q"] < 3 else ("none", "every") + xm.PLACES
        xm.check_planted(d["queries"], d["rows"][0], mask, d["where"], listed, d["tile"])
        assert xm.largest_gap(mask) > 2 * max(MIN_LENS)
        tiles.add(d["tile"])
    assert tiles == {51, 64}


def exceptions_expected(queries, mask, row0):
    exc = xm.exceptions_of(queries, mask, row0)
    return np.r_[0, np.cumsum([len(e) for e in exc])].astype(np.uint64), np.concatenate(exc).astype(np.uint32)


def chain(pkg, d, seg_len):
    """source -> the rows held out -> the identity columns removed, the held-out rows carried along -> run and joined"""
    src = pkg.SegmentationContext(d["source"].shape[0], d["source"].shape[1], seg_len)
    src.set_sequences(d["source"])
    sub = src.without_rows(d["held"], seg_len)
    src.close()
    red = sub.without_identity_columns(seg_len, keep_held_out=True)
    sub.close()
    return red


@pytest.fixture(scope="module")
def runs(pkg):
    """name -> (case, the context after its run, {greedy, doctored: (permutations, full-length founders)}), made on first use
    and shared by the min_len cases"""
    made = {}

    def get(name):
        if name not in made:
            c, d = CASES[name], make_case(name)
            red = chain(pkg, d, L)
            assert red.n == N_KEPT and red.source_n == len(d["mask"]) and red.m == c["m"] and red.n_held == c["q"]
            res = red.run()
            segments = red.reduced_traceback()
            reduced = im.reduce_rows(d["rows"], d["mask"])
            perms = {"greedy": red.join_greedy()}
            perms["doctored"] = doctored(np.random.default_rng(c["m"] + c["q"]), perms["greedy"], c["m"])
            assert res.max_segment_size < c["m"]
            founders = {k: im.restore(founders_of(reduced, p, segments), d["mask"], d["rows"][0]) for k, p in perms.items()}
            made[name] = (d, red, {k: (perms[k], founders[k]) for k in perms})
        return made[name]

    yield get
    for _, red, _ in made.values():
        red.close()


def assert_exceptions(red, queries, mask, row0):
    off, cols = red.match_exceptions()
    want_off, want_cols = exceptions_expected(queries, mask, row0)
    assert np.array_equal(off, want_off) and np.array_equal(cols, want_cols)


@pytest.mark.parametrize("min_len", MIN_LENS)
@pytest.mark.parametrize("name", list(CASES))
def test_differential_against_the_model(pkg, runs, tmp_path, name, min_len):
    c = CASES[name]
    d, red, perms = runs(name)
    mask, queries, row0 = d["mask"], d["queries"], d["rows"][0]
    n_src = len(mask)
    # a byte outside the alphabet in an identity column and in a kept column of one row: host rows only
    with_foreign = queries.copy()
    kept = np.flatnonzero(~mask)
    r = c["q"] // 2
    with_foreign[r, kept[xm.A] - 1] = with_foreign[r, kept[20]] = FOREIGN
    assert mask[kept[xm.A] - 1]
    # the staged chunks of the host rows: 64 columns each (the patterns sit on both sides of column 64), or everything at once
    red.set_tuning("FSEQ_MATCH_STAGE_BYTES", "64" if min_len in (0, 3) else None)
    for how, (perm, founders) in perms.items():
        K = perm.shape[1]
        want = mm.match_rows(queries, founders, min_len)
        s = red.match_held_out_restored(perm, min_segment_length=min_len)
        print("%s %s min_len=%d: n_src=%d K=%d set_words=%d queries=%d exceptions=%d" % (name, how, min_len, n_src, K, s["set_words"], c["q"], len(red.match_exceptions()[1])))
        assert c["words"][0] <= s["set_words"] <= c["words"][1]
        assert_equals_model(pkg, red, s, want, K)
        assert_exceptions(red, queries, mask, row0)
        assert s["uncovered_cells"] >= sum(len(e) for e in xm.exceptions_of(queries, mask, row0))
        red.write_match(str(tmp_path / how))
        report = (tmp_path / how).read_bytes()
        if how == "doctored" or min_len != 1:                     # (min_len = 1: a piece a cell; one report of them is formatted here)
            assert report == report_of(want["pieces"], want["sets"])
        # the same rows' bytes from the host
        s2 = red.match_rows_restored(queries, perm, min_segment_length=min_len)
        assert_equals_model(pkg, red, s2, want, K)
        assert_exceptions(red, queries, mask, row0)
        red.write_match(str(tmp_path / (how + "_rows")))
        assert (tmp_path / (how + "_rows")).read_bytes() == report
        # ... and with the foreign bytes
        want_f = mm.match_rows(with_foreign, founders, min_len)
        s3 = red.match_rows_restored(with_foreign, perm, min_segment_length=min_len)
        assert_equals_model(pkg, red, s3, want_f, K)
        assert_exceptions(red, with_foreign, mask, row0)
        assert want_f["uncovered_cells"] >= want["uncovered_cells"] + 1
    red.set_tuning("FSEQ_MATCH_STAGE_BYTES", None)


def test_min_len_larger_than_every_gap(pkg):
    """a layout without a long gap: min_len = 50 closes no piece inside one"""
    rng = np.random.default_rng(7)
    alpha = np.frombuffer(b"ACG", dtype=np.uint8)
    mask = xm.layout(rng, N_KEPT, 64, first=3, long_gap=0, last=1, draw=(0, 1, 2, 7, 30, 45, 45, 45))
    assert xm.largest_gap(mask) < 50 and len(mask) >= 2000
    red_rows = founder_mosaic(6, 37, N_KEPT, brec=50, seed=3, alphabet=b"ACG")
    for k in np.flatnonzero((red_rows == red_rows[0:1]).all(axis=0)):
        red_rows[1, k] = alpha[(int(np.flatnonzero(alpha == red_rows[0, k])[0]) + 1) % 3]
    rows = np.empty((37, len(mask)), dtype=np.uint8)
    rows[:, ~mask] = red_rows
    rows[:, mask] = alpha[rng.integers(0, 3, size=int(mask.sum()))][None, :]
    queries = rows[rng.integers(0, 37, size=9)].copy()
    where = xm.plant(rng, queries, rows[0], mask, 64, ord("N"), lambda b: alpha[(int(np.flatnonzero(alpha == b)[0]) + 1) % 3])
    xm.check_planted(queries, rows[0], mask, where, ("none", "every", "ends", "run", "around_kept", "uncovered_then_exc", "tile_border"), 64)
    d = dict(source=np.ascontiguousarray(np.vstack([rows, queries])), held=np.arange(37, 46, dtype=np.uint32))
    red = chain(pkg, d, L)
    red.run()
    perm = red.join_greedy()
    founders = im.restore(founders_of(red_rows, perm, red.reduced_traceback()), mask, rows[0])
    for min_len in (0, 50):
        want = mm.match_rows(queries, founders, min_len)
        s = red.match_held_out_restored(perm, min_segment_length=min_len)
        assert_equals_model(pkg, red, s, want, perm.shape[1])
        s = red.match_rows_restored(queries, perm, min_segment_length=min_len)
        assert_equals_model(pkg, red, s, want, perm.shape[1])
    red.close()
    # the reconstruction's rows alone: three codes, so the host rows pack at 2 bits and the queries' 'N' is a byte outside the alphabet
    src = pkg.SegmentationContext(37, len(mask), L)
    src.set_sequences(rows)
    plain = src.without_identity_columns(L)
    src.close()
    plain.run()
    p2 = plain.join_greedy()
    assert np.array_equal(p2, perm)
    for min_len in (0, 3):
        s = plain.match_rows_restored(queries, p2, min_segment_length=min_len)
        assert_equals_model(pkg, plain, s, mm.match_rows(queries, founders, min_len), p2.shape[1])
        assert_exceptions(plain, queries, mask, rows[0])
    plain.close()


def test_keeping_the_held_out_rows_changes_nothing_else(pkg, tmp_path):
    """keep_held_out=True: the alignment, the mask, the kept columns, the segments, the boundary states and the restored founders
    file of the plain call, byte for byte; match_held_out on it is the match in reduced co-ordinates."""
    d = make_case("b4-w2-q256")
    src = pkg.SegmentationContext(d["source"].shape[0], d["source"].shape[1], L)
    src.set_sequences(d["source"])
    sub = src.without_rows(d["held"], L)
    src.close()
    plain = sub.without_identity_columns(L)
    both = sub.without_identity_columns(L, keep_held_out=True)
    with pytest.raises(pkg.FseqError) as e:                       # the plain one has forgotten the held-out rows
        plain.held_out()
    assert e.value.code == pkg.FSEQ_E_ARG
    kept_rows, held = both.held_out()
    want_kept, want_held = sub.held_out()
    assert np.array_equal(kept_rows, want_kept) and np.array_equal(held, want_held) and np.array_equal(held, d["held"])
    sub.close()
    got = {}
    for tag, ctx in (("plain", plain), ("both", both)):
        cols, bits = ctx.packed_columns()
        res = ctx.run()
        segments = ctx.reduced_traceback()
        perm = ctx.join_greedy()
        ctx.write_founders_restored(perm, str(tmp_path / tag))
        got[tag] = dict(cols=cols, bits=bits, mask=ctx.identity_mask(), kept=ctx.kept_columns(), max=res.max_segment_size, traceback=ctx.traceback(),
                        segments=segments, states=[ctx.boundary_state(i) for i in range(len(segments))], perm=perm, file=(tmp_path / tag).read_bytes())
    a, b = got["plain"], got["both"]
    assert a["bits"] == b["bits"] and a["max"] == b["max"] and a["file"] == b["file"]
    for f in ("cols", "mask", "kept", "traceback", "segments", "perm"):
        assert np.array_equal(a[f], b[f]), f
    assert np.array_equal(a["mask"], d["mask"])
    for (a0, d0), (a1, d1) in zip(a["states"], b["states"]):
        assert np.array_equal(a0, a1) and np.array_equal(d0, d1)
    # the reduced match: the held-out rows' kept columns against the reduced founders, as match_rows has it on a plain context
    # over the reduced rows (on `plain` itself match_rows is refused: its columns are the kept ones of a longer source)
    reduced, perm = im.reduce_rows(d["rows"], d["mask"]), b["perm"]
    reduced_founders = founders_of(reduced, perm, b["segments"])
    reduced_queries = np.ascontiguousarray(d["queries"][:, ~d["mask"]])
    fresh = pkg.SegmentationContext(reduced.shape[0], reduced.shape[1], L)
    fresh.set_sequences(reduced)
    for min_len in (0, 3):
        s = both.match_held_out(permutations=perm, min_segment_length=min_len)
        pieces, sets = both.match_pieces()
        want = mm.match_rows(reduced_queries, reduced_founders, min_len)
        assert_equals_model(pkg, both, s, want, perm.shape[1])
        fresh.match_rows(reduced_queries, founders=reduced_founders, min_segment_length=min_len)
        pieces2, sets2 = fresh.match_pieces()
        assert np.array_equal(pieces, pieces2) and np.array_equal(sets, sets2)
        with pytest.raises(pkg.FseqError) as e:                   # not a restored match of query rows
            both.match_exceptions()
        assert e.value.code == pkg.FSEQ_E_ARG
    fresh.close()
    plain.close()
    both.close()


def test_after_set_segment_length_the_match_is_that_of_a_fresh_chain(pkg):
    d = make_case("b2-w1-q255")
    red = chain(pkg, d, L)
    red.run()
    red.match_held_out_restored(red.join_greedy())
    red.set_segment_length(9)
    with pytest.raises(pkg.FseqError) as e:                       # the result and the last match went with the length
        red.match_held_out_restored(np.zeros((1, 2), dtype=np.uint32))
    assert e.value.code == pkg.FSEQ_E_ARG
    fresh = chain(pkg, d, 9)
    out = []
    for ctx in (red, fresh):
        ctx.run()
        perm = ctx.join_greedy()
        s = ctx.match_held_out_restored(perm, min_segment_length=3)
        out.append((perm, s, ctx.match_pieces(), ctx.match_exceptions(), ctx.reduced_traceback()))
    (p0, s0, m0, x0, t0), (p1, s1, m1, x1, t1) = out
    assert np.array_equal(p0, p1) and np.array_equal(t0, t1)
    assert np.array_equal(m0[0], m1[0]) and np.array_equal(m0[1], m1[1]) and np.array_equal(x0[0], x1[0]) and np.array_equal(x0[1], x1[1])
    assert {k: v for k, v in s0.items() if k != "ms_device"} == {k: v for k, v in s1.items() if k != "ms_device"}
    founders = im.restore(founders_of(im.reduce_rows(d["rows"], d["mask"]), p0, t0), d["mask"], d["rows"][0])
    assert_equals_model(pkg, red, s0, mm.match_rows(d["queries"], founders, 3), p0.shape[1])
    red.close()
    fresh.close()


def test_refusals_leave_the_last_match_readable(pkg):
    d = make_case("b2-w1-q257")
    src = pkg.SegmentationContext(d["source"].shape[0], d["source"].shape[1], L)
    src.set_sequences(d["source"])
    sub = src.without_rows(d["held"], L)
    with pytest.raises(pkg.FseqError) as e:                       # the source of the held call is a context made by without_rows
        src.without_identity_columns(L, keep_held_out=True)
    assert e.value.code == pkg.FSEQ_E_ARG and "fseq_create_without_rows" in str(e.value)
    src.close()
    red = sub.without_identity_columns(L, keep_held_out=True)
    plain = sub.without_identity_columns(L)
    sub.close()
    with pytest.raises(pkg.FseqError) as e:                       # nested: a context that carries held-out rows already is no source either
        red.without_identity_columns(L, keep_held_out=True)
    assert e.value.code == pkg.FSEQ_E_ARG
    reduced = im.reduce_rows(d["rows"], d["mask"])
    first = red.match_founders(founders=reduced[:2])              # (needs the alignment only)
    for call in (lambda: red.match_held_out_restored(np.zeros((1, 2), dtype=np.uint32)),          # before a run
                 lambda: red.match_rows_restored(d["queries"], np.zeros((1, 2), dtype=np.uint32))):
        with pytest.raises(pkg.FseqError) as e:
            call()
        assert e.value.code == pkg.FSEQ_E_ARG
        assert len(red.match_pieces()[0]) == first["pieces"]
    red.run()
    perm = red.join_greedy()
    good = red.match_held_out_restored(perm)
    kept_pieces, kept_exc = red.match_pieces(), red.match_exceptions()
    lib = pkg.load_library()
    ms = pkg.MatchSummary()
    import ctypes as C
    null_row = (C.c_void_p * 1)(None)
    one_row = (C.c_void_p * 1)(d["queries"].ctypes.data)
    for rc in (lib.fseq_match_rows_restored(red.h, perm.ctypes.data, None, 1, 0, C.byref(ms)),
               lib.fseq_match_rows_restored(red.h, perm.ctypes.data, one_row, 0, 0, C.byref(ms)),
               lib.fseq_match_rows_restored(red.h, perm.ctypes.data, null_row, 1, 0, C.byref(ms)),
               lib.fseq_match_rows_restored(red.h, None, one_row, 1, 0, C.byref(ms)),
               lib.fseq_match_held_out_restored(red.h, None, 0, C.byref(ms)),
               lib.fseq_match_held_out_restored(red.h, perm.ctypes.data, 0, None)):
        assert rc == pkg.FSEQ_E_ARG
        again, exc = red.match_pieces(), red.match_exceptions()
        assert np.array_equal(again[0], kept_pieces[0]) and np.array_equal(again[1], kept_pieces[1])
        assert np.array_equal(exc[0], kept_exc[0]) and np.array_equal(exc[1], kept_exc[1])
    assert len(kept_pieces[0]) == good["pieces"]
    # a context of the wrong kind: the plain reduced one has no held-out rows, but takes rows from the host
    plain.run()
    p2 = plain.join_greedy()
    before = plain.match_founders_restored(p2)
    with pytest.raises(pkg.FseqError) as e:
        plain.match_held_out_restored(p2)
    assert e.value.code == pkg.FSEQ_E_ARG and "fseq_create_without_identity_columns_held" in str(e.value)
    assert len(plain.match_pieces()[0]) == before["pieces"]
    with pytest.raises(pkg.FseqError) as e:
        plain.match_exceptions()
    assert e.value.code == pkg.FSEQ_E_ARG
    s = plain.match_rows_restored(d["queries"], p2)
    assert np.array_equal(p2, perm)
    assert {k: v for k, v in s.items() if k != "ms_device"} == {k: v for k, v in good.items() if k != "ms_device"}
    again = plain.match_pieces()
    assert np.array_equal(again[0], kept_pieces[0]) and np.array_equal(again[1], kept_pieces[1])
    assert_exceptions(plain, d["queries"], d["mask"], d["rows"][0])
    # ... and a context that is not reduced at all takes neither
    ctx = pkg.SegmentationContext(d["rows"].shape[0], d["rows"].shape[1], L)
    ctx.set_sequences(d["rows"])
    ctx.run()
    p3 = ctx.join_greedy()
    kept3 = ctx.match_founders(p3)
    for call in (lambda: ctx.match_held_out_restored(p3), lambda: ctx.match_rows_restored(d["queries"][:, :ctx.n], p3)):
        with pytest.raises((pkg.FseqError, ValueError)) as e:
            call()
        assert isinstance(e.value, ValueError) or e.value.code == pkg.FSEQ_E_ARG
        assert len(ctx.match_pieces()[0]) == kept3["pieces"]
    ctx.close()
    plain.close()
    red.close()


@pytest.mark.parametrize("min_len", [0, 7])
def test_cli_against_the_chain_of_tools(build, tmp_path, min_len):
    """founder_sequences --hold-out / --match-sequences with --remove-identity-columns: the PATH files equal the stdout of the
    project's own match_founder_sequences on the held-out sequences and the restored founders file the same run wrote."""
    cli = build.build_cli()
    tools = dict(zip(build.AUX_TOOLS, build.build_aux()))
    m, n = 24, 3000
    msa = founder_mosaic(6, m, n, brec=250, seed=11)
    rng = np.random.default_rng(11)
    held = [20, 3, 11, 17]
    keep = np.setdiff1d(np.arange(m), held)
    ident = rng.random(n) < 0.6
    ident[[0, n - 1]] = True
    msa[:, ident] = msa[keep[0]:keep[0] + 1, ident]
    for r in held:                                                # private variants of the held-out sequences, first and last column among them
        cols = np.flatnonzero(ident)[rng.integers(0, int(ident.sum()), size=12)]
        msa[r, cols] = ord("N")
    msa[held[0], [0, n - 1]] = ord("N")
    msa[held[1], rng.integers(0, n, size=6)] = ord("N")           # (kept columns too)
    names = []
    for i, row in enumerate(msa):
        (tmp_path / ("s%02d" % i)).write_bytes(row.tobytes())
        names.append(str(tmp_path / ("s%02d" % i)))
    (tmp_path / "list.txt").write_text("\n".join(names) + "\n")
    (tmp_path / "held.txt").write_text("\n".join(names[r] for r in held) + "\n")
    (tmp_path / "kept.txt").write_text("\n".join(names[r] for r in keep) + "\n")
    common = ["--remove-identity-columns", "--segment-length-bound", "20", "--segment-joining", "greedy", "--match-min-segment-length", str(min_len)]
    runs = {"H": [cli, "--input", str(tmp_path / "list.txt"), "--hold-out=" + ",".join(map(str, held)), "--output-founders=" + str(tmp_path / "F_H"),
                  "--output-held-out-restored-matches=" + str(tmp_path / "M_H")] + common,
            "Q": [cli, "--input", str(tmp_path / "kept.txt"), "--match-sequences", str(tmp_path / "held.txt"), "--output-founders=" + str(tmp_path / "F_Q"),
                  "--output-sequence-restored-matches=" + str(tmp_path / "M_Q")] + common}
    got = {}
    for tag, cmd in runs.items():
        r = subprocess.run(cmd, capture_output=True, timeout=120)
        assert r.returncode == 0, r.stderr
        assert b"Matched the input against" in r.stderr and b" 0 uncovered cells" not in r.stderr
        t = subprocess.run([tools["match_founder_sequences"], "--sequences", str(tmp_path / "held.txt"), "--founders", str(tmp_path / ("F_" + tag)),
                            "--founders-format", "text", "--single-threaded", "--min-segment-length", str(min_len)], capture_output=True, timeout=120)
        assert t.returncode == 0, t.stderr
        got[tag] = (tmp_path / ("M_" + tag)).read_bytes()
        assert got[tag] == t.stdout and got[tag].count(b"\n") > len(held)
    assert got["H"] == got["Q"] and (tmp_path / "F_H").read_bytes() == (tmp_path / "F_Q").read_bytes()
