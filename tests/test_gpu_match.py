"""The device matcher (fseq_match_founders / fseq_match_founder_rows, csrc/fseq_match.hpp) against its specification
(tests/match_model.py, pinned to the host tool by tests/test_match_abi.py).  Integer work: every comparison is exact."""
import importlib
import os
import subprocess
import threading

import numpy as np
import pytest

import fso
import match_model as mm
from helpers import founder_mosaic

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def pkg():
    return importlib.import_module("founder-sequences_amd")


@pytest.fixture(scope="module")
def build():
    return importlib.import_module("founder-sequences_amd.build")


def tile_cols(K, sigma):
    """match_shape of csrc/fseq_match.hpp: columns of a tile of the walk for K founders over sigma codes"""
    bsh = 2 if sigma <= 4 else 1 if sigma <= 16 else 0
    W = (K + 31) // 32
    WR = 1 if W <= 1 else 2 if W <= 2 else 4 if W <= 4 else 8 if W <= 8 else 0
    Wk, Kp = WR or W, (K + 63) // 64 * 64
    tc = max(1, min(64, 65536 // (sigma * Wk * 4), 16384 // Kp, 16384 // (256 >> bsh)))
    lds = lambda t: t * Kp + t * (256 >> bsh) + (t * sigma + 1) * Wk * 4 + (0 if WR else Wk * 1024)
    while tc > 1 and lds(tc) > 152 * 1024:
        tc -= 1
    return tc


def assert_equals_model(pkg, ctx, summary, want, K):
    pieces, sets = ctx.match_pieces()
    print("match: K=%d pieces=%d (model %d) uncovered=%d (%d) short=%d (%d) max/row=%d (%d) %.3f ms" % (
        K, summary["pieces"], len(want["pieces"]), summary["uncovered_cells"], want["uncovered_cells"], summary["short_pieces"],
        want["short_pieces"], summary["max_pieces_per_row"], want["max_pieces_per_row"], summary["ms_device"]))
    assert summary["n_founders"] == K and summary["set_words"] == (K + 31) // 32 == sets.shape[1]
    assert summary["pieces"] == len(want["pieces"]) == len(pieces)
    for f in ("row", "lb", "rb", "n_founders"):
        assert np.array_equal(pieces[f], want["pieces"][f]), f
    assert np.array_equal(sets, want["sets"])
    for f in ("uncovered_cells", "short_pieces", "max_pieces_per_row"):
        assert summary[f] == want[f], f


SIGMAS = [2, 4, 16, 40]                                            # 2-, 2-, 4- and 8-bit packing
# ... 33, 65, 129, 257: one above every boundary between the variants (1, 2, 4, 8 register words; live sets in LDS); 2048: the limit
FOUNDERS = [1, 2, 31, 32, 33, 64, 65, 128, 129, 255, 256, 257, 2048]
ROWS = [1, 3, 63, 64, 65, 1000, 1025]
COLUMNS = ["1", "2", "tile-1", "tile", "tile+1", "5000"]


@pytest.mark.parametrize("i", range(42))
def test_differential_against_the_model(pkg, i):
    """Every listed value of sigma, K, m and n occurs, every (m, n) pair once (42 = 6 x 7 cases), each with min_len 0, 1, 7 and
    n + 1.  The founders' 2,048 meets the short column counts here; test_the_limit_of_founders_over_many_tiles walks it over tiles."""
    sigma, K, m = SIGMAS[i % 4], FOUNDERS[i % 13], ROWS[i % 7]
    T = tile_cols(K, sigma)
    n = {"1": 1, "2": 2, "tile-1": max(1, T - 1), "tile": T, "tile+1": T + 1, "5000": 5003}[COLUMNS[i % 6]]
    msa, founders = mm.mosaic_case(1000 + i, m, n, K, sigma)
    ctx = pkg.SegmentationContext(m, n, max(1, n // 4))
    ctx.set_sequences(msa)
    print("case %d: sigma=%d K=%d m=%d n=%d tile=%d" % (i, sigma, K, m, n, T))
    for min_len in (0, 1, 7, n + 1):
        s = ctx.match_founders(founders=founders, min_segment_length=min_len)
        assert_equals_model(pkg, ctx, s, mm.match_rows(msa, founders, min_len), K)
    ctx.close()


@pytest.mark.parametrize("sigma", [4, 16])
def test_the_limit_of_founders_over_many_tiles(pkg, sigma):
    """2,048 founders (64 words of live set a lane in LDS, tiles of 8 columns) over some forty tiles: the tile loop, the next
    tile's loads and the live set carried from tile to tile at the limit."""
    K, m, n = 2048, 65, 331
    assert tile_cols(K, sigma) <= 8
    msa, founders = mm.mosaic_case(77 + sigma, m, n, K, sigma)
    ctx = pkg.SegmentationContext(m, n, 50)
    ctx.set_sequences(msa)
    for min_len in (0, 7):
        s = ctx.match_founders(founders=founders, min_segment_length=min_len)
        assert_equals_model(pkg, ctx, s, mm.match_rows(msa, founders, min_len), K)
    ctx.close()


def founders_of(msa, perm, segments):
    """the lines fseq_write_founders_device writes: founder r in segment s is row perm[s][r], a slot >= m is '-'"""
    m, n = msa.shape
    out = np.full((perm.shape[1], n), ord("-"), dtype=np.uint8)
    for s, seg in enumerate(segments):
        ok = perm[s] < m
        out[ok, int(seg["lb"]):int(seg["rb"])] = msa[perm[s][ok], int(seg["lb"]):int(seg["rb"])]
    return out


def rows_with_a_slot(msa, perm, segments):
    """[S, m]: the row's text in the segment is the text of some founder slot there"""
    m = msa.shape[0]
    has = np.zeros((len(segments), m), dtype=bool)
    for s, seg in enumerate(segments):
        block = np.ascontiguousarray(msa[:, int(seg["lb"]):int(seg["rb"])])
        keys = block.view([("", "V%d" % block.shape[1])]).ravel()
        has[s] = np.isin(keys, keys[perm[s][perm[s] < m]])
    return has


def check_validator_properties(pieces, summary, segments, n, m, has_slot=None):
    """no uncovered cell; every row's pieces tile [0, n); a piece that starts inside merged segment i ends at or after its rb."""
    assert summary["uncovered_cells"] == 0
    row, lb, rb = pieces["row"].astype(np.int64), pieces["lb"].astype(np.int64), pieces["rb"].astype(np.int64)
    first = np.flatnonzero(np.r_[True, row[1:] != row[:-1]])
    last = np.r_[first[1:] - 1, len(row) - 1]
    assert np.array_equal(row[first], np.arange(m)) and (lb[first] == 0).all() and (rb[last] == n).all()
    inner = np.flatnonzero(row[1:] == row[:-1])
    assert np.array_equal(lb[inner + 1], rb[inner]) and (rb > lb).all()
    seg = np.searchsorted(segments["rb"].astype(np.int64), lb, side="right")
    reaches = rb >= segments["rb"].astype(np.int64)[seg]
    if has_slot is None:
        assert reaches.all()
        assert summary["max_pieces_per_row"] <= len(segments)
        return m
    assert reaches[has_slot[seg, row]].all()
    good = has_slot.all(axis=0)                                    # rows whose every text has a slot
    per_row = np.bincount(row, minlength=m)
    assert (per_row[good] <= len(segments)).all()
    return int(good.sum())


@pytest.mark.parametrize("config", ["C1", "C2"])
def test_validator_property_on_real_output(pkg, tmp_path, config):
    """After run() and each joiner: the founders just produced cover every row in no more pieces than segments, and the match by
    permutations is the match by the rows of the founders file and the model's on those rows.
    The greedy and the random joiner give every distinct substring of a segment a slot by construction.  The bipartite
    joiner matches texts between neighbouring segments and may leave a text without a slot; the segment property is asserted
    there on the rows whose text has one, which must be at least nine rows in ten."""
    c = fso.CONFIGS[config]
    m, n, L = c["m"], c["n"], c["L"]
    ctx = pkg.SegmentationContext(m, n, L)
    if config == "C1":
        msa = np.ascontiguousarray(fso.synth_msa(fso.config_spec(config), m, n))
        ctx.set_sequences(msa)
    else:
        ctx.generate_synthetic(c["seed"], c["K"], c["B"], c["mu"], c["kind"])
        msa = np.ascontiguousarray(ctx.get_sequences())
    res = ctx.run()
    segments = ctx.reduced_traceback()
    for name in ("greedy", "bipartite", "random"):
        perm = getattr(ctx, "join_" + name)()
        s = ctx.match_founders(perm)
        pieces, sets = ctx.match_pieces()
        has = rows_with_a_slot(msa, perm, segments)
        if name != "bipartite":
            assert has.all()
        good = check_validator_properties(pieces, s, segments, n, m, None if name != "bipartite" else has)
        print("%s %s: K=%d segments=%d pieces=%d max/row=%d rows with every text in a slot=%d of %d, %.3f ms" % (
            config, name, res.max_segment_size, len(segments), s["pieces"], s["max_pieces_per_row"], good, m, s["ms_device"]))
        assert 10 * good >= 9 * m
        path = str(tmp_path / ("founders_%s.txt" % name))
        ctx.write_founders_device(perm, path)
        rows = np.frombuffer(open(path, "rb").read(), dtype=np.uint8).reshape(res.max_segment_size, n + 1)[:, :n]
        assert np.array_equal(rows, founders_of(msa, perm, segments))
        s2 = ctx.match_founders(founders=rows)
        pieces2, sets2 = ctx.match_pieces()
        assert np.array_equal(pieces, pieces2) and np.array_equal(sets, sets2)
        assert {k: v for k, v in s.items() if k != "ms_device"} == {k: v for k, v in s2.items() if k != "ms_device"}
        assert_equals_model(pkg, ctx, s2, mm.match_rows(msa, rows, 0), res.max_segment_size)
    ctx.close()


def small_run(pkg, seed=3, X=6, m=40, n=2000, L=20):
    msa = founder_mosaic(X, m, n, brec=100, seed=seed)
    ctx = pkg.SegmentationContext(m, n, L)
    ctx.set_sequences(msa)
    ctx.run()
    return msa, ctx


def test_a_bad_founder_set_is_caught(pkg):
    msa, ctx = small_run(pkg)
    m, n = msa.shape
    segments = ctx.reduced_traceback()
    perm = ctx.join_greedy()
    clean = ctx.match_founders(perm)
    clean_pieces, _ = ctx.match_pieces()
    assert clean["uncovered_cells"] == 0 and clean["max_pieces_per_row"] <= len(segments)
    # one slot of a middle segment takes a row of another class: the class it stood for has no founder there any more
    s = len(segments) // 2
    lb, rb = int(segments["lb"][s]), int(segments["rb"][s])
    victim = int(perm[s, 0])
    other = next(r for r in range(m) if r != victim and bytes(msa[r, lb:rb]) != bytes(msa[victim, lb:rb]))
    bad = perm.copy()
    bad[s, 0] = other
    got = ctx.match_founders(bad)
    assert_equals_model(pkg, ctx, got, mm.match_rows(msa, founders_of(msa, bad, segments), 0), perm.shape[1])
    pieces, _ = ctx.match_pieces()
    assert len(pieces) != len(clean_pieces) or not np.array_equal(pieces, clean_pieces)
    assert got["pieces"] > clean["pieces"]
    ctx.close()


@pytest.mark.parametrize("min_len", [0, 7])
def test_report_bytes_are_the_host_tools(pkg, build, tmp_path, min_len):
    msa, ctx = small_run(pkg, seed=5)
    m, n = msa.shape
    tools = dict(zip(build.AUX_TOOLS, build.build_aux()))
    cli = build.build_cli()
    paths = []
    for r in range(m):
        (tmp_path / ("s%d.txt" % r)).write_bytes(bytes(msa[r]))
        paths.append(str(tmp_path / ("s%d.txt" % r)))
    (tmp_path / "seqs.txt").write_text("\n".join(paths) + "\n")

    def tool(founders_path):
        r = subprocess.run([tools["match_founder_sequences"], "--sequences", str(tmp_path / "seqs.txt"), "--founders", founders_path,
                            "--founders-format", "text", "--single-threaded", "--min-segment-length", str(min_len)], capture_output=True, timeout=300)
        assert r.returncode == 0, r.stderr
        return r.stdout

    perm = ctx.join_greedy()
    ctx.write_founders_device(perm, str(tmp_path / "founders_api.txt"))
    ctx.match_founders(perm, min_segment_length=min_len)
    ctx.write_match(str(tmp_path / "match_api.txt"))
    want = tool(str(tmp_path / "founders_api.txt"))
    assert want.count(b"\n") > m and (tmp_path / "match_api.txt").read_bytes() == want
    ctx.close()
    r = subprocess.run([cli, "--input", str(tmp_path / "seqs.txt"), "--segment-length-bound", "20", "--segment-joining", "greedy",
                        "--output-founders", str(tmp_path / "founders_cli.txt"), "--output-matches", str(tmp_path / "match_cli.txt"),
                        "--match-min-segment-length", str(min_len)], capture_output=True, timeout=300)
    assert r.returncode == 0, r.stderr
    assert b"uncovered cells" in r.stderr
    assert (tmp_path / "match_cli.txt").read_bytes() == tool(str(tmp_path / "founders_cli.txt"))


@pytest.mark.parametrize("min_len", [0, 7])
def test_front_end_report_on_the_short_path(build, tmp_path, min_len):
    """n < 2L: no permutations; the founders are the distinct rows the front end writes, and the report is the host tool's on them."""
    rng = np.random.default_rng(21)
    distinct = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, size=(5, 30))]
    msa = distinct[rng.integers(0, 5, size=14)]
    tools = dict(zip(build.AUX_TOOLS, build.build_aux()))
    paths = []
    for r in range(len(msa)):
        (tmp_path / ("s%d.txt" % r)).write_bytes(bytes(msa[r]))
        paths.append(str(tmp_path / ("s%d.txt" % r)))
    (tmp_path / "seqs.txt").write_text("\n".join(paths) + "\n")
    r = subprocess.run([build.build_cli(), "--input", str(tmp_path / "seqs.txt"), "--segment-length-bound", "20", "--output-founders", str(tmp_path / "founders.txt"),
                        "--output-matches", str(tmp_path / "match.txt"), "--match-min-segment-length", str(min_len)], capture_output=True, timeout=300)
    assert r.returncode == 0, r.stderr
    assert b"0 uncovered cells" in r.stderr
    t = subprocess.run([tools["match_founder_sequences"], "--sequences", str(tmp_path / "seqs.txt"), "--founders", str(tmp_path / "founders.txt"),
                        "--founders-format", "text", "--single-threaded", "--min-segment-length", str(min_len)], capture_output=True, timeout=300)
    assert t.returncode == 0, t.stderr
    assert t.stdout.count(b"\n") >= 1 + len(msa) and (tmp_path / "match.txt").read_bytes() == t.stdout


def test_borrowed_input_gives_the_same_pieces(pkg):
    import torch
    m, n, sigma, K = 333, 700, 4, 9
    rng = np.random.default_rng(17)
    founders = rng.integers(0, sigma, size=(K, n)).astype(np.uint8)
    codes = np.empty((m, n), dtype=np.uint8)
    pick = rng.integers(0, K, size=(m, (n + 49) // 50))
    for b in range(pick.shape[1]):
        codes[:, b * 50:(b + 1) * 50] = founders[pick[:, b], b * 50:(b + 1) * 50]
    noise = rng.random((m, n)) < 5e-3
    codes[noise] = rng.integers(0, sigma, size=int(noise.sum()))
    assert len(np.unique(codes)) == sigma                         # uploaded: dense codes in byte order = the codes themselves
    results = []
    for how in ("uploaded", "device columns", "packed"):
        ctx = pkg.SegmentationContext(m, n, 20)
        if how == "uploaded":
            ctx.set_sequences(codes)
        elif how == "device columns":
            ld = (m + 15) // 16 * 16 + 32                         # ld > m
            cols = np.full((n, ld), 0xEE, dtype=np.uint8)
            cols[:, :m] = codes.T
            dev = torch.from_numpy(cols).to("cuda")
            ctx.set_device_columns(dev.data_ptr(), ld, sigma, keepalive=dev)
        else:
            packed, ld = pkg.pack_columns(codes, 2)
            dev = torch.from_numpy(packed).to("cuda")
            ctx.set_device_columns_packed(dev.data_ptr(), ld, sigma, 2, keepalive=dev)
        for min_len in (0, 7):
            s = ctx.match_founders(founders=founders, min_segment_length=min_len)
            results.append((how, min_len, s, ctx.match_pieces()))
        ctx.close()
    for min_len in (0, 7):
        same = [r for r in results if r[1] == min_len]
        assert_model = mm.match_rows(codes, founders, min_len)
        for how, _, s, (pieces, sets) in same:
            assert np.array_equal(pieces, same[0][3][0]) and np.array_equal(sets, same[0][3][1]), how
            assert s["pieces"] == len(assert_model["pieces"]) and np.array_equal(sets, assert_model["sets"]), how
            assert np.array_equal(pieces["lb"], assert_model["pieces"]["lb"]) and np.array_equal(pieces["rb"], assert_model["pieces"]["rb"])


def state_of(ctx):
    red = ctx.reduced_traceback()
    return ctx.traceback(), red, [ctx.boundary_state(i) for i in range(len(red))]


def assert_same_state(a, b):
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and len(a[2]) == len(b[2])
    for (a0, d0), (a1, d1) in zip(a[2], b[2]):
        assert np.array_equal(a0, a1) and np.array_equal(d0, d1)


def test_the_context_is_unharmed(pkg):
    msa, ctx = small_run(pkg, seed=9)
    m, n = msa.shape
    before = state_of(ctx)
    perm = ctx.join_greedy()
    with pytest.raises(pkg.FseqError) as e:                       # nothing matched yet
        ctx.match_pieces()
    assert e.value.code == pkg.FSEQ_E_ARG
    first = ctx.match_founders(perm)
    assert_same_state(before, state_of(ctx))
    assert np.array_equal(perm, ctx.join_greedy())
    # a second match, with other founders, replaces the first
    two = msa[:2]
    second = ctx.match_founders(founders=two, min_segment_length=5)
    assert_equals_model(pkg, ctx, second, mm.match_rows(msa, two, 5), 2)
    assert second["pieces"] != first["pieces"]
    # more founders than the largest variant holds
    too_many = np.repeat(msa[:1], pkg.MATCH_MAX_FOUNDERS + 1, axis=0)
    with pytest.raises(pkg.FseqError) as e:
        ctx.match_founders(founders=too_many)
    assert e.value.code == pkg.FSEQ_E_UNSUPPORTED and "2048" in str(e.value)
    with pytest.raises(pkg.FseqError) as e:                       # (a refused match leaves the last result where it was)
        ctx.match_founders(founders=np.zeros((0, n), dtype=np.uint8))
    assert e.value.code == pkg.FSEQ_E_ARG
    assert len(ctx.match_pieces()[0]) == second["pieces"]
    ctx.run()
    assert_same_state(before, state_of(ctx))
    assert_same_state(before, state_of(ctx))
    ctx.close()
    # the short path has no permutations: refused, and the rows it names are the founders
    sp = pkg.SegmentationContext(m, 30, 20)
    sp.set_sequences(np.ascontiguousarray(msa[:, :30]))
    assert sp.run().short_path == 1
    with pytest.raises(pkg.FseqError) as e:
        sp.match_founders(np.zeros((1, sp.result.max_segment_size), dtype=np.uint32))
    assert e.value.code == pkg.FSEQ_E_ARG
    rows, _ = sp.short_path_runs()
    s = sp.match_founders(founders=np.ascontiguousarray(msa[rows, :30]))
    assert s["uncovered_cells"] == 0 and s["pieces"] == m == m * s["max_pieces_per_row"]
    sp.close()


def test_a_sharded_context_refuses_and_still_runs(pkg):
    from test_gpu_shard import run_world
    m, n, L = 40, 6000, 20
    msa = founder_mosaic(6, m, n, brec=100, seed=4)
    ctxs = run_world(pkg, 2, lambda c: c.set_sequences(msa), m, n, L)
    red = [c.reduced_traceback() for c in ctxs]
    for c in ctxs:
        with pytest.raises(pkg.FseqError) as e:
            c.match_founders(founders=msa[:3])
        assert e.value.code == pkg.FSEQ_E_UNSUPPORTED
        with pytest.raises(pkg.FseqError) as e:
            c.match_founders(np.zeros((len(red[0]), c.result.max_segment_size), dtype=np.uint32))
        assert e.value.code == pkg.FSEQ_E_UNSUPPORTED
    errs = []

    def again(r):
        try:
            ctxs[r].run()
        except BaseException as e:
            errs.append(e)

    ths = [threading.Thread(target=again, args=(r,), daemon=True) for r in range(2)]
    for t in ths:
        t.start()
    for t in ths:
        t.join(timeout=120)
        assert not t.is_alive()
    assert not errs
    for r, c in enumerate(ctxs):
        assert np.array_equal(c.reduced_traceback(), red[r])


def test_config_c3_full_size(pkg):
    """BASELINE C3 (m = 2,504, n = 1,000,000) with the greedy join: the validator's properties over all rows, and eight rows
    chosen by a fixed seed piece by piece against the numpy model."""
    c = fso.CONFIGS["C3"]
    m, n, L = c["m"], c["n"], c["L"]
    ctx = pkg.SegmentationContext(m, n, L)
    ctx.generate_synthetic(c["seed"], c["K"], c["B"], c["mu"], c["kind"])
    res = ctx.run()
    segments = ctx.reduced_traceback()
    perm = ctx.join_greedy()
    s = ctx.match_founders(perm)
    pieces, sets = ctx.match_pieces()
    print("C3 greedy: K=%d W=%d segments=%d pieces=%d max/row=%d uncovered=%d, %.3f ms on the device" % (
        s["n_founders"], s["set_words"], len(segments), s["pieces"], s["max_pieces_per_row"], s["uncovered_cells"], s["ms_device"]))
    assert s["n_founders"] == res.max_segment_size and s["short_pieces"] == 0
    check_validator_properties(pieces, s, segments, n, m)
    msa = ctx.get_sequences()
    founders = founders_of(msa, perm, segments)
    start = np.flatnonzero(np.r_[True, pieces["row"][1:] != pieces["row"][:-1], True])
    for r in np.random.default_rng(0xC3).choice(m, size=8, replace=False):
        want, unc = mm.match_row_fast(np.ascontiguousarray(msa[r]), founders)
        mine = slice(start[r], start[r + 1])
        assert unc == 0 and len(want) == start[r + 1] - start[r]
        assert [(int(a), int(b)) for a, b, _ in want] == list(zip(pieces["lb"][mine].tolist(), pieces["rb"][mine].tolist()))
        assert mm.sets_to_lists(sets[mine]) == [idx.tolist() for _, _, idx in want]
    ctx.close()
