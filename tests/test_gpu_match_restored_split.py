"""The restored match walk split along the kept columns on the device (csrc/fseq_match.hpp, k_match_walk_split with RST / EXC,
behind fseq_match_held_out_restored, fseq_match_rows_restored and fseq_match_founders_restored) against its specification,
tests/match_restored_split_model.py: pieces, founder sets, the three counters, the most pieces in a row, the report's bytes and
what match_split() reports -- EQUAL, so a run cannot pass by falling back everywhere (tests/test_match_restored_split_model.py
proves the model equal to the definition on the full-length data, and which cases stand).  Integer work: every comparison is exact.

A case of the model's table becomes a context like this: its K founders, restored, are the alignment (three of them once more:
the run then finds K founders among K + 3 rows), its queries are held out of that alignment, and the permutations hand slot f
of every segment to row f -- the restored founders are the case's."""
import importlib
import os
import subprocess

import numpy as np
import pytest

import identity_model as im
import match_exceptions_model as xm
import match_restored_split_model as rsm
from helpers import founder_mosaic
from test_gpu_match import founders_of
from test_gpu_match_restored import report_of

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def pkg():
    return importlib.import_module("founder-sequences_amd")


@pytest.fixture(scope="module")
def build():
    return importlib.import_module("founder-sequences_amd.build")


L = 20
BITS = (2, 4, 8)
# min_lens of a case on the device (the CPU test runs all of rsm.MIN_LENS on every case)
MIN_LENS_OF = {"mosaic K=5": (0, 3, 37), "planted": (0, 3, 37), "periodic": (0,), "mixed groups": (0,), "long piece": (0,), "G = n_kept": (0, 3)}
WORDS = {5: 1, 40: 2, 70: 4, 200: 8, 300: 64}                   # founders -> words the kernel holds a live set in (64: in LDS)


def widened(d, bits):
    """the case over an alphabet that packs at `bits`: row 0's identity columns redrawn from 10 (4 bits) or 30 (8 bits) symbols,
    none of them the private one; every cell of a query that was row 0's is row 0's again, every exception stays one"""
    if bits == 2:
        return d
    rng = np.random.default_rng(bits)
    wide = np.arange(48, 48 + (10 if bits == 4 else 30), dtype=np.uint8)
    assert rsm.PRIVATE not in wide
    mask = d["mask"]
    row0 = d["row0"].copy()
    row0[mask] = wide[rng.integers(0, len(wide), size=int(mask.sum()))]
    row0[np.flatnonzero(mask)[:len(wide)]] = wide                 # (every symbol occurs)
    queries = np.where((d["queries"] == d["row0"][None, :]) & mask[None, :], row0[None, :], d["queries"])
    return dict(d, row0=row0, queries=np.ascontiguousarray(queries))


_built, _wanted = {}, {}


def case_of(name):
    if name not in _built:
        _built[name] = rsm.CASES[name]["build"]()
    return _built[name]


def wanted(key, make):
    """the model's results do not depend on the alphabet: one call per (case, rows, founders, min_len), shared by the packings"""
    if key not in _wanted:
        _wanted[key] = make()
    return _wanted[key]


def chain(pkg, d):
    """-> (the reduced context that carries the held-out queries, the alignment's rows [K + 3, n_src])"""
    rows = im.restore(d["founders"], d["mask"], d["row0"])
    rows = np.vstack([rows, rows[[0, 1, 0]]])
    source = np.ascontiguousarray(np.vstack([rows, d["queries"]]))
    held = np.arange(len(rows), len(source), dtype=np.uint32)
    src = pkg.SegmentationContext(source.shape[0], source.shape[1], L)
    src.set_sequences(source)
    sub = src.without_rows(held, L)
    src.close()
    red = sub.without_identity_columns(L, keep_held_out=True)
    sub.close()
    return red, rows


def assert_equals_model(ctx, summary, want, K, tmp_path=None):
    pieces, sets = ctx.match_pieces()
    info = ctx.match_split()
    print("match: K=%d pieces=%d (model %d) uncovered=%d (%d) short=%d (%d) max/row=%d (%d) split=%s %.3f ms" % (
        K, summary["pieces"], len(want["pieces"]), summary["uncovered_cells"], want["uncovered_cells"], summary["short_pieces"],
        want["short_pieces"], summary["max_pieces_per_row"], want["max_pieces_per_row"], info, summary["ms_device"]))
    assert info == want["split"]
    assert summary["n_founders"] == K and summary["set_words"] == (K + 31) // 32 == sets.shape[1]
    assert summary["pieces"] == len(want["pieces"]) == len(pieces)
    for f in ("row", "lb", "rb", "n_founders"):
        assert np.array_equal(pieces[f], want["pieces"][f]), f
    assert np.array_equal(sets, want["sets"])
    for f in ("uncovered_cells", "short_pieces", "max_pieces_per_row"):
        assert summary[f] == want[f], f
    if tmp_path is not None:
        ctx.write_match(str(tmp_path / "match.txt"))
        assert (tmp_path / "match.txt").read_bytes() == report_of(want["pieces"], want["sets"])


def assert_exceptions(red, queries, mask, row0):
    off, cols = red.match_exceptions()
    exc = xm.exceptions_of(queries, mask, row0)
    assert np.array_equal(off, np.r_[0, np.cumsum([len(e) for e in exc])].astype(np.uint64))
    assert np.array_equal(cols, np.concatenate(exc).astype(np.uint32))


def test_the_table_covers_the_live_set_forms_and_the_packings():
    """(no GPU work)"""
    assert {len(case_of(n)["founders"]) for n in rsm.CASES} >= set(WORDS)
    assert any(len(case_of(n)["queries"]) == 257 for n in rsm.CASES)
    for bits in BITS:
        d = widened(case_of("planted"), bits)
        symbols = len(np.unique(np.concatenate([d["queries"].reshape(-1), d["row0"]])))
        assert {2: symbols <= 4, 4: 4 < symbols <= 16, 8: symbols > 16}[bits]
        assert [e.tolist() for e in xm.exceptions_of(d["queries"], d["mask"], d["row0"])] == \
               [e.tolist() for e in xm.exceptions_of(case_of("planted")["queries"], d["mask"], case_of("planted")["row0"])]


@pytest.mark.parametrize("bits", BITS)
@pytest.mark.parametrize("name", list(rsm.CASES))
def test_case_table(pkg, tmp_path, name, bits):
    """every case of the model's table through the three restored entries under the case's forced G and overlap: the held-out
    buffer, the same bytes from the host in staged chunks of 64 columns, and the alignment's own rows (no exceptions) against
    founders that take slot f + s in segment s (the alignment is the case's founders, and where the run finds one segment every
    row is one piece and its group falls back: test_the_alignments_own_rows has the rows that stand)"""
    case, d = rsm.CASES[name], widened(case_of(name), bits)
    mask, queries, row0 = d["mask"], d["queries"], d["row0"]
    K = len(d["founders"])
    red, rows = chain(pkg, d)
    assert red.n == int((~mask).sum()) and red.source_n == len(mask) and red.n_held == len(queries)
    res = red.run()
    assert res.max_segment_size == K
    segments = red.reduced_traceback()
    perm = np.tile(np.arange(K, dtype=np.uint32), (len(segments), 1))
    reduced = im.reduce_rows(rows, mask)
    assert np.array_equal(founders_of(reduced, perm, segments), d["founders"])
    turning = np.ascontiguousarray((perm + np.arange(len(segments), dtype=np.uint32)[:, None]) % np.uint32(K))
    turned = founders_of(reduced, turning, segments)
    red.set_tuning("FSEQ_MATCH_SPLIT", case["G"])
    red.set_tuning("FSEQ_MATCH_OVERLAP", case["overlap"])
    red.set_tuning("FSEQ_MATCH_STAGE_BYTES", "64")
    for i, min_len in enumerate(MIN_LENS_OF.get(name, (0, 37))):
        base = case_of(name)
        want = wanted((name, "queries", min_len), lambda: rsm.split_match(base["queries"], base["founders"], base["mask"], base["row0"], min_len, case["G"], case["overlap"]))
        rsm.check_expectation(name, want, min_len)
        s = red.match_held_out_restored(perm, min_segment_length=min_len)
        assert s["set_words"] <= WORDS.get(K, 1)
        assert_equals_model(red, s, want, K, tmp_path if i == 0 else None)
        assert_exceptions(red, queries, mask, row0)
        s = red.match_rows_restored(queries, perm, min_segment_length=min_len)
        assert_equals_model(red, s, want, K, tmp_path if i == 0 else None)
        assert_exceptions(red, queries, mask, row0)
        own = wanted((name, "own rows", min_len, segments.tobytes()),
                     lambda: rsm.split_match(im.restore(reduced, base["mask"], base["row0"]), turned, base["mask"], base["row0"], min_len, case["G"], case["overlap"]))
        s = red.match_founders_restored(turning, min_segment_length=min_len)
        assert_equals_model(red, s, own, K, tmp_path if i == 0 else None)
    red.close()


# founders of the mosaic, rows, bits of the packing: every live-set form (1, 2, 4, 8 register words; LDS) of the walk without
# exception lists.  (In test_case_table the alignment is the case's K founders: its own rows are one piece each.)
OWN_ROWS = [(6, 40, 2), (40, 100, 4), (100, 300, 8), (200, 300, 2), (280, 330, 4)]
ALPHABETS = {2: b"ACG", 4: b"ACGT-", 8: bytes(range(48, 88))}


@pytest.mark.parametrize("X,m,bits", OWN_ROWS)
def test_the_alignments_own_rows(pkg, tmp_path, X, m, bits):
    """fseq_match_founders_restored under the knobs: a founder mosaic over 2,000 kept columns (helpers.founder_mosaic: rows that
    change founders every 50 columns) between the model's gaps, against founders that take the greedy join's slot f + s in
    segment s -- a row's founder changes at nearly every segment, so every row closes often and stands at min_len = 0."""
    G, overlap, n_kept = 4, 300, 2000
    alpha = np.frombuffer(ALPHABETS[bits], dtype=np.uint8)
    rng = np.random.default_rng(X + m)
    mask = rsm.layout(rng, n_kept, G, overlap)
    red_rows = founder_mosaic(X, m, n_kept, brec=50, seed=X + m, alphabet=ALPHABETS[bits])
    for k in np.flatnonzero((red_rows == red_rows[0:1]).all(axis=0)):         # (a kept column is one in which the rows differ)
        red_rows[1, k] = alpha[(int(np.flatnonzero(alpha == red_rows[0, k])[0]) + 1) % len(alpha)]
    rows = np.empty((m, len(mask)), dtype=np.uint8)
    rows[:, ~mask] = red_rows
    rows[:, mask] = alpha[rng.integers(0, len(alpha), size=int(mask.sum()))][None, :]
    src = pkg.SegmentationContext(m, len(mask), L)
    src.set_sequences(rows)
    red = src.without_identity_columns(L)
    src.close()
    assert red.n == n_kept and red.source_n == len(mask)
    res = red.run()
    segments = red.reduced_traceback()
    greedy = red.join_greedy()
    K = greedy.shape[1]
    assert K == res.max_segment_size and len(segments) > 8
    perm = np.ascontiguousarray(np.stack([np.roll(greedy[s], -s) for s in range(len(segments))]))
    founders = founders_of(red_rows, perm, segments)
    red.set_tuning("FSEQ_MATCH_SPLIT", G)
    red.set_tuning("FSEQ_MATCH_OVERLAP", overlap)
    for min_len in (0, 37):
        want = rsm.split_match(rows, founders, mask, rows[0], min_len, G, overlap)
        if min_len == 0:
            assert want["stands"].all()
        s = red.match_founders_restored(perm, min_segment_length=min_len)
        assert_equals_model(red, s, want, K, tmp_path)
    red.close()


def test_the_knobs_and_the_walk_without_them(pkg):
    """FSEQ_MATCH_SPLIT=1 (the split kernel's one segment) gives bit for bit what the call without the knob gives (the unsplit
    kernel: these inputs are too short for two segments by itself); a split match in between leaves nothing behind; the exception
    lists answer after a split match."""
    name = "planted"
    case, d = rsm.CASES[name], case_of(name)
    red, rows = chain(pkg, d)
    red.run()
    S, K = len(red.reduced_traceback()), len(d["founders"])
    perm = np.tile(np.arange(K, dtype=np.uint32), (S, 1))
    one = {"segments": 1, "overlap": 0, "row_groups": 1, "flagged_groups": 0, "rows_not_standing": 0}
    calls = {"held": lambda ml: red.match_held_out_restored(perm, min_segment_length=ml),
             "rows": lambda ml: red.match_rows_restored(d["queries"], perm, min_segment_length=ml),
             "own": lambda ml: red.match_founders_restored(perm, min_segment_length=ml)}
    for how, call in calls.items():
        for min_len in (0, 37):
            plain = call(min_len)
            plain_pieces, plain_sets = red.match_pieces()
            assert red.match_split() == dict(one, row_groups=red.match_split()["row_groups"])
            red.set_tuning("FSEQ_MATCH_SPLIT", 1)
            got = call(min_len)
            pieces, sets = red.match_pieces()
            assert np.array_equal(pieces, plain_pieces) and np.array_equal(sets, plain_sets), (how, min_len)
            assert {k: v for k, v in got.items() if k != "ms_device"} == {k: v for k, v in plain.items() if k != "ms_device"}
            assert red.match_split()["segments"] == 1
            red.set_tuning("FSEQ_MATCH_SPLIT", case["G"])
            red.set_tuning("FSEQ_MATCH_OVERLAP", case["overlap"])
            got = call(min_len)
            pieces, sets = red.match_pieces()
            assert red.match_split()["segments"] == case["G"] and red.match_split()["overlap"] == case["overlap"]
            assert np.array_equal(pieces, plain_pieces) and np.array_equal(sets, plain_sets), (how, min_len)
            if how != "own":
                assert_exceptions(red, d["queries"], d["mask"], d["row0"])
            red.set_tuning("FSEQ_MATCH_SPLIT", None)
            red.set_tuning("FSEQ_MATCH_OVERLAP", None)
            call(min_len)
            assert red.match_split()["segments"] == 1
    red.close()


def test_cli_under_the_knobs(build, tmp_path):
    """founder_sequences --hold-out --remove-identity-columns --output-held-out-restored-matches with FSEQ_MATCH_SPLIT=3
    FSEQ_MATCH_OVERLAP=64 in the environment: the report equals the project's own match_founder_sequences on the held-out
    sequences and the restored founders file the same run wrote, byte for byte."""
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
    for r in held:
        msa[r, np.flatnonzero(ident)[rng.integers(0, int(ident.sum()), size=12)]] = ord("N")
    msa[held[0], [0, n - 1]] = ord("N")
    msa[held[1], rng.integers(0, n, size=6)] = ord("N")
    names = []
    for i, row in enumerate(msa):
        (tmp_path / ("s%02d" % i)).write_bytes(row.tobytes())
        names.append(str(tmp_path / ("s%02d" % i)))
    (tmp_path / "list.txt").write_text("\n".join(names) + "\n")
    (tmp_path / "held.txt").write_text("\n".join(names[r] for r in held) + "\n")
    for min_len in (0, 7):
        cmd = [cli, "--input", str(tmp_path / "list.txt"), "--hold-out=" + ",".join(map(str, held)), "--output-founders=" + str(tmp_path / "F"),
               "--output-held-out-restored-matches=" + str(tmp_path / "M"), "--remove-identity-columns", "--segment-length-bound", "20",
               "--segment-joining", "greedy", "--match-min-segment-length", str(min_len)]
        r = subprocess.run(cmd, capture_output=True, timeout=120, env=dict(os.environ, FSEQ_MATCH_SPLIT="3", FSEQ_MATCH_OVERLAP="64"))
        assert r.returncode == 0, r.stderr
        t = subprocess.run([tools["match_founder_sequences"], "--sequences", str(tmp_path / "held.txt"), "--founders", str(tmp_path / "F"),
                            "--founders-format", "text", "--single-threaded", "--min-segment-length", str(min_len)], capture_output=True, timeout=120)
        assert t.returncode == 0, t.stderr
        got = (tmp_path / "M").read_bytes()
        assert got == t.stdout and got.count(b"\n") > len(held)
