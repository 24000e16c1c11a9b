"""The restored match (fseq_match_founders_restored, csrc/fseq_match.hpp) against its definition: match_model.match_rows on
the full-length rows and the full-length restored founders (identity_model.restore of the reduced founders).  Integer work:
every comparison is exact.  tests/test_match_restored_abi.py pins the gap step the kernel follows to the same definition."""
import importlib
import subprocess

import numpy as np
import pytest

import identity_model as im
import match_model as mm
from helpers import founder_mosaic
from test_gpu_match import assert_equals_model, founders_of, tile_cols

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def pkg():
    return importlib.import_module("founder-sequences_amd")


@pytest.fixture(scope="module")
def build():
    return importlib.import_module("founder-sequences_amd.build")


ALPHABETS = {4: b"ACGT", 5: b"ACGT-", 40: bytes(range(48, 88))}
MIN_LENS = [0, 1, 5, 50]
L = 5
# name: rows, sigma, founders of the mosaic over the kept columns, kept columns, first gap, last gap, the other gaps, set words
# of the live-set form (1, 2, 4, 8 register words; more: LDS).  m = 37: part of one workgroup of the walk, 300 and 700: two and
# three.  Kept counts around the 64-column tile (tile_cols; 51 columns for the 300 founders of `lds`).
CASES = {
    "w1-kept63":   dict(m=37,  sigma=4,  X=6,   kept=63,  first=0,  last=0,   gaps="mixed", words=(1, 1)),     # source column 0 and the last one kept
    "w1-nogap":    dict(m=37,  sigma=4,  X=6,   kept=65,  first=0,  last=0,   gaps="none",  words=(1, 1)),     # no identity column at all
    "w2-kept64":   dict(m=300, sigma=5,  X=40,  kept=64,  first=9,  last=17,  gaps="mixed", words=(2, 2)),     # both of them identity columns
    "w4-kept65":   dict(m=300, sigma=40, X=100, kept=65,  first=1,  last=1,   gaps="mixed", words=(3, 4)),     # a gap over the tile border 64 | 65
    "w8-kept130":  dict(m=300, sigma=4,  X=200, kept=130, first=110, last=120, gaps="long",  words=(5, 8)),    # gaps of more than 100 columns
    "lds-kept130": dict(m=700, sigma=4,  X=300, kept=130, first=3,  last=0,   gaps="short", words=(9, 64)),
}


def make_case(name):
    """-> (msa [m, n_src], mask): the kept columns are a founder mosaic (helpers.founder_mosaic: its smallest maximum segment
    size is X), the identity columns between them carry one symbol each."""
    c = CASES[name]
    rng = np.random.default_rng(sum(name.encode()))
    alpha = np.frombuffer(ALPHABETS[c["sigma"]], dtype=np.uint8)
    red = founder_mosaic(c["X"], c["m"], c["kept"], brec=50, seed=c["kept"] + c["X"], alphabet=ALPHABETS[c["sigma"]])
    k = c["kept"]
    draw = {"none": [0], "mixed": [0, 0, 1, 2, 7, 30], "long": [0, 1, 3, 11], "short": [0, 1, 2, 3, 6]}[c["gaps"]]
    gaps = rng.choice(draw, size=k + 1)
    if c["gaps"] == "long":
        gaps[[40, 64, 101]] = [120, 133, 151]
    T = tile_cols(c["X"], c["sigma"])
    if c["gaps"] != "none" and k > T:
        gaps[T] = max(gaps[T], 41 if c["gaps"] == "mixed" else 6)  # in front of the first column of the second tile
    gaps[0], gaps[k] = c["first"], c["last"]
    mask = np.concatenate([np.r_[np.ones(g, dtype=bool), False] for g in gaps[:k]] + [np.ones(gaps[k], dtype=bool)])
    msa = np.empty((c["m"], len(mask)), dtype=np.uint8)
    msa[:, ~mask] = red
    msa[:, mask] = alpha[rng.integers(0, len(alpha), size=int(mask.sum()))][None, :]
    return np.ascontiguousarray(msa), mask


def test_the_cases_cover_what_they_claim():
    """(no GPU work) the layouts of the sources: kept counts around the tile, source lengths, first and last columns, the gap
    over a tile border, the gaps of more than 100 columns."""
    for name, c in CASES.items():
        msa, mask = make_case(name)
        n_src, kept = len(mask), np.flatnonzero(~mask)
        assert np.array_equal(im.identity_mask(msa), mask), name   # (every column of the mosaic has two symbols)
        assert len(kept) == c["kept"] and len(np.unique(msa)) == c["sigma"]
        assert (mask[0], mask[-1]) == (c["first"] > 0, c["last"] > 0)
        if c["gaps"] == "none":
            assert n_src == c["kept"]
        else:
            assert 3 * c["kept"] <= n_src <= 10 * c["kept"], (name, n_src)
        T = tile_cols(c["X"], c["sigma"])
        if c["kept"] > T and c["gaps"] != "none":
            assert kept[T] - kept[T - 1] > 1                       # identity columns between the last column of a tile and the next
        if c["gaps"] == "long":
            assert (np.diff(kept) > 101).sum() >= 3 and kept[0] > 100 and n_src - kept[-1] > 101
    assert {c["kept"] for c in CASES.values()} >= {63, 64, 65, 130}
    assert {c["sigma"] for c in CASES.values()} == {4, 5, 40} and {c["m"] for c in CASES.values()} >= {37, 300}
    assert [tile_cols(c["X"], c["sigma"]) for c in CASES.values()] == [64, 64, 64, 64, 64, 51]


def doctored(rng, perm, m):
    """permutations no joiner gives: every slot a row of a handful, some slots without a row (>= m)"""
    hand = rng.choice(m, size=5, replace=False)
    bad = hand[rng.integers(0, len(hand), size=perm.shape)].astype(np.uint32)
    holes = rng.random(perm.shape) < 0.05
    holes[0, 0] = holes[-1, -1] = True
    bad[holes] = rng.choice([m, m + 7, (1 << int(m).bit_length()) - 1], size=int(holes.sum()))
    return bad


def report_of(pieces, sets):
    lists = mm.sets_to_lists(sets)
    lines = ["SEQUENCE_INDEX\tLB\tRB\tFOUNDER_INDICES"]
    lines += ["%d\t%d\t%d\t%s" % (r, lb, rb, ",".join(map(str, idx))) for r, lb, rb, idx in zip(pieces["row"].tolist(), pieces["lb"].tolist(), pieces["rb"].tolist(), lists)]
    return ("\n".join(lines) + "\n").encode()


REPORT_INDICES = 8000000      # founder indices of a report the test formats in Python (a report is a function of pieces and sets)


@pytest.fixture(scope="module")
def runs(pkg):
    """name -> (msa, mask, the reduced context after its run, {greedy, doctored: (permutations, full-length founders)}),
    made on first use and shared by the min_len cases"""
    made = {}

    def get(name):
        if name not in made:
            c = CASES[name]
            msa, mask = make_case(name)
            src = pkg.SegmentationContext(c["m"], msa.shape[1], L)
            src.set_sequences(msa)
            red = src.without_identity_columns(L)
            src.close()
            assert red.n == c["kept"] and red.source_n == msa.shape[1]
            res = red.run()
            segments = red.reduced_traceback()
            reduced = im.reduce_rows(msa, mask)
            perms = {"greedy": red.join_greedy()}
            perms["doctored"] = doctored(np.random.default_rng(c["m"] + c["kept"]), perms["greedy"], c["m"])
            assert (perms["doctored"] >= c["m"]).any() and res.max_segment_size < c["m"]
            founders = {k: im.restore(founders_of(reduced, p, segments), mask, msa[0]) for k, p in perms.items()}
            made[name] = (msa, mask, red, {k: (perms[k], founders[k]) for k in perms})
        return made[name]

    yield get
    for _, _, red, _ in made.values():
        red.close()


@pytest.mark.parametrize("min_len", MIN_LENS)
@pytest.mark.parametrize("name", list(CASES))
def test_differential_against_the_model(pkg, runs, tmp_path, name, min_len):
    c = CASES[name]
    msa, mask, red, perms = runs(name)
    n_src = msa.shape[1]
    for how, (perm, founders) in perms.items():
        K = perm.shape[1]
        want = mm.match_rows(msa, founders, min_len)
        s = red.match_founders_restored(perm, min_segment_length=min_len)
        print("%s %s min_len=%d: n_src=%d kept=%d K=%d set_words=%d" % (name, how, min_len, n_src, red.n, K, s["set_words"]))
        assert c["words"][0] <= s["set_words"] <= c["words"][1]
        assert_equals_model(pkg, red, s, want, K)
        pieces, sets = red.match_pieces()
        assert int(pieces["rb"].max()) == n_src
        if how == "doctored":
            assert s["uncovered_cells"] > 0
        else:
            assert s["uncovered_cells"] == 0
        if c["gaps"] == "none":                                   # no identity column: the reduced match itself
            s2 = red.match_founders(perm, min_segment_length=min_len)
            pieces2, sets2 = red.match_pieces()
            assert np.array_equal(pieces, pieces2) and np.array_equal(sets, sets2)
            assert {k: v for k, v in s.items() if k != "ms_device"} == {k: v for k, v in s2.items() if k != "ms_device"}
            red.match_founders_restored(perm, min_segment_length=min_len)
        if min_len == 50 and c["gaps"] == "long":                 # a piece that starts and ends inside a run of identity columns
            lb, rb = pieces["lb"].astype(np.int64), pieces["rb"].astype(np.int64)
            inside = np.add.accumulate(np.r_[0, mask.astype(np.int64)])
            assert ((rb - lb == 50) & (inside[rb] - inside[lb] == 50)).any()
        if int(want["pieces"]["n_founders"].sum()) <= REPORT_INDICES:
            red.write_match(str(tmp_path / how))
            assert (tmp_path / how).read_bytes() == report_of(want["pieces"], want["sets"])
        else:
            assert min_len in (1, 5)                              # (every case is compared as a report for min_len 0 and 50)
    if min_len == 0:                                              # the founders matched are the ones the context writes
        red.write_founders_restored(perms["doctored"][0], str(tmp_path / "F"))
        assert np.array_equal(im.lines_of(str(tmp_path / "F")), perms["doctored"][1])


def test_refusals_leave_the_context_and_its_last_match_alone(pkg):
    m, L_ = 30, 20
    msa, mask = make_case("w1-kept63")
    msa = np.ascontiguousarray(np.tile(msa[:m], (1, 4)))          # 252 kept columns: a long path at L = 20
    n = msa.shape[1]
    ctx = pkg.SegmentationContext(m, n, L_)
    ctx.set_sequences(msa)
    ctx.run()
    perm = ctx.join_greedy()
    before = ctx.match_founders(perm)
    kept_pieces = ctx.match_pieces()
    with pytest.raises(pkg.FseqError) as e:                       # a plain context
        ctx.match_founders_restored(perm)
    assert e.value.code == pkg.FSEQ_E_ARG and "not a context made by fseq_create_without_identity_columns" in str(e.value)
    again = ctx.match_pieces()
    assert np.array_equal(again[0], kept_pieces[0]) and np.array_equal(again[1], kept_pieces[1])
    assert {k: v for k, v in ctx.match_founders(perm).items() if k != "ms_device"} == {k: v for k, v in before.items() if k != "ms_device"}
    red = ctx.without_identity_columns(L_)
    reduced = im.reduce_rows(msa, im.identity_mask(msa))
    first = red.match_founders(founders=reduced[:2])              # (needs the alignment only)
    with pytest.raises(pkg.FseqError) as e:                       # before a run
        red.match_founders_restored(np.zeros((1, 2), dtype=np.uint32))
    assert e.value.code == pkg.FSEQ_E_ARG
    assert len(red.match_pieces()[0]) == first["pieces"]
    red.run()
    p2 = red.join_greedy()
    s = red.match_founders_restored(p2)
    mask = im.identity_mask(msa)
    want = mm.match_rows(msa, im.restore(founders_of(reduced, p2, red.reduced_traceback()), mask, msa[0]), 0)
    assert_equals_model(pkg, red, s, want, p2.shape[1])
    red.close()
    short = ctx.without_identity_columns(reduced.shape[1])        # n < 2 L: the short path
    ctx.close()
    kept = short.match_founders(founders=reduced[:3])
    try:
        short.run()
    except pkg.NoReduction:                                      # (the rows may all differ over the whole length)
        pass
    assert short.result.short_path
    with pytest.raises(pkg.FseqError) as e:
        short.match_founders_restored(perm)
    assert e.value.code == pkg.FSEQ_E_ARG
    assert len(short.match_pieces()[0]) == kept["pieces"]
    again = short.match_founders(founders=reduced[:3])
    assert again["pieces"] == kept["pieces"]
    short.close()


@pytest.mark.parametrize("min_len", [0, 7])
def test_cli_against_the_chain_of_tools(build, tmp_path, min_len):
    """founder_sequences --remove-identity-columns --output-founders F --output-restored-matches M against the project's own
    match_founder_sequences on the original rows and F: the same bytes."""
    cli = build.build_cli()
    tools = dict(zip(build.AUX_TOOLS, build.build_aux()))
    m, n = 20, 3000
    msa = founder_mosaic(6, m, n, brec=250, seed=11)
    ident = np.random.default_rng(11).random(n) < 0.6
    msa[:, ident] = msa[0:1, ident]
    ident[-9:] = True
    msa[:, -9:] = ord("N")                                        # the source ends in identity columns
    names = []
    for i, row in enumerate(msa):
        (tmp_path / ("s%02d" % i)).write_bytes(row.tobytes())
        names.append(str(tmp_path / ("s%02d" % i)))
    (tmp_path / "list.txt").write_text("\n".join(names) + "\n")
    r = subprocess.run([cli, "--input", str(tmp_path / "list.txt"), "--remove-identity-columns", "--segment-length-bound", "20", "--segment-joining", "greedy",
                        "--output-founders=" + str(tmp_path / "F"), "--output-restored-matches=" + str(tmp_path / "M"),
                        "--match-min-segment-length", str(min_len)], capture_output=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert b"Matched the input against" in r.stderr and b"0 uncovered cells" in r.stderr
    t = subprocess.run([tools["match_founder_sequences"], "--sequences", str(tmp_path / "list.txt"), "--founders", str(tmp_path / "F"),
                        "--founders-format", "text", "--single-threaded", "--min-segment-length", str(min_len)], capture_output=True, timeout=120)
    assert t.returncode == 0, t.stderr
    got = (tmp_path / "M").read_bytes()
    assert got == t.stdout and got.count(b"\n") > m
    assert got.rstrip(b"\n").rsplit(b"\n", 1)[1].split(b"\t")[2] == str(n).encode()      # the last piece ends at the source's length
