"""The split of the restored match walk (tests/match_restored_split_model.py, the specification of k_match_walk_split's
restored forms) against the definition: match_model.match_rows on the full-length data, the queries against
identity_model.restore(founders, mask, row 0).  For every case and min_len the pieces, sets and counters are the definition's,
and the case meets what it is listed for -- so a device run that equals the model cannot pass by falling back everywhere.  No GPU."""
import numpy as np
import pytest

import identity_model as im
import match_exceptions_model as xm
import match_model as mm
import match_restored_split_model as rsm


@pytest.fixture(scope="module")
def built():
    made = {}

    def get(name):
        if name not in made:
            made[name] = rsm.CASES[name]["build"]()
        return made[name]
    return get


@pytest.mark.parametrize("min_len", rsm.MIN_LENS)
@pytest.mark.parametrize("name", list(rsm.CASES))
def test_the_split_walk_is_the_definition(built, name, min_len):
    case, d = rsm.CASES[name], built(name)
    got = rsm.split_match(d["queries"], d["founders"], d["mask"], d["row0"], min_len, case["G"], case["overlap"])
    want = mm.match_rows(d["queries"], im.restore(d["founders"], d["mask"], d["row0"]), min_len)
    print("%s min_len=%d: %s pieces=%d uncovered=%d short=%d" % (name, min_len, got["split"], len(got["pieces"]), got["uncovered_cells"], got["short_pieces"]))
    assert np.array_equal(got["pieces"], want["pieces"]) and np.array_equal(got["sets"], want["sets"])
    for f in ("uncovered_cells", "short_pieces", "max_pieces_per_row"):
        assert got[f] == want[f], f
    rsm.check_expectation(name, got, min_len)


def test_every_segment_alone_is_the_definition_where_it_stands(built):
    """not through split_match's choice: the closes every single cold walk keeps are the definition's closes at the source
    positions the segment owns, for the rows that stand up to that segment"""
    name = "planted"
    case, d = rsm.CASES[name], built(name)
    T = rsm._Tables(d["queries"], d["founders"], d["mask"], d["row0"])
    G, _, c, s = rsm.plan(T.n_kept, case["G"], case["overlap"])
    for min_len in rsm.MIN_LENS:
        want = mm.match_rows(d["queries"], im.restore(d["founders"], d["mask"], d["row0"]), min_len)["pieces"]
        walks = [rsm.cold_walk(T, min_len, s[g], c[g], c[g + 1], g > 0) for g in range(G)]
        ok = np.ones(T.m, dtype=bool)
        for g in range(G):
            if g:
                ok &= walks[g]["head"] == walks[g - 1]["tail"]
            P_lo = 0 if g == 0 else int(T.kept[c[g]])
            P_hi = T.n_src if g == G - 1 else int(T.kept[c[g + 1]])
            rb = want["rb"].astype(np.int64)
            owned = (rb >= P_lo) & ((rb < P_hi) | (g == G - 1)) & ok[want["row"]]
            w = walks[g]
            keep = ok[w["rows"]]
            order = np.lexsort((w["rb"][keep], w["lb"][keep], w["rows"][keep]))
            assert np.array_equal(w["rows"][keep][order], want["row"][owned]) and np.array_equal(w["rb"][keep][order], rb[owned])
            assert np.array_equal(w["lb"][keep][order], want["lb"][owned].astype(np.int64))
        assert ok.all()


def test_the_table_covers_what_the_cases_are_listed_for(built):
    names = set(rsm.CASES)
    assert {"periodic", "mixed groups", "long piece", "G = n_kept", "planted"} <= names
    expects = [c["expect"] for c in rsm.CASES.values()]
    assert "all stand" in expects and "none stands" in expects and "some" in expects and [1] in expects and [0] in expects
    Ks, rows = set(), set()
    for name, case in rsm.CASES.items():
        d = built(name)
        mask, queries, row0 = d["mask"], d["queries"], d["row0"]
        kept = np.flatnonzero(~mask)
        G, ov, c, s = rsm.plan(len(kept), case["G"], case["overlap"])
        Ks.add(len(d["founders"]))
        rows.add(len(queries))
        assert np.array_equal(im.identity_mask(im.restore(d["founders"], mask, row0)), mask), name
        if name != "G = n_kept":
            assert 2000 <= len(kept) <= 4100 and 40 <= len(queries) <= 600 and 2 <= G <= 8 and 256 <= ov <= 700, name
            assert mask[0] and mask[-1]                             # a leading and a trailing gap
            for j in c[1:-1] + s[1:]:                               # long gaps in front of and behind every bound and cold start
                assert j > 0 and kept[j] - kept[j - 1] > 2 * max(rsm.MIN_LENS) and kept[j + 1] - kept[j] > 2 * max(rsm.MIN_LENS), (name, j)
        else:
            assert len(kept) == 70 and (G, ov) == (70, 1)
        assert len(mask) < 2 ** 15
    assert Ks >= {5, 40, 70, 200, 300} and {257, 600} <= rows
    # the planted rows: what each is listed for is in it
    for name in ("planted", "planted last"):
        case, d = rsm.CASES[name], built(name)
        mask, kept = d["mask"], np.flatnonzero(~d["mask"])
        G, _, c, s = rsm.plan(len(kept), case["G"], case["overlap"])
        g = G - 1 if name == "planted last" else G // 2
        exc = xm.exceptions_of(d["queries"], mask, d["row0"])
        w = d["where"]
        assert len(exc[w["none"]]) == 0 and len(exc[w["every"]]) == int(mask.sum())
        assert exc[w["exc c_g-1"]].tolist() == [kept[c[g]] - 1] and exc[w["exc c_g+1"]].tolist() == [kept[c[g]] + 1]
        assert exc[w["exc s_g-1"]].tolist() == [kept[s[g]] - 1] and exc[w["exc s_g+1"]].tolist() == [kept[s[g]] + 1]
        assert exc[w["run across P_g"]].tolist() == [kept[c[g]] + x for x in (-2, -1, 1, 2)]
        assert exc[w["ends"]].tolist() == [0, len(mask) - 1]
        restored = im.restore(d["founders"], mask, d["row0"])
        for r, cells in ((w["uncovered c_g-1"], [c[g] - 1]), (w["uncovered c_g-1 c_g"], [c[g] - 1, c[g]])):
            assert [k for k in kept.tolist() if not (restored[:, k] == d["queries"][r, k]).any()] == [int(kept[j]) for j in cells]
        # the close behind the uncovered cell lies in front of P_g: it is segment g - 1's
        got = rsm.split_match(d["queries"], d["founders"], mask, d["row0"], 0, case["G"], case["overlap"])
        mine = got["pieces"][got["pieces"]["row"] == w["uncovered c_g-1"]]
        assert int(kept[c[g] - 1]) + 1 in mine["rb"].tolist() and int(kept[c[g] - 1]) + 1 < kept[c[g]]
