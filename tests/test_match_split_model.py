"""The model of the matcher's split walk (tests/match_split_model.py) proved on its table of cases: for every row the pieces,
sets and counters are match_model.match_row's -- a standing row's from the split walks alone -- and every case's listed
condition holds.  The GPU test (tests/test_gpu_match_rows.py) takes every expected count from the model, so it cannot pass by
falling back everywhere: the mosaics here have no row that does not stand."""
import numpy as np
import pytest

import match_model as mm
import match_split_model as sm


def rows_of(got, m):
    """per row: ([(lb, rb, [founders])], ...) from a split_match result"""
    lists = mm.sets_to_lists(got["sets"])
    out = [[] for _ in range(m)]
    for p, idx in zip(got["pieces"], lists):
        out[int(p["row"])].append((int(p["lb"]), int(p["rb"]), idx))
    return out


@pytest.mark.parametrize("name", list(sm.CASES))
def test_case_is_the_unsplit_walk_and_meets_its_condition(name):
    case = sm.CASES[name]
    rows, founders = case["build"]()
    fb = [bytes(f) for f in founders]
    for min_len in case["min_lens"]:
        got = sm.split_match(rows, founders, min_len, case["G"], case["overlap"])
        print("%s min_len=%d: %s flagged=%s" % (name, min_len, got["split"], got["flagged"]))
        sm.check_expectation(name, got)
        want = [mm.match_row(bytes(r), fb, min_len) for r in rows]
        assert rows_of(got, len(rows)) == [w[0] for w in want]
        assert got["uncovered_cells"] == sum(w[1] for w in want) and got["short_pieces"] == sum(w[2] for w in want)
        assert got["max_pieces_per_row"] == max(len(w[0]) for w in want)
        assert got["split"]["rows_not_standing"] == int((~got["stands"]).sum())
        assert got["split"]["flagged_groups"] == len(got["flagged"]) <= got["split"]["row_groups"]


def test_mosaics_need_the_long_overlap():
    """the same mosaic under overlaps below its longest piece: rows fall out of step (what the check is for)"""
    rows, founders = sm.CASES["mosaic K=70"]["build"]()
    bad = [sm.split_match(rows, founders, 0, 5, ov)["split"]["rows_not_standing"] for ov in (64, 256)]
    print("rows that do not stand at overlap 64, 256:", bad)
    assert bad[0] > bad[1] > 0


@pytest.mark.parametrize("n,G,overlap", [(1, 1, 1), (1, 7, 300), (5, 64, 1), (63, 7, 9), (64, 2, 32), (65, 64, 1), (65, 7, 10 ** 6), (4099, 4097, 1)])
def test_plan_tiles_the_columns(n, G, overlap):
    Ge, ov, c, s = sm.plan(n, G, overlap)
    assert 1 <= Ge <= min(n, sm.SPLIT_MAX, max(G, 1)) and c[0] == 0 and c[-1] == n and s[0] == 0
    assert all(c[g] < c[g + 1] for g in range(Ge))
    assert all(c[g - 1] <= s[g] < c[g] for g in range(1, Ge))
    assert (ov == 0) == (Ge == 1)


@pytest.mark.parametrize("n,G,overlap,min_len", [(1, 3, 1, 0), (5, 64, 1, 0), (63, 7, 9, 1), (64, 2, 32, 37), (65, 64, 1, 0), (65, 7, 100, 66), (331, 7, 5, 7)])
def test_small_shapes_with_planted_cells(n, G, overlap, min_len):
    """closes and uncovered cells at s_g, c_g - 1, c_g, column 0 and n - 1, and mosaics with uncovered cells, at small n"""
    for rows, founders in (sm.planted_case(n, G, overlap), mm.mosaic_case(n + G, 9, n, 5, 4)):
        fb = [bytes(f) for f in founders]
        got = sm.split_match(rows, founders, min_len, G, overlap)
        want = [mm.match_row(bytes(r), fb, min_len) for r in rows]
        assert rows_of(got, len(rows)) == [w[0] for w in want]
        assert got["uncovered_cells"] == sum(w[1] for w in want) and got["short_pieces"] == sum(w[2] for w in want)
        whole = mm.match_rows(rows, founders, min_len)
        assert np.array_equal(got["pieces"], whole["pieces"]) and np.array_equal(got["sets"], whole["sets"])
