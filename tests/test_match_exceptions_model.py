"""The merged walk of tests/match_exceptions_model.py (kept columns, exception columns, the closed-form gap) against the
definition: match_model.match_row on the full-length query and the full-length restored founders, which tests/test_match_abi.py
pins to the host tool.  Plain Python on small cases; the GPU test plants the same patterns at its own sizes."""
import numpy as np
import pytest

import identity_model as im
import match_exceptions_model as xm
import match_model as mm

MIN_LENS = [0, 1, 3, 50]


@pytest.fixture(scope="module")
def cases():
    return {name: xm.small_case(name) for name in xm.CASES}


def test_the_table_lists_every_pattern():
    listed = set().union(*(c["listed"] for c in xm.CASES.values()))
    assert listed == set(xm.PATTERNS)
    assert {c["q"] for c in xm.CASES.values()} >= {1, 3} and {c["tile"] for c in xm.CASES.values()} == {51, 64}


@pytest.mark.parametrize("name", list(xm.CASES))
def test_every_case_has_what_it_is_listed_for(cases, name):
    c, d = xm.CASES[name], cases[name]
    assert np.array_equal(im.identity_mask(d["msa"]), d["mask"])      # identity columns among the reconstruction's rows, exactly
    assert len(d["kept"]) == c["n_kept"] and d["queries"].shape == (c["q"], len(d["mask"]))
    xm.check_planted(d["queries"], d["msa"][0], d["mask"], d["where"], c["listed"], c["tile"])
    if "min_len_larger" in c["listed"]:
        assert xm.largest_gap(d["mask"]) < max(MIN_LENS)
    else:
        assert xm.largest_gap(d["mask"]) > 2 * max(MIN_LENS)
    if "foreign" in c["listed"]:
        r, cols, cells = d["where"]["foreign"][0]
        assert d["queries"][r, cols[0]] == 0x7E == d["queries"][r, d["kept"][cells[0]]]


@pytest.mark.parametrize("min_len", MIN_LENS)
@pytest.mark.parametrize("name", list(xm.CASES))
def test_the_merged_walk_is_the_definition(cases, name, min_len):
    d = cases[name]
    mask, kept, row0 = d["mask"], d["kept"], d["msa"][0]
    full = im.restore(d["founders"], mask, row0)
    exc = xm.exceptions_of(d["queries"], mask, row0)
    closes_around = 0
    for r, q in enumerate(d["queries"]):
        want = mm.match_row(q.tolist(), full.tolist(), min_len)
        got = xm.match_row_merged(q[kept].tolist(), d["founders"].tolist(), kept, exc[r], len(mask), min_len)
        assert got == want, (name, r, min_len)
        for e in exc[r].tolist():                                      # an exception cell: uncovered, a one-column piece without founders
            if e + 1 < len(mask):
                assert (e, e + 1, []) in want[0]
        for row, cols, _ in d["where"].get("min_len_gap", []):
            if row == r and min_len in (3, 50):                        # a close of min_len columns on either side, inside the gap
                e = cols[0]
                lo, hi = int(kept[xm.G - 1]), int(kept[xm.G])
                before = [p for p in want[0] if lo < p[1] <= e and p[1] - p[0] == min_len]
                after = [p for p in want[0] if p[0] == e + 1 and p[1] < hi and p[1] - p[0] == min_len]
                closes_around += bool(before and after)
    if "min_len_gap" in xm.CASES[name]["listed"] and min_len in (3, 50):
        assert closes_around
    # the same through match_model.match_rows, the form the GPU test compares with
    both = mm.match_rows(d["queries"], full, min_len)
    assert both["uncovered_cells"] == sum(mm.match_row(q.tolist(), full.tolist(), min_len)[1] for q in d["queries"])


def test_a_match_in_reduced_coordinates_is_not_this_match(cases):
    """what the issue rests on: the exception cells are invisible to a walk over the kept columns alone"""
    d = cases["rows"]
    mask, kept, row0 = d["mask"], d["kept"], d["msa"][0]
    r = d["where"]["every"][0][0]
    q = d["queries"][r]
    with_exc = xm.match_row_merged(q[kept].tolist(), d["founders"].tolist(), kept, xm.exceptions_of(d["queries"], mask, row0)[r], len(mask), 0)
    without = xm.match_row_merged(q[kept].tolist(), d["founders"].tolist(), kept, [], len(mask), 0)
    assert with_exc[1] >= int(mask.sum()) > without[1]
