"""The cases of tests/reduced_capacity_cases.py have the properties they are there for (CPU, oracle only).

For every row of the table: block 6 = [600, 700) has exactly R representatives and blocks 0 to 5 have R - 1 (distinct rows,
and the oracle's pBWT: rows with a divergence >= 1 behind the block); the oracle's segmentation is the one boundary at column
687 with R - 1 rows on either side, inside block 6 and behind a stride state of phase C; the lists of block 6 hold dozens of
values below the threshold and the one at column 686 is open at the default capacity; the row count keeps the block below
70 % of the rows.  The table itself covers both sides of every capacity of both families, and its hand-written
configurations agree with the hand-written thresholds.  A case that fails a condition is a defect of the table."""
import numpy as np
import pytest

import fso
import reduced_capacity_cases as rcc


def distinct(types, lo, hi):
    """Distinct rows over the columns [lo, hi)."""
    part = np.ascontiguousarray(types[:, lo:hi])
    return len(np.unique(part.view(np.dtype((np.void, hi - lo)))))


@pytest.mark.parametrize("name", list(rcc.CASES))
def test_case_has_exactly_R_representatives_and_one_boundary_in_block_6(name):
    case = rcc.CASES[name]
    R, m = case.R, case.m
    n, L, B, c = rcc.N, rcc.L, rcc.BLOCK, rcc.C
    rows, types, src = rcc.make(case, with_types=True)
    assert rows.shape == (m, n) and types.shape == (R, n) and np.array_equal(rows, types[src])
    assert len(np.unique(types)) == len(rcc.SYMS[case.bits]) == {2: 4, 4: 16, 8: 40}[case.bits]
    # every type is there, so distinct rows are distinct types: counted on the R types, not on the m rows
    assert np.array_equal(np.unique(src), np.arange(R))
    # the geometry: block 6 is the last exact block, every legal boundary lies strictly inside it, the task starts at 672
    b0, b1 = rcc.BLOCK_UNDER_TEST * B, (rcc.BLOCK_UNDER_TEST + 1) * B
    assert b0 + 2 <= L < b1 + 2 and b0 < L and n - L < b1 and n < 3 * L
    for stride in (16, 32):                                   # phase C's reduced stride states: LDS-resident rows, streamed rows
        assert (c - 1) // stride * stride == 672 > b0
    assert distinct(types, 0, b0) == R - 1 and distinct(types, 0, b1) == R
    assert distinct(types, 0, c) == R - 1 and distinct(types, c, n) == R - 1
    # (a wider range never has fewer distinct rows: a cut in front of 687 has R rows on its right, one behind it R on its left)
    assert distinct(types, 0, c + 1) == R and distinct(types, c - 1, n) == R
    # the share of the rows
    assert 10 * R <= 7 * m or case.on_all_rows
    if case.least_rows:
        assert m % 50 == 0 and 0 <= m - -(-10 * R // 7) < 50
        assert (m >= rcc.STREAMED_FROM) == (R > 7884)
    else:
        assert m == 1000 and R in (700, 701) and (10 * R > 7 * m) == case.on_all_rows
    # the oracle: one boundary, at 687
    ref = fso.segment_long(rows, L, threads=8)
    assert ref["status"] == 0 and ref["max_segment_size"] == R - 1
    for res in (ref["traceback"], ref["reduced"]):
        assert res["lb"].tolist() == [0, c] and res["rb"].tolist() == [c, n] and res["segment_size"].tolist() == [R - 1, R - 1]
    assert c % B != 0 and c // B == rcc.BLOCK_UNDER_TEST
    # the oracle's pBWT: the representatives of an exact block are the rows with a divergence >= 1 behind it; the lists
    p = fso.Pbwt(rows, debug=False)
    below = {}
    for k in range(b1):
        p.step()
        if k + 1 in (b0, b1):
            assert int((p.d >= 1).sum()) == (R - 1 if k + 1 == b0 else R), k + 1
        if k in (640, c - 1):
            v, cnt = p.counts()
            under = v < k + 2 - L
            below[k] = (int(under.sum()), int(cnt[under].sum()))
    assert 34 <= below[640][0] <= 40, below
    assert 65 <= below[c - 1][0] <= 81 and below[c - 1][0] > rcc.DEFAULT_LIST_CAP, below
    ev, ec = rcc.expected_list(v, cnt, c - 1, L)
    assert len(ev) == below[c - 1][0] + 1 and ec[1:].sum() == below[c - 1][1] and ec.sum() == m and ev[0] == c


def test_the_cases_cover_what_they_claim():
    """Both sides of every capacity of either family, at 2 bits; the subset at 4 and 8 bits; the 70 % edge; the hand-written
    configurations of every row are what the hand-written thresholds give; every case runs in exactly one child."""
    capacities = sorted({most for most, _, _ in rcc.PHASE_C} | {most for most, _, _ in rcc.PASS_2})
    assert capacities == [192, 320, 448, 576, 768, 960, 1280, 2240, 2560, 3136, 3584, 4800, 5120, 6720, 7168, 7680, 8640, 9216, 9600, 10240,
                          10560, 11264]
    assert [R for R, _, _, _ in rcc.TABLE_2_BITS] == [R for cap in capacities for R in (cap, cap + 1)]
    assert [R for R, _, _, _ in rcc.TABLE_WIDER_SYMBOLS] == [448, 449, 2240, 2241, 6720, 6721, 8640, 8641]
    assert [(R, m) for R, m, _, _ in rcc.TABLE_SHARE] == [(700, 1000), (701, 1000)]
    # the capacities are the configurations' rows: T x E, (T - 64) x E with a list wave
    assert [most for most, T, E in rcc.PHASE_C] == [min(rcc.rows_of(T, E, T > 64), rcc.RED_CAP) for _, T, E in rcc.PHASE_C]
    assert [most for most, T, E in rcc.PASS_2] == [rcc.rows_of(T, E, False) for _, T, E in rcc.PASS_2]
    assert rcc.phase_c_of(rcc.RED_CAP) == (1024, 12, 11520) and rcc.phase_c_of(rcc.RED_CAP + 1) is None
    for case in rcc.CASES.values():
        if case.on_all_rows:
            assert case.R == rcc.RED_CAP + 1 or 10 * case.R > 7 * case.m, case
            # (pass 2 sweeps the representatives of a block wherever the plan counted them: up to its cap)
            assert case.pass_2 == (None if case.R > rcc.RED_CAP else rcc.pass_2_of(case.R)[:2]), case
            assert rcc.phase_c_of(case.R - 1) is not None and 10 * (case.R - 1) <= 7 * case.m, case       # blocks 0 to 5 stay reduced
        else:
            assert rcc.phase_c_of(case.R)[:2] == case.phase_c and rcc.pass_2_of(case.R)[:2] == case.pass_2, case
    # every configuration of either family runs at its capacity and the next one at the capacity + 1, in phase C and in pass 2
    at = {(c.bits, c.R): c for c in rcc.CASES.values() if c.least_rows}
    for family, attr in ((rcc.PHASE_C, "phase_c"), (rcc.PASS_2, "pass_2")):
        for i, (most, T, E) in enumerate(family):
            assert getattr(at[2, most], attr) == (T, E), (attr, most)
            after = family[i + 1][1:] if i + 1 < len(family) else None
            assert getattr(at[2, most + 1], attr) == after, (attr, most)
    for bits in (4, 8):
        for R in (448, 449, 2240, 2241, 6720, 6721, 8640, 8641):
            assert (at[bits, R].m, at[bits, R].phase_c, at[bits, R].pass_2) == (at[2, R].m, at[2, R].phase_c, at[2, R].pass_2)
    grouped = [name for names in rcc.GROUPS.values() for name in names]
    assert sorted(grouped) == sorted(rcc.CASES) and len(rcc.GROUPS) <= 12
    for names in rcc.GROUPS.values():
        assert sum(rcc.CASES[x].m for x in names) * rcc.N <= 4 * 16100 * rcc.N
