"""The folding argument behind fseq_scan_segment_lengths, proven on the model (tests/proto_length_scan.py) against the CPU
oracle: a list built at L0 and folded to L >= L0 is a prefix of the uncut list at L with the header's cumulative count,
`complete` and count of value 0 unchanged -- but for one corner, a list cut short by its capacity of which every entry joined
the lump, which is a lone lump with a lower bound of its count and proves no cell; the oracle's DP step fed folded complete lists gives the oracle's DP entries at L; the
model's "unproven" predicate fires on the overflow case of the GPU table and on no other; K(L) does not fall as L grows."""
import numpy as np
import pytest

import fso
import proto_length_scan as P
from helpers import optimal_max_segment_size

SHAPES = [(3, 12, 400, 0.0), (5, 40, 900, 0.01), (8, 300, 1200, 0.002), (6, 64, 3000, 0.0)]      # founders, m, n, mu


def is_prefix(ent, hdr, full_ent, full_hdr):
    nent = int(hdr[0])
    return nent <= int(full_hdr[0]) and np.array_equal(ent[:nent], full_ent[:nent])


@pytest.mark.parametrize("founders,m,n,mu", SHAPES)
def test_folded_list_is_a_prefix_of_the_uncut_list(founders, m, n, mu):
    msa = P.mosaic(founders, m, n, seed=m + n, mu=mu)
    counts = P.column_counts(msa)
    rng = np.random.default_rng(m)
    checked = moved = lone = 0
    for L0, X in ((1, 3), (4, 7), (9, m), (30, 15)):
        for L in sorted({L0, L0 + 1, L0 + 5, 3 * L0 + 2, 60, 150, n // 2}):
            if L < L0:
                continue
            cols = range(L - 1, n) if n <= 500 else sorted(set(rng.integers(L - 1, n, size=120).tolist()) | {L - 1, L, n - 1})
            for k in cols:
                v, c = counts[k]
                ent, hdr = P.column_list(v, c, k, L0, X)
                fe, fh = P.relump(ent, hdr, k, L)
                full = P.column_list(v, c, k, L, P.UNCUT)
                assert tuple(fh[1:]) == tuple(hdr[1:]), (L0, X, L, k)
                if fh[0] > 1 or fh[2]:
                    assert is_prefix(fe, fh, *full), (L0, X, L, k)
                else:
                    # Every entry of a list that its capacity cut short joined the lump: values >= the new threshold may lie
                    # behind the cut, so the lone lump holds a lower bound of its true count.  Such a list proves no cell: it is
                    # incomplete, offers no candidate, and its cumulative count cannot pass a cell's value, which is at least
                    # the true lump's count.
                    assert fe[0, 0] == full[0][0, 0] and fe[0, 1] <= full[0][0, 1] and not fh[2], (L0, X, L, k)
                    assert P.unproven(fh, full[0][0, 1]), (L0, X, L, k)
                    lone += 1
                assert int(fe[:int(fh[0]), 1].sum()) == int(hdr[3])      # no count is lost
                moved += int(hdr[0]) - int(fh[0])
                checked += 1
    assert checked > 500 and moved > 0


@pytest.mark.parametrize("founders,m,n,mu", SHAPES[1:3])
def test_thresholds_on_both_sides_of_every_entry_value(founders, m, n, mu):
    """For a sampled column, every L with k + 2 - L equal to an entry's value (the entry joins the lump) and one above it (it
    stays)."""
    msa = P.mosaic(founders, m, n, seed=m + n, mu=mu)
    counts = P.column_counts(msa)
    L0, X = 2, m
    for k in (n // 3, n // 2, n - 1):
        v, c = counts[k]
        ent, hdr = P.column_list(v, c, k, L0, X)
        for i in range(1, int(hdr[0])):
            val = int(ent[i, 0])
            for L, joins in ((k + 2 - val, True), (k + 1 - val, False)):
                if L < L0:
                    continue
                fe, fh = P.relump(ent, hdr, k, L)
                assert (int(hdr[0]) - int(fh[0]) >= i) == joins, (k, i, L)
                assert is_prefix(fe, fh, *P.column_list(v, c, k, L, P.UNCUT))


@pytest.mark.parametrize("founders,m,n,mu", SHAPES[:3])
def test_dp_step_on_folded_complete_lists_gives_the_oracles_entries(founders, m, n, mu):
    msa = P.mosaic(founders, m, n, seed=m + n, mu=mu)
    counts = P.column_counts(msa)
    L0 = 3
    for L in (3, 4, 11, 40, n // 4):
        dp = fso.segment_long(msa, L, keep_dp=True, threads=4)["dp"]
        rmq = fso.Rmq(dp["segment_max_size"], debug=False)
        for i in range(63, len(dp), 64):
            rmq.update(i)
        cells = 0
        for k in range(min(2 * L, n - L) - 1, n - L, max(1, (n - 3 * L) // 150)):
            v, c = counts[k]
            ent, hdr = P.relump(*P.column_list(v, c, k, L0, m), k, L)
            assert hdr[2]                                                # X >= m: complete
            av, ac = P.ascending(ent, hdr)
            got = fso.dp_step(av, ac, dp, rmq.h, m, L, 0, k, (0, k + 1, m, m), debug=False)
            t = k + 1 - L
            assert got == (int(dp["lb"][t]), k + 1, int(dp["segment_max_size"][t]), int(dp["segment_size"][t])), (L, k, got)
            cells += 1
        assert cells > 20


@pytest.mark.parametrize("name", sorted(P.CASES))
def test_unproven_predicate_fires_where_the_case_is_listed_for_it(name):
    c = P.CASES[name]
    msa = P.case_msa(name)
    assert msa.shape == (c["m"], c["n"])
    plan, retries = P.simulate_scan(msa, c["lengths"], c["list_cap"])
    rebuilt = [L for L, built, _ in plan[1:] if built]
    assert bool(rebuilt) == c["overflow"], (name, plan)
    if not c["overflow"]:
        assert plan[0][2] >= c["m"] and retries == 0                    # complete lists: nothing can be unproven


def test_max_segment_size_does_not_fall_as_the_length_grows():
    for founders, m, n, seed in ((3, 10, 60, 1), (4, 14, 90, 2), (5, 12, 75, 3)):
        msa = P.mosaic(founders, m, n, seed=seed, mu=0.03, brec=12)
        sizes = [optimal_max_segment_size(msa, L) for L in range(1, n // 2 + 1)]
        assert sizes == sorted(sizes), (seed, sizes)
        for L in (1, 2, 5, n // 4, n // 2):
            assert int(fso.segment_long(msa, L, threads=1)["max_segment_size"]) == sizes[L - 1]
