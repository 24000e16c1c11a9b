"""CPU proof of pass 2's chain step by runs (tests/proto_pass2_runs.py) against the step by stable sort and against the
oracle's pBWT state at the boundary."""
import numpy as np
import pytest

from oracle import fso
import proto_pass2_runs as pp


def _states(msa, cols):
    """The oracle's (a, d) in front of every column of `cols` (ascending)."""
    p = fso.Pbwt(msa)
    out = {}
    for k in cols:
        while p.idx < k:
            p.step()
        out[k] = (p.a.astype(np.int64), p.d.astype(np.int64))
    return out


def _check_block(msa, k0, bounds, caps):
    """Every boundary of `bounds` (columns inside the block that starts at k0) from the block's state; returns the runs of each."""
    st = _states(msa, [k0] + list(bounds))
    a0, d0 = st[k0]
    runs = []
    for c in bounds:
        ra, rd = st[c]
        key, headd = pp.block_classes(msa, k0, c, rd[0])
        sa, sd = pp.chain_step_sorted(a0, d0, key, headd)
        assert np.array_equal(sa, ra) and np.array_equal(sd, rd), (k0, c)
        R = len(pp.run_starts(a0, key))
        for cap in caps(R):
            a1, d1, r, by_runs = pp.chain_step_runs(a0, d0, key, headd, cap)
            assert r == R and by_runs == (cap != 0 and R <= cap), (k0, c, cap)
            assert np.array_equal(a1, ra) and np.array_equal(d1, rd), (k0, c, cap)
        runs.append((R, len(headd)))
    return runs


def _edges(R):
    return sorted({0, 1, max(R - 1, 0), R, R + 1, 1 << 30})


@pytest.mark.parametrize("m,n,K,Brec,mu,seed,kind,k0,bounds", [
    (203, 900, 6, 300, 3e-3, 41, 0, 630, (631, 650, 730, 842)),       # m no multiple of 64
    (320, 700, 12, 200, 2e-3, 42, 0, 420, (421, 470, 599)),
    (150, 500, 5, 100, 5e-3, 43, 1, 310, (320, 399)),                     # sigma = 16
])
def test_founder_mosaics(m, n, K, Brec, mu, seed, kind, k0, bounds):
    """Blocks with no recombination boundary of the founders at their start or inside."""
    msa = fso.synth_msa(fso.synth_spec(seed, K, Brec, mu, kind), m, n)
    runs = _check_block(msa, k0, [b for b in bounds if b < n], _edges)
    # a pBWT order: the runs are few -- about two a class
    for R, D in runs:
        assert R <= 3 * D + 8, runs


def test_founders_boundary_inside_the_block():
    """Recombination every 150 columns, the block starts at 100: in front of column 150 the runs are few, behind it the rows of
    a class lie all over the old order."""
    m, n = 400, 400
    msa = fso.synth_msa(fso.synth_spec(44, 16, 150, 1e-3, 0), m, n)
    runs = _check_block(msa, 100, (120, 150, 151, 180, 199), _edges)
    assert runs[0][0] <= 3 * runs[0][1] + 8, runs
    assert runs[-1][0] > m // 2, runs


def test_all_rows_distinct():
    """Random rows: every row a class of its own after a few columns, every position a run (runs = m)."""
    rng = np.random.default_rng(45)
    m, n = 257, 120
    msa = np.asfortranarray(rng.integers(0, 4, size=(m, n)).astype(np.uint8) + ord("A"))
    runs = _check_block(msa, 40, (41, 44, 70, 119), _edges)
    assert runs[-1] == (m, m), runs


def test_one_class():
    """All rows equal: one class, one run; the state is the block's."""
    m, n = 130, 90
    msa = np.asfortranarray(np.tile(np.frombuffer(b"ACGT" * 30, dtype=np.uint8)[:n], (m, 1)))
    runs = _check_block(msa, 30, (31, 60, 89), _edges)
    assert all(r == (1, 1) for r in runs), runs
