"""The packed local pass of phase C's partition step on the device (csrc/fseq_localpass.hpp through fseq_debug_local_pass): one
workgroup of 64 and of 512 threads, 11, 12 and 15 rows a thread, against a numpy restatement of the plain pass, bit for bit --
the rows' new values (0 for an unused position) and the four tail maxima of every thread.

Every thread of a workgroup is a case of its own: the named ones first (one symbol only, each symbol absent, alternating symbols,
one to fourteen trailing unused positions, all values equal, strictly falling, strictly rising, no row), seeded random threads
behind them.  Values reach 0xFFFF: bit 15 is what no alignment of the suite sets."""
import importlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def pkg():
    importlib.import_module("founder-sequences_amd.build").build()
    return importlib.import_module("founder-sequences_amd")


def plain_pass(d, s):
    """partition_step's plain local pass, all threads at once: (dnew [T][E], tails [T][4])."""
    T, E = d.shape
    run = np.zeros((T, 4), dtype=np.uint32)
    dnew = np.zeros((T, E), dtype=np.uint32)
    for e in range(E):
        r = np.maximum(run, d[:, e:e + 1])
        own = s[:, e:e + 1] == np.arange(4, dtype=np.uint32)[None, :]
        dnew[:, e] = np.where(own, r, 0).max(axis=1)
        run = np.where(own, 0, r).astype(np.uint32)
    return dnew, run


def named_threads(E, rng):
    """[(d, s)] of the named cases for E rows a thread."""
    falling = (0xFFFF - 97 * np.arange(E)).astype(np.uint32)
    rising = (0x7FF8 + np.arange(E)).astype(np.uint32)           # through bit 15
    equal = np.full(E, 0x8000, dtype=np.uint32)
    out = []
    for vals in (falling, rising, equal, rng.integers(0, 1 << 16, size=E).astype(np.uint32)):
        for x in range(4):
            out.append((vals, np.full(E, x)))                                        # one symbol only
            three = np.arange(E) % 3
            out.append((vals, three + (three >= x)))                                 # symbol x absent
            for y in range(4):
                if y != x:
                    out.append((vals, np.where(np.arange(E) & 1, y, x)))             # alternating
        for tail in range(1, min(14, E - 1) + 1):                                    # trailing unused positions
            s = rng.integers(0, 4, size=E)
            v = vals.copy()
            s[E - tail:] = 4
            v[E - tail:] = 0
            out.append((v, s))
        out.append((vals, np.arange(E) & 3))
    out.append((np.zeros(E, dtype=np.uint32), np.full(E, 4)))                        # no row at all
    return out


def workgroup(T, E, seed):
    rng = np.random.default_rng(seed)
    edge = np.array([0, 1, 0x7FFF, 0x8000, 0xFFFE, 0xFFFF], dtype=np.uint32)
    d = rng.integers(0, 1 << 16, size=(T, E)).astype(np.uint32)
    d[1::3] = edge[rng.integers(0, 6, size=d[1::3].shape)]                           # a third of the threads: edge values only
    d[2::3] = rng.integers(0, 5, size=d[2::3].shape)                                 # a third: small values, many ties
    s = rng.integers(0, 4, size=(T, E)).astype(np.uint32)
    named = named_threads(E, rng)
    # 64 threads hold a slice of the named cases that moves with the seed, 512 all of them
    first = 0 if T >= len(named) else (seed * 64) % len(named)
    for t, (v, sy) in enumerate((named + named)[first:first + min(T, len(named))]):
        d[t], s[t] = v, sy
    return d, s


@pytest.mark.parametrize("E", [11, 12, 15])
@pytest.mark.parametrize("T", [64, 512])
def test_device_pass_is_the_plain_pass(pkg, T, E):
    seeds = (0,) if T == 512 else (0, 1, 2, 3)          # (64 threads: four workgroups walk through the named cases)
    for seed in seeds:
        d, s = workgroup(T, E, seed)
        want_new, want_tails = plain_pass(d, s)
        got_new, got_tails = pkg.local_pass_packed(d, s)
        assert np.array_equal(got_new, want_new), (T, E, seed, np.argwhere(got_new != want_new)[:4])
        assert np.array_equal(got_tails, want_tails), (T, E, seed, np.argwhere(got_tails != want_tails)[:4])


def test_refuses_what_the_kernels_never_pass(pkg):
    d = np.zeros((64, 11), dtype=np.uint32)
    s = np.zeros((64, 11), dtype=np.uint32)
    for bad_d, bad_s in ((0x10000, 0), (0, 5), (7, 4)):
        dd, ss = d.copy(), s.copy()
        dd[3, 2], ss[3, 2] = bad_d, bad_s
        with pytest.raises(pkg.FseqError):
            pkg.local_pass_packed(dd, ss)
    with pytest.raises(pkg.FseqError):
        pkg.local_pass_packed(np.zeros((64, 13), dtype=np.uint32), np.zeros((64, 13), dtype=np.uint32))
