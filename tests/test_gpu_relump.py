"""k_relump_lists (csrc/fseq_lengthscan.hpp) on constructed lists, through fseq_debug_relump_lists: every word of the entry and
header arrays against the model (tests/proto_length_scan.py relump) -- the entries behind a list's new end and the three header
words the kernel leaves alone included.  A constructed column k holds `nent` entries of which exactly E join the lump at L_to."""
import importlib

import numpy as np
import pytest

import proto_length_scan as P

pytestmark = pytest.mark.gpu

L_FROM, L_TO, K0 = 4, 304, 2000


@pytest.fixture(scope="module")
def pkg():
    return importlib.import_module("founder-sequences_amd")


def make_column(k, nent, E, stride, rng, zero_tail=False, L_from=L_FROM, L_to=L_TO):
    """A list of nent entries at L_from whose entries 1 .. E have values >= k + 2 - L_to; garbage behind the list."""
    thr_from, thr_to = max(0, k + 2 - L_from), max(0, k + 2 - L_to)
    assert 0 <= E <= nent - 1 and nent <= stride and thr_to + E - 1 < thr_from and (E == nent - 1 or thr_to >= nent)
    ent = rng.integers(1, 1 << 30, size=(stride, 2)).astype(np.uint32)
    ent[0] = (k + 1, rng.integers(0, 50))
    for i in range(1, nent):
        ent[i, 0] = thr_to + (E - i) if i <= E else thr_to - (i - E)
    ent[1:nent, 1] = rng.integers(1, 9, size=nent - 1)
    cnt0 = 0
    if zero_tail:
        assert nent >= 2 and (E < nent - 1 or thr_to == 0)
        ent[nent - 1, 0] = 0
        cnt0 = int(ent[nent - 1, 1])
    cum = int(ent[:nent, 1].sum())
    return ent, np.array([nent, cnt0, int(rng.integers(0, 2)), cum], dtype=np.uint32)


def launch_and_compare(pkg, cols, k0, L_from, L_to):
    ent = np.stack([c[0] for c in cols])
    hdr = np.stack([c[1] for c in cols])
    got_ent, got_hdr = pkg.relump_lists(ent, hdr, k0, L_from, L_to)
    for j, (e, h) in enumerate(cols):
        want_ent, want_hdr = P.relump(e, h, k0 + j, L_to)
        assert np.array_equal(got_hdr[j], want_hdr), (j, got_hdr[j], want_hdr)
        assert np.array_equal(got_ent[j], want_ent), (j, int(h[0]))
    return got_ent, got_hdr


@pytest.mark.parametrize("stride", [256, 202])
def test_every_size_and_shift_across_strip_borders(pkg, stride):
    """Lists of 1, 2, 64, 65, 66, 128, 129, 130 and 200 entries with E = 0, 1, 63, 64, 65 and nent - 1 (only the lump is left):
    the shift crosses the borders of the 64-entry strips in both the reads and the writes."""
    rng = np.random.default_rng(stride)
    shapes = [(nent, E) for nent in (1, 2, 64, 65, 66, 128, 129, 130, 200) for E in sorted({0, 1, 63, 64, 65, nent - 1}) if E <= nent - 1]
    cols = [make_column(K0 + j, nent, E, stride, rng) for j, (nent, E) in enumerate(shapes)]
    _, hdr = launch_and_compare(pkg, cols, K0, L_FROM, L_TO)
    assert [int(h[0]) for h in hdr] == [nent - E for nent, E in shapes]


@pytest.mark.parametrize("ncols", [1, 3, 4, 5, 9])
def test_columns_per_launch(pkg, ncols):
    """Fewer columns than a workgroup has waves, exactly as many, one more, and more than two workgroups' worth."""
    rng = np.random.default_rng(ncols)
    cols = [make_column(K0 + j, 70 + j, 1 + (7 * j) % 60, 128, rng) for j in range(ncols)]
    launch_and_compare(pkg, cols, K0, L_FROM, L_TO)


def test_trailing_zero_entry(pkg):
    """The entry of value 0 stays where the threshold is positive and joins the lump where it is 0 (k + 2 <= L_to)."""
    rng = np.random.default_rng(3)
    cols = [make_column(K0 + j, nent, E, 128, rng, zero_tail=True) for j, (nent, E) in enumerate([(2, 0), (10, 3), (65, 63), (66, 64)])]
    ent, hdr = launch_and_compare(pkg, cols, K0, L_FROM, L_TO)
    assert all(ent[j, hdr[j, 0] - 1, 0] == 0 for j in range(len(cols)))
    # columns 40 .. 43 with L_to = 100: the threshold is 0, every entry joins the lump, the zero entry among them
    low = [make_column(40 + j, nent, nent - 1, 64, rng, zero_tail=True, L_from=1, L_to=100) for j, nent in enumerate([2, 5, 30, 41])]
    ent, hdr = launch_and_compare(pkg, low, 40, 1, 100)
    assert all(int(h[0]) == 1 for h in hdr)
    assert [int(ent[j, 0, 1]) for j in range(4)] == [int(c[0][:int(c[1][0]), 1].sum()) for c in low]


def test_same_length_changes_nothing(pkg):
    rng = np.random.default_rng(4)
    cols = [make_column(K0 + j, 20 + 50 * j, 0, 256, rng, L_to=L_FROM) for j in range(4)]
    ent, hdr = launch_and_compare(pkg, cols, K0, L_FROM, L_FROM)
    assert np.array_equal(ent, np.stack([c[0] for c in cols])) and np.array_equal(hdr, np.stack([c[1] for c in cols]))
