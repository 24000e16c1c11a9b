"""CPU checks of tests/dp_list_cases.py, the table tests/test_gpu_dp_lists.py runs on the device: the host validator of the debug
entry takes every case and refuses one broken variant per rule; every case asks what it is listed for (the model's per-cell
measurements); a case compared by arrays has no unproven cell; and the model on uncut lists from real alignments is the oracle's own
DP, field for field."""
import importlib

import numpy as np
import pytest

import dp_list_cases as D
import fso
import proto_length_scan as P


@pytest.fixture(scope="module")
def pkg():
    build = importlib.import_module("founder-sequences_amd.build")
    build.build()
    return importlib.import_module("founder-sequences_amd")


@pytest.mark.parametrize("name", list(D.CASES))
def test_case_is_valid_and_asks_what_it_is_listed_for(pkg, name):
    c = D.CASES[name]
    X, ent, hdr = D.device_lists(name)
    assert ent.shape == (c["n"], D.stride_of(X), 2) and X <= 261 and c["n"] <= 20000
    assert pkg.dp_lists_check(c["m"], c["L"], ent, hdr) is None
    asked = D.asks(name)                               # (the model runs under the oracle's debug build: its asserts take the lists)
    assert all(ok for ok, _ in asked.values()), asked
    if D.compared_by_arrays(name):
        assert D.expect_unproven(name) == 0
    else:
        assert D.expect_unproven(name) == 1
    if c["cuts"]:
        S = D.schedule(c["L"], c["n"])
        assert all(0 < a < b < S["nrounds"] for a, b in zip(c["cuts"], c["cuts"][1:]))


def test_table_covers_the_listed_paths():
    keys = set()
    for c in D.CASES.values():
        keys |= set(c["listed_for"])
    assert keys >= {"needed", "ties_across", "full_lists", "inside", "deep_far", "pair_far", "mixed", "level_ring", "level_mem", "on_border", "hot",
                    "rounds_mod", "block_on_round_end", "cut_residues", "cut_blocks", "cut_single", "cut_drain", "cut_final", "steps", "deciding",
                    "unproven", "takes_w"}
    assert {D.CASES[n]["listed_for"]["needed"] for n in D.CASES if n.startswith("strips_")} >= {32, 33, 63, 64, 65, 127, 128, 129, 250}
    assert {D.CASES[n]["L"] for n in D.CASES if n.startswith("edge_L")} == {1, 2, 55, 56, 57, 95, 96, 97, 192}
    assert any(D.CASES[n]["L"] < 96 for n in D.CASES if n.startswith("resume_")) and any(D.CASES[n]["L"] >= 96 for n in D.CASES if n.startswith("resume_"))


def _broken_variants(ent, hdr, k, m):
    """(rule, ent, hdr): one broken variant and more per rule of fseq_debug_dp_lists_check, at column k, whose list is complete, has
    at least four entries and ends in value 0."""
    ne = int(hdr[k, 0])
    assert ne >= 4 and ent[k, ne - 1, 0] == 0 and hdr[k, 2] == 1 and ent[k, 0, 1] > 0
    out = []

    def variant(rule, f):
        e, h = ent.copy(), hdr.copy()
        f(e, h)
        out.append((rule, e, h))

    def put(arr, idx, value):
        arr[idx] = value

    def without_zero(e, h):                            # the list without its value-0 entry: incomplete, and valid
        h[k, 0] = ne - 1
        h[k, 3] = int(h[k, 3]) - int(e[k, ne - 1, 1])
        h[k, 2] = 0

    def lump_plus(e, h, d):
        e[k, 0, 1] = int(e[k, 0, 1]) + d
        h[k, 3] = int(h[k, 3]) + d

    variant(None, without_zero)
    variant(1, lambda e, h: put(h, (k, 0), 0))
    variant(1, lambda e, h: put(h, (k, 0), ent.shape[1] + 1))
    variant(2, lambda e, h: put(e, (k, 0, 0), k + 2))
    variant(2, lambda e, h: put(e, (k, 0, 0), k))
    variant(3, lambda e, h: put(e, (k, 2, 0), e[k, 1, 0]))                            # equal values
    variant(3, lambda e, h: put(e, (k, 1, 0), e[k, 2, 0] - 1))                        # ascending
    variant(3, lambda e, h: put(e, (k, ne - 2, 0), 0))                                # value 0 twice: not in the last place alone
    variant(4, lambda e, h: put(h, (k, 1), h[k, 1] + 1))                              # the header's count of value 0 is not the entry's
    variant(4, lambda e, h: (lump_plus(e, h, -1), put(h, (k, 2), 0)))                 # value 0 last on an incomplete list
    variant(4, lambda e, h: (without_zero(e, h), lump_plus(e, h, int(ent[k, ne - 1, 1])), put(h, (k, 2), 1)))   # complete, no value 0, cnt0 > 0
    variant(5, lambda e, h: put(e, (k, 1, 1), 0))
    variant(5, lambda e, h: (without_zero(e, h), put(e, (k, ne - 2, 1), 0)))
    variant(6, lambda e, h: put(h, (k, 3), h[k, 3] - 1))
    variant(6, lambda e, h: (without_zero(e, h), lump_plus(e, h, m)))                 # the sum beyond m
    variant(7, lambda e, h: put(h, (k, 2), 0))
    variant(7, lambda e, h: put(h, (k, 2), 2))
    variant(7, lambda e, h: (without_zero(e, h), put(h, (k, 2), 1)))                  # complete by its flag only
    variant(7, lambda e, h: (without_zero(e, h), put(h, (k, 1), m + 1)))              # a count of value 0 beyond m
    return out


def test_validator_refuses_every_broken_rule(pkg):
    name = "strips_65"
    c = D.CASES[name]
    _, ent, hdr = D.device_lists(name)
    m, n, L = c["m"], c["n"], c["L"]
    cells = [k for k in P.cell_columns(n, L) if hdr[k, 0] >= 4]
    assert cells[-1] == n - 1 or hdr[n - 1, 0] < 4
    seen = set()
    for k in (cells[0], cells[len(cells) // 2], cells[-1]):
        for rule, e, h in _broken_variants(ent, hdr, k, m):
            got = pkg.dp_lists_check(m, L, e, h)
            assert got == (None if rule is None else (k, rule)), (rule, k, got)
            seen.add(rule)
    assert seen == {None, 1, 2, 3, 4, 5, 6, 7}
    # a column no cell reads may hold anything; the shapes are rule 0
    e, h = ent.copy(), hdr.copy()
    h[0] = 0
    h[n - L] = 0xFFFFFFFF
    assert pkg.dp_lists_check(m, L, e, h) is None
    assert pkg.dp_lists_check(m, n, e, h) == (-1, 0)                                  # n < 2L
    assert pkg.dp_lists_check(0, L, e, h) == (-1, 0)
    assert pkg.dp_lists_check(m, 0, e, h) == (-1, 0)


@pytest.mark.parametrize("shape", [dict(founders=6, m=60, n=3000, seed=11, mu=0.0, L=20), dict(founders=24, m=150, n=3000, seed=5, mu=0.02, L=100)])
def test_model_on_uncut_lists_is_the_oracles_dp(pkg, shape):
    """The lists of a real alignment, uncut, through the model: fso.segment_long's DP array, field for field, over the entries a cell
    writes."""
    msa = P.mosaic(shape["founders"], shape["m"], shape["n"], shape["seed"], mu=shape["mu"])
    m, n, L = shape["m"], shape["n"], shape["L"]
    counts = P.column_counts(msa)
    lists = [P.column_list(v, c, k, L, P.UNCUT) for k, (v, c) in enumerate(counts)]
    stride = max(len(e) for e, _ in lists)
    ent = np.zeros((n, stride, 2), dtype=np.uint32)
    hdr = np.zeros((n, 4), dtype=np.uint32)
    for k, (e, h) in enumerate(lists):
        ent[k, :len(e)] = e
        hdr[k] = h
    assert pkg.dp_lists_check(m, L, ent, hdr) is None
    LB, M, SZ = D.model(m, n, L, ent, hdr, debug=True)
    dp = fso.segment_long(msa, L, keep_dp=True)["dp"]
    w = D.written_entries(n, L)
    assert np.array_equal(LB[w], dp["lb"][w].astype(np.uint32))
    assert np.array_equal(M[w], dp["segment_max_size"][w])
    assert np.array_equal(SZ[w], dp["segment_size"][w])
    assert np.array_equal(dp["rb"][w], np.where(w == n - L, n, w + L))
    assert not len(D.unproven_cells(m, n, L, hdr, M))
