"""k_join_score and k_join_score_founders (csrc/fseq_joinscore.hpp) on constructed class arrays, through fseq_debug_join_score and
the launcher fseq_join_score uses, against the model's counting on the same arrays (tests/join_score_model.py, score_from_labels):
rows on both sides of a wave and of a workgroup's stride (1,024 threads), slot counts from 1 to the cap, a table of one entry,
keys that share a home entry and run round the table's end, keys of rows that no slot has and of slots that no row has, gaps on
either side, many workgroups, and the smallest and largest class ids."""
import importlib

import numpy as np
import pytest

import join_score_model as jm

pytestmark = pytest.mark.gpu
GAP16 = 0xFFFF


@pytest.fixture(scope="module")
def pkg():
    return importlib.import_module("founder-sequences_amd")


def check(pkg, of, left, right):
    """the device's score of (of, left, right) against the model's; returns the device's"""
    of, left, right = np.asarray(of), np.asarray(left), np.asarray(right)
    got = pkg.debug_join_score(of, left, right)
    as_label = lambda x: np.where(x == GAP16, jm.GAP, x.astype(np.int64))
    want = jm.score_from_labels(of, as_label(left), as_label(right))
    assert jm.same_score(got, want) is None, jm.same_score(got, want)
    j = got["junctions"]
    assert np.all(j["supported"] + j["unsupported"] + j["gaps"] == left.shape[1]) and np.all(j["rows_through"] <= of.shape[1])
    assert not j["rb"].any()
    return got


def random_case(rng, m, X, S, row_classes, slot_classes, gaps=0.1):
    of = rng.integers(0, row_classes, size=(S, m)).astype(np.uint16)
    left = rng.integers(0, slot_classes, size=(S - 1, X)).astype(np.uint16)
    right = rng.integers(0, slot_classes, size=(S - 1, X)).astype(np.uint16)
    left[rng.random(left.shape) < gaps] = GAP16
    right[rng.random(right.shape) < gaps] = GAP16
    return of, left, right


@pytest.mark.parametrize("m", [1, 63, 64, 65, 1023, 1025, 4099])
def test_rows_on_both_sides_of_a_wave_and_of_the_stride(pkg, m):
    # (12 classes a side among the rows, 14 among the slots: some slots' keys have no row)
    check(pkg, *random_case(np.random.default_rng(m), m, 65, 3, 12, 14))


@pytest.mark.parametrize("X", [1, 2, 64, 65, 4095, 4096])
def test_slot_counts_up_to_the_cap(pkg, X):
    # (90 x 90 pairs of classes: at X = 4,096 about 3,200 distinct keys in a table of 8,192 entries)
    check(pkg, *random_case(np.random.default_rng(X), 1025, X, 3, 90, 90, gaps=0.02))


@pytest.mark.parametrize("X", [1, 65, 4096])
def test_every_slot_with_the_same_key(pkg, X):
    rng = np.random.default_rng(X)
    of = rng.integers(0, 3, size=(2, 700)).astype(np.uint16)
    got = check(pkg, of, np.full((1, X), 2, dtype=np.uint16), np.full((1, X), 1, dtype=np.uint16))
    rows = int(np.count_nonzero((of[0] == 2) & (of[1] == 1)))
    assert rows > 0 and np.all(got["support"] == rows) and got["junctions"]["rows_through"][0] == rows and got["junctions"]["weight"][0] == rows * X


@pytest.mark.parametrize("X,home", [(300, 1021), (300, 0), (40, 127)])
def test_keys_that_share_a_home_entry(pkg, X, home):
    """X distinct keys with one home entry: a probe chain of X entries, from entry 1,021 of 1,024 (127 of 128) round the table's end.
    The rows carry these keys and as many others, some of which probe through the whole chain without a match."""
    l, r = jm.colliding_keys(X, home, classes=1024)
    rng = np.random.default_rng(X + home)
    order = rng.permutation(X)
    pick = rng.integers(0, X, size=3000)
    of = np.stack([l[pick], r[pick]]).astype(np.uint16)
    others = rng.random(3000) < 0.5
    of[0, others] = rng.integers(0, 1024, size=int(others.sum()))
    got = check(pkg, of, l[order][None, :].astype(np.uint16), r[order][None, :].astype(np.uint16))
    assert got["junctions"]["supported"][0] > X // 2


def test_keys_with_equal_low_bits(pkg):
    """4,096 slots whose keys differ in the left class alone (the low 16 bits of every key are equal), and rows with left classes
    beyond the slots'."""
    rng = np.random.default_rng(5)
    of = np.stack([rng.integers(0, 5000, size=4099), np.full(4099, 5)]).astype(np.uint16)
    of[1, ::7] = 6
    left = rng.permutation(4096).astype(np.uint16)[None, :]
    check(pkg, of, left, np.full((1, 4096), 5, dtype=np.uint16))


def test_keys_of_rows_in_no_slot_and_of_slots_in_no_row(pkg):
    of = np.array([[0, 0, 1, 1, 2, 2, 3], [0, 1, 0, 1, 0, 1, 3]], dtype=np.uint16)
    # slots: (0, 0) one row; (2, 1) one row; (3, 0) the classes exist, the pair does not; (9, 9) classes no row has; (1, 1) twice
    left = np.array([[0, 2, 3, 9, 1, 1]], dtype=np.uint16)
    right = np.array([[0, 1, 0, 9, 1, 1]], dtype=np.uint16)
    got = check(pkg, of, left, right)
    assert got["support"].tolist() == [[1, 1, 0, 0, 1, 1]] and got["breaks"].tolist() == [0, 0, 1, 1, 0, 0]
    assert got["junctions"]["rows_through"][0] == 3 and got["junctions"]["weight"][0] == 4      # (rows (0, 1), (1, 0), (2, 0), (3, 3) are in no slot)


def test_gaps_on_either_side(pkg):
    of = np.zeros((3, 100), dtype=np.uint16)
    left = np.array([[GAP16, 0, GAP16, 0], [0, 0, 0, 0]], dtype=np.uint16)
    right = np.array([[0, GAP16, GAP16, 0], [0, 0, 0, GAP16]], dtype=np.uint16)
    got = check(pkg, of, left, right)
    assert got["junctions"]["gaps"].tolist() == [3, 1] and got["support"].tolist() == [[0, 0, 0, 100], [100, 100, 100, 0]]
    assert not got["breaks"].any()                               # (a gap is no break)
    every = check(pkg, of, np.full((2, 4), GAP16, dtype=np.uint16), np.zeros((2, 4), dtype=np.uint16))
    assert every["summary"]["gaps"] == 8 and every["summary"]["rows_through"] == 0 and every["summary"]["min_rows_through"] == 0


@pytest.mark.parametrize("S", [2, 300])
def test_two_segments_and_many_workgroups(pkg, S):
    got = check(pkg, *random_case(np.random.default_rng(S), 333, 17, S, 6, 7))
    assert len(got["junctions"]) == S - 1 and got["summary"]["junctions"] == S - 1
    assert got["summary"]["max_breaks"] == got["breaks"].max() <= S - 1


def test_class_ids_0_and_0xfffe(pkg):
    rng = np.random.default_rng(9)
    of = rng.choice(np.array([0, 0xFFFE], dtype=np.uint16), size=(3, 1025))
    left = rng.choice(np.array([0, 0xFFFE, 77, GAP16], dtype=np.uint16), size=(2, 65))
    right = rng.choice(np.array([0, 0xFFFE, 77, GAP16], dtype=np.uint16), size=(2, 65))
    left[0, :4], right[0, :4] = [0xFFFE, 0xFFFE, 0, 0], [0xFFFE, 0, 0xFFFE, 0]      # (0xFFFE << 16 | 0xFFFE: the key next to the empty word)
    got = check(pkg, of, left, right)
    assert got["junctions"]["rows_through"][0] == 1025


def test_optional_outputs(pkg):
    of, left, right = random_case(np.random.default_rng(1), 200, 9, 4, 5, 5)
    full = pkg.debug_join_score(of, left, right)
    slim = pkg.debug_join_score(of, left, right, want_support=False)
    assert slim["support"] is None and np.array_equal(slim["junctions"], full["junctions"]) and np.array_equal(slim["breaks"], full["breaks"])
    lib = pkg.load_library()
    assert lib.fseq_debug_join_score(0, 200, 9, 4, of.ctypes.data, left.ctypes.data, right.ctypes.data, None, None, None, None) == pkg.FSEQ_OK
