"""tests/graph_nearest_model.py, the yardstick of the nearest-node GPU tests, on the CPU: with max_distance = 0 it is
tests/graph_thread_model.py's threading on every case that model lists; the alignment's own rows are at distance 0 from one class
of every segment; a substitution costs exactly one; k bytes outside the alphabet cost at least k; the admitted cells grow with
max_distance and are all cells from the longest segment on.  The segments are the oracle's (oracle/fseq_oracle.c)."""
import numpy as np
import pytest

import graph_nearest_model as nm
import graph_thread_model as tm
from test_graph_thread_model import mosaic


def same_threading(got, want):
    for what in ("nodes", "steps", "per_row", "per_segment"):
        assert got[what].dtype == want[what].dtype and np.array_equal(got[what], want[what]), what
    assert got["summary"] == want["summary"]


@pytest.mark.parametrize("name", tm.CASES)
def test_at_distance_0_the_model_is_the_threading(name):
    c = mosaic()
    msa, W, queries, listed = tm.case(name)
    near = nm.nearest_model(msa, c["lb"], c["rb"], queries, 0, graph=c["graph"])
    want = tm.thread_model(msa, c["lb"], c["rb"], queries, graph=c["graph"])
    want.pop("graph")
    same_threading(nm.as_threading(near), want)
    assert (near["ties"] >= 1).all() and (near["nodes"] != nm.NONE).all()
    assert (near["per_row"]["segments_exact"] == near["per_row"]["segments_admitted"]).all() and (near["per_row"]["mismatches_admitted"] == 0).all()
    assert ("unmatched" in listed) == bool((near["distances"] > 0).any())


def test_own_rows_are_at_distance_0_from_one_class():
    c = mosaic()
    msa, S = c["msa"], len(c["lb"])
    near = nm.nearest_model(msa, c["lb"], c["rb"], msa, 0, graph=c["graph"])
    assert (near["distances"] == 0).all() and (near["ties"] == 1).all()
    assert np.array_equal(near["nodes"], c["graph"]["row_nodes"])
    assert near["summary"]["rows_on_graph"] == len(msa) and near["summary"]["mismatches"] == 0 and near["summary"]["segments_exact"] == len(msa) * S
    assert (near["per_segment"]["max_distance"] == 0).all() and (near["per_segment"]["exact"] == len(msa)).all()


def test_a_substitution_costs_exactly_one():
    c = mosaic()
    msa, W, queries, listed = tm.case("substituted")
    near = nm.nearest_model(msa, c["lb"], c["rb"], queries, 0, graph=c["graph"])
    want = np.zeros((6, 4), dtype=np.uint32)
    want[3, 0] = want[0, 2] = want[5, 3] = 1                    # (segment, query) of tm.case("substituted")'s three substitutions
    assert np.array_equal(near["distances"], want)
    assert near["per_row"]["mismatches"].tolist() == [1, 0, 1, 1] and near["per_row"]["max_distance"].tolist() == [1, 0, 1, 1]
    # forgiven at max_distance = 1: each row is admitted everywhere, and the node of the substituted segment is the row's own
    one = nm.nearest_model(msa, c["lb"], c["rb"], queries, 1, graph=c["graph"])
    assert (one["per_row"]["segments_admitted"] == 6).all() and one["per_row"]["segments_exact"].tolist() == [5, 6, 5, 5]
    assert one["per_row"]["mismatches_admitted"].tolist() == [1, 0, 1, 1]
    for q, row in enumerate((7, 7, 11, 20)):
        own = c["graph"]["row_nodes"][:, row]
        if (one["ties"][:, q] == 1).all():
            assert np.array_equal(one["nodes"][:, q], own) and one["per_row"][q]["walks"] == 1


def test_bytes_outside_the_alphabet_cost_at_least_their_number():
    c = mosaic()
    msa, W = c["msa"], tm.MOSAIC[3]
    q = msa[[2, 9, 4, 5]].copy()
    q[0, 2 * W] = ord("N")
    q[1, 4 * W:4 * W + 3] = ord("-")
    q[3, 5 * W:6 * W] = ord("n")                               # a whole segment: its width from every class, every class tied
    outside = ~np.isin(q, np.frombuffer(b"ACGT", dtype=np.uint8))
    near = nm.nearest_model(msa, c["lb"], c["rb"], q, 0, graph=c["graph"])
    for s in range(6):
        k = outside[:, s * W:(s + 1) * W].sum(1)
        assert (near["distances"][s] >= k).all()
    assert near["distances"][2, 0] == 1 and near["distances"][4, 1] == 3 and near["distances"][5, 3] == W
    assert near["ties"][5, 3] == 5 and near["nodes"][5, 3] == c["graph"]["nodes"]["segment"].tolist().index(5)


def test_admitted_cells_grow_with_the_distance_allowed():
    c = mosaic()
    msa, W, queries, listed = tm.case("mixed")
    rng = np.random.default_rng(8)
    queries = queries.copy()
    for q in range(0, len(queries), 3):                         # a few rows with several substitutions in one segment
        queries[q, rng.integers(0, 2 * W, size=4)] = ord("A")
    longest = int((c["rb"] - c["lb"]).max())
    before = None
    for D in (0, 1, 2, 3, longest - 1, longest, 2 ** 32 - 1):
        near = nm.nearest_model(msa, c["lb"], c["rb"], queries, D, graph=c["graph"])
        admitted = near["distances"] <= D
        assert near["summary"]["segments_admitted"] == int(admitted.sum())
        assert np.array_equal(near["per_segment"]["admitted"], admitted.sum(1))
        if before is not None:
            assert (admitted | ~before).all()                   # monotone
            assert np.array_equal(near["distances"], first["distances"]) and np.array_equal(near["nodes"], first["nodes"]) and np.array_equal(near["ties"], first["ties"])
        else:
            first = near
        if D >= longest:
            assert admitted.all() and (near["per_row"]["columns_admitted"] == msa.shape[1]).all()
            assert (near["per_row"]["mismatches_admitted"] == near["per_row"]["mismatches"]).all()
        before = admitted
    assert first["summary"]["segments_admitted"] < before.size and (first["distances"] > 1).any()


def test_hand_made_distances_and_table():
    """Segments of widths 2 and 1, rows AAx, ABy, BBy: AB is one from AA and from BB (a tie of two, the smaller class wins) and 0
    from AB."""
    msa = np.array([list(b"AAx"), list(b"ABy"), list(b"BBy")], dtype=np.uint8)
    lb, rb = np.array([0, 2]), np.array([2, 3])
    q = np.array([list(b"BAx"), list(b"ABz"), list(b"CCy")], dtype=np.uint8)
    near = nm.nearest_model(msa, lb, rb, q, 1)
    assert near["distances"].tolist() == [[1, 0, 2], [0, 1, 0]] and near["ties"].tolist() == [[2, 1, 3], [1, 2, 1]]
    assert near["nodes"].tolist() == [[0, 1, 0], [3, 3, 4]]
    assert near["per_row"]["segments_admitted"].tolist() == [2, 2, 1] and near["per_row"]["segments_exact"].tolist() == [1, 1, 1]
    assert near["per_row"]["junctions_linked"].tolist() == [1, 0, 0] and near["per_row"]["junctions_novel"].tolist() == [0, 1, 0]
    assert near["per_row"]["max_distance"].tolist() == [1, 1, 2] and near["summary"]["mismatches"] == 4
    t = nm.table(near, 1)
    assert t.count(b"\n") == 1 + 3 + 1 and t.startswith(nm.TABLE_HEADER) and b"#\tMAX_DISTANCE_ALLOWED=1\tROWS=3\tSEGMENTS=2\t" in t and t.endswith(b"\tMISMATCHES=4\n")
