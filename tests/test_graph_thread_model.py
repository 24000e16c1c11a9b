"""tests/graph_thread_model.py, the yardstick of the graph threading's GPU tests, on the CPU: the alignment's own rows thread to
row_nodes, mosaics of the founders recombine as no row does, one cell unmatches one segment, and every case the GPU tests run
reaches what it is listed for.  The segments are the oracle's (oracle/fseq_oracle.c)."""
import numpy as np
import pytest

import fso
import block_graph_model as gm
import graph_thread_model as tm
from helpers import optimal_max_segment_size

_mosaic = {}


def mosaic():
    """(msa, founders, lb, rb, graph) of the mosaic alignment: computed once, shared, never written to."""
    if not _mosaic:
        X, m, S, W, seed = tm.MOSAIC
        msa, founders = tm.full_mosaic(X, m, S, W, seed)
        res = fso.segment_long(np.ascontiguousarray(msa), W, debug=True)
        assert res["status"] == 0
        lb, rb = res["reduced"]["lb"], res["reduced"]["rb"]
        assert lb.tolist() == [b * W for b in range(S)] and rb.tolist() == [(b + 1) * W for b in range(S)]
        assert res["reduced"]["segment_size"].tolist() == [X] * S
        graph = gm.block_graph_model(msa, lb, rb)
        msa.setflags(write=False)
        _mosaic.update(msa=msa, founders=founders, lb=lb, rb=rb, graph=graph)
    return _mosaic


def test_the_generator_is_the_block_graph_tests():
    """Draw for draw: the same alignment as tests/test_gpu_block_graph.py's full_mosaic, and the optimum the issue names."""
    X, m, S, W, seed = tm.MOSAIC
    rng = np.random.default_rng(seed)
    alpha = np.frombuffer(b"ACGT", dtype=np.uint8)
    founders = alpha[rng.integers(0, 4, size=(X, S * W))]
    want = np.empty((m, S * W), dtype=np.uint8)
    for b in range(S):
        pick = rng.permutation(np.concatenate([np.arange(X), rng.integers(0, X, size=m - X)]))
        want[:, b * W:(b + 1) * W] = founders[pick, b * W:(b + 1) * W]
    msa, got_founders = tm.full_mosaic(X, m, S, W, seed)
    assert np.array_equal(msa, want) and np.array_equal(got_founders, founders)
    assert optimal_max_segment_size(msa, W) == X


def test_own_rows_thread_to_row_nodes():
    c = mosaic()
    msa, S = c["msa"], len(c["lb"])
    t = tm.thread_model(msa, c["lb"], c["rb"], msa, graph=c["graph"])
    assert np.array_equal(t["nodes"], c["graph"]["row_nodes"])
    assert (t["steps"] != tm.NONE).all()
    edges = c["graph"]["edges"]
    assert np.array_equal(edges["from"][t["steps"]], t["nodes"][:-1]) and np.array_equal(edges["to"][t["steps"]], t["nodes"][1:])
    pr = t["per_row"]
    assert (pr["walks"] == 1).all() and (pr["longest_walk_segments"] == S).all() and (pr["junctions_linked"] == S - 1).all()
    assert (pr["junctions_novel"] == 0).all() and (pr["columns_matched"] == msa.shape[1]).all() and (pr["longest_walk_columns"] == msa.shape[1]).all()
    assert (t["per_segment"]["matched"] == len(msa)).all() and t["per_segment"]["linked"].tolist() == [len(msa)] * (S - 1) + [0]
    assert t["summary"]["rows_on_graph"] == len(msa) and t["summary"]["walks"] == len(msa)


def test_mosaic_queries_recombine_as_no_row_does():
    c = mosaic()
    msa, W, queries, listed = tm.case("mosaic")
    assert listed == {"novel"} and queries.shape == (40, msa.shape[1])
    t = tm.thread_model(msa, c["lb"], c["rb"], queries, graph=c["graph"])
    sm = t["summary"]
    print("novel", sm["junctions_novel"], "linked", sm["junctions_linked"], "edges", len(c["graph"]["edges"]), "of", 5 * 5 * 5)
    assert (t["nodes"] != tm.NONE).all() and sm["segments_matched"] == 40 * 6
    assert sm["junctions_novel"] > 0 and sm["junctions_linked"] > 0 and sm["junctions_novel"] + sm["junctions_linked"] == 40 * 5
    # a novel junction ends a walk: the walks of a row are its novel junctions + 1, and the longest is the longest run of linked ones
    assert (t["per_row"]["walks"] == t["per_row"]["junctions_novel"] + 1).all()
    assert sm["rows_on_graph"] == int((t["per_row"]["junctions_novel"] == 0).sum())
    assert t["per_segment"]["novel"].sum() == sm["junctions_novel"] and t["per_segment"]["novel"][-1] == 0


def test_one_cell_unmatches_its_segment():
    c = mosaic()
    for name in ("outside", "substituted"):
        msa, W, queries, listed = tm.case(name)
        t = tm.thread_model(msa, c["lb"], c["rb"], queries, graph=c["graph"])
        unmatched = {(int(s), int(q)) for s, q in np.argwhere(t["nodes"] == tm.NONE)}
        want = {(2, 0), (4, 1)} if name == "outside" else {(3, 0), (0, 2), (5, 3)}
        assert unmatched == want, (name, unmatched)
        # the junctions on both sides of an unmatched segment are neither linked nor novel
        for s, q in unmatched:
            assert all(t["steps"][p, q] == tm.NONE for p in (s - 1, s) if 0 <= p < 5)
        assert t["summary"]["junctions_novel"] == 0
        row = t["per_row"][0]
        if name == "outside":
            assert (row["walks"], row["longest_walk_segments"], row["segments_matched"], row["junctions_linked"]) == (2, 3, 5, 3)
            assert (row["columns_matched"], row["longest_walk_columns"]) == (5 * W, 3 * W)
            assert t["per_row"][2]["walks"] == 1 and t["summary"]["rows_on_graph"] == 1


def test_hand_made_walks():
    """Three segments of one column, rows AAA, ABA, BBB: the edges are A-A, A-B, B-A, B-B on the left and A-A, B-A, B-B on the
    right; AAB matches everywhere and its second junction (A, B) is no row's."""
    msa = np.array([list(b"AAA"), list(b"ABA"), list(b"BBB")], dtype=np.uint8)
    lb, rb = np.array([0, 1, 2]), np.array([1, 2, 3])
    q = np.array([list(b"AAB"), list(b"BAA"), list(b"ACA"), list(b"CCC"), list(b"BBB")], dtype=np.uint8)
    t = tm.thread_model(msa, lb, rb, q)
    pr = t["per_row"]
    assert pr["junctions_novel"].tolist() == [1, 1, 0, 0, 0] and pr["junctions_linked"].tolist() == [1, 1, 0, 0, 2]
    assert pr["walks"].tolist() == [2, 2, 2, 0, 1] and pr["longest_walk_segments"].tolist() == [2, 2, 1, 0, 3]
    assert pr["segments_matched"].tolist() == [3, 3, 2, 0, 3] and t["summary"]["rows_on_graph"] == 1
    assert t["per_segment"]["matched"].tolist() == [4, 3, 4] and t["per_segment"]["novel"].tolist() == [1, 1, 0]
    assert tm.table(t).count(b"\n") == 1 + 5 + 1 and tm.table(t).endswith(b"\tROWS_ON_GRAPH=1\n")


@pytest.mark.parametrize("name", tm.CASES)
def test_listed_cases_reach_what_they_are_listed_for(name):
    c = mosaic()
    msa, W, queries, listed = tm.case(name)
    assert np.array_equal(msa, c["msa"]) and W == tm.MOSAIC[3]
    t = tm.thread_model(msa, c["lb"], c["rb"], queries, graph=c["graph"])
    alphabet = set(np.unique(msa).tolist())
    reached = set()
    if t["summary"]["junctions_novel"]:
        reached.add("novel")
    if (t["nodes"] == tm.NONE).any():
        reached.add("unmatched")
    if any(int(b) not in alphabet for b in np.unique(queries)):
        reached.add("outside")
    assert reached == listed, (name, reached)
