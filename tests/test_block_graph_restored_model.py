"""tests/block_graph_restored_model.py on the CPU: the graph of the full-length rows over the restored bounds has the classes, ids,
edges and row_nodes of the graph of the reduced rows over the reduced bounds (so fseq_block_graph and the L and P lines need no
restored form); its file spells the full-length rows; the restored threading of a query without exception cells is the reduced
threading of its kept columns; and every case the GPU tests run reaches what it is listed for."""
import numpy as np
import pytest

import block_graph_model as gm
import block_graph_restored_model as rm
import graph_thread_model as tm
import identity_model as im

WIDTHS = [1, 63, 64, 65, 129]


def same_graph(full, R, lb, rb):
    want = gm.block_graph_model(R, lb, rb)
    got, src_lb, src_rb = rm.restored_graph(full, lb, rb)
    assert np.array_equal(got["count"], want["count"]) and np.array_equal(got["row_nodes"], want["row_nodes"])
    assert np.array_equal(got["edges"], want["edges"])
    for f in ("segment", "cls", "rep_row", "rows"):
        assert np.array_equal(got["nodes"][f], want["nodes"][f]), f
    assert int(src_lb[0]) == 0 and int(src_rb[-1]) == full.shape[1] and np.array_equal(src_lb[1:], src_rb[:-1])
    return got, want


@pytest.mark.parametrize("W", WIDTHS)
def test_label_cases(W):
    full, R, kept, L = rm.label_case(W)
    mask, kept_again = rm.kept_of(full)
    assert np.array_equal(kept, kept_again) and np.array_equal(full[:, kept], R)        # the planted runs are the identity columns, all of them
    lb, rb = rm.blocks(6, W)
    got, want = same_graph(full, R, lb, rb)
    for gap in (b"-", None, b"A"):
        blob = rm.expected_gfa(full, lb, rb, paths=True, gap=gap)
        gm.check_file_spells_rows(blob, full, gap)
        reduced = gm.gfa_bytes(R, want, paths=True, gap=gap)
        keep = lambda b: [x for x in b.split(b"\n") if not x.startswith(b"S\t")]
        assert keep(blob) == keep(reduced)                                              # the header, the L and the P lines
    have = rm.reaches(full, lb, rb)
    listed = {"identity in front of kept[0]", "identity behind kept[n-1]", "run=1", "run=64", "run=130", "strip without a kept column",
              "kept column on lane 0", "kept column on lane 63", "row 0 is a gap in an identity column", "empty label", "S=6", "range=%d" % (W + 2)}
    if W >= 64:
        listed.add("strip of 64 kept columns")
    assert listed <= have, sorted(listed - have)
    assert b"\t*\tLN:i:0\t" in rm.expected_gfa(full, lb, rb)


def test_the_widths_reach_every_listed_range():
    """source ranges of 1, 63, 64, 65 and 129 positions: a segment of W kept columns with no identity column of its own.  Block 5
    of label_case has its end run, block 0 its front run; the plain one is made here."""
    for W in WIDTHS:
        R, _ = rm.gapped(W, b"ACGT", W)
        full, kept = rm.with_runs(R, {0: b"AC-", 6 * W: b"G"})
        lb, rb = rm.blocks(6, W)
        same_graph(full, R, lb, rb)
        assert "range=%d" % W in rm.reaches(full, lb, rb)


@pytest.mark.parametrize("S", [1, 2])
def test_few_segments(S):
    R, _ = rm.mosaic(3, 9, S, 40, seed=2)
    full, kept = rm.with_runs(R, {0: b"AC-G", 17: b"T" * 70, S * 40: b"-A"})
    lb, rb = rm.blocks(S, 40)
    same_graph(full, R, lb, rb)
    gm.check_file_spells_rows(rm.expected_gfa(full, lb, rb, paths=True), full)
    assert "S=%d" % S in rm.reaches(full, lb, rb)


@pytest.mark.parametrize("alphabet,sigma", [(b"ACG", 4), (b"ACGT", 5), (bytes(range(48, 88)), 41)])
def test_code_widths(alphabet, sigma):
    full, R, kept, L = rm.label_case(65, alphabet, seed=sigma)
    assert len(np.unique(full)) == sigma and len(np.unique(R)) == sigma                 # (with the gap: 2, 4 and 8 bits a code)
    same_graph(full, R, *rm.blocks(6, 65))


@pytest.mark.parametrize("X", [181, 182])
def test_class_counts(X):
    R, _ = rm.mosaic(X, 2 * X + 3, 4, 30, seed=X)
    full, kept = rm.with_runs(R, {0: b"ACGT-", 45: rm.run_bytes(70, b"ACGT"), 120: b"AC-"})
    lb, rb = rm.blocks(4, 30)
    same_graph(full, R, lb, rb)
    assert "classes=%d" % X in rm.reaches(full, lb, rb)


# ---- threading

def test_threading_without_exception_cells_is_the_reduced_threading():
    full, R, founders, kept, W = rm.thread_rows()
    S = tm.MOSAIC[2]
    lb, rb = rm.blocks(S, W)
    reduced_queries = tm.mosaic_queries(founders, S, W, 40, 3)
    queries = rm.expand(reduced_queries, full, kept)
    assert all(len(c) == 0 for c in rm.exception_cells(queries, full))
    got, want = rm.expected_threading(full, lb, rb, queries), tm.thread_model(R, lb, rb, reduced_queries)
    for f in ("nodes", "steps", "per_segment"):
        assert np.array_equal(got[f], want[f]), f
    for f in ("segments_matched", "junctions_linked", "junctions_novel", "walks", "longest_walk_segments"):
        assert np.array_equal(got["per_row"][f], want["per_row"][f]), f
    assert got["summary"] == want["summary"] and got["summary"]["junctions_novel"] > 0
    # the columns are the source's
    src = rm.restored_graph(full, lb, rb)
    widths = (src[2] - src[1]).astype(np.int64)
    for q in range(len(queries)):
        assert int(got["per_row"]["columns_matched"][q]) == int(widths[got["nodes"][:, q] != tm.NONE].sum())


def test_own_rows_thread_to_their_nodes():
    full, R, founders, kept, W = rm.thread_rows()
    lb, rb = rm.blocks(tm.MOSAIC[2], W)
    got = rm.expected_threading(full, lb, rb, full)
    assert np.array_equal(got["nodes"], got["graph"]["row_nodes"]) and got["summary"]["rows_on_graph"] == len(full)
    assert (got["per_row"]["columns_matched"] == full.shape[1]).all()


def test_one_exception_cell_unmatches_its_segment_alone():
    full, R, founders, kept, W = rm.thread_rows()
    S = tm.MOSAIC[2]
    lb, rb = rm.blocks(S, W)
    _, src_lb, src_rb = rm.restored_graph(full, lb, rb)
    mask = im.identity_mask(full)
    assert mask[0] and mask[-1] and all(mask[int(x) - 1] for x in src_rb) and not any(mask[int(x)] for x in src_lb[1:])
    base = rm.expected_threading(full, lb, rb, full[5:6])
    for s, cell in [(0, 0), (S - 1, full.shape[1] - 1), (2, int(src_rb[2]) - 1), (0, int(src_lb[0])), (3, int(src_rb[3]) - 1)]:
        q = rm.plant(full[5], full, cell)
        got = rm.expected_threading(full, lb, rb, q[None, :])
        assert [x for x in range(S) if got["nodes"][x, 0] != base["nodes"][x, 0]] == [s] and got["nodes"][s, 0] == tm.NONE
        lost = [p for p in range(S - 1) if got["steps"][p, 0] != base["steps"][p, 0]]
        assert lost == [p for p in (s - 1, s) if 0 <= p < S - 1] and all(got["steps"][p, 0] == tm.NONE for p in lost)
    # chunks of 64 source columns: identity columns on both sides of the border at 64, and behind the one at 128
    assert mask[63] and mask[64] and mask[128] and full.shape[1] > 130


def test_a_cell_in_every_segment_and_bytes_outside_the_alphabet():
    full, R, founders, kept, W = rm.thread_rows()
    S = tm.MOSAIC[2]
    lb, rb = rm.blocks(S, W)
    _, src_lb, src_rb = rm.restored_graph(full, lb, rb)
    q = full[7].copy()
    for s in range(S):
        q = rm.plant(q, full, int(src_rb[s]) - 1)
    got = rm.expected_threading(full, lb, rb, q[None, :])
    assert (got["nodes"] == tm.NONE).all() and got["summary"]["walks"] == 0
    outside_identity = rm.plant(full[7], full, int(src_rb[1]) - 1, byte=ord("N"))
    outside_kept = full[7].copy()
    outside_kept[int(kept[3 * W + 2])] = ord("N")
    got = rm.expected_threading(full, lb, rb, np.stack([outside_identity, outside_kept]))
    assert got["nodes"][1, 0] == tm.NONE and (np.delete(got["nodes"][:, 0], 1) != tm.NONE).all()
    assert got["nodes"][3, 1] == tm.NONE and (np.delete(got["nodes"][:, 1], 3) != tm.NONE).all()
