"""tests/block_graph_model.py, the yardstick of the block graph's GPU tests, on the CPU: its class numbering against the rule the
boundary states imply (oracle/fseq_oracle.c's states, oracle/join_oracle.py's classes), the graph's own invariants, the file's
properties and the formatter's lengths."""
import numpy as np
import pytest

import fso
import join_oracle as jo
import block_graph_model as gm
from helpers import founder_mosaic

# m, n, L, founders, recombination block, mutation rate, seed
CASES = [(8, 600, 10, 3, 100, 5e-3, 0x5EED0001), (24, 400, 7, 4, 60, 1e-2, 11), (70, 500, 9, 6, 45, 8e-3, 21), (200, 900, 15, 6, 150, 3e-3, 31)]
_cases = {}


def segmented(case):
    """(msa with planted gaps, oracle result, the model's graph) of a case: computed once, shared, never written to."""
    if case not in _cases:
        m, n, L, K, brec, mu, seed = case
        msa = np.array(fso.synth_msa(fso.synth_spec(seed, K, brec, mu), m, n))
        rng = np.random.default_rng(seed)
        msa[rng.random(msa.shape) < 0.02] = ord("-")
        msa[:, n // 3:n // 3 + 2 * L] = ord("-")               # an all-gap stretch: whole labels may be empty
        msa = np.ascontiguousarray(msa)
        res = fso.segment_long(msa, L, debug=True)
        assert res["status"] == 0 and len(res["reduced"]) >= 2
        graph = gm.block_graph_model(msa, res["reduced"]["lb"], res["reduced"]["rb"])
        msa.setflags(write=False)
        _cases[case] = (msa, res, graph)
    return _cases[case]


@pytest.mark.parametrize("case", CASES)
def test_numbering_is_the_one_the_boundary_states_imply(case):
    """A position starts a class iff i = 0 or d[i] > lb: the classes in pBWT order at rb, the representative the row at the first
    position.  The model gets the same from the rows' bytes."""
    msa, res, graph = segmented(case)
    red, m = res["reduced"], msa.shape[0]
    first = 0
    for s in range(len(red)):
        cls = jo.classes(m, int(red["lb"][s]), res["a"][s], res["d"][s])
        assert graph["count"][s] == len(cls) == red["segment_size"][s]
        nodes = graph["nodes"][first:first + len(cls)]
        assert nodes["rep_row"].tolist() == [c[0] for c in cls] and nodes["rows"].tolist() == [len(c) for c in cls]
        assert nodes["cls"].tolist() == list(range(len(cls))) and (nodes["segment"] == s).all()
        for c, rows in enumerate(cls):
            assert (graph["row_nodes"][s, rows] == first + c).all()
        # for distinct substrings the order is that of the reversed substrings' bytes
        keys = [msa[r, int(red["lb"][s]):int(red["rb"][s])][::-1].tobytes() for r in nodes["rep_row"]]
        assert keys == sorted(keys) and len(set(keys)) == len(keys)
        first += len(cls)
    assert first == len(graph["nodes"])


@pytest.mark.parametrize("case", CASES)
def test_weights_add_up(case):
    msa, res, graph = segmented(case)
    m, S = msa.shape[0], len(res["reduced"])
    nodes, edges = graph["nodes"], graph["edges"]
    assert np.array_equal(np.bincount(edges["junction"], weights=edges["rows"], minlength=S - 1), np.full(S - 1, m))
    out_w = np.bincount(edges["from"], weights=edges["rows"], minlength=len(nodes))
    in_w = np.bincount(edges["to"], weights=edges["rows"], minlength=len(nodes))
    last, first = nodes["segment"] == S - 1, nodes["segment"] == 0
    assert np.array_equal(out_w[~last], nodes["rows"][~last]) and not out_w[last].any()
    assert np.array_equal(in_w[~first], nodes["rows"][~first]) and not in_w[first].any()
    # an edge joins adjacent segments; the order is junction, then (from, to)
    assert np.array_equal(nodes["segment"][edges["from"]], edges["junction"]) and np.array_equal(nodes["segment"][edges["to"]], edges["junction"] + 1)
    order = list(zip(edges["junction"].tolist(), edges["from"].tolist(), edges["to"].tolist()))
    assert order == sorted(order) and len(set(order)) == len(order)


@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("gap", [b"-", None, b"A"])
def test_paths_spell_the_rows_and_lengths_are_the_bytes(case, gap):
    msa, res, graph = segmented(case)
    blob = gm.gfa_bytes(msa, graph, paths=True, gap=gap)
    parsed = gm.check_file_spells_rows(blob, msa, gap)
    assert len(parsed["nodes"]) == len(graph["nodes"]) and len(parsed["links"]) == len(graph["edges"])
    sections = gm.format_gfa(msa, graph, paths=True, gap=gap)
    lengths = gm.line_lengths(msa, graph, paths=True, gap=gap)
    for lines, lens in zip(sections, lengths):
        assert [len(x) for x in lines] == lens and all(x.endswith(b"\n") and x.count(b"\n") == 1 for x in lines)
    without = gm.gfa_bytes(msa, graph, paths=False, gap=gap)
    assert blob.startswith(without) and b"\nP\t" not in without


def test_hand_made_case():
    """The yardstick itself, on a case small enough to count by eye: three rows, two segments of two columns."""
    msa = np.frombuffer(b"A-CC" b"A-GG" b"T-GG", dtype=np.uint8).reshape(3, 4)
    graph = gm.block_graph_model(msa, [0, 2], [2, 4])
    # segment 0 at rb = 2: the order by the reversed prefixes "-A", "-A", "-T" is 0, 1, 2: classes {0, 1}, {2};
    # segment 1 at rb = 4: "CC-A" < "GG-A" < "GG-T": classes {0}, {1, 2}
    assert graph["nodes"].tolist() == [(0, 2, 0, 0, 0, 2), (0, 2, 0, 1, 2, 1), (2, 4, 1, 0, 0, 1), (2, 4, 1, 1, 1, 2)]
    assert graph["edges"].tolist() == [(0, 2, 1, 0), (0, 3, 1, 0), (1, 3, 1, 0)]
    assert graph["row_nodes"].tolist() == [[0, 0, 1], [2, 3, 3]]
    assert gm.gfa_bytes(msa, graph, paths=True) == (
        b"H\tVN:Z:1.0\n"
        b"S\t1\tA\tLN:i:1\tRC:i:2\tsg:i:0\tlb:i:0\trb:i:2\n" b"S\t2\tT\tLN:i:1\tRC:i:1\tsg:i:0\tlb:i:0\trb:i:2\n"
        b"S\t3\tCC\tLN:i:2\tRC:i:1\tsg:i:1\tlb:i:2\trb:i:4\n" b"S\t4\tGG\tLN:i:2\tRC:i:2\tsg:i:1\tlb:i:2\trb:i:4\n"
        b"L\t1\t+\t3\t+\t0M\tRC:i:1\n" b"L\t1\t+\t4\t+\t0M\tRC:i:1\n" b"L\t2\t+\t4\t+\t0M\tRC:i:1\n"
        b"P\t0\t1+,3+\t*\n" b"P\t1\t1+,4+\t*\n" b"P\t2\t2+,4+\t*\n")
    assert gm.gfa_bytes(msa, graph, gap=None).split(b"\n")[1] == b"S\t1\tA-\tLN:i:2\tRC:i:2\tsg:i:0\tlb:i:0\trb:i:2"
    # a segment of gaps alone: one class, an empty label
    gaps = np.frombuffer(b"AC--GT" b"TC--GA", dtype=np.uint8).reshape(2, 6)
    blob = gm.gfa_bytes(gaps, gm.block_graph_model(gaps, [0, 2, 4], [2, 4, 6]), paths=True)
    assert b"S\t3\t*\tLN:i:0\tRC:i:2\tsg:i:1\tlb:i:2\trb:i:4\n" in blob and gm.check_file_spells_rows(blob, gaps)["labels"][3] == b""
    assert [gm.digits(v) for v in (0, 9, 10, 99, 100, 999, 1000, 4294967295)] == [1, 1, 2, 2, 3, 3, 4, 10]


def test_one_segment_has_no_link():
    msa = founder_mosaic(3, 9, 40, brec=40, seed=2)
    graph = gm.block_graph_model(msa, [0], [40])
    assert len(graph["edges"]) == 0 and len(graph["nodes"]) == 3 and graph["row_nodes"].shape == (1, 9)
    blob = gm.gfa_bytes(msa, graph, paths=True)
    assert b"\nL\t" not in blob
    gm.check_file_spells_rows(blob, msa)
