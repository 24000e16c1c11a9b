"""The founder block graph (include/fseq.h: fseq_block_graph, fseq_write_block_graph) from the raw alignment alone: numpy, no
boundary state and no class table of the library.

Given the merged segments [lb_s, rb_s) of a run, the classes of a segment are the distinct msa[i, lb:rb].  They are numbered in
the order of their first position in the pBWT order at rb -- the stable co-lexicographic order of the prefixes [0, rb), built
here column by column with one stable sort a column, under the byte order (the library's codes ascend with the bytes) -- and a
class's representative is the row at that first position.  tests/test_block_graph_model.py confirms that this is the numbering
the boundary states imply (a position starts a class iff i = 0 or d[i] > lb), which is the definition."""
import numpy as np

NODE_DTYPE = np.dtype([("lb", "<u8"), ("rb", "<u8"), ("segment", "<u4"), ("cls", "<u4"), ("rep_row", "<u4"), ("rows", "<u4")])
EDGE_DTYPE = np.dtype([("from", "<u4"), ("to", "<u4"), ("rows", "<u4"), ("junction", "<u4")])
HEADER = b"H\tVN:Z:1.0\n"


def pbwt_orders(msa, columns):
    """{k: the pBWT order in front of column k} for the k asked for: a_0 = 0 .. m - 1, a_{k+1} = a_k sorted stably by column k."""
    want, out = set(int(k) for k in columns), {}
    a = np.arange(msa.shape[0])
    for k in range(max(want) + 1):
        if k in want:
            out[k] = a.copy()
        if k < msa.shape[1]:
            a = a[np.argsort(msa[a, k], kind="stable")]
    return out


def block_graph_model(msa, lb, rb):
    """{"nodes", "edges" (structured arrays, the ABI's layouts), "row_nodes" [S, m], "count" [S]} of the segments [lb[s], rb[s])."""
    m, S = msa.shape[0], len(lb)
    orders = pbwt_orders(msa, rb)
    of_row = np.zeros((S, m), dtype=np.int64)
    nodes, count = [], []
    for s in range(S):
        l, r = int(lb[s]), int(rb[s])
        seen, rep, size = {}, [], []
        for row in orders[r]:
            key = msa[row, l:r].tobytes()
            c = seen.get(key)
            if c is None:
                c = seen[key] = len(rep)
                rep.append(int(row))
                size.append(0)
            size[c] += 1
            of_row[s, row] = c
        nodes += [(l, r, s, c, rep[c], size[c]) for c in range(len(rep))]
        count.append(len(rep))
    first = np.concatenate([[0], np.cumsum(count)]).astype(np.int64)
    edges = []
    for p in range(S - 1):
        pair, rows = np.unique(of_row[p] * 65536 + of_row[p + 1], return_counts=True)      # ascending (l, r)
        edges += [(first[p] + (k >> 16), first[p + 1] + (k & 0xFFFF), n, p) for k, n in zip(pair.tolist(), rows.tolist())]
    return {"nodes": np.array(nodes, dtype=NODE_DTYPE), "edges": np.array(edges, dtype=EDGE_DTYPE),
            "row_nodes": (of_row + first[:-1, None]).astype(np.uint32), "count": np.array(count, dtype=np.uint32)}


def label(msa, node, gap):
    raw = msa[int(node["rep_row"]), int(node["lb"]):int(node["rb"])].tobytes()
    return raw if not gap else raw.replace(gap, b"")


def format_gfa(msa, graph, paths=False, gap=b"-"):
    """The file's bytes, by section: (S lines, L lines, P lines), each a list of lines with their newlines; gap None or b"":
    every byte stays."""
    s_lines = []
    for i, nd in enumerate(graph["nodes"]):
        lab = label(msa, nd, gap)
        s_lines.append(b"S\t%d\t%s\tLN:i:%d\tRC:i:%d\tsg:i:%d\tlb:i:%d\trb:i:%d\n" %
                       (i + 1, lab or b"*", len(lab), nd["rows"], nd["segment"], nd["lb"], nd["rb"]))
    l_lines = [b"L\t%d\t+\t%d\t+\t0M\tRC:i:%d\n" % (e["from"] + 1, e["to"] + 1, e["rows"]) for e in graph["edges"]]
    p_lines = []
    if paths:
        for row in range(msa.shape[0]):
            p_lines.append(b"P\t%d\t%s\t*\n" % (row, b",".join(b"%d+" % (v + 1) for v in graph["row_nodes"][:, row].tolist())))
    return s_lines, l_lines, p_lines


def gfa_bytes(msa, graph, paths=False, gap=b"-"):
    return HEADER + b"".join(b"".join(sec) for sec in format_gfa(msa, graph, paths, gap))


def digits(v):
    """Decimal digits of v >= 0, by comparisons as the kernels count them."""
    d, p = 1, 10
    while v >= p:
        d, p = d + 1, p * 10
    return d


def line_lengths(msa, graph, paths=False, gap=b"-"):
    """What the device's count passes compute, by arithmetic on digit counts: the bytes of every line, by section."""
    s_len = []
    for i, nd in enumerate(graph["nodes"]):
        n = len(label(msa, nd, gap))
        s_len.append(2 + digits(i + 1) + 1 + max(n, 1) + 6 + digits(n) + 6 + digits(int(nd["rows"])) + 6 + digits(int(nd["segment"]))
                     + 6 + digits(int(nd["lb"])) + 6 + digits(int(nd["rb"])) + 1)
    l_len = [17 + digits(int(e["from"]) + 1) + digits(int(e["to"]) + 1) + digits(int(e["rows"])) for e in graph["edges"]]
    p_len = []
    if paths:
        for row in range(msa.shape[0]):
            p_len.append(2 + digits(row) + 1 + sum(digits(v + 1) + 2 for v in graph["row_nodes"][:, row].tolist()) - 1 + 3)
    return s_len, l_len, p_len


def parse_gfa(blob):
    """{"labels": {id: bytes}, "nodes": [(id, len, rows, segment, lb, rb)], "links": [(from, to, rows)], "paths": {row: [ids]}} of a
    file, ids as printed (1-based); every line's shape is asserted."""
    lines = blob.split(b"\n")
    assert lines[0] == HEADER[:-1] and lines[-1] == b""
    labels, nodes, links, paths = {}, [], [], {}
    for ln in lines[1:-1]:
        f = ln.split(b"\t")
        if f[0] == b"S":
            assert len(f) == 8 and [x[:5] for x in f[3:]] == [b"LN:i:", b"RC:i:", b"sg:i:", b"lb:i:", b"rb:i:"], ln
            nid, n = int(f[1]), int(f[3][5:])
            assert (f[2] == b"*" and n == 0) or (len(f[2]) == n and n > 0), ln
            labels[nid] = b"" if n == 0 else f[2]
            nodes.append((nid, n) + tuple(int(x[5:]) for x in f[4:]))
        elif f[0] == b"L":
            assert len(f) == 7 and f[2] == f[4] == b"+" and f[5] == b"0M" and f[6][:5] == b"RC:i:", ln
            links.append((int(f[1]), int(f[3]), int(f[6][5:])))
        else:
            assert f[0] == b"P" and len(f) == 4 and f[3] == b"*", ln
            steps = f[2].split(b",")
            assert all(x.endswith(b"+") for x in steps), ln
            paths[int(f[1])] = [int(x[:-1]) for x in steps]
    return {"labels": labels, "nodes": nodes, "links": links, "paths": paths}


def spelled_rows(parsed):
    """Every P line with its nodes' labels concatenated: {row: bytes}."""
    return {row: b"".join(parsed["labels"][v] for v in steps) for row, steps in parsed["paths"].items()}


def check_file_spells_rows(blob, msa, gap=b"-"):
    """The property a reader of the file relies on: a P line per row, and each spells its row without the gap byte; the links a
    path walks exist."""
    parsed = parse_gfa(blob)
    spelled = spelled_rows(parsed)
    assert sorted(spelled) == list(range(msa.shape[0]))
    for row, text in spelled.items():
        raw = msa[row].tobytes()
        assert text == (raw.replace(gap, b"") if gap else raw), row
    linked = {(a, b) for a, b, _ in parsed["links"]}
    for steps in parsed["paths"].values():
        assert all((a, b) in linked for a, b in zip(steps, steps[1:]))
    return parsed
