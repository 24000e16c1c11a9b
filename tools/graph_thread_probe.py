"""graph_thread_probe.py [CONFIG] [--rows=256] [OUT] -- held-out rows threaded through the founder block graph, measured in one
process (CONFIG: a name of oracle/fso.py's CONFIGS, C3 by default; writes profiles/graph_thread_CONFIG.txt or OUT).

The last ROWS rows are held out of the resident alignment as tools/hold_out_probe.py does, and the others are segmented.  On that
one context, alternating, medians of RUNS after a warm-up of each, wall time of the whole call:
  graph_thread_held_out, statistics only;  graph_thread_held_out with nodes and steps;  graph_thread_rows on the same bytes;
  block_graph();  match_held_out with the greedy permutations.
Then the counts: rows on the graph, novel junctions, segments unmatched, beside the pieces of match_held_out for the same rows."""
import importlib
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "oracle")):
    sys.path.insert(0, p)
RUNS = 3


def main():
    import fso
    args = [a for a in sys.argv[1:] if not a.startswith("--rows=")]
    rows = ([int(a[7:]) for a in sys.argv[1:] if a.startswith("--rows=")] or [256])[0]
    config = args[0] if args else "C3"
    out_path = args[1] if len(args) > 1 else os.path.join(ROOT, "profiles", "graph_thread_%s.txt" % config)
    pkg = importlib.import_module("founder-sequences_amd")
    c = fso.CONFIGS[config]
    m, n, L = c["m"], c["n"], c["L"]
    src = pkg.SegmentationContext(m, n, L)
    src.generate_synthetic(c["seed"], c["K"], c["B"], c["mu"], c["kind"])
    held = np.arange(m - rows, m, dtype=np.uint32)
    held_bytes = np.ascontiguousarray(src.get_sequences()[m - rows:])
    ctx = src.without_rows(held, L)
    src.close()
    res = ctx.run()
    perm = ctx.join_greedy()
    S = res.segment_count
    lines = ["graph_thread_probe %s: m = %d, n = %d, L = %d; %d rows held out, %d segmented: max_segment_size %d, %d merged segments; wall ms of the whole call, median (min .. max) of %d, alternating" % (
        config, m, n, L, rows, m - rows, res.max_segment_size, S, RUNS)]
    out = {}

    def stats_only():
        out["stats"] = ctx.graph_thread_held_out(want_nodes=False, want_steps=False)

    def with_arrays():
        out["arrays"] = ctx.graph_thread_held_out()

    def uploaded():
        out["rows"] = ctx.graph_thread_rows(held_bytes)

    def graph():
        out["graph"] = ctx.block_graph()

    def match():
        out["match"] = ctx.match_held_out(permutations=perm)

    variants = [("graph_thread_held_out, statistics only", stats_only), ("graph_thread_held_out, nodes and steps (%.1f MB)" % ((2 * S - 1) * rows * 4 / 1e6), with_arrays),
                ("graph_thread_rows on the same bytes (%.1f MB up)" % (rows * n / 1e6), uploaded), ("block_graph()", graph),
                ("match_held_out, greedy permutations", match)]
    times = {name: [] for name, _ in variants}
    for name, call in variants:                                   # warm-up of each
        call()
    for _ in range(RUNS):
        for name, call in variants:
            t0 = time.perf_counter()
            call()
            times[name].append((time.perf_counter() - t0) * 1e3)
    for name, _ in variants:
        t = times[name]
        lines.append("    %-58s %9.2f ms (%.2f .. %.2f)" % (name, statistics.median(t), min(t), max(t)))
    med = {name: statistics.median(t) for name, t in times.items()}
    lines.append("    statistics only / block_graph() = %.2f; with arrays / block_graph() = %.2f; statistics only / match_held_out = %.2f" % (
        med[variants[0][0]] / med[variants[3][0]], med[variants[1][0]] / med[variants[3][0]], med[variants[0][0]] / med[variants[4][0]]))
    sm, info = out["stats"]["summary"], ctx.graph_thread_info()
    same = all(np.array_equal(out["arrays"][k], out["rows"][k]) for k in ("nodes", "steps", "per_row", "per_segment")) and np.array_equal(out["stats"]["per_row"], out["arrays"]["per_row"])
    lines.append("the graph: %d nodes, %d edges" % (out["graph"]["summary"]["nodes"], out["graph"]["summary"]["edges"]))
    lines.append("the held-out rows through it: %d of %d rows on the graph; %d of %d segments unmatched; of %d junctions %d linked, %d novel; %d walks, at most %d in a row; the longest walk of a row: median %d segments%s" % (
        sm["rows_on_graph"], sm["rows"], sm["rows"] * S - sm["segments_matched"], sm["rows"] * S, sm["rows"] * (S - 1), sm["junctions_linked"], sm["junctions_novel"],
        sm["walks"], int(out["stats"]["per_row"]["walks"].max()), int(np.median(out["stats"]["per_row"]["longest_walk_segments"])), "" if same else "  THE THREE CALLS DIFFER"))
    lines.append("    keys of %d bits, %d slots a table: %d candidates compared, %d rejected, %d cells with a byte outside the alphabet" % (
        info["key_bits"], info["table_slots"], info["candidates_verified"], info["candidates_rejected"], info["queries_out_of_alphabet"]))
    mt = out["match"]
    lines.append("the same rows through the %d greedy founders (match_held_out): %d pieces, at most %d in a row, %d uncovered cells" % (
        mt["n_founders"], mt["pieces"], mt["max_pieces_per_row"], mt["uncovered_cells"]))
    ctx.close()
    print("\n".join(lines))
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")
    return 0 if same else 1


if __name__ == "__main__":
    sys.exit(main())
