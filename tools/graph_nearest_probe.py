"""graph_nearest_probe.py [CONFIG] [--rows=256] [OUT] -- the nearest node of every segment for held-out rows, measured in one
process (CONFIG: a name of oracle/fso.py's CONFIGS, C3 by default; writes profiles/graph_nearest_CONFIG.txt or OUT).

The last ROWS rows are held out of the resident alignment as tools/graph_thread_probe.py does, and the others are segmented.  On
that one context, alternating, medians of RUNS after a warm-up of each, wall time of the whole call:
  graph_thread_held_out, statistics only (the yardstick);  graph_nearest_held_out, statistics only;  graph_nearest_held_out with
  the four arrays;  graph_nearest_rows on the same bytes, statistics only;  block_graph().
Then what the feature exists for: the histogram of `distance` over the cells the exact threading leaves unmatched, the ties there,
and the walks at max_distance 0, 1, 2, 4."""
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
DISTANCES = (0, 1, 2, 4)


def main():
    import fso
    args = [a for a in sys.argv[1:] if not a.startswith("--rows=")]
    rows = ([int(a[7:]) for a in sys.argv[1:] if a.startswith("--rows=")] or [256])[0]
    config = args[0] if args else "C3"
    out_path = args[1] if len(args) > 1 else os.path.join(ROOT, "profiles", "graph_nearest_%s.txt" % config)
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
    S = res.segment_count
    lines = ["graph_nearest_probe %s: m = %d, n = %d, L = %d; %d rows held out, %d segmented: max_segment_size %d, %d merged segments; wall ms of the whole call, median (min .. max) of %d, alternating" % (
        config, m, n, L, rows, m - rows, res.max_segment_size, S, RUNS)]
    out = {}
    slim = dict(want_nodes=False, want_distances=False, want_ties=False, want_steps=False)

    def thread_stats():
        out["thread"] = ctx.graph_thread_held_out(want_nodes=False, want_steps=False)

    def stats_only():
        out["stats"] = ctx.graph_nearest_held_out(0, **slim)

    def with_arrays():
        out["arrays"] = ctx.graph_nearest_held_out(0)

    def uploaded():
        out["rows"] = ctx.graph_nearest_rows(held_bytes, 0, **slim)

    def graph():
        out["graph"] = ctx.block_graph()

    variants = [("graph_thread_held_out, statistics only (the yardstick)", thread_stats), ("graph_nearest_held_out, statistics only", stats_only),
                ("graph_nearest_held_out, four arrays (%.1f MB)" % ((4 * S - 1) * rows * 4 / 1e6), with_arrays),
                ("graph_nearest_rows on the same bytes, statistics only", uploaded), ("block_graph()", graph)]
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
    lines.append("    nearest, statistics only / threading, statistics only = %.2f; nearest with arrays / threading = %.2f; nearest / block_graph() = %.2f" % (
        med[variants[1][0]] / med[variants[0][0]], med[variants[2][0]] / med[variants[0][0]], med[variants[1][0]] / med[variants[4][0]]))
    info = ctx.graph_nearest_info()
    lines.append("    packed at %d bits: %d batch(es), %d words of class representatives (%.1f MB), %d words a query (%.1f MB for the %d queries)" % (
        info["bits"], info["batches"], info["packed_words"], info["packed_words"] * 4 / 1e6, info["query_words"], info["query_words"] * 4 * rows / 1e6, rows))
    # the exact threading against the nearest nodes at distance 0
    th, near = out["thread"], out["arrays"]
    shared = (("segments_matched", "segments_admitted"), ("junctions_linked",) * 2, ("junctions_novel",) * 2, ("walks",) * 2, ("longest_walk_segments",) * 2)
    same = (all(np.array_equal(th["per_row"][a], near["per_row"][b]) for a, b in shared) and np.array_equal(out["stats"]["per_row"], near["per_row"])
            and np.array_equal(out["rows"]["per_row"], near["per_row"]))
    dist, ties = near["distances"], near["ties"]
    missed = dist > 0
    lines.append("the graph: %d nodes, %d edges; the exact threading leaves %d of %d cells unmatched, %d walks%s" % (
        out["graph"]["summary"]["nodes"], out["graph"]["summary"]["edges"], int(missed.sum()), dist.size, th["summary"]["walks"], "" if same else "  THE CALLS DIFFER"))
    hist = np.bincount(np.minimum(dist[missed], 17))
    lines.append("distance to the nearest node over those cells: " + ", ".join("%s: %d" % ("%d" % d if d < 17 else ">= 17", k) for d, k in enumerate(hist) if d and k))
    lines.append("    median %d, mean %.2f, largest %d; %d cells (%.1f %%) at distance 1; the nearest node is unique in %d of them (%.1f %%), most ties %d" % (
        int(np.median(dist[missed])), float(dist[missed].mean()), int(dist.max()), int((dist == 1).sum()), 100.0 * (dist == 1).sum() / max(1, missed.sum()),
        int((ties[missed] == 1).sum()), 100.0 * (ties[missed] == 1).sum() / max(1, missed.sum()), int(ties[missed].max())))
    lines.append("walks once max_distance mismatches a segment are forgiven (statistics only):")
    for D in DISTANCES:
        sm = ctx.graph_nearest_held_out(D, **slim)
        s, pr = sm["summary"], sm["per_row"]
        lines.append("    D = %d: %d of %d cells admitted, %d junctions linked, %d novel, %d walks (%.1f a row), %d rows on the graph, the longest walk of a row: median %d segments" % (
            D, s["segments_admitted"], dist.size, s["junctions_linked"], s["junctions_novel"], s["walks"], s["walks"] / rows, s["rows_on_graph"],
            int(np.median(pr["longest_walk_segments"]))))
    ctx.close()
    print("\n".join(lines))
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")
    return 0 if same else 1


if __name__ == "__main__":
    sys.exit(main())
