"""block_graph_restored_probe.py [CONFIG] [--share=0.6] [--rows=256] [OUT] -- the block graph in source co-ordinates
(fseq_write_block_graph_restored) beside the one in reduced co-ordinates (fseq_write_block_graph) on the same context, and the
restored threading of the held-out rows beside their restored match, measured in one process (CONFIG: a name of oracle/fso.py's
CONFIGS, C3 by default; writes profiles/block_graph_restored_CONFIG.txt or OUT).

The input is CONFIG's synthetic alignment with about SHARE of its columns overwritten with row 0's symbol (identity columns); the
last ROWS rows are held out and carried along.  One context, made by without_rows() and without_identity_columns(keep_held_out=True),
one run.  The two writers alternate after a warm-up of each, both to tmpfs, with and without the P lines; whole-call wall time,
medians of RUNS.  The reduced writer is the existing code and the yardstick: the two files differ in their S sections alone, so the
figure is what the restored S section's extra bytes cost beside the reduced writer's rate per byte.  Then
graph_thread_held_out_restored(), graph_thread_rows_restored() on the same rows from the host, and match_held_out_restored()
alternate the same way.  The reduced threading (graph_thread_held_out) refuses an identity-reduced context, so its figure comes
from a second context that holds the kept columns as an alignment of its own with the same rows held out: the same graph, the
same kernels but k_gt_exceptions."""
import importlib
import os
import statistics
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "oracle")):
    sys.path.insert(0, p)
RUNS = 3


def alternate(variants):
    """[(name, call)] -> {name: (median wall ms, the walls)} after a warm-up of each"""
    times = {name: [] for name, _ in variants}
    for _, call in variants:
        call()
    for _ in range(RUNS):
        for name, call in variants:
            t0 = time.perf_counter()
            call()
            times[name].append((time.perf_counter() - t0) * 1e3)
    return {name: (statistics.median(t), t) for name, t in times.items()}


def main():
    import fso
    opts = {a.split("=")[0]: a.split("=")[1] for a in sys.argv[1:] if a.startswith("--")}
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    share, rows = float(opts.get("--share", 0.6)), int(opts.get("--rows", 256))
    config = args[0] if args else "C3"
    out_path = args[1] if len(args) > 1 else os.path.join(ROOT, "profiles", "block_graph_restored_%s.txt" % config)
    pkg = importlib.import_module("founder-sequences_amd")
    c = fso.CONFIGS[config]
    m, n, L = c["m"], c["n"], c["L"]
    gen = pkg.SegmentationContext(m, n, L)
    gen.generate_synthetic(c["seed"], c["K"], c["B"], c["mu"], c["kind"])
    msa = gen.get_sequences()
    gen.close()
    rng = np.random.default_rng(c["seed"])
    ident = np.flatnonzero(rng.random(n) < share)
    msa[:, ident] = msa[0:1, ident]
    # the held-out rows differ from row 0 in one of 10,000 of their cells, identity columns included: exception cells
    alphabet = np.unique(msa[0])
    nxt = np.zeros(256, dtype=np.uint8)
    nxt[alphabet] = np.roll(alphabet, -1)
    tail = msa[m - rows:]
    hit = rng.random(tail.shape) < 1e-4
    tail[hit] = nxt[tail[hit]]
    del hit
    msa = np.ascontiguousarray(msa)
    held = np.arange(m - rows, m, dtype=np.uint32)
    src = pkg.SegmentationContext(m, n, L)
    src.set_sequences(msa)
    sub = src.without_rows(held, L)
    src.close()
    red = sub.without_identity_columns(L, keep_held_out=True)
    sub.close()
    res = red.run()
    perm = red.join_greedy()
    kept = red.kept_columns().astype(np.int64)
    seg = red.segments_restored()
    ok = seg["lb"][0] == 0 and seg["rb"][-1] == n and np.array_equal(seg["lb"][1:], seg["rb"][:-1])
    lines = ["block_graph_restored_probe %s: m = %d (the last %d held out), n = %d, L = %d; identity share %.2f: kept %d columns; %d merged segments, "
             "max_segment_size %d; whole-call wall time, medians of %d after a warm-up, the calls alternating" % (
                 config, m, rows, n, L, share, red.n, res.segment_count, res.max_segment_size, RUNS)]
    base = "/dev/shm" if os.path.isdir("/dev/shm") and os.access("/dev/shm", os.W_OK) else None
    with tempfile.TemporaryDirectory(dir=base) as tmp:
        for paths in (False, True):
            stats = {}

            def writer(name, call):
                def go():
                    call(os.path.join(tmp, name + ".gfa"), paths=paths)
                    stats[name] = red.graph_file_stats()
                return go

            med = alternate([("reduced", writer("reduced", red.write_block_graph)), ("restored", writer("restored", red.write_block_graph_restored))])
            size = {w: os.path.getsize(os.path.join(tmp, w + ".gfa")) for w in med}
            for w in med:
                ok = ok and size[w] == 11 + sum(stats[w][k]["bytes"] for k in stats[w])
            ok = ok and all(stats["reduced"][k] == stats["restored"][k] for k in ("links", "paths")) and stats["reduced"]["nodes"]["lines"] == stats["restored"]["nodes"]["lines"]
            lines.append("the file %s the P lines: %d S lines, %d L lines, %d P lines" % (
                "with" if paths else "without", stats["restored"]["nodes"]["lines"], stats["restored"]["links"]["lines"], stats["restored"]["paths"]["lines"]))
            for w in ("reduced", "restored"):
                lines.append("    %-8s %12d bytes, of them %12d in the S section: %8.1f ms (%s)  %.3f ns a byte" % (
                    w, size[w], stats[w]["nodes"]["bytes"], med[w][0], " ".join("%.1f" % x for x in med[w][1]), med[w][0] * 1e6 / size[w]))
            extra_b, extra_ms = size["restored"] - size["reduced"], med["restored"][0] - med["reduced"][0]
            lines.append("    restored / reduced: %.2fx the bytes, %.2fx the time; the %d extra bytes of the S section cost %.1f ms = %.3f ns a byte, %.2fx the reduced writer's rate" % (
                size["restored"] / size["reduced"], med["restored"][0] / med["reduced"][0], extra_b, extra_ms, extra_ms * 1e6 / max(extra_b, 1),
                (extra_ms / max(extra_b, 1)) / (med["reduced"][0] / size["reduced"])))
    # the threads beside the restored match of the same rows
    queries = np.ascontiguousarray(msa[m - rows:])
    last = {}
    calls = [("graph_thread_held_out_restored", lambda: last.__setitem__("held", red.graph_thread_held_out_restored(want_nodes=False, want_steps=False))),
             ("graph_thread_rows_restored", lambda: last.__setitem__("rows", red.graph_thread_rows_restored(queries, want_nodes=False, want_steps=False))),
             ("match_held_out_restored", lambda: last.__setitem__("match", red.match_held_out_restored(perm)))]
    med = alternate(calls)
    ok = ok and np.array_equal(last["held"]["per_row"], last["rows"]["per_row"])
    exc = red.match_exceptions()
    sm = last["held"]["summary"]
    lines.append("the %d held-out rows, full length, %d exception cells: %d of %d (row, segment) pairs matched, %d rows on the graph" % (
        rows, len(exc[1]), sm["segments_matched"], rows * res.segment_count, sm["rows_on_graph"]))
    device = {"graph_thread_held_out_restored": last["held"]["summary"]["ms_device"], "graph_thread_rows_restored": last["rows"]["summary"]["ms_device"],
              "match_held_out_restored": last["match"]["ms_device"]}
    for name, _ in calls:
        lines.append("    %-32s %8.1f ms (%s)  (ms_device %.1f)" % (name, med[name][0], " ".join("%.1f" % x for x in med[name][1]), device[name]))
    red.close()
    # the reduced threading of the same rows' kept columns: a context of its own (the reduced twin refuses an identity-reduced one)
    plain = pkg.SegmentationContext(m, len(kept), L)
    plain.set_sequences(np.ascontiguousarray(msa[:, kept]))
    sub = plain.without_rows(held, L)
    plain.close()
    sub.run()
    med2 = alternate([("graph_thread_held_out", lambda: last.__setitem__("plain", sub.graph_thread_held_out(want_nodes=False, want_steps=False)))])
    lines.append("    %-32s %8.1f ms (%s)  (ms_device %.1f; a second context over the kept columns alone, the same rows held out: no exception pass)" % (
        "graph_thread_held_out", med2["graph_thread_held_out"][0], " ".join("%.1f" % x for x in med2["graph_thread_held_out"][1]), last["plain"]["summary"]["ms_device"]))
    lines.append("    restored - reduced held-out threading: %.1f ms" % (med["graph_thread_held_out_restored"][0] - med2["graph_thread_held_out"][0]))
    sub.close()
    lines.append("not measured here: C4, 4- and 8-bit inputs")
    lines.append("the source bounds tile the source, the stats fit the files, both thread entries agree: %s" % ("yes" if ok else "NO"))
    print("\n".join(lines))
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
