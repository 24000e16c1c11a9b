#!/usr/bin/env python3
"""The founder block graph (fseq_block_graph, fseq_write_block_graph; csrc/fseq_graph.hpp) on a BASELINE configuration: what the
graph costs beside the device front of the greedy joiner, whose two kernels it shares, and what the GFA file costs per byte
beside the segments file from the device.

    python tools/block_graph_probe.py C3 [--reps=3] [--out=PATH] [--dir=/dev/shm]
    python tools/block_graph_probe.py C4                            # nodes and links only, one call each

One context in one process (generate_synthetic, run).  Every call is made once untimed, then --reps times in turn with the calls
it stands beside (a, b, c, a, b, c, ...); reported are the median and the spread of the whole call's wall time, which ends
synchronised.  The files go to --dir (tmpfs), so a file's time is the device's work, the copies and the write into memory.
Writes profiles/block_graph_<configuration>.txt (or --out) as well as stdout."""
import importlib
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

LINES = []


def say(text):
    print(text, flush=True)
    LINES.append(text)


def arg(name, default):
    for a in sys.argv[1:]:
        if a.startswith("--%s=" % name):
            return a.split("=", 1)[1]
    return default


def timed(fn):
    t0 = time.perf_counter()
    out = fn()
    return (time.perf_counter() - t0) * 1e3, out


def in_turn(calls, reps):
    """{name: [ms]} of the calls made one after the other, reps times, after one untimed round."""
    ms = {name: [] for name, _ in calls}
    for it in range(reps + 1):
        for name, fn in calls:
            dt, _ = timed(fn)
            if it:
                ms[name].append(dt)
    return ms


def summary(ms):
    v = sorted(ms)
    return "%10.1f ms (%.1f .. %.1f, %d calls)" % (v[len(v) // 2], v[0], v[-1], len(v))


def median(ms):
    return sorted(ms)[len(ms) // 2]


def main():
    import bench
    words = [a for a in sys.argv[1:] if not a.startswith("--")]
    name = "C4" if "C4" in words else "C3"
    reps = int(arg("reps", "3"))
    where = arg("dir", "/dev/shm" if os.path.isdir("/dev/shm") else tempfile.gettempdir())
    pkg = importlib.import_module("founder-sequences_amd")
    w = bench.WORKLOADS[name]
    m, n = w["m"], w["n"]
    say("# tools/block_graph_probe.py %s on kernel sources %s: m = %d, n = %d, L = %d; ms are wall time of the whole call, median (min .. max); files in %s"
        % (name, bench.csrc_sha(), m, n, w["L"], where))
    ctx = pkg.SegmentationContext(m, n, w["L"], device=0)
    ctx.generate_synthetic(w["seed"], w["K"], w["B"], w["mu"], w["kind"])
    r = ctx.run()
    S, X = int(r.segment_count), int(r.max_segment_size)
    say("max_segment_size %d, %d merged segments" % (X, S))
    tmp = tempfile.mkdtemp(prefix="block_graph_probe_", dir=where)
    gfa, gfa_p, seg = (os.path.join(tmp, x) for x in ("graph.gfa", "graph_paths.gfa", "segments.txt"))
    try:
        if name == "C4":
            try:
                dt, g = timed(ctx.block_graph)
                say("fseq_block_graph (nodes and edges, no row_nodes) %10.1f ms (one call): %d nodes, %d edges" % (dt, g["summary"]["nodes"], g["summary"]["edges"]))
                del g
                dt, _ = timed(lambda: ctx.write_block_graph(gfa, paths=False))
                st = ctx.graph_file_stats()
                size = os.path.getsize(gfa)
                say("fseq_write_block_graph without paths            %10.1f ms (one call): %d bytes, %.2f ns per byte; S lines %d in %d batches, L lines %d in %d batches"
                    % (dt, size, dt * 1e6 / size, st["nodes"]["lines"], st["nodes"]["batches"], st["links"]["lines"], st["links"]["batches"]))
            except pkg.FseqError as e:
                say("refused or failed (code %d): %s" % (e.code, e))
            say("# one call each, no warm-up.  Not measured: the paths, the graph with row_nodes, the segments file beside it, repeats")
            return
        front = []

        def greedy():
            ctx.join_greedy()
            front.append(ctx.join_profile()["ms_d2h"])

        ms = in_turn([("graph", ctx.block_graph), ("greedy", greedy), ("graph_rows", lambda: ctx.block_graph(want_row_nodes=True))], reps)
        g = ctx.block_graph()
        fr = front[1:]
        say("%d nodes, %d edges" % (g["summary"]["nodes"], g["summary"]["edges"]))
        say("fseq_block_graph, nodes and edges                 %s" % summary(ms["graph"]))
        say("fseq_block_graph, with row_nodes (%.1f MB)        %s" % (S * m * 4 / 1e6, summary(ms["graph_rows"])))
        say("fseq_join_greedy, whole call                      %s" % summary(ms["greedy"]))
        say("    its device front (join_profile ms_d2h: classes, edges, copies; path %d) %s" % (ctx.join_path(), summary(fr)))
        say("    the graph is %.2f x the front" % (median(ms["graph"]) / median(fr)))
        del g
        calls = [("gfa", lambda: ctx.write_block_graph(gfa, paths=False)), ("gfa_paths", lambda: ctx.write_block_graph(gfa_p, paths=True)),
                 ("segments", lambda: ctx.write_segments_device(pkg.JOIN_BIPARTITE, seg))]
        ms = in_turn(calls, reps)
        ctx.write_block_graph(gfa_p, paths=True)
        st = ctx.graph_file_stats()
        sizes = {"gfa": os.path.getsize(gfa), "gfa_paths": os.path.getsize(gfa_p), "segments": os.path.getsize(seg)}
        label = {"gfa": "fseq_write_block_graph without paths", "gfa_paths": "fseq_write_block_graph with paths   ", "segments": "fseq_write_segments_device bipartite"}
        for k in ("gfa", "gfa_paths", "segments"):
            say("%s %s: %d bytes, %.2f ns per byte (%.2f .. %.2f)" % (label[k], summary(ms[k]), sizes[k], median(ms[k]) * 1e6 / sizes[k],
                                                                    min(ms[k]) * 1e6 / sizes[k], max(ms[k]) * 1e6 / sizes[k]))
        say("    sections of the file with paths: S %d lines, %d bytes, %d batches; L %d lines, %d bytes, %d batches; P %d lines, %d bytes, %d batches"
            % tuple(st[k][f] for k in ("nodes", "links", "paths") for f in ("lines", "bytes", "batches")))
        extra_ms, extra_bytes = median(ms["gfa_paths"]) - median(ms["gfa"]), sizes["gfa_paths"] - sizes["gfa"]
        say("    the paths alone (difference of the medians): %.1f ms for %d bytes, %.2f ns per byte" % (extra_ms, extra_bytes, extra_ms * 1e6 / max(1, extra_bytes)))
    finally:
        for f in (gfa, gfa_p, seg):
            if os.path.exists(f):
                os.remove(f)
        os.rmdir(tmp)
        ctx.close()
        out = arg("out", os.path.join(ROOT, "profiles", "block_graph_%s.txt" % name))
        os.makedirs(os.path.dirname(out), exist_ok=True)
        with open(out, "w") as f:
            f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
