#!/usr/bin/env python3
"""The segments file from the device (fseq_write_segments_device, csrc/fseq_segfile.hpp) beside the host writer, and
fseq_join_random through its device front beside the host joiner, on a BASELINE configuration.

    python tools/segments_probe.py C3 [--reps=3]     # both writers, both joinings; the random join through both paths
    python tools/segments_probe.py C4                # random joining only, one run each: the join through both paths, the device writer

One context in one process (generate_synthetic, run).  C3: the host writer gets its rows from get_sequences(); host and
device writer alternate, --reps times after one untimed call each, to files on tmpfs; the random join alternates between its
paths (FSEQ_JOIN_HOST set and cleared, with the run a knob asks for, outside the timed region).  Times are the wall time of
the whole call, which ends synchronised (the file is closed, the permutations are on the host); reported are the median and
the spread.  C4: the bipartite file would be about 20 GB of text (segments x m row indices) and the host writer needs 500 GB
of rows: neither is run.  Writes profiles/segments_device_<configuration>.txt as well as stdout."""
import importlib
import os
import sys
import tempfile
import time

import numpy as np

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


def summary(ms):
    v = sorted(ms)
    return "%10.1f ms (%.1f .. %.1f, %d calls)" % (v[len(v) // 2], v[0], v[-1], len(v))


def random_join_both_paths(pkg, ctx, reps, S, m):
    ms, perms, d2h = {0: [], 1: []}, {}, {}
    for it in range(reps + 1):                                 # (the first round is untimed)
        for path in (0, 1):
            ctx.set_tuning("FSEQ_JOIN_HOST", "1" if path == 0 else None)
            ctx.run()
            dt, perm = timed(lambda: ctx.join_random(7))
            assert ctx.random_path() == path
            if it == 0 and reps:
                continue
            ms[path].append(dt)
            perms[path], d2h[path] = perm, ctx.join_profile()["bytes_d2h"]
    say("join_random, host joiner          %s, %d bytes to the host" % (summary(ms[0]), d2h[0]))
    say("join_random, device class tables  %s, %d bytes to the host (segments x m x 8 = %d)" % (summary(ms[1]), d2h[1], S * m * 8))
    say("the permutations are %s" % ("the same" if np.array_equal(perms[0], perms[1]) else "DIFFERENT"))


def main():
    import bench
    name = "C4" if "C4" in sys.argv[1:] else "C3"
    reps = int(arg("reps", "3")) if name == "C3" else 0
    pkg = importlib.import_module("founder-sequences_amd")
    w = bench.WORKLOADS[name]
    m, n = w["m"], w["n"]
    shm = os.path.isdir("/dev/shm")
    tmp = tempfile.mkdtemp(dir="/dev/shm" if shm else None)
    say("# tools/segments_probe.py %s on kernel sources %s: m = %d, n = %d, L = %d; files %s; ms are wall time of the whole call, median (min .. max)"
        % (name, bench.csrc_sha(), m, n, w["L"], "on tmpfs" if shm else "in the temporary directory"))
    ctx = pkg.SegmentationContext(m, n, w["L"], device=0)
    ctx.generate_synthetic(w["seed"], w["K"], w["B"], w["mu"], w["kind"])
    r = ctx.run()
    S, X = int(r.segment_count), int(r.max_segment_size)
    say("max_segment_size %d, %d merged segments, %.3f GB of boundary states" % (X, S, S * m * 8 / 1e9))
    if name == "C3":
        rows = np.ascontiguousarray(ctx.get_sequences())
        for joining, label in ((pkg.JOIN_BIPARTITE, "bipartite"), (pkg.JOIN_RANDOM, "random")):
            h, d = os.path.join(tmp, "host.txt"), os.path.join(tmp, "device.txt")
            ms = {"host": [], "device": []}
            for it in range(reps + 1):                         # (the first round is untimed)
                for who in ("host", "device"):
                    dt, _ = timed((lambda: ctx.write_segments(rows, joining, h)) if who == "host" else (lambda: ctx.write_segments_device(joining, d)))
                    if it:
                        ms[who].append(dt)
            same = open(h, "rb").read() == open(d, "rb").read()
            st = ctx.segments_file_stats()
            say("segments file, %-9s host writer   %s, %d bytes of boundary states to the host" % (label, summary(ms["host"]), S * m * 8))
            say("segments file, %-9s device writer %s, %d bytes in %d lines, %d batch(es), longest line %d; the files are %s"
                % (label, summary(ms["device"]), st["bytes"], st["lines"], st["batches"], st["longest_line"], "the same" if same else "DIFFERENT"))
            os.remove(h)
            os.remove(d)
        del rows
        random_join_both_paths(pkg, ctx, reps, S, m)
    else:
        random_join_both_paths(pkg, ctx, 0, S, m)
        d = os.path.join(tmp, "device.txt")
        dt, _ = timed(lambda: ctx.write_segments_device(pkg.JOIN_RANDOM, d))
        st = ctx.segments_file_stats()
        say("segments file, random    device writer %10.1f ms (one call), %d bytes in %d lines, %d batch(es), longest line %d"
            % (dt, st["bytes"], st["lines"], st["batches"], st["longest_line"]))
        say("# one run each.  Not run: the bipartite file (about segments x m row indices of text) and the host writer (500 GB of rows)")
        os.remove(d)
    os.rmdir(tmp)
    ctx.close()
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "segments_device_%s.txt" % name), "w") as f:
        f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
