#!/usr/bin/env python3
"""The score of a join (fseq_join_score, csrc/fseq_joinscore.hpp) on a BASELINE configuration: what each joiner's permutations are
worth, beside what the score costs.

    python tools/join_score_probe.py C3 [--reps=3] [--out=PATH]     # the three joiners, the floor, the host form
    python tools/join_score_probe.py C4 greedy                      # one joiner, one call each

One context in one process (generate_synthetic, run).  Per joiner: the join once (its wall time is the figure the score stands
beside), then fseq_join_score --reps times after one untimed call, and its summary.  The floor: fseq_join_random through its
device front on the same context -- the same class-table kernel and a copy of the tables; the score adds one pass over
segments x m x 4 bytes of classes.  The host form: fseq_join_score_host on the boundary states copied to the host (the copy is
not timed).  Times are the wall time of the whole call, which ends synchronised; reported are the median and the spread.
Writes profiles/join_score_<configuration>.txt (or --out) as well as stdout."""
import importlib
import os
import sys
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


def repeated(fn, reps):
    ms, out = [], None
    for it in range(reps + 1):                                 # (the first call is untimed)
        dt, out = timed(fn)
        if it or not reps:
            ms.append(dt)
    return ms, out


def main():
    import bench
    words = [a for a in sys.argv[1:] if not a.startswith("--")]
    name = "C4" if "C4" in words else "C3"
    joiners = [w for w in words if w in ("greedy", "bipartite", "random")] or ["greedy", "bipartite", "random"]
    reps = int(arg("reps", "3")) if name == "C3" else 0
    pkg = importlib.import_module("founder-sequences_amd")
    w = bench.WORKLOADS[name]
    m, n = w["m"], w["n"]
    say("# tools/join_score_probe.py %s on kernel sources %s: m = %d, n = %d, L = %d; ms are wall time of the whole call, median (min .. max)"
        % (" ".join([name] + joiners), bench.csrc_sha(), m, n, w["L"]))
    ctx = pkg.SegmentationContext(m, n, w["L"], device=0)
    ctx.generate_synthetic(w["seed"], w["K"], w["B"], w["mu"], w["kind"])
    r = ctx.run()
    S, X = int(r.segment_count), int(r.max_segment_size)
    say("max_segment_size %d, %d merged segments, %.3f GB of boundary states, %.1f MB of classes (segments x m x 2)" % (X, S, S * m * 8 / 1e9, S * m * 2 / 1e6))
    join = {"greedy": ctx.join_greedy, "bipartite": ctx.join_bipartite, "random": lambda: ctx.join_random(7)}
    perms = {}
    for how in joiners:
        dt_join, perm = timed(join[how])
        perms[how] = perm
        ms, score = repeated(lambda: ctx.join_score(perm), reps)
        assert ctx.join_score_path() == 1, "the score left the device"
        sm = score["summary"]
        say("join_%-9s %10.1f ms (one call); fseq_join_score %s" % (how, dt_join, summary(ms)))
        say("    supported %d, unsupported %d, gaps %d of %d slots; weight %d; rows through a junction: %.1f of %d on average, %d at the worst (junction %d); "
            "the founder with most breaks has %d" % (sm["supported"], sm["unsupported"], sm["gaps"], sm["junctions"] * X, sm["weight"],
                                                     sm["rows_through"] / max(1, sm["junctions"]), m, sm["min_rows_through"], sm["min_rows_through_junction"], sm["max_breaks"]))
    ms, _ = repeated(lambda: ctx.join_random(7), reps)
    assert ctx.random_path() == 1
    say("the floor, fseq_join_random through its device front (class tables + host shuffles) %s" % summary(ms))
    if name == "C3":
        segs = ctx.reduced_traceback()
        a, d = np.zeros((S, m), dtype=np.uint32), np.zeros((S, m), dtype=np.uint32)
        for i in range(S):
            a[i], d[i] = ctx.boundary_state(i)
        how = joiners[0]
        ms, host = repeated(lambda: pkg.join_score_host(m, X, segs["lb"], segs["rb"], a, d, perms[how]), reps)
        device = ctx.join_score(perms[how])
        same = np.array_equal(host["junctions"], device["junctions"]) and np.array_equal(host["breaks"], device["breaks"])
        say("fseq_join_score_host on the copied boundary states (%s permutations) %s; junctions and breaks are %s" % (how, summary(ms), "the same" if same else "DIFFERENT"))
    else:
        say("# one call each.  Not run: the other joiners (bipartite: minutes), the host form (%.1f GB of boundary states on the host)" % (S * m * 8 / 1e9))
    ctx.close()
    out = arg("out", os.path.join(ROOT, "profiles", "join_score_%s.txt" % name))
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as f:
        f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
