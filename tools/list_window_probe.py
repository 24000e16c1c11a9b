#!/usr/bin/env python3
"""The list budget (fseq_set_list_memory) on one bench input: both modes on ONE context, alternating, with hashes of what
they produce, or the first run of a fresh process (cold: allocations, code objects, the capacity estimate).

    python tools/list_window_probe.py C4 --list-memory=16 --steps=5     # unbounded / 16 GiB alternating, 5 timed steps each
    python tools/list_window_probe.py C4 --cold [--list-memory=16]      # one cold first run (run each in a fresh process)

A switch of mode re-sizes the list buffer inside the next run, so every timed step follows an untimed one in the same mode.
Hashes: the merged segments, and the boundary states of every 64th segment plus the last (all of them would be ~18 GB of
copies at C4)."""
import hashlib
import importlib
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "oracle")):
    if p not in sys.path:
        sys.path.insert(0, p)


def arg(name, default):
    for a in sys.argv[1:]:
        if a.startswith("--%s=" % name):
            return a.split("=", 1)[1]
    return default


def hashes(ctx):
    red = ctx.reduced_traceback()
    hs = hashlib.sha256(red.tobytes()).hexdigest()[:16]
    h = hashlib.sha256()
    for i in sorted(set(list(range(0, len(red), 64)) + [len(red) - 1])):
        a, d = ctx.boundary_state(i)
        h.update(a.tobytes())
        h.update(d.tobytes())
    return hs, h.hexdigest()[:16]


def line(tag, ms, ctx):
    t = ctx.timings()
    w = ctx.list_windows()
    return ("%-10s %9.1f ms | A %.1f B %.1f C %.1f D %.1f host %.1f p2 %.1f | X %d | windows %d (%d columns, %.2f GB held, merge pass %d)"
            % (tag, ms, t["ms_phase_a"], t["ms_phase_b"], t["ms_phase_c"], t["ms_dp"], t["ms_host"], t["ms_pass2"], t["list_cap_used"],
               w["windows"], w["columns_per_window"], w["bytes_held"] / 1e9, w["merge_windows"]))


def main():
    import torch
    import bench
    pkg = importlib.import_module("founder-sequences_amd")
    name = next((a for a in sys.argv[1:] if not a.startswith("-")), "C4")
    w = bench.WORKLOADS[name]
    m, n, L = w["m"], w["n"], w["L"]
    budget = int(float(arg("list-memory", "16")) * (1 << 30))
    if "--cold" in sys.argv:
        lm = budget if any(a.startswith("--list-memory=") for a in sys.argv) else 0
        t0 = time.perf_counter()
        ctx = pkg.SegmentationContext(m, n, L, device=0, list_memory=lm)
        ctx.generate_synthetic(w["seed"], w["K"], w["B"], w["mu"], w["kind"])
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        ctx.run()
        t2 = time.perf_counter()
        print("cold %s list_memory=%d: context + input %.1f ms, first run %.1f ms | %s" % (name, lm, (t1 - t0) * 1e3, (t2 - t1) * 1e3, line("first", (t2 - t1) * 1e3, ctx)), flush=True)
        return
    steps = int(arg("steps", "5"))
    print("# tools/list_window_probe.py %s on kernel sources %s: one context, unbounded and %.0f GiB list budget alternating, %d timed steps each"
          % (name, bench.csrc_sha(), budget / (1 << 30), steps), flush=True)
    ctx = pkg.SegmentationContext(m, n, L, device=0)
    ctx.generate_synthetic(w["seed"], w["K"], w["B"], w["mu"], w["kind"])
    seen = {}
    ms = {0: [], budget: []}
    for s in range(steps):
        for lm in (0, budget):
            ctx.set_list_memory(lm)
            ctx.run()                                       # (untimed: the list buffer is re-sized for this mode)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            ctx.run()
            torch.cuda.synchronize()
            dt = (time.perf_counter() - t0) * 1e3
            ms[lm].append(dt)
            tag = "unbounded" if lm == 0 else "windowed"
            extra = ""
            if s in (0, steps - 1):
                hs = hashes(ctx)
                seen.setdefault(hs, []).append(tag)
                extra = " | segments %s states %s" % hs
            print(line(tag, dt, ctx) + extra, flush=True)
    for lm, v in ms.items():
        v = sorted(v)
        print("# %s: median %.1f ms a step (min %.1f, max %.1f)" % ("unbounded" if lm == 0 else "windowed ", v[len(v) // 2], v[0], v[-1]))
    print("# hashes: %s" % ("IDENTICAL in both modes" if len(seen) == 1 else "DIFFER: %r" % seen))


if __name__ == "__main__":
    main()
