#!/usr/bin/env python3
"""fseq_scan_segment_lengths on one bench input: 16 segment lengths spaced geometrically from a quarter to four times the
workload's own, on ONE context, alternating after a warm-up of each

    (a) the scan                        (lists built once, folded from length to length, the DP alone per length)
    (b) the scan with FSEQ_SCAN_REBUILD (the lists built at every length: what the library falls back to by itself)
    (c) C3 only: 16 full runs through fseq_set_segment_length -- these INCLUDE traceback, merge and pass 2, which a scan does not do

    python tools/length_scan_probe.py C3 [--steps=3] > profiles/length_scan_C3.txt
    python tools/length_scan_probe.py C4 [--steps=2] [--lo=1 --hi=1.5] >> profiles/length_scan_C4.txt

--lo / --hi: the range as factors of the workload's own length (default 0.25 and 4).  A mode that fails (FSEQ_E_OOM: the lists of
a length do not fit beside the alignment) is reported with the library's message and left out of the steps that follow.

Per entry: how its lists came about, the capacity, the DP's chunks, the event time of the entry alone (a folded entry: the fold
and the DP; a built one: phase C and the DP)."""
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


def main():
    import torch
    import bench
    pkg = importlib.import_module("founder-sequences_amd")
    name = next((a for a in sys.argv[1:] if not a.startswith("-")), "C3")
    w = bench.WORKLOADS[name]
    m, n, L = w["m"], w["n"], w["L"]
    steps = int(arg("steps", "3"))
    lo, hi = float(arg("lo", "0.25")), float(arg("hi", "4"))
    lengths = sorted({max(1, int(round(L * lo * (hi / lo) ** (i / 15)))) for i in range(16)})
    print("# tools/length_scan_probe.py %s on kernel sources %s: m %d, n %d, own L %d; lengths %s; %d timed steps of each mode, alternating, one warm-up each"
          % (name, bench.csrc_sha(), m, n, L, lengths, steps), flush=True)
    ctx = pkg.SegmentationContext(m, n, L, device=0)
    ctx.generate_synthetic(w["seed"], w["K"], w["B"], w["mu"], w["kind"])
    modes = ["scan", "rebuild"] + (["runs"] if name == "C3" else [])
    names = {0: "built", 1: "folded", 2: "none"}

    def one(mode, show):
        ctx.set_tuning("FSEQ_SCAN_REBUILD", "1" if mode == "rebuild" else None)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        if mode == "runs":
            sizes = []
            for x in lengths:
                ctx.set_segment_length(x)
                try:
                    ctx.run()
                except pkg.NoReduction:
                    pass
                sizes.append(ctx.result.max_segment_size)
            ctx.set_segment_length(L)
            torch.cuda.synchronize()
            dt = (time.perf_counter() - t0) * 1e3
            if show:
                print("runs     %9.1f ms | 16 full runs through fseq_set_segment_length (with traceback, merge and pass 2) | sizes %s" % (dt, sizes), flush=True)
            return dt, sizes
        entries, sm = ctx.scan_segment_lengths(lengths)
        torch.cuda.synchronize()
        dt = (time.perf_counter() - t0) * 1e3
        if show:
            print("%-8s %9.1f ms | A %.1f B %.1f | built %d folded %d short %d retries %d" % (mode, dt, sm["ms_phase_a"], sm["ms_phase_b"], sm["lists_built"],
                                                                                          sm["lists_folded"], sm["short_entries"], sm["retries"]), flush=True)
            for e in entries:
                print("    L %7d  K %6d  %-6s X %5d  chunks %4d  %9.3f ms" % (e["segment_length"], e["max_segment_size"], names[int(e["lists"])], e["list_cap"],
                                                                          e["dp_chunks"], e["ms_device"]), flush=True)
        return dt, [int(e["max_segment_size"]) for e in entries]

    for mode in list(modes):
        try:
            one(mode, False)                                # warm-up: allocations, code objects
        except pkg.FseqError as e:
            print("# %-8s FAILED in its warm-up and is left out: %s" % (mode, e), flush=True)
            modes.remove(mode)
    ms = {mode: [] for mode in modes}
    sizes = {}
    for s in range(steps):
        for mode in modes:
            dt, sz = one(mode, s == 0)
            ms[mode].append(dt)
            sizes.setdefault(tuple(sz), []).append(mode)
    for mode in modes:
        v = sorted(ms[mode])
        if not v:
            continue
        print("# %-8s median %.1f ms a call (min %.1f, max %.1f)" % (mode, v[len(v) // 2], v[0], v[-1]))
    print("# sizes: %s" % ("IDENTICAL in every mode" if len(sizes) == 1 else "DIFFER: %r" % sizes))


if __name__ == "__main__":
    main()
