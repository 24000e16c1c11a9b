#!/usr/bin/env python3
"""fseq_join_greedy through the all-host joiner and through the wide device front (fseq_joinprep.hpp), on the same contexts.

    python tools/join_wide_probe.py sweep [--reps=5] [--max-gb=2.5] [--budget-s=0]     # the sweep behind JOIN_WIDE_MIN_BYTES
    python tools/join_wide_probe.py C4                                   # BASELINE C4 end to end through the wide front

sweep: founder mosaics (tests/helpers.founder_mosaic) with max_segment_size 256 and 1,024 whose boundary states
(segments x m x 8 bytes) go from about 1 MB to a few GB.  Every point holds two contexts on one input, one with
FSEQ_JOIN_HOST and one with FSEQ_JOIN_WIDE, segmented once; the two joins then alternate, --reps times (fewer where one
join takes seconds), after one untimed join each.  Reported: the median and the spread (min .. max) of the call's wall time,
which ends in the host's drawing, and whether the permutations agree.  The threshold is the smallest swept size from which
the wide front is faster at every larger swept point, and never below 16 MiB.  A point whose alignment would not fit the
host's free memory, or that would start after --budget-s seconds (0: no limit), is skipped and named.

C4: generate_synthetic, run, join_greedy (no knob), write_founders_device to /dev/null: the join profile, the path that ran
and the edge total."""
import importlib
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

FLOOR = 16 << 20
L, BREC = 10, 40                                               # segment length and the mosaic's block: short, to keep the alignment small
# (X, m, blocks): blocks x m x 8 bytes of boundary states where every block stays a segment of its own
POINTS = [(256, 512, 256), (256, 1024, 512), (256, 2048, 1024), (256, 4096, 2048), (256, 8192, 4096), (256, 16384, 8192), (256, 32768, 8192),
          (1024, 2048, 64), (1024, 2048, 256), (1024, 4096, 512), (1024, 4096, 2048), (1024, 8192, 4096), (1024, 16384, 8192), (1024, 32768, 8192)]


def arg(name, default):
    for a in sys.argv[1:]:
        if a.startswith("--%s=" % name):
            return a.split("=", 1)[1]
    return default


def mem_available():
    for line in open("/proc/meminfo"):
        if line.startswith("MemAvailable:"):
            return int(line.split()[1]) * 1024
    return 0


def timed_join(ctx):
    t0 = time.perf_counter()
    perm = ctx.join_greedy()
    return (time.perf_counter() - t0) * 1e3, perm


def sweep():
    import bench
    from helpers import founder_mosaic
    pkg = importlib.import_module("founder-sequences_amd")
    reps, max_bytes, budget = int(arg("reps", "5")), float(arg("max-gb", "2.5")) * 1e9, float(arg("budget-s", "0"))
    t_start = time.perf_counter()
    print("# tools/join_wide_probe.py sweep on kernel sources %s: fseq_join_greedy, all-host joiner (FSEQ_JOIN_HOST) against the wide device front"
          % bench.csrc_sha())
    print("# (FSEQ_JOIN_WIDE) on the same input, alternating; founder mosaics, L = %d, blocks of %d columns; ms are wall time of the whole call" % (L, BREC))
    print("# %5s %6s %8s %6s %10s | %9s %19s | %9s %19s %10s | %4s %6s %5s" % ("X", "m", "n", "S", "state MB", "host ms", "(min .. max)", "wide ms", "(min .. max)",
                                                                             "edges", "reps", "faster", "same"))
    rows = []
    for X, m, nb in sorted(POINTS, key=lambda p: (p[1] * p[2], p[0])):
        n = nb * BREC
        if nb * m * 8 > max_bytes:
            continue
        if budget and time.perf_counter() - t_start > budget:
            print("# skipped X = %d m = %d n = %d: it would start after the %.0f s the sweep was given" % (X, m, n, budget), flush=True)
            continue
        if 2.5 * m * n > mem_available():
            print("# skipped X = %d m = %d n = %d: the alignment (%.1f GB) does not fit the host's free memory" % (X, m, n, m * n / 1e9), flush=True)
            continue
        msa = founder_mosaic(X, m, n, brec=BREC, seed=X)
        ctxs = {}
        for knob in ("FSEQ_JOIN_HOST", "FSEQ_JOIN_WIDE"):
            ctx = pkg.SegmentationContext(m, n, L)
            ctx.set_tuning(knob)
            ctx.set_sequences(msa)
            r = ctx.run()
            ctxs[knob] = ctx
        del msa
        S, Xgot = int(r.segment_count), int(r.max_segment_size)
        ms = {k: [] for k in ctxs}
        perms = {}
        k_reps = reps
        for it in range(reps + 1):                           # (the first round is untimed)
            if it > k_reps:
                break
            for knob, ctx in ctxs.items():
                dt, perm = timed_join(ctx)
                if it == 0:
                    perms[knob] = perm
                    assert ctx.join_path() == (0 if knob == "FSEQ_JOIN_HOST" else 2), (knob, ctx.join_path())
                    if dt > 4000.0:
                        k_reps = min(k_reps, 3 if dt < 20000.0 else 2)
                else:
                    ms[knob].append(dt)
        wide_ctx = ctxs["FSEQ_JOIN_WIDE"]
        edges = (wide_ctx.join_profile()["bytes_d2h"] - S * (2 * Xgot + 3) * 4) // 8
        h, w = sorted(ms["FSEQ_JOIN_HOST"]), sorted(ms["FSEQ_JOIN_WIDE"])
        same = np.array_equal(perms["FSEQ_JOIN_HOST"], perms["FSEQ_JOIN_WIDE"])
        med = lambda v: v[len(v) // 2]
        faster = "wide" if med(w) < med(h) else "host"
        rows.append((S * m * 8, Xgot, faster))
        print("  %5d %6d %8d %6d %10.1f | %9.2f (%7.2f .. %7.2f) | %9.2f (%7.2f .. %7.2f) %10d | %4d %6s %5s"
              % (Xgot, m, n, S, S * m * 8 / 1e6, med(h), h[0], h[-1], med(w), w[0], w[-1], edges, len(h), faster, "yes" if same else "NO"), flush=True)
        for ctx in ctxs.values():
            ctx.close()
    rows.sort()
    last_host = max([i for i, r in enumerate(rows) if r[2] == "host"], default=-1)
    if last_host + 1 < len(rows):
        t = rows[last_host + 1][0]
        print("# the wide front is faster at every swept size from %.1f MB on; with the 16 MiB floor the threshold is %d bytes (%.1f MiB)"
              % (t / 1e6, max(t, FLOOR), max(t, FLOOR) / float(1 << 20)))
    else:
        print("# the host joiner is faster at the largest swept size: the sweep supports no threshold")


def c4():
    import bench
    pkg = importlib.import_module("founder-sequences_amd")
    w = bench.WORKLOADS["C4"]
    m, n = w["m"], w["n"]
    print("# tools/join_wide_probe.py C4 on kernel sources %s: m = %d, n = %d, L = %d, no knob set" % (bench.csrc_sha(), m, n, w["L"]), flush=True)
    ctx = pkg.SegmentationContext(m, n, w["L"], device=0)
    ctx.generate_synthetic(w["seed"], w["K"], w["B"], w["mu"], w["kind"])
    ctx.run()
    t0 = time.perf_counter()
    r = ctx.run()
    print("segmentation %.1f ms: max_segment_size %d, %d merged segments, %.2f GB of boundary states"
          % ((time.perf_counter() - t0) * 1e3, r.max_segment_size, r.segment_count, r.segment_count * m * 8 / 1e9), flush=True)
    dt, perm = timed_join(ctx)
    jp = ctx.join_profile()
    S, X = int(r.segment_count), int(r.max_segment_size)
    print("join_greedy %.1f ms through path %d (0 host, 1 LDS front, 2 wide front): %s" % (dt, ctx.join_path(), jp), flush=True)
    print("edges %d (%.1f a pair)" % ((jp["bytes_d2h"] - S * (2 * X + 3) * 4) // 8, (jp["bytes_d2h"] - S * (2 * X + 3) * 4) / 8.0 / max(1, S - 1)), flush=True)
    assert perm.max() < m
    t0 = time.perf_counter()
    ctx.write_founders_device(perm, "/dev/null")
    print("write_founders_device to /dev/null %.1f ms (%d lines of %d bytes)" % ((time.perf_counter() - t0) * 1e3, X, n + 1), flush=True)


if __name__ == "__main__":
    if "C4" in sys.argv[1:]:
        c4()
    else:
        sweep()
