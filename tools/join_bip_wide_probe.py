#!/usr/bin/env python3
"""fseq_join_bipartite through the host joiner and through the wide device form (fseq_joinbipw.hpp), on the same contexts.

    python tools/join_bip_wide_probe.py sweep [--reps=5] [--max-gb=2.5] [--budget-s=0]    # the sweep behind JOIN_BIP_WIDE_MIN_BYTES
    python tools/join_bip_wide_probe.py C4 [--limit-s=900]               # BASELINE C4 once through fseq_join_bipartite, no knob set

sweep: founder mosaics (tests/helpers.founder_mosaic) with max_segment_size 256 and 1,024 whose boundary states
(segments x m x 8 bytes) go from about 1 MB to about 2 GB.  Every point holds two contexts on one input, one with
FSEQ_JOIN_HOST and one with FSEQ_JOIN_BIP_WIDE, segmented once; the two joins then alternate, --reps times (3 from 1 GB of
boundary states on, and fewer where one join takes seconds), after one untimed join each.  Reported: the median and the
spread (min .. max) of the whole call's wall time, and whether the permutations agree.  The threshold is the smallest swept
size from which the wide form is faster at every larger swept point, and never below 16 MiB.  A point whose alignment would
not fit the host's free memory, or that would start after --budget-s seconds (0: no limit), is skipped and named: a sweep
cut short supports a threshold only up to its largest point.

C4: generate_synthetic, run, join_bipartite in a child process under --limit-s seconds.  If the join does not finish within
them the tool says so and ends the child; a second run is not made."""
import importlib
import multiprocessing
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
PATHS = "0 host, 1 LDS form, 2 wide form"


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
    perm = ctx.join_bipartite()
    return (time.perf_counter() - t0) * 1e3, perm


def sweep():
    import bench
    from helpers import founder_mosaic
    pkg = importlib.import_module("founder-sequences_amd")
    reps, max_bytes, budget = int(arg("reps", "5")), float(arg("max-gb", "2.5")) * 1e9, float(arg("budget-s", "0"))
    t_start = time.perf_counter()
    print("# tools/join_bip_wide_probe.py sweep on kernel sources %s: fseq_join_bipartite, host joiner (FSEQ_JOIN_HOST) against the wide device form"
          % bench.csrc_sha())
    print("# (FSEQ_JOIN_BIP_WIDE) on the same input, alternating; founder mosaics, L = %d, blocks of %d columns; ms are wall time of the whole call" % (L, BREC))
    print("# %5s %6s %8s %6s %10s | %9s %19s | %9s %19s | %4s %6s %5s" % ("X", "m", "n", "S", "state MB", "host ms", "(min .. max)", "wide ms", "(min .. max)",
                                                                      "reps", "faster", "same"))
    rows = []
    cut = False
    for X, m, nb in sorted(POINTS, key=lambda p: (p[1] * p[2], p[0])):
        n = nb * BREC
        if nb * m * 8 > max_bytes:
            cut = True
            continue
        if budget and time.perf_counter() - t_start > budget:
            print("# skipped X = %d m = %d n = %d: it would start after the %.0f s the sweep was given" % (X, m, n, budget), flush=True)
            cut = True
            continue
        if 2.5 * m * n > mem_available():
            print("# skipped X = %d m = %d n = %d: the alignment (%.1f GB) does not fit the host's free memory" % (X, m, n, m * n / 1e9), flush=True)
            cut = True
            continue
        msa = founder_mosaic(X, m, n, brec=BREC, seed=X)
        ctxs = {}
        for knob in ("FSEQ_JOIN_HOST", "FSEQ_JOIN_BIP_WIDE"):
            ctx = pkg.SegmentationContext(m, n, L)
            ctx.set_tuning(knob)
            ctx.set_sequences(msa)
            r = ctx.run()
            ctxs[knob] = ctx
        del msa
        S, Xgot = int(r.segment_count), int(r.max_segment_size)
        ms = {k: [] for k in ctxs}
        perms = {}
        k_reps = min(reps, 3) if S * m * 8 >= 1e9 else reps
        for it in range(reps + 1):                           # (the first round is untimed)
            if it > k_reps:
                break
            for knob, ctx in ctxs.items():
                dt, perm = timed_join(ctx)
                if it == 0:
                    perms[knob] = perm
                    assert ctx.bipartite_path() == (0 if knob == "FSEQ_JOIN_HOST" else 2), (knob, ctx.bipartite_path())
                    if dt > 4000.0:
                        k_reps = min(k_reps, 3 if dt < 20000.0 else 1)
                else:
                    ms[knob].append(dt)
        h, w = sorted(ms["FSEQ_JOIN_HOST"]), sorted(ms["FSEQ_JOIN_BIP_WIDE"])
        same = np.array_equal(perms["FSEQ_JOIN_HOST"], perms["FSEQ_JOIN_BIP_WIDE"])
        med = lambda v: v[len(v) // 2]
        faster = "wide" if med(w) < med(h) else "host"
        rows.append((S * m * 8, Xgot, faster))
        print("  %5d %6d %8d %6d %10.1f | %9.2f (%7.2f .. %7.2f) | %9.2f (%7.2f .. %7.2f) | %4d %6s %5s"
              % (Xgot, m, n, S, S * m * 8 / 1e6, med(h), h[0], h[-1], med(w), w[0], w[-1], len(h), faster, "yes" if same else "NO"), flush=True)
        for ctx in ctxs.values():
            ctx.close()
    rows.sort()
    last_host = max([i for i, r in enumerate(rows) if r[2] == "host"], default=-1)
    if rows and last_host + 1 < len(rows):
        t = rows[last_host + 1][0]
        print("# the wide form is faster at every swept size from %.1f MB to %.1f MB; with the 16 MiB floor the threshold would be %d bytes (%.1f MiB)"
              % (t / 1e6, rows[-1][0] / 1e6, max(t, FLOOR), max(t, FLOOR) / float(1 << 20)))
    elif rows:
        print("# the host joiner is faster at the largest swept size: the sweep supports no threshold")
    if cut:
        print("# the sweep was cut short (points skipped above): nothing is measured beyond %.1f MB of boundary states" % (rows[-1][0] / 1e6 if rows else 0.0))


def c4_child(out):
    import bench
    pkg = importlib.import_module("founder-sequences_amd")
    w = bench.WORKLOADS["C4"]
    m, n = w["m"], w["n"]
    print("# tools/join_bip_wide_probe.py C4 on kernel sources %s: m = %d, n = %d, L = %d, no knob set" % (bench.csrc_sha(), m, n, w["L"]), flush=True)
    ctx = pkg.SegmentationContext(m, n, w["L"], device=0)
    ctx.generate_synthetic(w["seed"], w["K"], w["B"], w["mu"], w["kind"])
    ctx.run()
    t0 = time.perf_counter()
    r = ctx.run()
    print("segmentation %.1f ms: max_segment_size %d, %d merged segments, %.2f GB of boundary states"
          % ((time.perf_counter() - t0) * 1e3, r.max_segment_size, r.segment_count, r.segment_count * m * 8 / 1e9), flush=True)
    out.put("joining")
    dt, perm = timed_join(ctx)
    print("join_bipartite %.1f ms through path %d (%s): %s" % (dt, ctx.bipartite_path(), PATHS, ctx.join_profile()), flush=True)
    assert perm.max() < m
    out.put("done")


def c4():
    limit = float(arg("limit-s", "900"))
    ctx = multiprocessing.get_context("spawn")                 # (a fresh child: the parent never opens the device)
    q = ctx.Queue()
    child = ctx.Process(target=c4_child, args=(q,))
    t0 = time.perf_counter()
    child.start()
    child.join(limit)
    if child.is_alive():
        child.terminate()
        child.join(30)
        if child.is_alive():
            child.kill()
            child.join()
        said = []
        while not q.empty():
            said.append(q.get())
        print("# fseq_join_bipartite on C4 did not finish: ended after %.0f s (limit %.0f s, last stage: %s); no second run is made"
              % (time.perf_counter() - t0, limit, said[-1] if said else "setup"), flush=True)
        return 2
    return child.exitcode


if __name__ == "__main__":
    if "C4" in sys.argv[1:]:
        sys.exit(c4())
    else:
        sweep()
