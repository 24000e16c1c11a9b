"""segments_restored_probe.py [CONFIG] [--share=0.6] [OUT] -- the segments file in source co-ordinates
(fseq_write_segments_restored) beside the one in reduced co-ordinates (fseq_write_segments_device) on the same context, measured
in one process (CONFIG: a name of oracle/fso.py's CONFIGS, C3 by default; writes profiles/segments_restored_CONFIG.txt or OUT).

The input is CONFIG's synthetic alignment with about SHARE of its columns overwritten with row 0's symbol (identity columns).
One context made by without_identity_columns(), one run.  For bipartite-matching and for random joining the two writers alternate
after a warm-up of each, both to tmpfs; whole-call wall time, medians of RUNS.  The reduced writer is the existing code and the
yardstick: the figure is the time per byte of file of either, and what the restored file's extra bytes cost."""
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


def main():
    import fso
    opts = {a.split("=")[0]: a.split("=")[1] for a in sys.argv[1:] if a.startswith("--")}
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    share = float(opts.get("--share", 0.6))
    config = args[0] if args else "C3"
    out_path = args[1] if len(args) > 1 else os.path.join(ROOT, "profiles", "segments_restored_%s.txt" % config)
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
    msa = np.ascontiguousarray(msa)
    src = pkg.SegmentationContext(m, n, L)
    src.set_sequences(msa)
    red = src.without_identity_columns(L)
    src.close()
    res = red.run()
    seg = red.segments_restored()
    ok = seg["lb"][0] == 0 and seg["rb"][-1] == n and np.array_equal(seg["lb"][1:], seg["rb"][:-1])
    widths = (seg["rb"] - seg["lb"]).astype(np.int64)
    kept_widths = (red.reduced_traceback()["rb"] - red.reduced_traceback()["lb"]).astype(np.int64)
    lines = ["segments_restored_probe %s: m = %d, n = %d, L = %d; identity share %.2f: kept %d columns; %d merged segments, max_segment_size %d; "
             "whole-call wall time to tmpfs, medians of %d, the two writers alternating" % (config, m, n, L, share, red.n, res.segment_count, res.max_segment_size, RUNS),
             "a segment's width, median / most: %d / %d kept columns, %d / %d source columns" % (
                 np.median(kept_widths), kept_widths.max(), np.median(widths), widths.max())]
    base = "/dev/shm" if os.path.isdir("/dev/shm") and os.access("/dev/shm", os.W_OK) else None
    with tempfile.TemporaryDirectory(dir=base) as tmp:
        for name, joining in (("bipartite-matching", pkg.JOIN_BIPARTITE), ("random", pkg.JOIN_RANDOM)):
            writers = (("reduced", red.write_segments_device), ("restored", red.write_segments_restored))
            ms = {w: [] for w, _ in writers}
            stats = {}
            for rnd in range(RUNS + 1):                          # (round 0: the warm-up of each)
                for w, call in writers:
                    path = os.path.join(tmp, "%s_%s.txt" % (w, joining))
                    t0 = time.perf_counter()
                    call(joining, path)
                    dt = (time.perf_counter() - t0) * 1e3
                    if rnd:
                        ms[w].append(dt)
                    stats[w] = red.segments_file_stats()
                    ok = ok and stats[w]["bytes"] == os.path.getsize(path)
            med = {w: statistics.median(ms[w]) for w in ms}
            b = {w: stats[w]["bytes"] for w in stats}
            ok = ok and stats["reduced"]["lines"] == stats["restored"]["lines"]
            lines.append("%s joining: %d lines" % (name, stats["restored"]["lines"]))
            for w in ("reduced", "restored"):
                lines.append("    %-8s %12d bytes in %d batch(es), longest line %8d: %8.1f ms (%s)  %.3f ns a byte" % (
                    w, b[w], stats[w]["batches"], stats[w]["longest_line"], med[w], " ".join("%.1f" % x for x in ms[w]), med[w] * 1e6 / b[w]))
            extra_b, extra_ms = b["restored"] - b["reduced"], med["restored"] - med["reduced"]
            lines.append("    restored / reduced: %.2fx the bytes, %.2fx the time; the %d extra bytes cost %.1f ms = %.3f ns a byte, %.2fx the reduced writer's rate" % (
                b["restored"] / b["reduced"], med["restored"] / med["reduced"], extra_b, extra_ms, extra_ms * 1e6 / extra_b,
                (extra_ms / extra_b) / (med["reduced"] / b["reduced"])))
    red.close()
    lines.append("the source bounds tile the source and the stats fit the files: %s" % ("yes" if ok else "NO"))
    print("\n".join(lines))
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
