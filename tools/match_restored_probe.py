"""match_restored_probe.py CONFIG [SHARE] [OUT] -- the restored match beside the reduced one and the yardstick, on one machine
in one session.

CONFIG: a name of oracle/fso.py's CONFIGS (C3: BASELINE's m = 2,504 x n = 1,000,000).  About SHARE (default 0.6) of its columns
are overwritten with row 0's symbol, which makes them identity columns; the context over the others
(fseq_create_without_identity_columns) is segmented and joined greedily.  Three times:
(a) fseq_match_founders_restored, min_segment_length 0 and MIN_LEN: the full-length rows against the restored founders;
(b) fseq_match_founders on the same reduced context: the walk without source positions and gap steps;
(c) host/match_founder_sequences.cpp as built by build_aux, on at most 16 CPUs, on the full-length rows (one file each) and the
    founders file fseq_write_founders_restored wrote, all on tmpfs; its time includes reading them.
(a) and (b): ms_device (HIP events: the founders' columns and both walks) and the wall time of the call, median of RUNS after a
warm-up.  The reports of (a) and (c) must be the same bytes.  Writes profiles/match_restored_CONFIG.txt (or OUT)."""
import importlib
import os
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "oracle")):
    sys.path.insert(0, p)
RUNS = 5
MIN_LEN = 50


def timed(call):
    call()                                                        # warm-up (allocates the buffers, loads the kernels)
    dev, wall = [], []
    for _ in range(RUNS):
        t0 = time.perf_counter()
        s = call()
        wall.append((time.perf_counter() - t0) * 1e3)
        dev.append(s["ms_device"])
    return s, dev, wall


def line_of(what, s, dev, wall):
    return "%s: ms_device %.1f (median of %d: %s), wall time of the call %.1f ms; pieces %d, most in a row %d, uncovered cells %d, short pieces %d" % (
        what, statistics.median(dev), RUNS, " ".join("%.1f" % x for x in dev), statistics.median(wall), s["pieces"], s["max_pieces_per_row"],
        s["uncovered_cells"], s["short_pieces"])


def main():
    import fso
    args = sys.argv[1:]
    config = args[0]
    share = float(args[1]) if len(args) > 1 else 0.6
    out_path = args[2] if len(args) > 2 else os.path.join(ROOT, "profiles", "match_restored_%s.txt" % config)
    build = importlib.import_module("founder-sequences_amd.build")
    pkg = importlib.import_module("founder-sequences_amd")
    tool = dict(zip(build.AUX_TOOLS, build.build_aux()))["match_founder_sequences"]
    c = fso.CONFIGS[config]
    m, n, L = c["m"], c["n"], c["L"]
    src = pkg.SegmentationContext(m, n, L)
    src.generate_synthetic(c["seed"], c["K"], c["B"], c["mu"], c["kind"])
    msa = src.get_sequences()
    src.close()
    ident = np.flatnonzero(np.random.default_rng(c["seed"]).random(n) < share)
    msa[:, ident] = msa[0:1, ident]                               # (columns are contiguous in what get_sequences returns)
    msa = np.ascontiguousarray(msa)                               # rows contiguous: they are written out one file each below
    src = pkg.SegmentationContext(m, n, L)
    src.set_sequences(msa)
    red = src.without_identity_columns(L)
    src.close()
    res = red.run()
    perm = red.join_greedy()
    s0, dev0, wall0 = timed(lambda: red.match_founders_restored(perm))
    base = "/dev/shm" if os.path.isdir("/dev/shm") and os.access("/dev/shm", os.W_OK) else None
    with tempfile.TemporaryDirectory(dir=base) as tmp:
        t0 = time.perf_counter()
        red.write_match(os.path.join(tmp, "match_device.txt"))
        ms_report = (time.perf_counter() - t0) * 1e3
        red.write_founders_restored(perm, os.path.join(tmp, "founders.txt"))
        sl, devl, walll = timed(lambda: red.match_founders_restored(perm, min_segment_length=MIN_LEN))
        sr, devr, wallr = timed(lambda: red.match_founders(perm))
        srl, devrl, wallrl = timed(lambda: red.match_founders(perm, min_segment_length=MIN_LEN))
        paths = []
        for r in range(m):
            paths.append(os.path.join(tmp, "s%d.txt" % r))
            with open(paths[-1], "wb") as f:
                f.write(msa[r].tobytes())
        del msa
        with open(os.path.join(tmp, "seqs.txt"), "w") as f:
            f.write("\n".join(paths) + "\n")
        cpus = sorted(os.sched_getaffinity(0))[:16]
        ms_host = []
        for _ in range(2):                                        # (the second run has every file in the page cache for sure)
            with open(os.path.join(tmp, "match_host.txt"), "wb") as f:
                t0 = time.perf_counter()
                subprocess.run([tool, "--sequences", os.path.join(tmp, "seqs.txt"), "--founders", os.path.join(tmp, "founders.txt"), "--founders-format", "text"],
                               stdout=f, stderr=subprocess.DEVNULL, check=True, preexec_fn=lambda: os.sched_setaffinity(0, cpus))
                ms_host.append((time.perf_counter() - t0) * 1e3)
        same = open(os.path.join(tmp, "match_host.txt"), "rb").read() == open(os.path.join(tmp, "match_device.txt"), "rb").read()
    host = min(ms_host)
    lines = [
        "match_restored_probe %s, identity share %.2f: m = %d, source n = %d, kept %d; L = %d; %d founders (%d words a set), %d merged segments" % (
            config, share, m, n, red.n, L, s0["n_founders"], s0["set_words"], res.segment_count),
        line_of("(a) device  fseq_match_founders_restored, min_len 0", s0, dev0, wall0),
        line_of("(a) device  fseq_match_founders_restored, min_len %d" % MIN_LEN, sl, devl, walll),
        line_of("(b) device  fseq_match_founders (reduced co-ordinates), min_len 0", sr, devr, wallr),
        line_of("(b) device  fseq_match_founders (reduced co-ordinates), min_len %d" % MIN_LEN, srl, devrl, wallrl),
        "    device  fseq_write_match of (a), min_len 0 (pieces to the host and the report on tmpfs): %.1f ms" % ms_report,
        "(c) host    match_founder_sequences, %d threads, full-length rows and restored founders read from tmpfs, report to tmpfs: %.1f ms (runs: %s)" % (
            len(cpus), host, " ".join("%.1f" % x for x in ms_host)),
        "(a) / (b), ms_device, min_len 0: %.2f; min_len %d: %.2f; (c) / (a) wall, min_len 0: %.1fx; the reports of (a) and (c) are %s" % (
            statistics.median(dev0) / statistics.median(devr), MIN_LEN, statistics.median(devl) / statistics.median(devrl),
            host / statistics.median(wall0), "the same bytes" if same else "DIFFERENT"),
    ]
    print("\n".join(lines))
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")
    red.close()
    return 0 if same else 1


if __name__ == "__main__":
    sys.exit(main())
