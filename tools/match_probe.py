"""match_probe.py CONFIG JOIN [OUT] -- the device matcher beside the yardstick, on one machine in one session.

CONFIG: a name of oracle/fso.py's CONFIGS (C3: BASELINE's m = 2,504 x n = 1,000,000), JOIN: greedy | bipartite | random.
Device: fseq_match_founders on the resident alignment after run() and the join -- ms_device (HIP events: the founders'
columns and both walks) and the wall time of the call, median of RUNS after a warm-up, plus fseq_write_match.
Host: host/match_founder_sequences.cpp as built by build_aux, on at most 16 CPUs, on the same rows (one file each) and the
founders file fseq_write_founders_device wrote, all on tmpfs; its time includes reading them, as every use of the tool does.
Both reports must be the same bytes.  Writes profiles/match_CONFIG.txt (or OUT)."""
import importlib
import os
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "oracle")):
    sys.path.insert(0, p)
RUNS = 5


def main():
    import fso
    config, join = sys.argv[1], sys.argv[2]
    out_path = sys.argv[3] if len(sys.argv) > 3 else os.path.join(ROOT, "profiles", "match_%s.txt" % config)
    build = importlib.import_module("founder-sequences_amd.build")
    pkg = importlib.import_module("founder-sequences_amd")
    tool = dict(zip(build.AUX_TOOLS, build.build_aux()))["match_founder_sequences"]
    c = fso.CONFIGS[config]
    m, n, L = c["m"], c["n"], c["L"]
    ctx = pkg.SegmentationContext(m, n, L)
    ctx.generate_synthetic(c["seed"], c["K"], c["B"], c["mu"], c["kind"])
    res = ctx.run()
    perm = getattr(ctx, "join_" + join)()
    ctx.match_founders(perm)                                      # warm-up (allocates the buffers, loads the kernels)
    ms_device, ms_wall = [], []
    for _ in range(RUNS):
        t0 = time.perf_counter()
        s = ctx.match_founders(perm)
        ms_wall.append((time.perf_counter() - t0) * 1e3)
        ms_device.append(s["ms_device"])
    base = "/dev/shm" if os.path.isdir("/dev/shm") and os.access("/dev/shm", os.W_OK) else None
    with tempfile.TemporaryDirectory(dir=base) as tmp:
        t0 = time.perf_counter()
        ctx.write_match(os.path.join(tmp, "match_device.txt"))
        ms_report = (time.perf_counter() - t0) * 1e3
        ctx.write_founders_device(perm, os.path.join(tmp, "founders.txt"))
        msa = ctx.get_sequences()
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
    dev, wall, host = statistics.median(ms_device), statistics.median(ms_wall), min(ms_host)
    lines = [
        "match_probe %s %s: m = %d, n = %d, L = %d; %d founders (%d words a set), %d merged segments" % (config, join, m, n, L, s["n_founders"], s["set_words"], res.segment_count),
        "pieces %d, most in a row %d, uncovered cells %d, short pieces %d" % (s["pieces"], s["max_pieces_per_row"], s["uncovered_cells"], s["short_pieces"]),
        "device  fseq_match_founders: ms_device %.1f (median of %d: %s), wall time of the call %.1f ms (%s)" % (
            dev, RUNS, " ".join("%.1f" % x for x in ms_device), wall, " ".join("%.1f" % x for x in ms_wall)),
        "device  fseq_write_match (pieces to the host and the report on tmpfs): %.1f ms" % ms_report,
        "host    match_founder_sequences, %d threads, rows and founders read from tmpfs, report to tmpfs: %.1f ms (runs: %s)" % (len(cpus), host, " ".join("%.1f" % x for x in ms_host)),
        "host / device call (wall): %.1fx; the two reports are %s" % (host / wall, "the same bytes" if same else "DIFFERENT"),
    ]
    print("\n".join(lines))
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")
    ctx.close()
    return 0 if same else 1


if __name__ == "__main__":
    sys.exit(main())
