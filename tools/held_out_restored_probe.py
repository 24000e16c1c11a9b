"""held_out_restored_probe.py [CONFIG] [--rows=256] [--share=0.6] [--rate=1e-4] [OUT] -- held-out rows matched against the restored
founders, measured in one process (CONFIG: a name of oracle/fso.py's CONFIGS, C3 by default; writes
profiles/held_out_restored_CONFIG.txt or OUT).

The input is CONFIG's synthetic alignment with about SHARE of its columns overwritten with row 0's symbol (identity columns); the
last ROWS rows are held out.  Twice: the held-out rows agree with row 0 in every identity column (no exception cell), and they
carry another symbol of the alphabet than they had in about RATE of their cells, in identity and kept columns alike (the
alphabet and with it the packing stay the same).
(a) without_rows + without_identity_columns(keep_held_out=True) beside the two plain calls (ms_device: the summaries' HIP event
    times, which do not cover the held-out rows' part of the second call; wall: both calls);
(b) match_held_out_restored beside match_founders_restored on the same context: the same unsplit walk, over ROWS query rows with
    their exception lists and over the alignment's rows;
(c) host/match_founder_sequences.cpp as built by build_aux on at most 16 CPUs, on the full-length held-out rows (one file each)
    and the founders file write_founders_restored wrote, all on tmpfs; its report must be the bytes of (b)'s.
(a) and (b) alternate after a warm-up of each; medians of RUNS."""
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
RUNS = 3


def alternate(variants):
    """[(name, call -> (ms_device, wall))] -> {name: (median ms_device, median wall)} after a warm-up of each"""
    times = {name: ([], []) for name, _ in variants}
    for _, call in variants:
        call()
    for _ in range(RUNS):
        for name, call in variants:
            dev, wall = call()
            times[name][0].append(dev)
            times[name][1].append(wall)
    return {name: (statistics.median(d), statistics.median(w)) for name, (d, w) in times.items()}


def main():
    import fso
    opts = {a.split("=")[0]: a.split("=")[1] for a in sys.argv[1:] if a.startswith("--")}
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    rows, share, rate = int(opts.get("--rows", 256)), float(opts.get("--share", 0.6)), float(opts.get("--rate", 1e-4))
    config = args[0] if args else "C3"
    out_path = args[1] if len(args) > 1 else os.path.join(ROOT, "profiles", "held_out_restored_%s.txt" % config)
    build = importlib.import_module("founder-sequences_amd.build")
    pkg = importlib.import_module("founder-sequences_amd")
    tool = dict(zip(build.AUX_TOOLS, build.build_aux()))["match_founder_sequences"]
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
    held = np.arange(m - rows, m, dtype=np.uint32)
    lines = ["held_out_restored_probe %s: m = %d, n = %d, L = %d; identity share %.2f; the last %d rows held out; medians of %d, alternating" % (
        config, m, n, L, share, rows, RUNS)]
    ok = True
    alphabet = np.unique(msa[0])
    nxt = np.zeros(256, dtype=np.uint8)
    nxt[alphabet] = np.roll(alphabet, -1)
    for tag, cell_rate in (("no exception cell", 0.0), ("another symbol in %.0e of the held-out rows' cells" % rate, rate)):
        if cell_rate:
            hit = rng.random((rows, n)) < cell_rate
            tail = msa[m - rows:]
            tail[hit] = nxt[tail[hit]]
            del hit
        src = pkg.SegmentationContext(m, n, L)
        src.set_sequences(msa)

        def plain_calls():
            t0 = time.perf_counter()
            sub = src.without_rows(held, L)
            red = sub.without_identity_columns(L)
            wall = (time.perf_counter() - t0) * 1e3
            dev = sub.held_out_summary["ms_device"] + red.identity_summary["ms_device"]
            sub.close()
            red.close()
            return dev, wall

        def held_calls():
            t0 = time.perf_counter()
            sub = src.without_rows(held, L)
            red = sub.without_identity_columns(L, keep_held_out=True)
            wall = (time.perf_counter() - t0) * 1e3
            dev = sub.held_out_summary["ms_device"] + red.identity_summary["ms_device"]
            sub.close()
            red.close()
            return dev, wall

        made = alternate([("plain", plain_calls), ("held", held_calls)])
        sub = src.without_rows(held, L)
        src.close()
        red = sub.without_identity_columns(L, keep_held_out=True)
        sub.close()
        res = red.run()
        perm = red.join_greedy()
        last = {}

        def restored_rows():
            t0 = time.perf_counter()
            s = red.match_founders_restored(perm)
            return s["ms_device"], (time.perf_counter() - t0) * 1e3

        def restored_held():
            t0 = time.perf_counter()
            last["s"] = red.match_held_out_restored(perm)
            return last["s"]["ms_device"], (time.perf_counter() - t0) * 1e3

        walked = alternate([("rows", restored_rows), ("held", restored_held)])
        s = last["s"]
        off, _ = red.match_exceptions()
        per_row = np.diff(off.astype(np.int64))
        base = "/dev/shm" if os.path.isdir("/dev/shm") and os.access("/dev/shm", os.W_OK) else None
        with tempfile.TemporaryDirectory(dir=base) as tmp:
            red.write_match(os.path.join(tmp, "match_device.txt"))
            red.write_founders_restored(perm, os.path.join(tmp, "founders.txt"))
            paths = []
            for r in range(m - rows, m):
                paths.append(os.path.join(tmp, "s%d.txt" % r))
                with open(paths[-1], "wb") as f:
                    f.write(msa[r].tobytes())
            with open(os.path.join(tmp, "seqs.txt"), "w") as f:
                f.write("\n".join(paths) + "\n")
            cpus = sorted(os.sched_getaffinity(0))[:16]
            ms_host = []
            for _ in range(2):                                    # (the second run has every file in the page cache for sure)
                with open(os.path.join(tmp, "match_host.txt"), "wb") as f:
                    t0 = time.perf_counter()
                    subprocess.run([tool, "--sequences", os.path.join(tmp, "seqs.txt"), "--founders", os.path.join(tmp, "founders.txt"), "--founders-format", "text"],
                                   stdout=f, stderr=subprocess.DEVNULL, check=True, preexec_fn=lambda: os.sched_setaffinity(0, cpus))
                    ms_host.append((time.perf_counter() - t0) * 1e3)
            same = open(os.path.join(tmp, "match_host.txt"), "rb").read() == open(os.path.join(tmp, "match_device.txt"), "rb").read()
        ok = ok and same
        lines += [
            "%s: kept %d of %d columns; %d founders (%d words a set), %d merged segments; exception cells a held-out row: mean %.1f, most %d, %d in all" % (
                tag, red.n, n, s["n_founders"], s["set_words"], res.segment_count, per_row.mean(), per_row.max(), per_row.sum()),
            "    (a) without_rows + without_identity_columns                       ms_device %9.2f  wall %9.1f" % made["plain"],
            "    (a) without_rows + without_identity_columns(keep_held_out=True)   ms_device %9.2f  wall %9.1f" % made["held"],
            "    (b) match_founders_restored, %4d rows of the alignment           ms_device %9.2f  wall %9.1f" % ((red.m,) + walked["rows"]),
            "    (b) match_held_out_restored, %4d held-out rows                   ms_device %9.2f  wall %9.1f; pieces %d, most in a row %d, uncovered cells %d" % (
                (rows,) + walked["held"] + (s["pieces"], s["max_pieces_per_row"], s["uncovered_cells"])),
            "    (c) host match_founder_sequences, %d threads, files on tmpfs: %.1f ms (runs: %s); (c) / (b) wall %.1fx; the reports are %s" % (
                len(cpus), min(ms_host), " ".join("%.1f" % x for x in ms_host), min(ms_host) / walked["held"][1], "the same bytes" if same else "DIFFERENT"),
            "    held / rows, ms_device of the walk: %.2f; keep_held_out / plain, wall of the two calls: %.2f" % (
                walked["held"][0] / walked["rows"][0], made["held"][1] / made["plain"][1]),
        ]
        red.close()
    print("\n".join(lines))
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
