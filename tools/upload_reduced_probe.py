"""upload_reduced_probe.py CONFIG [--columns N] [--staging-mib S] [OUT] -- the chunked input that drops the identity columns on
the way beside the existing way to the same context, on the same rows in one process.

CONFIG: a name of oracle/fso.py's CONFIGS (C3: BASELINE's m = 2,504 x n = 1,000,000, 2.5 GB of raw rows); --columns takes the
first N columns.  The rows are the config's founder mosaic over ACGT (K founders, recombination every B columns) with a few cells
changed, so that no column is an identity column by itself, and then 0, 0.6 and 0.95 of the columns overwritten with row 0's byte.
At each share, alternating in one process, wall ms as the median of RUNS after a warm-up of each, every run on fresh contexts:
  new   fseq_set_rows_streamed_without_identity_columns
  old   fseq_set_rows_streamed, then fseq_create_without_identity_columns (the source closed afterwards)
both at the same staging (default 256 MiB), with the peak of the device bytes of the contexts of a run together
(fseq_debug_device_bytes: accounting).  The warm-up runs compare the two contexts: packed columns, mask and kept list.
At the first share also the scan passes alone: fseq_input_scan_identity beside fseq_input_scan over [0, n).
Expectation to confirm or correct: both ways are bound by two passes over PCIe, so the new one is no slower at 0.6 and 0.95; the
identity scan costs about what the presence scan costs; at 0 the scattered encode may be slower than k_input_encode.
Writes profiles/upload_reduced_CONFIG.txt (or OUT)."""
import importlib
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "oracle")):
    sys.path.insert(0, p)
RUNS = 3
MiB = 1 << 20
SHARES = [0.0, 0.6, 0.95]


def mosaic(m, n, K, B, seed):
    rng = np.random.default_rng(seed & 0x7FFFFFFF)
    alpha = np.frombuffer(b"ACGT", dtype=np.uint8)
    founders = alpha[rng.integers(0, 4, size=(K, n), dtype=np.uint8)]
    msa = np.empty((m, n), dtype=np.uint8)
    for b0 in range(0, n, B):
        msa[:, b0:b0 + B] = founders[rng.integers(0, K, size=m), b0:b0 + B]
    # every column differs from row 0 somewhere: one cell of it, in a row of its own, takes another byte
    rows = rng.integers(1, m, size=n)
    cols = np.arange(n)
    msa[rows, cols] = alpha[(np.searchsorted(alpha, msa[0]) + 1) % 4]
    return msa


def new_way(pkg, m, n, L, msa, staging):
    src = pkg.SegmentationContext(m, n, L)
    t0 = time.perf_counter()
    new = src.set_sequences_without_identity_columns(msa, L, staging_bytes=staging)
    ms = (time.perf_counter() - t0) * 1e3
    peak = src.device_bytes()[1] + new.device_bytes()[1]
    src.close()
    return ms, peak, new


def old_way(pkg, m, n, L, msa, staging):
    src = pkg.SegmentationContext(m, n, L)
    t0 = time.perf_counter()
    src.set_sequences(msa, staging_bytes=staging)
    new = src.without_identity_columns(L)
    ms = (time.perf_counter() - t0) * 1e3
    peak = src.device_bytes()[1] + new.device_bytes()[1]
    src.close()
    return ms, peak, new


def scan_alone(pkg, m, n, L, msa, staging, identity):
    ctx = pkg.SegmentationContext(m, n, L)
    t0 = time.perf_counter()
    ctx.input_begin(staging_bytes=staging)
    width = ctx.input_chunk_columns()
    if width >= 128:
        width &= ~63
    for c0 in range(0, n, width):
        (ctx.input_scan_identity if identity else ctx.input_scan)(c0, msa[:, c0:c0 + width])
    ctx.device_bytes()                                         # (a call returns when its copies are done: the last kernel is waited for by close)
    ctx.close()
    return (time.perf_counter() - t0) * 1e3


def main():
    import fso
    args = sys.argv[1:]
    config = args.pop(0)
    columns, staging = None, 256
    while args and args[0].startswith("--"):
        a = args.pop(0)
        if a == "--columns":
            columns = int(args.pop(0))
        elif a == "--staging-mib":
            staging = int(args.pop(0))
        else:
            raise SystemExit("unknown option " + a)
    out_path = args[0] if args else os.path.join(ROOT, "profiles", "upload_reduced_%s.txt" % config)
    pkg = importlib.import_module("founder-sequences_amd")
    c = fso.CONFIGS[config]
    m, n, L = c["m"], columns or c["n"], c["L"]
    base = mosaic(m, n, c["K"], c["B"], c["seed"])
    raw = m * n
    lines = ["upload_reduced_probe %s: m = %d, n = %d, %.1f MiB of raw rows, %.1f MiB packed at 2 bits, %d MiB staging; wall ms, median of %d, alternating; peak = the device bytes of a run's contexts together"
             % (config, m, n, raw / MiB, ((m + 3) // 4 + 15) // 16 * 16 * n / MiB, staging, RUNS)]

    def say(text):
        lines.append(text)
        print(text, flush=True)

    for share in SHARES:
        msa = base
        if share:
            msa = np.array(base)
            ident = np.random.default_rng(17).random(n) < share
            msa[:, ident] = msa[0:1, ident]
        t = {"new": [], "old": []}
        peaks = {"new": 0, "old": 0}
        kept = 0
        for run in range(RUNS + 1):
            got = {}
            for way, fn in (("new", new_way), ("old", old_way)):
                ms, peak, ctx = fn(pkg, m, n, L, msa, staging * MiB)
                t[way].append(ms)
                peaks[way] = max(peaks[way], peak)
                if run == 0:
                    k = ctx.n
                    got[way] = (k, ctx.packed_columns(0, min(k, 2048))[0].tobytes(), ctx.packed_columns(max(0, k - 2048), k)[0].tobytes(),
                                ctx.identity_mask().tobytes(), ctx.kept_columns().tobytes())
                    kept = k
                ctx.close()
            if run == 0:
                assert got["new"] == got["old"], "the two ways disagree"
        new_ms, old_ms = statistics.median(t["new"][1:]), statistics.median(t["old"][1:])
        say("identity share %.2f (%d of %d columns kept):" % (share, kept, n))
        say("  %-66s %10.2f ms  %7.2f GB/s of raw rows  peak %10.1f MiB" % ("new  fseq_set_rows_streamed_without_identity_columns", new_ms, raw / new_ms / 1e6, peaks["new"] / MiB))
        say("  %-66s %10.2f ms  %7.2f GB/s of raw rows  peak %10.1f MiB" % ("old  fseq_set_rows_streamed + fseq_create_without_identity_columns", old_ms, raw / old_ms / 1e6, peaks["old"] / MiB))
        say("  new / old = %.3f" % (new_ms / old_ms))
        if share == SHARES[0]:
            s = {True: [], False: []}
            for run in range(RUNS + 1):
                for identity in (True, False):
                    s[identity].append(scan_alone(pkg, m, n, L, msa, staging * MiB, identity))
            a, b = statistics.median(s[True][1:]), statistics.median(s[False][1:])
            say("  %-66s %10.2f ms  %7.2f GB/s of raw rows" % ("scan pass alone: fseq_input_scan_identity over [0, n)", a, raw / a / 1e6))
            say("  %-66s %10.2f ms  %7.2f GB/s of raw rows" % ("scan pass alone: fseq_input_scan over [0, n)", b, raw / b / 1e6))
            say("  identity scan / presence scan = %.3f" % (a / b))
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("wrote", out_path)


if __name__ == "__main__":
    main()
