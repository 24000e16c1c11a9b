"""upload_probe.py CONFIG [--columns N] [--staging-mib A,B,...] [OUT] -- the input in column chunks beside fseq_set_rows, on the
same rows in one process.

CONFIG: a name of oracle/fso.py's CONFIGS (C3: BASELINE's m = 2,504 x n = 1,000,000, 2.5 GB of raw rows); --columns takes the
first N columns.  The rows are the config's founder mosaic over ACGT (K founders, recombination every B columns), made on the
host.  Timed (wall, median of RUNS after a warm-up, each on a fresh context): fseq_set_rows; fseq_set_rows_streamed at every
staging size (default 16, 64, 256, 1024 MiB); the scan pass alone (fseq_input_begin and fseq_input_scan over [0, n)) and, from a
supplied alphabet, the encode pass alone (fseq_input_columns over [0, n), fseq_input_end).  With every figure the peak of the
context's device bytes (fseq_debug_device_bytes: accounting).  Every upload's matrix is read back once and compared.
Expectation to confirm or correct: the encode pass alone is no slower than fseq_set_rows (the same PCIe bytes), the whole
streamed call about one more pass over PCIe.  Writes profiles/upload_stream_CONFIG.txt (or OUT)."""
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


def mosaic(m, n, K, B, seed):
    rng = np.random.default_rng(seed & 0x7FFFFFFF)
    founders = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, size=(K, n), dtype=np.uint8)]
    msa = np.empty((m, n), dtype=np.uint8)
    for b0 in range(0, n, B):
        msa[:, b0:b0 + B] = founders[rng.integers(0, K, size=m), b0:b0 + B]
    return msa


def timed(pkg, m, n, L, upload, msa, check):
    """(median wall ms, peak device bytes) of upload(ctx) over RUNS fresh contexts after a warm-up"""
    ms, peak = [], 0
    for run in range(RUNS + 1):
        ctx = pkg.SegmentationContext(m, n, L)
        t0 = time.perf_counter()
        upload(ctx)
        ms.append((time.perf_counter() - t0) * 1e3)
        peak = max(peak, ctx.device_bytes()[1])
        if run == 0 and check:
            assert np.array_equal(ctx.get_sequences(0, min(n, 4096)), msa[:, :4096])
            assert np.array_equal(ctx.get_sequences(max(0, n - 4096), n), msa[:, max(0, n - 4096):])
        ctx.close()
    return statistics.median(ms[1:]), peak


def passes(ctx, msa, staging, scan, encode, alphabet=None):
    n = msa.shape[1]
    ctx.input_begin(alphabet=alphabet, staging_bytes=staging)
    width = ctx.input_chunk_columns()
    if width >= 128:
        width &= ~63
    for c0 in range(0, n, width) if scan else []:
        ctx.input_scan(c0, msa[:, c0:c0 + width])
    for c0 in range(0, n, width) if encode else []:
        ctx.input_columns(c0, msa[:, c0:c0 + width])
    if encode:
        ctx.input_end()


def main():
    import fso
    args = sys.argv[1:]
    config = args.pop(0)
    columns, stagings = None, [16, 64, 256, 1024]
    while args and args[0].startswith("--"):
        a = args.pop(0)
        if a == "--columns":
            columns = int(args.pop(0))
        elif a == "--staging-mib":
            stagings = [int(x) for x in args.pop(0).split(",")]
        else:
            raise SystemExit("unknown option " + a)
    out_path = args[0] if args else os.path.join(ROOT, "profiles", "upload_stream_%s.txt" % config)
    pkg = importlib.import_module("founder-sequences_amd")
    c = fso.CONFIGS[config]
    m, n, L = c["m"], columns or c["n"], c["L"]
    msa = mosaic(m, n, c["K"], c["B"], c["seed"])
    raw = m * n
    lines = ["upload_probe %s: m = %d, n = %d, %.1f MiB of raw rows, %.1f MiB packed at 2 bits; wall ms, median of %d; peak = the context's device bytes"
             % (config, m, n, raw / MiB, ((m + 3) // 4 + 15) // 16 * 16 * n / MiB, RUNS)]

    def row(name, ms, peak):
        lines.append("%-44s %10.2f ms  %8.2f GB/s of raw rows  peak %10.1f MiB" % (name, ms, raw / ms / 1e6, peak / MiB))
        print(lines[-1], flush=True)

    row("fseq_set_rows", *timed(pkg, m, n, L, lambda ctx: ctx.set_sequences(msa), msa, True))
    for s in stagings:
        row("fseq_set_rows_streamed, %d MiB staging" % s, *timed(pkg, m, n, L, lambda ctx: ctx.set_sequences(msa, staging_bytes=s * MiB), msa, True))
    s = stagings[len(stagings) // 2]
    row("scan pass alone, %d MiB staging" % s, *timed(pkg, m, n, L, lambda ctx: passes(ctx, msa, s * MiB, True, False), msa, False))
    row("encode pass alone (alphabet ACGT), %d MiB" % s, *timed(pkg, m, n, L, lambda ctx: passes(ctx, msa, s * MiB, False, True, b"ACGT"), msa, True))
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("wrote", out_path)


if __name__ == "__main__":
    main()
