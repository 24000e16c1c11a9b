"""identity_probe.py CONFIG [--columns N] [--share S] [--no-host] [OUT] -- the identity-column path beside a copy of the same
bytes and beside the host tool, on one machine in one session.

CONFIG: a name of oracle/fso.py's CONFIGS (C3: BASELINE's m = 2,504 x n = 1,000,000); --columns takes the first N columns of
it (C4's 125 GB and a copy of them do not fit one card together).  The alignment is the config's founder mosaic (K founders,
recombination every B columns, no mutations), put together packed at 2 bits on the device by torch and handed over as
borrowed packed columns; a share S (default 0.9) of the columns is overwritten with row 0's symbol.
Timed, median of RUNS after a warm-up: the mask pass (fseq_identity_columns, HIP events), mask + scan + gather
(fseq_create_without_identity_columns, HIP events), one hipMemcpyAsync device-to-device of the same alignment bytes (HIP
events, same process), and -- after run() and the greedy join on the reduced context -- fseq_write_founders_restored to tmpfs
(wall).  Host (unless --no-host): host/remove_identity_columns.cpp as built by build_aux on the same rows, one file each on
tmpfs, at most 16 CPUs; its mask must be the same bytes.  Writes profiles/identity_columns_CONFIG.txt (or OUT)."""
import ctypes
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


def mosaic_packed(torch, m, n, K, B, share, seed):
    """[n, ld] bytes: column-major 2-bit codes of a K-founder mosaic, `share` of the columns all row 0's code"""
    g = torch.Generator(device="cuda").manual_seed(seed & 0x7FFFFFFF)
    ld = ((m + 3) // 4 + 15) // 16 * 16
    founders = torch.randint(0, 4, (K, n), dtype=torch.uint8, device="cuda", generator=g)
    ident = torch.rand(n, device="cuda", generator=g) < share
    out = torch.empty((n, ld), dtype=torch.uint8, device="cuda")
    step = max(1, min(B, (1 << 28) // (4 * ld)))                   # (at most 256 MB of unpacked codes at a time)
    pick = None
    for c0 in range(0, n, step):
        c1 = min(n, c0 + step)
        if pick is None or c0 % B < step:
            pick = torch.randint(0, K, (m,), device="cuda", generator=g)
        codes = torch.zeros((c1 - c0, 4 * ld), dtype=torch.uint8, device="cuda")
        codes[:, :m] = founders[:, c0:c1].t()[:, pick]
        codes[:, :m] = torch.where(ident[c0:c1, None], codes[:, :1], codes[:, :m])
        q = codes.view(c1 - c0, ld, 4)
        out[c0:c1] = q[..., 0] | (q[..., 1] << 2) | (q[..., 2] << 4) | (q[..., 3] << 6)
    return out, ld


def main():
    import fso
    import torch
    args = sys.argv[1:]
    config = args.pop(0)
    columns, share, host = None, 0.9, True
    while args and args[0].startswith("--"):
        a = args.pop(0)
        if a == "--columns":
            columns = int(args.pop(0))
        elif a == "--share":
            share = float(args.pop(0))
        elif a == "--no-host":
            host = False
        else:
            raise SystemExit("unknown option " + a)
    out_path = args[0] if args else os.path.join(ROOT, "profiles", "identity_columns_%s.txt" % config)
    build = importlib.import_module("founder-sequences_amd.build")
    pkg = importlib.import_module("founder-sequences_amd")
    c = fso.CONFIGS[config]
    m, n, L = c["m"], columns or c["n"], c["L"]
    buf, ld = mosaic_packed(torch, m, n, c["K"], c["B"], share, c["seed"])
    nbytes = buf.numel()
    ctx = pkg.SegmentationContext(m, n, L)
    ctx.set_device_columns_packed(buf.data_ptr(), ld, 4, 2, keepalive=buf)

    ctx.identity_columns()                                        # warm-up (loads the kernels)
    ms_mask = []
    for _ in range(RUNS):
        mask, s = ctx.identity_columns()
        ms_mask.append(s["ms_device"])
    ms_all = []
    for _ in range(RUNS):
        red = ctx.without_identity_columns(L)
        ms_all.append(red.identity_summary["ms_device"])
        red.close()

    # the same bytes once more, device to device, by the runtime's own copy
    hip = ctypes.CDLL("libamdhip64.so")
    hip.hipMemcpyAsync.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_void_p]
    ms_copy = []
    dst = torch.empty_like(buf)
    for i in range(RUNS + 1):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        rc = hip.hipMemcpyAsync(dst.data_ptr(), buf.data_ptr(), nbytes, 3, torch.cuda.current_stream().cuda_stream)
        e1.record()
        torch.cuda.synchronize()
        assert rc == 0
        if i:
            ms_copy.append(e0.elapsed_time(e1))
    del dst

    red = ctx.without_identity_columns(L)
    res = red.run()
    perm = red.join_greedy()
    base = "/dev/shm" if os.path.isdir("/dev/shm") and os.access("/dev/shm", os.W_OK) else None
    same, ms_host = None, []
    with tempfile.TemporaryDirectory(dir=base) as tmp:
        ms_write = []
        for _ in range(3):
            t0 = time.perf_counter()
            red.write_founders_restored(perm, os.path.join(tmp, "founders.txt"))
            ms_write.append((time.perf_counter() - t0) * 1e3)
        founders_bytes = os.path.getsize(os.path.join(tmp, "founders.txt"))
        if host:
            tool = dict(zip(build.AUX_TOOLS, build.build_aux()))["remove_identity_columns"]
            red.write_identity_columns(os.path.join(tmp, "mask_device.txt"))
            msa = ctx.get_sequences()
            os.mkdir(os.path.join(tmp, "in"))
            os.mkdir(os.path.join(tmp, "out"))
            paths = []
            for r in range(m):
                paths.append(os.path.join(tmp, "in", "s%d" % r))
                with open(paths[-1], "wb") as f:
                    f.write(msa[r].tobytes())
            del msa
            with open(os.path.join(tmp, "list.txt"), "w") as f:
                f.write("\n".join(paths) + "\n")
            cpus = sorted(os.sched_getaffinity(0))[:16]
            for _ in range(2):                                    # (the second run has every file in the page cache for sure)
                with open(os.path.join(tmp, "mask_host.txt"), "wb") as f:
                    t0 = time.perf_counter()
                    subprocess.run([tool, "--input", os.path.join(tmp, "list.txt"), "--overwrite"], stdout=f, stderr=subprocess.DEVNULL, check=True,
                                   cwd=os.path.join(tmp, "out"), preexec_fn=lambda: os.sched_setaffinity(0, cpus))
                    ms_host.append((time.perf_counter() - t0) * 1e3)
            same = open(os.path.join(tmp, "mask_host.txt"), "rb").read() == open(os.path.join(tmp, "mask_device.txt"), "rb").read()
    med = statistics.median
    fmt = lambda xs: " ".join("%.3f" % x for x in xs)
    lines = [
        "identity_probe %s: m = %d, n = %d, L = %d; %d bytes a column (ld %d), %.3f GB of alignment; %d of %d columns are identity columns (%.1f %%)" % (
            config, m, n, L, (m + 3) // 4, ld, nbytes / 1e9, s["identity"], n, 100.0 * s["identity"] / n),
        "mask pass (fseq_identity_columns, HIP events): %.3f ms = %.0f GB/s read (median of %d: %s)" % (med(ms_mask), nbytes / med(ms_mask) / 1e6, RUNS, fmt(ms_mask)),
        "hipMemcpyAsync device to device of the same %.3f GB (HIP events): %.3f ms = %.0f GB/s read + as much written (%s)" % (nbytes / 1e9, med(ms_copy), nbytes / med(ms_copy) / 1e6, fmt(ms_copy)),
        "mask pass / copy: %.2f" % (med(ms_mask) / med(ms_copy)),
        "mask + scan + gather (fseq_create_without_identity_columns, HIP events): %.3f ms (%s)" % (med(ms_all), fmt(ms_all)),
        "reduced context: n = %d, max segment size %d, %d merged segments" % (red.n, res.max_segment_size, res.segment_count),
        "fseq_write_founders_restored, greedy join, %d lines of %d bytes to tmpfs (wall): %.1f ms (%s)" % (res.max_segment_size, n + 1, min(ms_write), fmt(ms_write)),
    ]
    assert founders_bytes == res.max_segment_size * (n + 1)
    if host:
        lines += [
            "host    remove_identity_columns, rows read from tmpfs, reduced rows and mask to tmpfs, %d CPUs allowed: %.1f ms (runs: %s)" % (len(cpus), min(ms_host), fmt(ms_host)),
            "host / device (mask + scan + gather): %.0fx; the two masks are %s" % (min(ms_host) / med(ms_all), "the same bytes" if same else "DIFFERENT"),
        ]
    print("\n".join(lines))
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")
    red.close()
    ctx.close()
    return 0 if same in (None, True) else 1


if __name__ == "__main__":
    sys.exit(main())
