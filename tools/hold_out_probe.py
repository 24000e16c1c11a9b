"""hold_out_probe.py [CONFIG] [--rows=256] [OUT] -- rows held out of a resident alignment on the device, measured in one process
(CONFIG: a name of oracle/fso.py's CONFIGS, C3 by default; writes profiles/hold_out_CONFIG.txt or OUT).

(a) without_rows: the last ROWS rows held out (ms_device: the split pass by HIP events; wall: the whole call);
(b) a device-to-device hipMemcpyAsync of the packed alignment's bytes: the pass reads the alignment once and writes it once, and so
    does the copy -- the floor the pass is held against;
(c) the two-upload way -- a second context, set_sequences of the kept rows, match_rows of the held-out rows' bytes -- against
    without_rows plus match_held_out, both against the same founders (those of one reconstruction from the kept rows, which is
    not in either time);
(d) a five-fold loop on the one source: without_rows of every fifth row, five times.
(a) to (c) alternate after a warm-up of each; medians of RUNS.  The two ways of (c) must give the same pieces."""
import ctypes as C
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


class DeviceCopy:
    """two device buffers of `nbytes` and a timed hipMemcpyAsync between them"""

    def __init__(self, nbytes):
        self.hip = C.CDLL("libamdhip64.so")
        self.nbytes = nbytes
        self.a, self.b, self.e0, self.e1 = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_void_p()
        for buf in (self.a, self.b):
            assert self.hip.hipMalloc(C.byref(buf), C.c_size_t(nbytes)) == 0
            assert self.hip.hipMemset(buf, 1, C.c_size_t(nbytes)) == 0
        for ev in (self.e0, self.e1):
            assert self.hip.hipEventCreate(C.byref(ev)) == 0

    def run(self):
        hip = self.hip
        assert hip.hipEventRecord(self.e0, None) == 0
        assert hip.hipMemcpyAsync(self.b, self.a, C.c_size_t(self.nbytes), 3, None) == 0      # hipMemcpyDeviceToDevice
        assert hip.hipEventRecord(self.e1, None) == 0
        assert hip.hipEventSynchronize(self.e1) == 0
        ms = C.c_float()
        assert hip.hipEventElapsedTime(C.byref(ms), self.e0, self.e1) == 0
        return ms.value

    def close(self):
        for buf in (self.a, self.b):
            self.hip.hipFree(buf)
        for ev in (self.e0, self.e1):
            self.hip.hipEventDestroy(ev)


def main():
    import fso
    args = [a for a in sys.argv[1:] if not a.startswith("--rows=")]
    rows = ([int(a[7:]) for a in sys.argv[1:] if a.startswith("--rows=")] or [256])[0]
    config = args[0] if args else "C3"
    out_path = args[1] if len(args) > 1 else os.path.join(ROOT, "profiles", "hold_out_%s.txt" % config)
    pkg = importlib.import_module("founder-sequences_amd")
    c = fso.CONFIGS[config]
    m, n, L = c["m"], c["n"], c["L"]
    src = pkg.SegmentationContext(m, n, L)
    src.generate_synthetic(c["seed"], c["K"], c["B"], c["mu"], c["kind"])
    ld, bits = src.packed_columns(0, 0)[0].shape[1], src.packed_columns(0, 0)[1]
    nbytes = ld * n
    held = np.arange(m - rows, m, dtype=np.uint32)
    lines = ["hold_out_probe %s: m = %d, n = %d, L = %d; %d bits a code, %d bytes a column, %.1f MB packed; %d rows held out; medians of %d, alternating" % (
        config, m, n, L, bits, ld, nbytes / 1e6, rows, RUNS)]
    # the founders of one reconstruction from the kept rows (not timed)
    sub = src.without_rows(held, L)
    res = sub.run()
    perm = sub.join_greedy()
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "founders.txt")
        sub.write_founders_device(perm, path)
        founders = np.frombuffer(open(path, "rb").read(), dtype=np.uint8).reshape(res.max_segment_size, n + 1)[:, :n].copy()
    sub.close()
    msa = src.get_sequences()
    kept_rows, held_rows = np.ascontiguousarray(msa[:m - rows]), np.ascontiguousarray(msa[m - rows:])
    del msa
    copy = DeviceCopy(nbytes)
    result = {}

    def split_only():
        t0 = time.perf_counter()
        s = src.without_rows(held, L)
        wall = (time.perf_counter() - t0) * 1e3
        dev = s.held_out_summary["ms_device"]
        s.close()
        return dev, wall

    def device_copy():
        t0 = time.perf_counter()
        dev = copy.run()
        return dev, (time.perf_counter() - t0) * 1e3

    def two_uploads():
        t0 = time.perf_counter()
        ctx = pkg.SegmentationContext(m - rows, n, L)
        ctx.set_sequences(kept_rows)
        s = ctx.match_rows(held_rows, founders=founders)
        wall = (time.perf_counter() - t0) * 1e3
        result["two"] = ctx.match_pieces()
        ctx.close()
        return s["ms_device"], wall

    def on_the_device():
        t0 = time.perf_counter()
        ctx = src.without_rows(held, L)
        s = ctx.match_held_out(founders=founders)
        wall = (time.perf_counter() - t0) * 1e3
        result["one"] = ctx.match_pieces()
        dev = ctx.held_out_summary["ms_device"] + s["ms_device"]
        ctx.close()
        return dev, wall

    variants = [("(a) without_rows", split_only), ("(b) hipMemcpyAsync, device to device", device_copy),
                ("(c) second context + set_sequences + match_rows", two_uploads), ("(c) without_rows + match_held_out", on_the_device)]
    times = {name: ([], []) for name, _ in variants}
    for name, call in variants:                                   # warm-up of each
        call()
    for _ in range(RUNS):
        for name, call in variants:
            dev, wall = call()
            times[name][0].append(dev)
            times[name][1].append(wall)
    med = {name: (statistics.median(d), statistics.median(w)) for name, (d, w) in times.items()}
    for name, _ in variants:
        lines.append("    %-50s ms_device %9.2f  wall %9.1f" % (name, med[name][0], med[name][1]))
    a, b = med["(a) without_rows"][0], med["(b) hipMemcpyAsync, device to device"][0]
    lines.append("    the split pass moves %.1f MB in and %.1f MB out: %.0f GB/s; the copy %.0f GB/s; pass / copy = %.2f" % (
        nbytes / 1e6, nbytes / 1e6, 2 * nbytes / a / 1e6, 2 * nbytes / b / 1e6, a / b))
    lines.append("    (c) wall, two uploads / on the device = %.1f" % (med["(c) second context + set_sequences + match_rows"][1] / med["(c) without_rows + match_held_out"][1]))
    same = np.array_equal(result["two"][0], result["one"][0]) and np.array_equal(result["two"][1], result["one"][1])
    lines.append("    (c) %d pieces either way%s" % (len(result["one"][0]), "" if same else "  DIFFERENT PIECES"))
    # (d)
    t0 = time.perf_counter()
    devs = []
    for fold in range(5):
        s = src.without_rows(np.arange(fold, m, 5, dtype=np.uint32), L)
        devs.append(s.held_out_summary["ms_device"])
        s.close()
    lines.append("(d) five folds (every fifth row held out) on the one source: ms_device %s, wall %.1f in all" % (
        " ".join("%.2f" % d for d in devs), (time.perf_counter() - t0) * 1e3))
    copy.close()
    src.close()
    print("\n".join(lines))
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")
    return 0 if same else 1


if __name__ == "__main__":
    sys.exit(main())
