"""match_split_probe.py [CONFIG [OUT]] -- the matcher's walk split along the columns beside the unsplit walk, on one context
in one session (CONFIG: a name of oracle/fso.py's CONFIGS, C3 by default; writes profiles/match_split_CONFIG.txt or OUT).

(a) fseq_match_founders as it is against the same call under FSEQ_MATCH_SPLIT at several G and overlaps;
(b) fseq_match_rows on 8, 256 and 2,504 held-out mosaic rows (mosaics of the founders just joined, blocks of 1,000 columns, one
    cell in 200 changed), split by itself against FSEQ_MATCH_SPLIT=1;
(c) the share of flagged groups and of rows that did not stand at each overlap, from the same calls;
(d) a true hold-out: CONFIG's alignment without its last 256 rows segmented and joined on a second context, those 256 rows
    matched against its founders -- split by itself, by itself under longer overlaps, and FSEQ_MATCH_SPLIT=1.
Every pair alternates after a warm-up of each; medians of RUNS; ms_device (HIP events: the founders' columns and the walks) and
the wall time of the call (for fseq_match_rows that includes the upload of the queries).  Every split result must be the
unsplit one, piece for piece."""
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
SPLITS = [(8, 4096), (64, 4096), (64, 1024), (512, 256), (64, 64), (8, 32768), (16, 32768), (30, 32768), (8, 125000)]


def timed(call):
    t0 = time.perf_counter()
    s = call()
    return s["ms_device"], (time.perf_counter() - t0) * 1e3


def alternate(ctx, variants):
    """variants: [(name, setup, call)] -> {name: (median ms_device, median wall, split info, pieces, sets)}"""
    out = {}
    for name, setup, call in variants:                            # warm-up of each
        setup()
        call()
        out[name] = {"dev": [], "wall": [], "info": ctx.match_split(), "result": ctx.match_pieces()}
    for _ in range(RUNS):
        for name, setup, call in variants:
            setup()
            d, w = timed(call)
            out[name]["dev"].append(d)
            out[name]["wall"].append(w)
    return out


def main():
    import fso
    config = sys.argv[1] if len(sys.argv) > 1 else "C3"
    out_path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "match_split_%s.txt" % config)
    pkg = importlib.import_module("founder-sequences_amd")
    c = fso.CONFIGS[config]
    m, n, L = c["m"], c["n"], c["L"]
    ctx = pkg.SegmentationContext(m, n, L)
    ctx.generate_synthetic(c["seed"], c["K"], c["B"], c["mu"], c["kind"])
    res = ctx.run()
    perm = ctx.join_greedy()

    def knobs(G, overlap):
        def go():
            ctx.set_tuning("FSEQ_MATCH_SPLIT", G)
            ctx.set_tuning("FSEQ_MATCH_OVERLAP", overlap)
        return go

    lines = ["match_split_probe %s: m = %d, n = %d, L = %d; %d founders, %d merged segments; medians of %d, alternating" % (
        config, m, n, L, res.max_segment_size, res.segment_count, RUNS)]
    ok = True
    # (a), (c)
    variants = [("unsplit", knobs(None, None), lambda: ctx.match_founders(perm))]
    variants += [("G=%d overlap=%d" % (G, ov), knobs(G, ov), lambda: ctx.match_founders(perm)) for G, ov in SPLITS]
    got = alternate(ctx, variants)
    base = got["unsplit"]
    lines.append("(a) fseq_match_founders, %d pieces" % len(base["result"][0]))
    for name, _, _ in variants:
        g = got[name]
        same = np.array_equal(g["result"][0], base["result"][0]) and np.array_equal(g["result"][1], base["result"][1])
        ok &= same
        i = g["info"]
        lines.append("    %-22s ms_device %8.1f  wall %8.1f  (x%.2f of unsplit)  flagged groups %d of %d, rows not standing %d of %d%s" % (
            name, statistics.median(g["dev"]), statistics.median(g["wall"]), statistics.median(base["dev"]) / statistics.median(g["dev"]),
            i["flagged_groups"], i["row_groups"], i["rows_not_standing"], m, "" if same else "  DIFFERENT PIECES"))
    # (b): held-out mosaics of the founders
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "founders.txt")
        ctx.write_founders_device(perm, path)
        founders = np.frombuffer(open(path, "rb").read(), dtype=np.uint8).reshape(res.max_segment_size, n + 1)[:, :n]
    rng = np.random.default_rng(1)
    block = 1000
    lines.append("(b) fseq_match_rows on held-out mosaics of the founders (by permutations)")
    for rows in (8, 256, 2504):
        held = np.empty((rows, n), dtype=np.uint8)
        for b in range(0, n, block):
            blk = founders[rng.integers(0, len(founders), size=rows), b:b + block]
            noise = rng.random(blk.shape) < 5e-3
            blk[noise] = founders[rng.integers(0, len(founders), size=int(noise.sum())), b + np.nonzero(noise)[1]]
            held[:, b:b + block] = blk
        variants = [("FSEQ_MATCH_SPLIT=1", knobs(1, None), lambda: ctx.match_rows(held, permutations=perm)),
                    ("by itself", knobs(None, None), lambda: ctx.match_rows(held, permutations=perm))]
        got = alternate(ctx, variants)
        base = got["FSEQ_MATCH_SPLIT=1"]
        for name, _, _ in variants:
            g = got[name]
            same = np.array_equal(g["result"][0], base["result"][0]) and np.array_equal(g["result"][1], base["result"][1])
            ok &= same
            i = g["info"]
            lines.append("    %5d rows  %-20s G=%-4d overlap=%-5d ms_device %8.1f  wall %8.1f  flagged groups %d of %d, rows not standing %d%s" % (
                rows, name, i["segments"], i["overlap"], statistics.median(g["dev"]), statistics.median(g["wall"]),
                i["flagged_groups"], i["row_groups"], i["rows_not_standing"], "" if same else "  DIFFERENT PIECES"))
        del held
    # (d): rows of the same population kept out of the reconstruction
    msa = ctx.get_sequences()
    ctx.close()
    keep = m - 256
    held = np.ascontiguousarray(msa[keep:])
    ctx = pkg.SegmentationContext(keep, n, L)
    ctx.set_sequences(np.ascontiguousarray(msa[:keep]))
    del msa
    res2 = ctx.run()
    perm = ctx.join_greedy()
    lines.append("(d) fseq_match_rows on the last 256 rows of %s, kept out of a reconstruction from the other %d (%d founders)" % (config, keep, res2.max_segment_size))
    variants = [("FSEQ_MATCH_SPLIT=1", knobs(1, None), lambda: ctx.match_rows(held, permutations=perm)),
                ("by itself", knobs(None, None), lambda: ctx.match_rows(held, permutations=perm))]
    variants += [("by itself, overlap %d" % ov, knobs(None, ov), lambda: ctx.match_rows(held, permutations=perm)) for ov in (16384, 32768, 65536)]
    variants += [("G=%d overlap=%d" % (G, ov), knobs(G, ov), lambda: ctx.match_rows(held, permutations=perm)) for G, ov in ((30, 32768), (61, 16384))]
    got = alternate(ctx, variants)
    base = got["FSEQ_MATCH_SPLIT=1"]
    for name, _, _ in variants:
        g = got[name]
        same = np.array_equal(g["result"][0], base["result"][0]) and np.array_equal(g["result"][1], base["result"][1])
        ok &= same
        i = g["info"]
        lines.append("    %-28s G=%-4d overlap=%-6d ms_device %8.1f  wall %8.1f  flagged groups %d of %d, rows not standing %d of 256; %d pieces, most in a row %d%s" % (
            name, i["segments"], i["overlap"], statistics.median(g["dev"]), statistics.median(g["wall"]), i["flagged_groups"], i["row_groups"],
            i["rows_not_standing"], len(g["result"][0]), int(np.bincount(g["result"][0]["row"]).max()), "" if same else "  DIFFERENT PIECES"))
    print("\n".join(lines))
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")
    ctx.close()
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
