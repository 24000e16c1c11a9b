"""match_restored_split_probe.py [CONFIG] [--rows=256] [--share=0.6] [--rate=1e-4] [OUT] -- the restored match walk split along
the kept columns, measured in one process (CONFIG: a name of oracle/fso.py's CONFIGS, C3 by default; writes
profiles/match_restored_split_CONFIG.txt or OUT).

The input is tools/held_out_restored_probe.py's: CONFIG's synthetic alignment with about SHARE of its columns overwritten with
row 0's symbol (identity columns), the last ROWS rows held out, once without an exception cell and once with another symbol of
the alphabet in about RATE of the held-out rows' cells.  On one context (without_rows + without_identity_columns(keep_held_out=
True), run, greedy join) the variants of match_held_out_restored alternate after a warm-up of each, medians of RUNS of ms_device:
FSEQ_MATCH_SPLIT=1 (one segment), the split by itself, forced G in GS at the overlap by itself, the overlaps OVERLAPS (kept
columns) at the G by itself; then match_founders_restored on the alignment's own rows unsplit and at the same G.  Every variant's
match_split() is recorded -- segments, overlap, flagged groups, rows that do not stand -- and its pieces and sets must be those
of the first variant."""
import importlib
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "oracle")):
    sys.path.insert(0, p)
RUNS = 3
GS = (8, 16, 32, 61)
OVERLAPS = (4096, 16384, 32768)


def main():
    import fso
    opts = {a.split("=")[0]: a.split("=")[1] for a in sys.argv[1:] if a.startswith("--")}
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    rows, share, rate = int(opts.get("--rows", 256)), float(opts.get("--share", 0.6)), float(opts.get("--rate", 1e-4))
    config = args[0] if args else "C3"
    out_path = args[1] if len(args) > 1 else os.path.join(ROOT, "profiles", "match_restored_split_%s.txt" % config)
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
    held = np.arange(m - rows, m, dtype=np.uint32)
    lines = ["match_restored_split_probe %s: m = %d, n = %d, L = %d; identity share %.2f; the last %d rows held out; medians of %d of ms_device, alternating" % (
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
        sub = src.without_rows(held, L)
        src.close()
        red = sub.without_identity_columns(L, keep_held_out=True)
        sub.close()
        res = red.run()
        perm = red.join_greedy()

        def variant(split, overlap, own_rows=False):
            def call():
                red.set_tuning("FSEQ_MATCH_SPLIT", split)
                red.set_tuning("FSEQ_MATCH_OVERLAP", overlap)
                s = red.match_founders_restored(perm) if own_rows else red.match_held_out_restored(perm)
                return s, red.match_split()
            return call

        held_variants = [("FSEQ_MATCH_SPLIT=1", variant(1, None)), ("by itself", variant(None, None))]
        held_variants += [("G = %d" % g, variant(g, None)) for g in GS]
        held_variants += [("overlap %d" % ov, variant(None, ov)) for ov in OVERLAPS]
        own_variants = [("own rows, unsplit", variant(None, None, True))] + [("own rows, G = %d" % g, variant(g, None, True)) for g in GS]
        lines.append("%s: kept %d of %d columns; %d merged segments" % (tag, red.n, n, res.segment_count))
        for variants, what in ((held_variants, "match_held_out_restored, %d held-out rows" % rows), (own_variants, "match_founders_restored, %d rows of the alignment" % red.m)):
            first = None
            times = {name: [] for name, _ in variants}
            info = {}
            for name, call in variants:                           # the warm-up of each; its result against the first variant's
                s, info[name] = call()
                got = red.match_pieces()
                if first is None:
                    first = got
                same = np.array_equal(got[0], first[0]) and np.array_equal(got[1], first[1])
                ok = ok and same
                info[name] = dict(info[name], pieces=s["pieces"], same=same)
            for _ in range(RUNS):
                for name, call in variants:
                    times[name].append(call()[0]["ms_device"])
            lines.append("  %s" % what)
            for name, _ in variants:
                i = info[name]
                lines.append("    %-22s ms_device %9.2f   segments %4d  overlap %6d  flagged groups %d of %d  rows not standing %d  pieces %d%s" % (
                    name, statistics.median(times[name]), i["segments"], i["overlap"], i["flagged_groups"], i["row_groups"], i["rows_not_standing"], i["pieces"],
                    "" if i["same"] else "  DIFFERENT PIECES"))
        red.set_tuning("FSEQ_MATCH_SPLIT", None)
        red.set_tuning("FSEQ_MATCH_OVERLAP", None)
        red.close()
    print("\n".join(lines))
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
