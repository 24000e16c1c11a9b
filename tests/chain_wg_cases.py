"""Cases for phase B's chain-per-workgroup kernel (k_chain_wg, csrc/fseq_chainsort.hpp), shared by tests/test_chain_wg_cases.py (CPU:
every case has the property it is listed for, on the inputs alone) and tests/test_gpu_chain_wg.py (the kernel against the model).
The model is tests/chain_step_cases.py's (chain, chain_step, run_starts); here only which of the kernel's three forms a step takes,
and key blocks built step by step so that the ORDER IN FRONT of a block has the runs a case asks for.  No GPU and no library in
here.  TEST INFRASTRUCTURE.

A step of the kernel goes "ident" (the first step of a chain that starts from the identity), "runs" (the knob is not 0, the bits of
nkeys - 1 and of m - 1 fit 32 together, and the keys of the order in front of the block form at most run_cap runs) or "sort".

Runs are maximal, so two neighbouring runs differ in key: the range of a run's head -- behind the previous run of its key up to
itself -- always holds at least ONE whole run.  A range of no whole run, or a previous run of the same key right in front, cannot be
built; the nearest that can is a range of one whole run of one position (keys 0 1 0 on three positions), which "alternate" has at
every head.  test_chain_wg_cases.py states this on the inputs."""
import numpy as np

import chain_step_cases as cs

CW_RUN_CAP = 16384          # csrc/fseq_chainsort.hpp
CW_STATS = 4 + cs.P2_HIST
NW = 16                     # waves of the workgroup: a wave sweeps a chunk of whole 64-groups


def chunk(m):
    return ((m + NW - 1) // NW + 63) & ~63


def counts_runs(m, nkeys, run_cap):
    return run_cap != 0 and cs.bits_of(nkeys - 1) + cs.bits_of(m - 1) <= 32


def step_path(m, nkeys, runs, run_cap, ident):
    if ident:
        return "ident"
    return "runs" if counts_runs(m, nkeys, run_cap) and runs <= run_cap else "sort"


def walk(rank, keyd, nkeys, G, cols_per_block, first_chain, chains, start_a, start_d, keys, run_cap):
    """Per chain of the launch, per block it steps through: (block, path, runs in the order in front of it) -- and the kernel's
    counters.  The states are chain_step_cases.chain_step's."""
    nb, m = np.shape(rank)
    stats = np.zeros(CW_STATS, dtype=np.int64)
    out = []
    for c, blocks in enumerate(cs.stepped_blocks(nb, G, first_chain, chains, keys)):
        b0 = (first_chain + c) * G
        ident = start_a is None
        a = np.arange(m, dtype=np.int64) if ident else np.asarray(start_a[c], dtype=np.int64)
        d = np.full(m, (b0 * cols_per_block) & 0xFFFFFFFF, dtype=np.int64) if ident else np.asarray(start_d[c], dtype=np.int64)
        steps = []
        for b in blocks:
            R = len(cs.run_starts(a, rank[b]))
            path = step_path(m, int(nkeys[b]), R, run_cap, ident)
            steps.append((b, path, R))
            stats[{"runs": 0, "sort": 1, "ident": 2}[path]] += 1
            if not ident and counts_runs(m, int(nkeys[b]), run_cap):
                stats[3] = max(stats[3], R)
                stats[4 + min(cs.P2_HIST - 1, int(R - 1).bit_length())] += 1
            a, d = cs.chain_step(a, d, rank[b], keyd[b])
            ident = False
        out.append(steps)
    return out, stats


# ---------------------------------------------------------------------------------------------- keys by position
def keys_alternate(m, rng):
    """0 1 0 2 0 3 ...: every even position a run of key 0 of one position, every odd position a key of its own -- every head of
    key 0 but the first has a range of exactly one whole run of one position."""
    kp = np.zeros(m, dtype=np.int64)
    kp[1::2] = 1 + np.arange(len(kp[1::2]))
    return kp, 1 + m // 2


def keys_by_position(spec, m, rng):
    """(keys by position, nkeys).  ("runs", R, D): exactly R runs, run j of key j mod D -- the range of a head spans D - 1 whole runs;
    ("one",): one key; ("perm",): every position a key of its own; ("random", D); ("alternate",); ("borders",): runs that start and
    end three positions off the multiples of 64, so that every border of a 64-group and of a wave's chunk lies inside a run."""
    if spec[0] == "runs":
        return cs.keys_runs(m, spec[1], spec[2], rng), spec[2]
    if spec[0] == "one":
        return np.zeros(m, dtype=np.int64), 1
    if spec[0] == "perm":
        return rng.permutation(m).astype(np.int64), m
    if spec[0] == "random":
        return cs.keys_random(m, spec[1], rng), spec[1]
    if spec[0] == "alternate":
        return keys_alternate(m, rng)
    assert spec[0] == "borders"
    cuts = np.r_[0, np.arange(64, m - 3, 64) + 3]
    D = spec[1]
    return np.repeat(np.arange(len(cuts)) % D, np.diff(np.r_[cuts, m])).astype(np.int64), D


def _c(name, m, blocks, G, paths, first=0, chains=None, own_start=True, states=True, keys=False, run_cap=CW_RUN_CAP, workgroups=1, runs=None, start="random"):
    """blocks: a key spec per block of the level; paths: what every stepped block of the launch takes, chain by chain, written out;
    runs: the runs in front of the stepped blocks where the case is about their number (None: not claimed)."""
    nb = len(blocks)
    return dict(name=name, m=m, blocks=tuple(blocks), G=G, first=first, chains=(nb + G - 1) // G - first if chains is None else chains,
                own_start=own_start, states=states, keys=keys, run_cap=run_cap, workgroups=workgroups, paths=tuple(paths), runs=runs, start=start)


def _table():
    T = []
    for m in (11265, 12288):                                             # not a multiple of 64; a multiple of 1,024
        # one step from a constructed state (an expansion of one chain of one block, the last of all)
        T.append(_c("cap", m, [("runs", 100, 40)], 1, ["runs"], run_cap=100, runs=[100]))
        T.append(_c("cap+1", m, [("runs", 101, 40)], 1, ["sort"], run_cap=100, runs=[101]))
        T.append(_c("cap0", m, [("runs", 100, 40)], 1, ["sort"], run_cap=0))
        T.append(_c("one-key", m, [("one",)], 1, ["runs"], runs=[1]))
        T.append(_c("all-heads", m, [("perm",)], 1, ["runs"], runs=[m]))
        T.append(_c("all-heads-sorted", m, [("perm",)], 1, ["sort"], run_cap=m - 1, runs=[m]))
        T.append(_c("borders", m, [("borders", 7)], 1, ["runs"], start="spikes"))
        T.append(_c("one-between", m, [("runs", 3000, 2)], 1, ["runs"], runs=[3000], start="spikes"))
        T.append(_c("alternate", m, [("alternate",)], 1, ["runs"], runs=[m]))
        T.append(_c("many-between", m, [("runs", 9000, 3)], 1, ["runs"], runs=[9000], start="spikes"))   # (gaps of 2 whole runs; 141 blocks of runs)
        T.append(_c("far-between", m, [("runs", 10000, 4000)], 1, ["runs"], runs=[10000]))           # (gaps of 3,999 runs: the table's levels 0 .. 5)
        # the identity: compositions of chains of one block and of three, the emit behind them
        T.append(_c("ident-G1", m, [("random", 700), ("runs", 50, 9), ("one",)], 1, ["ident"] * 3, own_start=False, states=False, keys=True))
        T.append(_c("ident-G3", m, [("random", 700), ("runs", 50, 9), ("runs", 300, 100), ("random", 5), ("one",), ("perm",), ("runs", 20, 20)], 3,
                    ["ident", "runs", "runs", "ident", "runs", "runs", "ident"], own_start=False, states=False, keys=True, workgroups=3))
        T.append(_c("ident-expand-G2", m, [("random", 300), ("runs", 60, 9)], 2, ["ident", "runs"], own_start=False))
        # expansion: chains of two over five blocks -- the last block of chains 0 and 1 is not the last of all
        five = [("runs", 400, 50), ("random", 513), ("runs", 90, 30), ("perm",), ("runs", 8000, 4000)]
        T.append(_c("expand-G2", m, five, 2, ["runs", "runs", "runs"], workgroups=3))
        T.append(_c("expand-G2-first1", m, five, 2, ["runs", "runs"], first=1, chains=2, workgroups=2))
        # chain 1 alone: the state behind its last block (block 3) is chain 2's to write, and chain 2 is not in the launch
        T.append(_c("expand-G2-chain1-alone", m, five, 2, ["runs"], first=1, chains=1))
        T.append(_c("both-G2", m, five, 2, ["runs", "sort", "runs", "sort", "runs"], states=True, keys=True, run_cap=9000))
        # more chains than workgroups: five chains on one and on three
        for wg in (1, 3):
            T.append(_c("five-chains-wg%d" % wg, m, five, 1, ["ident"] * 5, own_start=False, states=False, keys=True, workgroups=wg))
            T.append(_c("five-chains-G2-wg%d" % wg, m, five + five, 2, ["runs"] * 6, workgroups=wg))
    # 20 position bits: 4,096 keys share a word with a position, 4,097 do not -- such a step sorts whatever its runs
    m = 524289
    T.append(_c("bits-32", m, [("runs", 6000, 4096)], 1, ["runs"], runs=[6000]))
    T.append(_c("bits-33", m, [("runs", 6000, 4097)], 1, ["sort"], runs=[6000]))
    for i, c in enumerate(T):
        c["seed"] = 9000 + i
        c["id"] = "%d-%s" % (c["m"], c["name"])
    return T


WG_CASES = _table()


def build_wg(case):
    """Key blocks whose keys BY POSITION in the order in front of them are the case's: own_start -- the launch's chains start from the
    sequential states behind a constructed state in front of block 0; else every chain from the identity."""
    rng = np.random.default_rng(case["seed"])
    m, G, specs = case["m"], case["G"], case["blocks"]
    nb = len(specs)
    rank = np.empty((nb, m), dtype=np.int64)
    keyd = np.empty((nb, m), dtype=np.int64)
    nkeys = np.empty(nb, dtype=np.int64)
    a0, d0 = cs.make_perm("random", m, rng), cs.make_d0(case["start"], m, rng)
    a, d = a0, d0
    for b, spec in enumerate(specs):
        if not case["own_start"] and b % G == 0:
            a, d = np.arange(m, dtype=np.int64), np.full(m, b * cs.COLS, dtype=np.int64)
        kp, nkeys[b] = keys_by_position(spec, m, rng)
        rank[b] = cs.key_by_row(a, kp)
        keyd[b] = rng.integers(0, (b + 1) * cs.COLS + 1, size=m)
        a, d = cs.chain_step(a, d, rank[b], keyd[b])
    return dict(m=m, rank=rank, keyd=keyd, nkeys=nkeys, a=a0, d=d0)


def launch_args(case, B):
    """(start_a, start_d) of the launch's chains: the sequential model's states, or None."""
    if not case["own_start"]:
        return None, None
    seq_a, seq_d = cs.sequential_states(B["a"], B["d"], B["rank"], B["keyd"])
    G, first = case["G"], case["first"]
    return [seq_a[(first + c) * G] for c in range(case["chains"])], [seq_d[(first + c) * G] for c in range(case["chains"])]
