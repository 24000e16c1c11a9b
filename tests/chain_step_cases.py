"""The streamed chain step (csrc/fseq_chainsort.hpp) as a vectorised numpy model, seeded generators of constructed states and
keys, and the tables of cases tests/test_chain_step_cases.py (CPU: the conditions every case claims, on the inputs alone) and
tests/test_gpu_chain_step.py (the kernels against the model) share.  No GPU and no library in here.  TEST INFRASTRUCTURE.

A chain step takes an order (a0, d0) to the order behind a key block {key[row], headd[class]}: a1 = the stable sort of a0 by
key[a0]; the first position of a class takes headd[class]; any other position takes the maximum of d0 over the old positions
behind its predecessor's up to its own (tests/proto_pass2_runs.py states the same with a loop per position)."""
import numpy as np

NOT_WRITTEN = 0xFFFFFFFF
P2_CLS_CAP = 11264          # csrc/fseq_chainsort.hpp
P2_RUN_CAP = 8832
P2_CLS_BITS = 14
P2_HIST = 19                # csrc/fseq_types.hpp
CS_MAX_DIGIT_BITS = 9
D_LIMIT = 1 << 25           # every divergence of a case is below this
COLS = 1000                 # columns of a key block in the phase B cases

M_MIN, M_MAX = 11265, 589824


# ---------------------------------------------------------------------------------------------- the model
def chain_step(a0, d0, key, headd):
    """(a1, d1) as int64 arrays; key by row, headd by class."""
    a0 = np.asarray(a0, dtype=np.int64)
    d0 = np.asarray(d0, dtype=np.int64)
    key = np.asarray(key, dtype=np.int64)
    headd = np.asarray(headd, dtype=np.int64)
    m = len(a0)
    k = key[a0]
    order = np.argsort(k, kind="stable")
    ks = k[order]
    first = np.r_[True, ks[1:] != ks[:-1]]
    d1 = np.empty(m, dtype=np.int64)
    d1[first] = headd[ks[first]]
    nf = np.flatnonzero(~first)
    if len(nf):
        # max d0[lo .. hi] for every pair at once: reduceat over (lo, hi + 1, lo', hi' + 1, ...), every other result
        idx = np.empty(2 * len(nf), dtype=np.int64)
        idx[0::2] = order[nf - 1] + 1
        idx[1::2] = order[nf] + 1
        d1[nf] = np.maximum.reduceat(np.r_[d0, 0], idx)[0::2]
    return a0[order], d1


def run_starts(a0, key):
    k = np.asarray(key)[np.asarray(a0)]
    return np.flatnonzero(np.r_[True, k[1:] != k[:-1]])


def bits_of(x):
    """The kernels' `bits = 1; while (x >> bits) ++bits`: bits of x, at least one."""
    return max(1, int(x).bit_length())


def digit_passes(D):
    return (bits_of(D - 1) + CS_MAX_DIGIT_BITS - 1) // CS_MAX_DIGIT_BITS


def pass2_counts_runs(m, run_cap):
    """Whether k_chain_snap_grouped counts a task's runs at all: the knob is not 0 and a class shares a word with a position."""
    return run_cap != 0 and P2_CLS_BITS + bits_of(m - 1) <= 32


def pass2_path(m, D, runs, run_cap):
    """Which form of the step a task of k_chain_snap_grouped takes: "runs", "p4" (pass2_step<true>) or "wide" (pass2_step<false>)."""
    if pass2_counts_runs(m, run_cap) and runs <= run_cap:
        return "runs"
    return "p4" if bits_of(D - 1) + bits_of(m - 1) <= 32 else "wide"


def cm_pair_is_one_word(m, nkeys):
    return bits_of(nkeys - 1) + bits_of(m - 1) <= 32


def emit_keys(a, d, kstart):
    """stream_emit_ranks: a position starts a key iff it is position 0 or d > kstart; rank by row, keyd per key."""
    m = len(a)
    first = np.asarray(d) > kstart
    first[0] = True
    r = np.cumsum(first) - 1
    rank = np.empty(m, dtype=np.int64)
    rank[a] = r
    keyd = np.full(m, NOT_WRITTEN, dtype=np.int64)
    keyd[:r[-1] + 1] = np.asarray(d)[first]
    return rank, keyd, int(r[-1]) + 1


def chain(rank, keyd, nkeys, G, cols_per_block, first_chain, chains, start_a=None, start_d=None, states=True, keys=False):
    """The model of fseq_debug_chain_launch: chain c of the launch is chain first_chain + c of the level, over the blocks
    [grp G, min(nb, (grp + 1) G)); an expansion (no composite keys) does not step through a chain's last block unless that is the last
    of all; a state is written in front of every block of a chain and behind the last block of all."""
    nb, m = np.shape(rank)
    out = {}
    sa = np.full((nb + 1, m), NOT_WRITTEN, dtype=np.int64)
    sd = np.full((nb + 1, m), NOT_WRITTEN, dtype=np.int64)
    kr = np.full((chains, m), NOT_WRITTEN, dtype=np.int64)
    kd = np.full((chains, m), NOT_WRITTEN, dtype=np.int64)
    kn = np.full(chains, NOT_WRITTEN, dtype=np.int64)
    for c in range(chains):
        b0 = (first_chain + c) * G
        b1 = min(nb, b0 + G)
        kstart = (b0 * cols_per_block) & 0xFFFFFFFF
        a = np.arange(m, dtype=np.int64) if start_a is None else np.asarray(start_a[c], dtype=np.int64)
        d = np.full(m, kstart, dtype=np.int64) if start_a is None else np.asarray(start_d[c], dtype=np.int64)
        sa[b0], sd[b0] = a, d
        for b in range(b0, b1):
            if not (keys or b + 1 < b1 or b + 1 == nb):
                break
            a, d = chain_step(a, d, rank[b], keyd[b])
            if b + 1 < b1 or b + 1 == nb:
                sa[b + 1], sd[b + 1] = a, d
        if keys:
            kr[c], kd[c], kn[c] = emit_keys(a, d, kstart)
    if states:
        out["state_a"], out["state_d"] = sa, sd
    if keys:
        out["rank"], out["keyd"], out["nkeys"] = kr, kd, kn
    return out


def sequential_states(a, d, rank, keyd):
    """The states in front of every block and behind the last, one step after the other."""
    sa, sd = [np.asarray(a, dtype=np.int64)], [np.asarray(d, dtype=np.int64)]
    for b in range(len(rank)):
        a, d = chain_step(sa[-1], sd[-1], rank[b], keyd[b])
        sa.append(a)
        sd.append(d)
    return np.array(sa), np.array(sd)


def range_categories(a0, d0, key, heads_only=False):
    """The non-first positions of the step by the branch their range [lo, hi] must take, from the inputs alone.  Inside one
    64-block: "prefix" (the prefix maximum at hi exceeds the one at lo - 1, or lo starts the block), else "suffix" (the suffix
    maximum at lo exceeds the one behind hi, or hi ends the block), else "scan".  "adjacent": neighbouring blocks.  A gap of
    g = bh - bl - 1 >= 1 whole blocks, k = floor(log2 g): ("gap", k, "lo") where g == 2^k, ("gap", k, "hi") where g is the largest
    gap of the level, min(2^(k + 1) - 1, nblk - 2), and ("gap", k, "mid") otherwise (g == 1 is both ends of level 0).
    heads_only: only the ranges of more than one position, those of the heads of runs -- the only range maxima the run path takes
    (a position behind its run's head has its predecessor right in front of it and keeps its own d0)."""
    a0 = np.asarray(a0, dtype=np.int64)
    d0 = np.asarray(d0, dtype=np.int64)
    m = len(a0)
    nblk = (m + 63) // 64
    k = np.asarray(key, dtype=np.int64)[a0]
    order = np.argsort(k, kind="stable")
    ks = k[order]
    nf = np.flatnonzero(np.r_[False, ks[1:] == ks[:-1]])
    lo, hi = order[nf - 1] + 1, order[nf]
    if heads_only:
        lo, hi = lo[lo < hi], hi[lo < hi]
    bl, bh = lo >> 6, hi >> 6
    out = {}
    blocks = np.zeros((nblk, 64), dtype=np.int64)
    blocks.reshape(-1)[:m] = d0
    pm = np.maximum.accumulate(blocks, axis=1).reshape(-1)
    sm = np.maximum.accumulate(blocks[:, ::-1], axis=1)[:, ::-1]
    behind = np.c_[sm[:, 1:], np.zeros(nblk, dtype=np.int64)].reshape(-1)      # the suffix maximum from i + 1 inside i's block
    sm = sm.reshape(-1)
    same = bl == bh
    l, h = lo[same], hi[same]
    prefix = ((l & 63) == 0) | (pm[h] > pm[l - 1])
    suffix = ~prefix & (((h & 63) == 63) | (sm[l] > behind[h]))
    out["prefix"] = int(prefix.sum())
    out["suffix"] = int(suffix.sum())
    out["scan"] = int((~prefix & ~suffix).sum())
    out["adjacent"] = int((bh == bl + 1).sum())
    g = (bh - bl - 1)[bh > bl + 1]
    if len(g):
        lv = np.floor(np.log2(g)).astype(np.int64)
        for kk in np.unique(lv):
            gk = g[lv == kk]
            top = min((2 << int(kk)) - 1, nblk - 2)
            out[("gap", int(kk), "lo")] = int((gk == (1 << int(kk))).sum())
            out[("gap", int(kk), "hi")] = int((gk == top).sum())
            out[("gap", int(kk), "mid")] = int(((gk != (1 << int(kk))) & (gk != top)).sum())
    return out


def top_level(m):
    """The highest level of the sparse table a range of m rows can use: floor(log2(nblk - 2))."""
    return int(np.floor(np.log2((m + 63) // 64 - 2)))


# ---------------------------------------------------------------------------------------------- the generators
PERMS = ("identity", "reversal", "random")
D0_FAMILIES = ("equal", "increasing", "decreasing", "random", "spikes")
# the in-block branches a d0 family asks for where ranges inside one 64-block exist (equal values: neither rule can tell, a scan;
# increasing: the prefix maximum always grows; decreasing: the suffix maximum always does)
D0_BRANCHES = {"equal": ("scan",), "increasing": ("prefix",), "decreasing": ("suffix",), "random": ("prefix", "suffix", "scan"),
               "spikes": ("prefix", "suffix", "scan")}


def make_perm(kind, m, rng):
    if kind == "identity":
        return np.arange(m, dtype=np.int64)
    if kind == "reversal":
        return np.arange(m, dtype=np.int64)[::-1].copy()
    return rng.permutation(m).astype(np.int64)


def make_d0(kind, m, rng):
    if kind == "equal":
        return np.full(m, 12345, dtype=np.int64)
    if kind == "increasing":
        return np.arange(m, dtype=np.int64) + 7
    if kind == "decreasing":
        return m - np.arange(m, dtype=np.int64) + 3
    if kind == "random":
        return rng.integers(0, D_LIMIT, size=m).astype(np.int64)
    # sparse spikes: zero but for distinct values at about one position in fifty
    d = np.zeros(m, dtype=np.int64)
    at = np.flatnonzero(rng.random(m) < 0.02)
    d[at] = rng.choice(D_LIMIT - 1, size=len(at), replace=False) + 1
    return d


def keys_random(m, D, rng):
    """By position: a random class per position, every one of the D classes present."""
    kp = rng.integers(0, D, size=m).astype(np.int64)
    kp[rng.choice(m, size=D, replace=False)] = np.arange(D)
    return kp


def keys_stretches(m, D, rng, every64=False):
    """By position: stretches of consecutive positions of one class, lengths from {1, 63, 64, 65, a few thousand}; every64: a
    stretch starts at every multiple of 64 (and at a few hundred other positions)."""
    if every64:
        cuts = np.union1d(np.arange(0, m, 64), rng.choice(np.arange(1, m), size=300, replace=False))
    else:
        lens = rng.choice(np.array([1, 63, 64, 65, 2500, 4100]), size=m, p=[0.3, 0.22, 0.22, 0.22, 0.03, 0.01])
        cuts = np.r_[0, np.cumsum(lens)]
        cuts = cuts[cuts < m]
    cls = rng.integers(0, D, size=len(cuts))
    cls[:min(D, len(cuts))] = rng.permutation(D)[:min(D, len(cuts))]
    return np.repeat(cls, np.diff(np.r_[cuts, m])).astype(np.int64)


def keys_runs(m, R, D, rng):
    """By position: exactly R runs of equal class, run j of class j mod D (D >= 2 unless R == 1)."""
    assert 1 <= R <= m and (D >= 2 or R == 1) and D <= R
    cuts = np.r_[0, np.sort(rng.choice(np.arange(1, m), size=R - 1, replace=False))] if R > 1 else np.array([0])
    return np.repeat(np.arange(R) % D, np.diff(np.r_[cuts, m])).astype(np.int64)


def planted_gaps(m, levels):
    """Both ends of every level's range of gaps: 2^k and min(2^(k + 1) - 1, nblk - 2)."""
    nblk = (m + 63) // 64
    gaps = []
    for k in levels:
        for g in (1 << k, min((2 << k) - 1, nblk - 2)):
            if g not in gaps:
                gaps.append(g)
    return gaps


def keys_planted(kp, D_bg, gaps):
    """Into a background kp (by position) of D_bg classes: for every gap a class of exactly two positions whose range spans that
    many whole 64-blocks (pair i: from block i, or as far down as the gap needs to fit).  Returns (kp, D)."""
    m = len(kp)
    nblk = (m + 63) // 64
    kp = kp.copy()
    used = set()
    for i, g in enumerate(gaps):
        bl = min(i, nblk - 2 - g)
        bh = bl + g + 1
        p1 = bl * 64 + (2 * i) % 62                       # (lo = p1 + 1 lies in the same block)
        p2 = min(bh * 64 + (2 * i + 1) % 64, m - 1)
        assert p1 not in used and p2 not in used and (p2 >> 6) == bh and ((p1 + 1) >> 6) == bl
        used.update((p1, p2))
        kp[p1] = kp[p2] = D_bg + i
    return kp, D_bg + len(gaps)


def key_by_row(a0, kp):
    key = np.empty(len(a0), dtype=np.int64)
    key[a0] = kp
    return key


def task_tables(key, D, cap, rng):
    """A block's rank by row and a task's class table for keys by row: class = cls[rank], several ranks a class where cap > D."""
    assert D <= cap <= P2_CLS_CAP
    rank = key + D * (rng.integers(0, 1 << 30, size=len(key)) % ((cap - 1 - key) // D + 1))
    cls = np.arange(cap, dtype=np.int64) % D
    headd = rng.integers(0, D_LIMIT, size=cap).astype(np.int64)
    return rank, cls, headd


# ---------------------------------------------------------------------------------------------- pass 2: the table
def _p2(name, m, keys, perm="random", d0="random", run_cap=P2_RUN_CAP, path=None, cats=(), runs=None, cap=None, passes=None):
    return dict(name=name, m=m, keys=keys, perm=perm, d0=d0, run_cap=run_cap, path=path, cats=tuple(cats), runs=runs, cap=cap, passes=passes)


def _levels(m, levels):
    out = []
    for k in levels:
        out += [("gap", k, "lo"), ("gap", k, "hi")]
    return out


def _pass2_table():
    T = []
    m = 11265                                                            # the fewest streamed rows: wave 15's chunk of 768 positions is empty
    for fam in D0_FAMILIES:
        br = D0_BRANCHES[fam]
        T.append(_p2("D1", m, ("random", 1), d0=fam, path="runs", runs=1))
        T.append(_p2("D2", m, ("random", 2), d0=fam, path="runs", cats=br))
        T.append(_p2("D513", m, ("random", 513), d0=fam, path="p4", cats=br + ("adjacent",), passes=2))
        T.append(_p2("stretches", m, ("stretches", 12), d0=fam, path="runs", cats=(("gap", 0, "lo"),)))
    T.append(_p2("R8832", m, ("runs", 8832, 4352), path="runs", runs=8832, cats=(("gap", 6, "mid"),)))
    T.append(_p2("R8833", m, ("runs", 8833, 4352), path="p4", runs=8833))
    T.append(_p2("R100cap99", m, ("runs", 100, 40), run_cap=99, path="p4", runs=100))
    T.append(_p2("R100cap100", m, ("runs", 100, 40), run_cap=100, path="runs", runs=100))
    T.append(_p2("R100cap0", m, ("runs", 100, 40), run_cap=0, path="p4", runs=100))
    T.append(_p2("planted", m, ("planted", 300, tuple(range(8))), path="p4", cats=_levels(m, range(8))))
    T.append(_p2("planted-runs", m, ("planted-stretches", 12, tuple(range(8))), d0="spikes", path="runs", cats=_levels(m, range(8))))
    T.append(_p2("planted-identity", m, ("planted", 300, tuple(range(8))), perm="identity", d0="spikes", path="p4", cats=_levels(m, range(8))))
    for m in (11328, 12288, 12289):                                      # a whole last block, a multiple of 1,024, one row over
        T.append(_p2("stretches64", m, ("stretches64", 40), d0="spikes", path="runs", cats=("adjacent",)))
        T.append(_p2("stretches64-reversal", m, ("stretches64", 40), perm="reversal", d0="random", path="runs", cats=("adjacent",)))
        for D, ps in ((511, 1), (512, 1), (513, 2)):
            T.append(_p2("D%d" % D, m, ("random", D), d0="spikes", path="p4", passes=ps, cats=("prefix", "scan", "adjacent")))
    for m in (65536, 65537):                                             # 16 and 17 position bits
        T.append(_p2("stretches", m, ("stretches", 100), path="runs", cats=(("gap", 8, "mid"), ("gap", 9, "mid"))))
        T.append(_p2("planted-runs", m, ("planted-stretches", 100, tuple(range(10))), d0="spikes", path="runs", cats=_levels(m, range(10))))
        T.append(_p2("D513", m, ("random", 513), d0="spikes", path="p4", passes=2, cats=("adjacent",)))
        T.append(_p2("planted", m, ("planted", 2000, tuple(range(10))), path="p4", cats=_levels(m, range(10))))
    m = 262144                                                           # 18 bits: the last m that may go by runs; 11,264 classes still share a word
    T.append(_p2("stretches", m, ("stretches", 500), path="runs", cats=(("gap", 10, "mid"), ("gap", 11, "mid"))))
    T.append(_p2("planted-runs", m, ("planted-stretches", 500, tuple(range(12))), path="runs", cats=_levels(m, range(12))))
    T.append(_p2("D11264", m, ("random", 11264), path="p4", passes=2, cats=("adjacent",), cap=11264))
    T.append(_p2("planted", m, ("planted", 3000, tuple(range(12))), d0="spikes", path="p4", cats=_levels(m, range(12))))
    m = 262145                                                           # 19 bits: no run path; one-word pairs up to 8,192 classes
    for fam in D0_FAMILIES:
        T.append(_p2("D8192", m, ("random", 8192), d0=fam, path="p4", passes=2, cap=8192))
        T.append(_p2("D8193", m, ("random", 8193), d0=fam, path="wide", passes=2, cap=8193, cats=("adjacent", ("gap", 0, "lo"))))
        T.append(_p2("D11264", m, ("random", 11264), d0=fam, path="wide", passes=2, cap=11264))
    # (the identity and the reversal: positions = rows, so the in-block branches fall where d0 puts them)
    T.append(_p2("D8193", m, ("random", 8193), perm="identity", d0="spikes", path="wide", passes=2, cap=8193, cats=("prefix", "suffix", "scan", "adjacent")))
    T.append(_p2("D8193", m, ("random", 8193), perm="reversal", d0="random", path="wide", passes=2, cap=8193, cats=("prefix", "suffix", "scan", "adjacent")))
    T.append(_p2("D11264", m, ("random", 11264), perm="reversal", d0="decreasing", path="wide", passes=2, cap=11264, cats=("suffix", "adjacent")))
    T.append(_p2("stretches", m, ("stretches", 4352), path="p4"))
    T.append(_p2("planted-p4", m, ("planted", 300, tuple(range(12))), path="p4", cats=_levels(m, range(12)) + list(D0_BRANCHES["random"])))
    T.append(_p2("planted-wide", m, ("planted", 9000, tuple(range(12))), d0="spikes", path="wide", cats=_levels(m, range(12))))
    for i, c in enumerate(T):
        c["seed"] = 1000 + i
        c["id"] = "%d-%s-%s-%s" % (c["m"], c["name"], c["perm"], c["d0"])
    return T


PASS2_CASES = _pass2_table()


def build_pass2(case):
    """The inputs of one task on one block: a0, d0, key by row, D, and the block's rank / the task's cls and headd of cap entries."""
    rng = np.random.default_rng(case["seed"])
    m, spec = case["m"], case["keys"]
    a0 = make_perm(case["perm"], m, rng)
    d0 = make_d0(case["d0"], m, rng)
    if spec[0] == "random":
        D, kp = spec[1], (keys_random(m, spec[1], rng) if spec[1] > 1 else np.zeros(m, dtype=np.int64))
    elif spec[0] in ("stretches", "stretches64"):
        D, kp = spec[1], keys_stretches(m, spec[1], rng, every64=spec[0] == "stretches64")
    elif spec[0] == "runs":
        D, kp = spec[2], keys_runs(m, spec[1], spec[2], rng)
    else:
        bg = keys_stretches(m, spec[1], rng) if spec[0] == "planted-stretches" else keys_random(m, spec[1], rng)
        kp, D = keys_planted(bg, spec[1], planted_gaps(m, spec[2]))
    key = key_by_row(a0, kp)
    cap = case["cap"] or min(P2_CLS_CAP, 2 * D + 5)
    rank, cls, headd = task_tables(key, D, cap, rng)
    return dict(m=m, a0=a0, d0=d0, key=key, D=D, cap=cap, rank=rank, cls=cls, headd=headd, run_cap=case["run_cap"])


def build_grouped(seed=77, m=11265):
    """One launch of 3 blocks (different states) and 7 tasks.  Block 1 holds, in this order, a task by runs, a task by sort, a
    border copy, a skipped task and another task by runs; blocks 0 and 2 one task each.  A block's rank by position is
    2 x (coarse class) + (position odd): a task that keeps the low bit forms m runs (more than any cap: by sort), a task that
    drops it the coarse stretches (by runs)."""
    rng = np.random.default_rng(seed)
    Dc = 600
    cap = 2 * Dc + 7
    a0, d0, rank = [], [], []
    for b, fam in enumerate(("random", "spikes", "decreasing")):
        a = make_perm("random", m, rng)
        kc = keys_stretches(m, Dc, rng)
        a0.append(a)
        d0.append(make_d0(fam, m, rng))
        rank.append(key_by_row(a, 2 * kc + (np.arange(m) & 1)))
    r = np.arange(cap, dtype=np.int64)
    coarse, fine, thirds = np.minimum(r >> 1, Dc - 1), np.minimum(r, 2 * Dc - 1), np.minimum(r >> 1, Dc - 1) % 200
    zeros = np.zeros(cap, dtype=np.int64)
    tasks = [(0, coarse, Dc), (1, coarse, Dc), (1, fine, 2 * Dc), (1, zeros, 0), (1, zeros, NOT_WRITTEN), (1, thirds, 200), (2, fine, 2 * Dc)]
    return dict(m=m, a0=np.array(a0), d0=np.array(d0), rank=np.array(rank), cap=cap, task_blk=np.array([t[0] for t in tasks]),
                cls=np.array([t[1] for t in tasks]), ncls=np.array([t[2] for t in tasks], dtype=np.int64),
                headd=rng.integers(0, D_LIMIT, size=(len(tasks), cap)).astype(np.int64), paths=["runs", "runs", "p4", "copy", "skip", "runs", "p4"])


def pass2_model(a0, d0, rank, task_blk, cls, headd, ncls, run_cap):
    """(snap_a, snap_d, stats) of one launch of k_chain_snap_grouped."""
    ntasks, m = len(task_blk), np.shape(a0)[1]
    sa = np.full((ntasks, m), NOT_WRITTEN, dtype=np.int64)
    sd = np.full((ntasks, m), NOT_WRITTEN, dtype=np.int64)
    stats = np.zeros(4 + P2_HIST, dtype=np.int64)
    for t in range(ntasks):
        b, D = int(task_blk[t]), int(ncls[t])
        if D == NOT_WRITTEN:
            continue
        if D == 0:
            sa[t], sd[t] = a0[b], d0[b]
            stats[2] += 1
            continue
        key = np.asarray(cls[t])[np.asarray(rank[b])]
        sa[t], sd[t] = chain_step(a0[b], d0[b], key, headd[t])
        R = len(run_starts(a0[b], key))
        stats[0 if pass2_path(m, D, R, run_cap) == "runs" else 1] += 1
        if pass2_counts_runs(m, run_cap):
            stats[3] = max(stats[3], R)
            stats[4 + min(P2_HIST - 1, int(R - 1).bit_length())] += 1
    return sa, sd, stats


# ---------------------------------------------------------------------------------------------- phase B: the table
def stepped_blocks(nb, G, first, chains, keys):
    """The blocks a launch steps through, per chain of the launch: all of a chain's blocks where composite keys are wanted; an
    expansion leaves out a chain's last block unless that is the last of all (chainmulti_geom's `active`, chain() above)."""
    out = []
    for c in range(chains):
        b0 = (first + c) * G
        b1 = min(nb, b0 + G)
        out.append([b for b in range(b0, b1) if keys or b + 1 < b1 or b + 1 == nb])
    return out


def _cm(name, m, nkeys, G, steps, first=0, chains=None, start="random", perm="random", states=True, keys=False, own_start=True):
    """steps: the blocks the launch steps through, written out per case (the CPU test holds them to stepped_blocks)."""
    nb = len(nkeys)
    return dict(name=name, m=m, nkeys=tuple(nkeys), G=G, first=first, chains=(nb + G - 1) // G - first if chains is None else chains,
                start=start, perm=perm, states=states, keys=keys, own_start=own_start, steps=tuple(steps))


def _chain_table():
    T = []
    for m in (11265, 12288, 12289):                                      # 12 parts on 3 part workgroups; 13 parts, the last of one row
        mixed = (1, 2, 512, 513, m, 300, 5000)                           # blocks of one and of two passes in one step of one launch
        T.append(_cm("expand-G1", m, mixed, 1, steps=(6,)))              # (chains of one block: only the last of all steps)
        T.append(_cm("expand-G2", m, mixed, 2, steps=(0, 2, 4, 6)))
        T.append(_cm("expand-G3", m, mixed, 3, steps=(0, 1, 3, 4, 6)))
        for G in (1, 2, 3):
            T.append(_cm("compose-G%d" % G, m, mixed, G, steps=range(7), states=False, keys=True, own_start=False))
        T.append(_cm("both-G3", m, mixed, 3, steps=range(7), states=True, keys=True))
        # 9, 8, 7 and 1 chains at work in the part and row kernels (the grid's y is rounded up to 8: workgroups without a chain):
        # compositions of chains of one block, and expansions of chains of two over seventeen blocks (nine chains, the last of one block)
        nine = (513, 2, m, 1, 512, 40, 513, 7000, 3)
        seventeen = (513, 2, 600, 1, 512, 40, 513, 7000, 3, 900, 2, 513, 64, 512, 5, 1000, 513)
        for first, chains in ((0, 9), (0, 8), (1, 7), (3, 1)):
            T.append(_cm("compose-G1-%d+%d" % (first, chains), m, nine, 1, steps=range(first, first + chains), first=first, chains=chains,
                         states=False, keys=True, own_start=False))
            T.append(_cm("expand-G2-%d+%d" % (first, chains), m, seventeen, 2, steps=[2 * g for g in range(first, first + chains)], first=first,
                         chains=chains, start="spikes"))
        T.append(_cm("compose-G2-1+3", m, nine, 2, steps=range(2, 8), first=1, chains=3, states=False, keys=True, own_start=False))
        for fam in D0_FAMILIES:
            for perm in ("identity", "reversal"):
                T.append(_cm("start", m, (513, 2, 4000), 2, steps=(0, 2), start=fam, perm=perm))
    # k_cm_output's own range maximum: pairs planted at both ends of every table level's gaps, in the order in front of block 0
    T.append(_cm("planted", 11265, (("planted", 300, tuple(range(8))), 513), 2, steps=(0, 1), start="spikes"))
    T.append(_cm("planted", 65537, (("planted", 2000, tuple(range(10))),), 1, steps=(0,)))
    T.append(_cm("planted", 300000, (("planted", 5000, tuple(range(13))),), 1, steps=(0,), start="spikes"))   # (4,688 blocks of 64: the one shape with level 12)
    m = 65537                                                            # 17 position bits: 32,768 keys share a word with a position, 32,769 do not
    T.append(_cm("one-launch", m, (32768, 32769), 2, steps=(0, 1), keys=True))
    T.append(_cm("apart-32768", m, (32768,), 1, steps=(0,)))
    T.append(_cm("apart-32769", m, (32769,), 1, steps=(0,)))
    m = 300000                                                           # 19 bits: two-word pairs throughout; three passes above 2^18 keys
    three = (262144, 262145, m)                                          # two passes, the fewest keys of three passes, all rows distinct
    T.append(_cm("compose-G1-passes-2-3-3", m, three, 1, steps=(0, 1, 2), states=False, keys=True, own_start=False))
    T.append(_cm("both-G3-passes-2-3-3", m, three, 3, steps=(0, 1, 2), states=True, keys=True, start="spikes"))
    T.append(_cm("mixed-chain", m, (262144, m), 2, steps=(0, 1), keys=True))
    for i, c in enumerate(T):
        c["seed"] = 5000 + i
        c["id"] = "%d-%s-%s-%s" % (c["m"], c["name"], c["perm"], c["start"])
    return T


CHAIN_CASES = _chain_table()


def build_chain(case):
    """Key blocks with exactly nkeys[b] keys each, divergences on both sides of every chain's first column, and the state in
    front of block 0 (where own_start: the launch's chains start from the sequential model's states, else from the identity)."""
    rng = np.random.default_rng(case["seed"])
    m, nk = case["m"], list(case["nkeys"])
    a, d = make_perm(case["perm"], m, rng), make_d0(case["start"], m, rng)
    rank = np.empty((len(nk), m), dtype=np.int64)
    keyd = np.empty((len(nk), m), dtype=np.int64)
    for b, n in enumerate(nk):
        if isinstance(n, tuple):
            # ("planted", background keys, levels): pairs planted in the order in front of the block, which must be the start state
            assert b == 0 and case["own_start"] and case["first"] == 0
            kp, nk[b] = keys_planted(keys_random(m, n[1], rng), n[1], planted_gaps(m, n[2]))
            rank[b] = key_by_row(a, kp)
        else:
            rank[b] = rng.permutation(m) if n == m else keys_random(m, n, rng) if n > 1 else 0
        keyd[b] = rng.integers(0, (b + 1) * COLS + 1, size=m)
    return dict(m=m, rank=rank, keyd=keyd, nkeys=np.array(nk, dtype=np.int64), a=a, d=d)
