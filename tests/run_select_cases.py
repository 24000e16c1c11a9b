"""The run steps' rank/select (csrc/fseq_chainsort.hpp, pass2_runs and chainwg_runs) as numpy, and the cases of
tests/test_proto_run_select.py (CPU) and tests/test_gpu_run_select.py (the kernels against the model of tests/chain_step_cases.py).
No GPU and no library in here.  TEST INFRASTRUCTURE.

The sorted runs of a step have first NEW positions off[0] = 0 < off[1] < ... < off[R - 1] < m.  The kernels keep a bitmap of them
(bit p of word p >> 6 set: new position p starts a run) and pre[w], the starts in front of word w; the run of position p is
pre[p >> 6] + popcount(bits[p >> 6] & (the bits up to and including p & 63)) - 1, and p is a head where its own bit is set."""
import numpy as np

import chain_step_cases as cs

NW = 16                     # waves of the workgroup
PIECE = 8                   # positions a lane reads at once in pass2_runs' sweeps over the 16-bit ranks (16 bytes)
SEL_ROWS = 1 << 18          # most rows the bitmap holds; k_chain_wg keeps the search above


def chunk(m):
    """Positions of a wave's chunk: whole groups of 64."""
    return ((m + NW - 1) // NW + 63) & ~63


# ---------------------------------------------------------------------------------------------- the select
def build_select(off, m):
    """(bits [ceil(m / 64)] uint64, pre [the same] int64) from the runs' first new positions."""
    off = np.asarray(off, dtype=np.int64)
    nw = (m + 63) // 64
    bits = np.zeros(nw, dtype=np.uint64)
    np.bitwise_or.at(bits, off >> 6, np.uint64(1) << (off & 63).astype(np.uint64))
    cnt = np.array([bin(int(x)).count("1") for x in bits], dtype=np.int64)
    return bits, np.cumsum(cnt) - cnt


def select(bits, pre, p):
    """(run, head) of the new positions p."""
    p = np.asarray(p, dtype=np.int64)
    w, lane = p >> 6, (p & 63).astype(np.uint64)
    word = bits[w]
    upto = word & (np.uint64(0xFFFFFFFFFFFFFFFF) >> (np.uint64(63) - lane))
    # popcount of 64-bit words: bytes of the array, bits of the bytes
    cnt = np.unpackbits(upto.view(np.uint8).reshape(-1, 8), axis=1).sum(axis=1).astype(np.int64)
    return pre[w] + cnt - 1, ((word >> lane) & np.uint64(1)).astype(bool)


def layout(lens):
    """(off, m) of runs of these lengths."""
    lens = np.asarray(lens, dtype=np.int64)
    assert len(lens) and lens.min() >= 1
    return np.cumsum(lens) - lens, int(lens.sum())


def _layouts():
    rng = np.random.default_rng(17)
    L = {}
    L["R1"] = [11265]
    L["every-position-a-head"] = [1] * 11265                      # (every word but the last holds 64 starts)
    L["starts-0-31-32-63"] = [31, 1, 31, 1] * 100 + [7]          # starts at 0, 31, 32, 63 mod 64, m = 6,407
    L["a-word-of-64-starts"] = [200] + [1] * 64 + [300, 56] + [1] * 64 + [9]   # starts 200 .. 263 straddle words; 820 .. 883 too
    L["a-whole-word-of-starts"] = [192] + [1] * 64 + [77]        # word 3 holds 64 starts
    L["long-runs"] = [129, 500, 64, 128, 1000, 3, 4097, 1]       # words with no start
    L["random-11265"] = list(np.diff(np.r_[0, np.sort(rng.choice(np.arange(1, 11265), size=8831, replace=False)), 11265]))
    L["random-100000"] = list(np.diff(np.r_[0, np.sort(rng.choice(np.arange(1, 100000), size=7900, replace=False)), 100000]))
    L["most-runs"] = list(np.diff(np.r_[0, np.sort(rng.choice(np.arange(1, SEL_ROWS), size=16383, replace=False)), SEL_ROWS]))
    return L


LAYOUTS = _layouts()


# ---------------------------------------------------------------------------------------------- pass 2: keys by position
def keys_from_starts(starts, m, D):
    """By position: runs that start at `starts` (sorted, 0 among them), run j of class j mod D (D >= 2: neighbours differ)."""
    starts = np.asarray(sorted(set(int(x) for x in starts)), dtype=np.int64)
    assert starts[0] == 0 and starts[-1] < m and D >= 2
    return np.repeat(np.arange(len(starts)) % D, np.diff(np.r_[starts, m])).astype(np.int64)


def edge_starts(m):
    """Run starts at every residue mod 8, at 63, 64, 65, on both sides of every border of a wave's chunk, and eight runs of one
    position inside one lane's piece (positions 2048 .. 2055)."""
    st = {0, 63, 64, 65}
    st.update(1000 + 9 * i for i in range(8))
    st.update(range(2048, 2057))
    c = chunk(m)
    for b in range(c, m, c):
        st.update((b - 1, b, b + 1))
    st.update((m - 1,))
    return sorted(x for x in st if x < m)


def keys_new_positions(m, n):
    """By position: n runs of classes of their own, laid out in a random order, whose lengths by class are 31, 1, 31, 1, ...: sorted
    by class their first new positions are 0, 31, 32, 63 mod 64; the rest of the positions one run of the last class.  Returns
    (keys by position, D)."""
    rng = np.random.default_rng(n)
    lens = np.array([31, 1] * (n // 2), dtype=np.int64)
    assert n % 2 == 0 and lens.sum() + 129 <= m
    order = rng.permutation(n)
    # the long run of class n first, then the n runs in a random order
    kp = np.r_[np.full(m - lens.sum(), n), np.repeat(order, lens[order])]
    return kp.astype(np.int64), n + 1


def keys_far_pair(m, rng):
    """By position: a background of 40 runs of 9 classes, and class 9 in two runs of five positions 300 positions apart.  Returns
    (keys by position, D, first position of the second run)."""
    kp = cs.keys_runs(m, 40, 9, rng)
    p1 = 3001
    kp[p1:p1 + 5] = 9
    kp[p1 + 305:p1 + 310] = 9
    return kp, 10, p1 + 305


def sorted_run_starts(kp):
    """First new positions of the runs of keys-by-position kp, runs by (class, start)."""
    kp = np.asarray(kp, dtype=np.int64)
    st = np.flatnonzero(np.r_[True, kp[1:] != kp[:-1]])
    ln = np.diff(np.r_[st, len(kp)])
    order = np.lexsort((st, kp[st]))
    return np.cumsum(ln[order]) - ln[order]


def _case(name, m, keys, run_cap=cs.P2_RUN_CAP, path="runs", runs=None, d0="random", blocks=("gathered",)):
    return dict(name=name, m=m, keys=keys, run_cap=run_cap, path=path, runs=runs, d0=d0, blocks=tuple(blocks))


def _pass2_table():
    T = []
    m = 11265
    T.append(_case("edges-handed-handed", m, ("edges", 5), blocks=("handed", "handed")))
    T.append(_case("edges-handed-gathered", m, ("edges", 5), blocks=("handed", "gathered")))
    T.append(_case("edges-gathered-handed", m, ("edges", 7), blocks=("gathered", "handed"), d0="spikes"))
    for mm in (11272, 12288, 12289):
        T.append(_case("runs-3000", mm, ("runs", 3000, 700), runs=3000, blocks=("handed", "handed")))
        T.append(_case("edges", mm, ("edges", 3), blocks=("gathered", "handed"), d0="spikes"))
    T.append(_case("R1", m, ("runs", 1, 1), runs=1, blocks=("gathered", "handed")))
    T.append(_case("R8832", m, ("runs", 8832, 4352), runs=8832, blocks=("gathered", "handed")))
    T.append(_case("R8833", m, ("runs", 8833, 4352), runs=8833, path="p4", blocks=("gathered", "handed")))
    T.append(_case("R100cap100", m, ("runs", 100, 40), run_cap=100, runs=100, blocks=("gathered", "handed")))
    T.append(_case("R101cap100", m, ("runs", 101, 40), run_cap=100, runs=101, path="p4", blocks=("gathered", "handed")))
    T.append(_case("new-positions", m, ("new-positions", 600), runs=601, blocks=("gathered", "handed")))
    T.append(_case("far-pair", m, ("far-pair",), runs=None, d0="spikes", blocks=("gathered", "handed")))
    for i, c in enumerate(T):
        c["seed"] = 1700 + i
        c["id"] = "%d-%s-cap%d" % (c["m"], c["name"], c["run_cap"])
    return T


PASS2_CASES = _pass2_table()


def case_keys(case, rng):
    """(keys by position, D) of one block of a case."""
    m, spec = case["m"], case["keys"]
    if spec[0] == "edges":
        return keys_from_starts(edge_starts(m), m, spec[1]), spec[1]
    if spec[0] == "runs":
        return (cs.keys_runs(m, spec[1], spec[2], rng) if spec[1] > 1 else np.zeros(m, dtype=np.int64)), spec[2]
    if spec[0] == "new-positions":
        return keys_new_positions(m, spec[1])
    kp, D, _ = keys_far_pair(m, rng)
    return kp, D


def build_pass2(case):
    """One launch: a block per entry of case["blocks"] (the same keys by position, a state of its own), one task a block.  hand_keys
    holds every block's ranks by position; the `rank` that goes to the kernel is zeroed for the blocks handed over (a kernel that
    gathered there would get one run)."""
    rng = np.random.default_rng(case["seed"])
    m = case["m"]
    a0, d0, rank, cls, headd, ncls, kps = [], [], [], [], [], [], []
    for _ in case["blocks"]:
        kp, D = case_keys(case, rng)
        a = cs.make_perm("random", m, rng)
        cap = min(cs.P2_CLS_CAP, 2 * D + 5)
        r, c, h = cs.task_tables(cs.key_by_row(a, kp), D, cap, rng)
        a0.append(a); d0.append(cs.make_d0(case["d0"], m, rng)); rank.append(r); cls.append(c); headd.append(h); ncls.append(D); kps.append(kp)
    rank = np.array(rank)
    a0 = np.array(a0)
    handed = np.array([b == "handed" for b in case["blocks"]])
    return dict(m=m, a0=a0, d0=np.array(d0), rank=rank, cls=np.array(cls), headd=np.array(headd), ncls=np.array(ncls, dtype=np.int64),
                task_blk=np.arange(len(case["blocks"])), kp=np.array(kps), hand_keys=np.take_along_axis(rank, a0, axis=1),
                hand_flag=handed.astype(np.int64), rank_given=np.where(handed[:, None], 0, rank))


# ---------------------------------------------------------------------------------------------- phase B: both sides of the bitmap
def _cw(name, m, blocks, paths, runs):
    import chain_wg_cases as cw
    c = cw._c(name, m, blocks, 1, paths, runs=runs, start="spikes")
    c["seed"] = 1790 + len(name) + (m & 1)
    c["id"] = "%d-%s" % (m, name)
    return c


def _cw_table():
    T = []
    for m in (SEL_ROWS, SEL_ROWS + 1):                                    # the last m of the bitmap; the first of the kept search
        T.append(_cw("runs-9000", m, [("runs", 9000, 3000)], ["runs"], [9000]))
    T.append(_cw("runs-16384", SEL_ROWS, [("runs", 16384, 5000)], ["runs"], [16384]))
    T.append(_cw("one-key", 11265, [("one",)], ["runs"], [1]))
    T.append(_cw("borders", 11265, [("borders", 7)], ["runs"], None))
    return T


CW_CASES = _cw_table()
