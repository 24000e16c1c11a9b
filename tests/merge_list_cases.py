"""The traceback and the greedy merge (k_tb_windows, k_tb_chain, k_tb_chain_part, k_tb_emit, k_seg_tau, k_seg_tau_tb, k_seg_count;
csrc/fseq_kernels.hpp) on constructed DP arrays and column lists: the model, the generators, the tables.

The model is the reference's own two loops, written from their text and from nothing of the library: follow_traceback follows lb
from entry n - L until lb == 0 and reverses; find_segments_greedy goes boundary by boundary, counts the rows whose divergence at
column rb - 1 exceeds current_lb, joins where the count is at most max_segment_size and else emits the segment in front at its last
size.  The count comes from the list of column rb - 1 expanded into its multiset of values, the lump standing at k + 1 (a lump holds
the values >= k + 2 - L, and current_lb <= rb - L lies below them).  On a cut list the model also says when the answer cannot be
told: the list is incomplete, its cumulative count never exceeds max_segment_size, and current_lb lies below its last value -- the
library must then report overflow.  The threshold a boundary's list gives ({tau, kind}, k_seg_tau) is a few lines of its own over
the cumulative counts.  test_merge_list_cases.py pins all of this to the oracle on real alignments.  Plain numpy; no device.

The traceback cases are chains: the entries the traceback visits, last segment first, laid into an lb array whose other entries are
0 (clean) or redrawn from everything a word can hold (garbage).  Their lists are {k + 1, m} lumps and max_size[n - L] = m, so no
merge runs.  The merge cases are boundaries with a list each, over lump lists elsewhere."""
import functools

import numpy as np

W = 8192                          # TB_WIN, csrc/fseq_kernels.hpp
FIRST_COPY = 4096                 # entries follow_traceback fetches with the count on a fresh context, csrc/fseq_path_dp.hip
GUESS_SLACK = 16                  # ... and behind the last run's count on a reused one
TAU_EXACT, TAU_OPEN, TAU_NEVER = 0, 1, 2
NONE = 0xFFFFFFFF

DPARG = np.dtype([("lb", "<u8"), ("rb", "<u8"), ("segment_max_size", "<u4"), ("segment_size", "<u4")])
SEGMENT = np.dtype([("lb", "<u8"), ("rb", "<u8"), ("segment_size", "<u4"), ("reserved", "<u4")])


def stride_of(X):
    return (X + 3) & ~1


# ---- the model
def traceback(n, L, lb, max_size, size):
    """follow_traceback: from entry n - L along arg_idx = lb - L until lb == 0, reversed."""
    out, t = [], n - L
    while True:
        out.append((int(lb[t]), t + L, int(max_size[t]), int(size[t])))
        if lb[t] == 0:
            break
        assert L <= lb[t] <= t, (t, int(lb[t]))
        t = int(lb[t]) - L
    return np.array(out[::-1], dtype=DPARG)


def chain_of(n, L, lb):
    """The entries the traceback visits, last segment first."""
    out, t = [], n - L
    while True:
        out.append(t)
        if lb[t] == 0:
            return out
        t = int(lb[t]) - L


def multiset(ent, hdr, k):
    """The divergence values column k's list stands for: every value as often as its count, the lump at k + 1."""
    ne = int(hdr[k, 0])
    assert ent[k, 0, 0] == k + 1
    return np.repeat(ent[k, :ne, 0].astype(np.int64), ent[k, :ne, 1].astype(np.int64))


def merge(m, tb, ent, hdr):
    """find_segments_greedy over the traceback tb: (segments as SEGMENT, overflow, the boundary it could not tell or None)."""
    max_seg = int(tb[-1]["segment_max_size"])
    out = []
    current_lb, prev_size, prev = 0, int(tb[0]["segment_size"]), 0
    for j in range(1, len(tb)):
        k = int(tb[j]["rb"]) - 1
        values = multiset(ent, hdr, k)
        if not hdr[k, 2] and len(values) <= max_seg and current_lb < values[-1]:
            return np.zeros(0, dtype=SEGMENT), True, j               # (the values the list left out may or may not exceed current_lb)
        count = int((values > current_lb).sum())
        if count <= max_seg:
            prev_size = count
        else:
            out.append((current_lb, int(tb[prev]["rb"]), prev_size, 0))
            prev_size = int(tb[j]["segment_size"])
            current_lb = int(tb[prev]["rb"])
        prev = j
    out.append((current_lb, int(tb[prev]["rb"]), prev_size, 0))
    return np.array(out, dtype=SEGMENT), False, None


def threshold(ent, hdr, k, max_seg):
    """{tau, kind} of column k's list: the value of the first entry at which the cumulative count exceeds max_seg -- NEVER where that
    is the lump --, else 0 on a complete list and the last value, OPEN, on one that was cut."""
    ne = int(hdr[k, 0])
    cum = np.cumsum(ent[k, :ne, 1].astype(np.int64))
    over = np.nonzero(cum > max_seg)[0]
    if len(over):
        return (NONE, TAU_NEVER) if over[0] == 0 else (int(ent[k, over[0], 0]), TAU_EXACT)
    return (0, TAU_EXACT) if hdr[k, 2] else (int(ent[k, ne - 1, 0]), TAU_OPEN)


def thresholds(tb, ent, hdr):
    max_seg = int(tb[-1]["segment_max_size"])
    return np.array([threshold(ent, hdr, int(e["rb"]) - 1, max_seg) for e in tb], dtype=np.uint32).reshape(len(tb), 2)


def excess_entry(ent, hdr, k, max_seg):
    """Index of the first entry at which the cumulative count exceeds max_seg, or None."""
    cum = np.cumsum(ent[k, :int(hdr[k, 0]), 1].astype(np.int64))
    over = np.nonzero(cum > max_seg)[0]
    return int(over[0]) if len(over) else None


# ---- what a chain asks of the traceback kernels, from the model alone
def doubling_rounds(L):
    """Rounds of k_tb_windows' doubling: span = 1, 2, 4, ... while span < W / L + 2."""
    r, span = 0, 1
    while span < W // L + 2:
        r, span = r + 1, span * 2
    return r


def window_profile(chain):
    """[(window, chain entries in it, entered at its top entry)] in the order the chain visits them."""
    out = []
    for t in chain:
        w = t // W
        if out and out[-1][0] == w:
            out[-1][1] += 1
        else:
            out.append([w, 1, t % W == W - 1])
    return [tuple(x) for x in out]


def part_profile(chain, part_lo, dp_size):
    """(entries per part, windows per part) of the chain over the parts [part_lo[g], part_lo[g + 1])."""
    hi = list(part_lo[1:]) + [dp_size]
    ents, wins = [], []
    for lo, h in zip(part_lo, hi):
        mine = [t for t in chain if lo <= t < h]
        ents.append(len(mine))
        wins.append(len({t // W for t in mine}))
    return np.array(ents, dtype=np.uint32), np.array(wins, dtype=np.uint32)


def part_features(chain, part_lo, dp_size):
    """Which of the placements the issue lists a layout of part borders reaches on this chain."""
    ents, _ = part_profile(chain, part_lo, dp_size)
    borders = list(part_lo[1:])
    on = set(chain)
    visited = [g for g in range(len(part_lo)) if ents[g]]
    f = set()
    if any(b % W == 0 for b in borders):
        f.add("window_border")
    if any(64 < b % W < W - 64 for b in borders):
        f.add("mid_window")
    if any(a // W == b // W for a, b in zip(borders, borders[1:])):
        f.add("shared_window")
    if any(not ents[g] and min(visited) < g < max(visited) for g in range(len(part_lo))):
        f.add("jumps_over_a_part")
    # the chain leaves the part above a border b to exactly b - 1; the chain stands at b, the part's first entry
    if any(b - 1 in on for b in borders):
        f.add("leaves_to_vlo_minus_1")
    if any(b in on for b in borders):
        f.add("stays_at_vlo")
    last_part = max(g for g in range(len(part_lo)) if part_lo[g] <= chain[-1])
    if 0 < last_part < len(part_lo) - 1:
        f.add("ends_in_a_middle_part")
    return f


# ---- the traceback cases
def lb_of_chain(n, L, chain):
    dp_size = n - L + 1
    assert chain[0] == n - L and all(a - b >= L for a, b in zip(chain, chain[1:])) and chain[-1] >= 0, (n, L, chain[:3], chain[-3:])
    assert len(chain) <= n // L + 2
    lb = np.zeros(dp_size, dtype=np.uint32)
    c = np.array(chain, dtype=np.int64)
    lb[c[:-1]] = c[1:] + L
    return lb


def stride_chain(top, L, stop=0):
    return list(range(top, stop - 1, -L))


def random_chain(top, L, S, seed):
    """S entries from `top` down, hops of at least L drawn from a fixed seed."""
    rng = np.random.default_rng(seed)
    spare = top - (S - 1) * L
    assert spare >= 0
    extra = rng.multinomial(rng.integers(0, spare + 1), np.ones(S - 1) / (S - 1)) if S > 1 else np.zeros(0, dtype=np.int64)
    return [top] + (top - np.cumsum(L + extra)).tolist()


def _min_stride(L, dp_size):
    """From the final entry to the top entry of the highest window below it (where it does not stand on one), then hops of L: that
    window holds ceil(W / L) chain entries and is entered at its top entry."""
    top = dp_size - 1
    if top % W == W - 1:
        return stride_chain(top, L)
    t = ((top - L + 1) // W) * W - 1
    assert t >= 0 and top - t >= L
    return [top] + stride_chain(t, L)


def _large_L(L):
    top = 5 * L + 37                                            # n = 6 L + 37
    return [top] + stride_chain(4 * W - 1, L)


TB_M = 40                                                       # rows of the traceback cases' contexts (their lists are lumps)
TB_CASES = {}


def _tb(name, L, dp_size, chain, listed_for):
    TB_CASES[name] = dict(L=L, n=dp_size + L - 1, chain=chain, listed_for=listed_for)


_tb("one_segment_100", 5, 100, [99], dict(S=1))
_tb("one_segment_W_plus_1", 5, W + 1, [W], dict(S=1, windows=[1]))
_tb("every_entry", 1, 3 * W + 5, stride_chain(3 * W + 4, 1), dict(S=3 * W + 5, full_window=W, rounds=14, second_copy=1))
for _L in (2, 3, 7):
    for _d in (2 * W - 1, 2 * W, 2 * W + 1):
        _tb("min_stride_L%d_%d" % (_L, _d), _L, _d, _min_stride(_L, _d), dict(full_window=-(-W // _L), rounds=doubling_rounds(_L)))
# borders (L = 3, four windows): a successor exactly at a window's first entry (3W), one below a window's first entry (2W - 1, from
# inside window 2), a chain entry at 0
_tb("borders", 3, 4 * W, [4 * W - 1, 3 * W + 100, 3 * W, 2 * W + 50, 2 * W - 1, W + 7, 5, 0],
    dict(successor_at_base=3 * W, successor_below_base=2 * W - 1, entry_at_0=1))
_tb("ends_in_window_2_of_4", 3, 4 * W, [4 * W - 1, 3 * W + 9, 2 * W + 77], dict(windows=[3, 2]))
# (the final entry 6W + 2 stands in window 6, so the chain begins there; below it, it visits windows 5, 2 and 0 only)
_tb("skipped_windows", 5, 6 * W + 3, [6 * W + 2, 5 * W + 4000, 5 * W + 100, 2 * W + 8000, 2 * W + 3, 500, 17], dict(windows=[6, 5, 2, 0]))
for _L in (8191, 8192, 8193):
    _tb("large_L%d" % _L, _L, 5 * _L + 38, _large_L(_L), dict(two_in_a_window=int(_L == 8191)))

# one context, L = 2, n = 12,000, calls in this order: S at, one above and far below the count of the call before + 16 (the issue's
# five, then 100 and 117 again: 117 behind 100 stands one above 116)
REUSE_L, REUSE_N = 2, 12000
REUSE_S = (5000, 100, 116, 117, 4097, 100, 117)


def reuse_chain(i):
    return random_chain(REUSE_N - REUSE_L, REUSE_L, REUSE_S[i], 900 + i)


def lump_lists(m, n, X, open_every=0):
    """Column k's list is the lump {k + 1, m}; open_every: every such column's is cut instead, {k + 1, m - 1} and incomplete, so that
    its threshold names the column ({k + 1, OPEN})."""
    ent = np.zeros((n, stride_of(X), 2), dtype=np.uint32)
    hdr = np.zeros((n, 4), dtype=np.uint32)
    ent[:, 0, 0] = np.arange(1, n + 1)
    ent[:, 0, 1] = m
    hdr[:] = (1, 0, 1, m)
    if open_every:
        ent[1::open_every, 0, 1] = m - 1
        hdr[1::open_every] = (1, 0, 0, m - 1)
    return ent, hdr


def garbage(n, L, lb, seed):
    """lb with every entry off the chain redrawn from: 0; 1 .. L - 1; lb - L >= t; beyond dp_size + L; 0xFFFFFFFF; valid-looking
    pointers (short hops, so that the doubling has chains to follow off the real one)."""
    dp_size = n - L + 1
    rng = np.random.default_rng(seed)
    t = np.arange(dp_size, dtype=np.int64)
    kind = rng.integers(0, 7, size=dp_size)
    out = np.zeros(dp_size, dtype=np.int64)
    out[kind == 1] = rng.integers(1, max(L, 2), size=dp_size)[kind == 1] if L > 1 else 0
    up = t + L + rng.integers(0, 50, size=dp_size)
    out[kind == 2] = up[kind == 2]
    out[kind == 3] = (dp_size + L + 1 + rng.integers(0, 1 << 20, size=dp_size))[kind == 3]
    out[kind == 4] = NONE
    hop = L + rng.integers(0, 3 * L + 3, size=dp_size)
    valid = np.where(t - hop >= 0, t - hop + L, 0)
    out[kind >= 5] = valid[kind >= 5]
    out = out.astype(np.uint32)
    on = np.array(chain_of(n, L, lb), dtype=np.int64)
    out[on] = lb[on]
    return out


def foreign_pointers(n, L, seed):
    """Valid-looking pointers in every entry: what a part would follow if it trusted entries that are not its own."""
    dp_size = n - L + 1
    rng = np.random.default_rng(seed)
    t = np.arange(dp_size, dtype=np.int64)
    hop = L + rng.integers(0, 2 * L + 2, size=dp_size)
    return np.where(t - hop >= 0, t - hop + L, 0).astype(np.uint32)


@functools.lru_cache(maxsize=None)
def tb_arrays(name, dirty):
    """(lb, max_size, size) of a traceback case; dirty: off-chain lb redrawn.  max_size and size are random everywhere but
    max_size[n - L] = m (no merge runs)."""
    c = TB_CASES[name]
    return chain_arrays(c["n"], c["L"], tuple(c["chain"]), dirty, sum(map(ord, name)))


@functools.lru_cache(maxsize=8)
def chain_arrays(n, L, chain, dirty, seed):
    lb = lb_of_chain(n, L, list(chain))
    if dirty:
        lb = garbage(n, L, lb, seed)
    rng = np.random.default_rng(seed + 1)
    mx = rng.integers(0, 1 << 32, size=n - L + 1, dtype=np.uint32)
    sz = rng.integers(0, 1 << 32, size=n - L + 1, dtype=np.uint32)
    mx[n - L] = TB_M
    for a in (lb, mx, sz):
        a.setflags(write=False)
    return lb, mx, sz


def part_layouts(name):
    """{layout: part_lo} for a traceback case, n_parts in {1, 2, 3, 8}: borders on a window border, in mid-window, two in one
    window, at a chain entry (the chain stays at vlo) and one behind a chain entry (it leaves to vlo - 1), a part the chain jumps
    over, a middle part the chain ends in."""
    c = TB_CASES[name]
    chain = c["chain"]
    dp_size = c["n"] - c["L"] + 1
    out = {"one": [0]}

    def put(key, borders):
        b = sorted({int(x) for x in borders if 0 < x < dp_size})
        if len(b) == len(borders):
            out[key] = [0] + b

    if dp_size > W:
        put("window_border_2", [W * ((dp_size - 1) // W)])
        put("shared_window_3", [W, W + 1000])                                                 # two borders in window 1
    put("mid_window_2", [dp_size // 2 + (1000 if dp_size // 2 % W == 0 and dp_size > 4000 else 0)])
    if len(chain) >= 3:
        low = chain[len(chain) // 2] if len(chain) >= 4 else chain[-1]
        put("at_entries_3", [low + 1, chain[1]])                                              # leaves to vlo - 1 = low; stays at vlo = chain[1]
    if len(chain) >= 2 and chain[-1] > 0:
        put("ends_in_middle_3", [chain[-1], chain[-2]])                                       # part 1 holds the last entry alone
    if len(chain) >= 2 and chain[0] - chain[1] > 1:
        put("jumped_3", [chain[1] + 1, chain[1] + 2])                                         # part 1 holds no chain entry
    if dp_size >= 64:
        put("eight", [dp_size * i // 8 for i in range(1, 8)])
    return out


# ---- the merge cases: m rows, L = 4, boundaries with a list each over lump lists
MG_M, MG_L = 1000, 4
MG_CASES = {}


class Merge:
    """A traceback of boundaries rb[0] < rb[1] < ... < rb[S - 1] = n and the list of every boundary's column rb - 1."""

    def __init__(self, n, X, max_seg, m=MG_M, L=MG_L):
        self.m, self.n, self.L, self.X, self.max_seg = m, n, L, X, max_seg
        self.ent, self.hdr = lump_lists(m, n, X)
        self.rbs = []

    def boundary(self, rb, values, counts, complete=None):
        """The list of column rb - 1: {rb, counts[0]} and the values behind it, descending and at most rb - L."""
        assert (not self.rbs or rb - self.rbs[-1] >= self.L) and rb >= self.L and (rb <= self.n - self.L or rb == self.n), rb
        vs = [rb] + list(values)
        assert len(vs) == len(counts) <= self.ent.shape[1] and all(a > b for a, b in zip(vs, vs[1:])) and (len(vs) == 1 or vs[1] <= rb - self.L), (rb, vs[:3])
        s = int(np.sum(counts))
        assert s <= self.m and all(c >= 1 for c in counts[1:])
        if complete is not None:
            assert complete == (s == self.m), (rb, s)
        k = rb - 1
        self.ent[k] = 0
        self.ent[k, :len(vs), 0] = vs
        self.ent[k, :len(vs), 1] = counts
        self.hdr[k] = (len(vs), counts[-1] if vs[-1] == 0 else 0, 1 if s == self.m else 0, s)
        self.rbs.append(rb)

    def arrays(self, seed=0):
        """(lb, max_size, size): the chain of the boundaries, sizes that name their entry, everything else random."""
        n, L = self.n, self.L
        assert self.rbs[-1] == n
        chain = [rb - L for rb in self.rbs][::-1]
        lb = lb_of_chain(n, L, chain)
        rng = np.random.default_rng(seed + 77)
        mx = rng.integers(0, 1 << 32, size=n - L + 1, dtype=np.uint32)
        sz = rng.integers(0, 1 << 32, size=n - L + 1, dtype=np.uint32)
        mx[n - L] = self.max_seg
        sz[np.array(chain)] = 100000 + np.array(chain)
        return lb, mx, sz


def excess_list(rb, nent, p, max_seg, m, complete, top_gap=0, last_value=None):
    """(values, counts) of a list of nent entries behind boundary rb whose cumulative count is exactly max_seg at entry p - 1 and
    exceeds it first at entry p (p = nent: never).  Single counts behind the lump, the rest of the rows on the last entry of a
    complete list."""
    top = rb - MG_L - top_gap
    values = [top - i for i in range(nent - 1)]
    if last_value is not None and nent > 1:
        values[-1] = last_value
    counts = [max_seg - p + 1] + [1] * (nent - 1)
    assert counts[0] >= 0
    if complete:
        counts[-1] += m - sum(counts)
    return values, counts


def _strips():
    """One boundary per (list length, entry of the first excess): lists of 1, 2, 63, 64, 65, 127, 128, 129 and 200 entries, the first
    excess at entry 0 (NEVER), 1, 63, 64, 65, 128 and the last entry, and none on a cut list (OPEN).  Behind entry p - 1 the cumulative
    count is exactly max_seg: p = 64 and p = 65 put that at entries 63 and 64.  The OPEN lists end in value 1, below every current_lb
    behind the first cut."""
    max_seg = 300
    specs = []
    for nent in (1, 2, 63, 64, 65, 127, 128, 129, 200):
        for p in sorted({0, 1, 63, 64, 65, 128, nent - 1}):
            if p < nent:
                specs.append((nent, p))
        specs.append((nent, nent))
    specs.remove((1, 1))                                           # (a cut list of the lump alone is undecided at any current_lb: undecided_first)
    specs.sort(key=lambda s: (s[0], s[1] != 0))                    # short lists in front; every length begins with its NEVER
    G = Merge(MG_L + 8 + 220 + 6 * len(specs), 198, max_seg)
    G.boundary(8, [], [G.m])                                       # the first segment, and a cut behind it: current_lb >= 8 from here on
    rb = 8
    for i, (nent, p) in enumerate(specs):
        rb = max(rb + 6, nent + MG_L + 2)
        if p == nent:
            v, c = excess_list(rb, nent, p, max_seg - 40, G.m, False, i % 3, last_value=1)
        else:
            v, c = excess_list(rb, nent, p, max_seg, G.m, complete=(i % 2 == 0), top_gap=i % 3)
        G.boundary(rb, v, c)
    G.boundary(G.n, [], [G.m])
    return G


def _walk(kind):
    """Short lists that steer the walk: see MG_CASES for what each kind is listed for."""
    max_seg = 50
    G = Merge(160, 8, max_seg)
    m = G.m
    rbs = list(range(10, 150, 10))
    if kind == "all_joins":
        # the first excess falls on the value-0 entry: tau = 0, every boundary joins at current_lb = 0
        for i, rb in enumerate(rbs):
            G.boundary(rb, [rb - 5, 0], [10 + i, 20, m - 30 - i])
        G.boundary(G.n, [100, 0], [7, 9, m - 16])
    elif kind == "all_cuts":
        for i, rb in enumerate(rbs):
            if i % 2:
                G.boundary(rb, [], [max_seg + 1 + i])                                     # NEVER
            else:
                G.boundary(rb, [rb - 4, rb - 5], [max_seg, 1, 3])                         # tau = rb - 4 > current_lb = the boundary before
        G.boundary(G.n, [], [m])
    elif kind == "alternating":
        for i, rb in enumerate(rbs):
            if i % 2:
                G.boundary(rb, [], [max_seg + 1])
            else:
                G.boundary(rb, [rb - 5, 3, 0], [20, 10, 40, m - 70])                      # tau = 3: joins behind any cut
        G.boundary(G.n, [3, 0], [30, 40, m - 70])
    elif kind == "tau_edges":
        # behind a cut current_lb = the boundary before: tau == current_lb joins, tau - 1 == current_lb cuts; a value equal to
        # current_lb is not counted into the merged size; a segment nothing joins keeps the DP's size
        G.boundary(10, [], [max_seg + 1])
        G.boundary(20, [], [max_seg + 1])                                                  # cut: current_lb = 10
        G.boundary(30, [12, 10, 9], [20, 30, 5, 7])                                        # tau = 10 == current_lb: joins, counts 50 (10 is not counted)
        G.boundary(40, [], [max_seg + 1])                                                  # cut: current_lb = 30; segment [10, 30) has the count of 30
        G.boundary(50, [33, 31, 29], [20, 30, 5, 7])                                       # tau = 31 == current_lb + 1: cuts; segment [30, 40) keeps the DP's size
        G.boundary(60, [41, 40, 0], [20, 30, 5, m - 55])                                   # current_lb = 40: tau = 40 joins; 40 itself not counted
        G.boundary(70, [50, 40, 39], [max_seg - 1, 1, 1, 4])                               # tau = 40: joins at current_lb = 40 with count max_seg exactly
        G.boundary(G.n, [], [m])
    else:
        raise KeyError(kind)
    return G


def _cut_lists(where):
    """Cut lists: OPEN and decided (current_lb >= the last value) at every third boundary, and undecided at the first, a middle or
    the last boundary the walk looks at (where = 0, 1, 2; None: nowhere)."""
    max_seg = 50
    G = Merge(120, 8, max_seg)
    G.boundary(10, [], [G.m])                                                               # the first segment: no boundary of the walk
    hit = {0: 20, 1: 60, 2: G.n}.get(where)
    for rb in list(range(20, 120, 10)) + [G.n]:
        if rb == hit and rb == 20:
            G.boundary(rb, [], [max_seg - 1])                                               # OPEN, the lump alone: undecided at any current_lb
        elif rb == hit:
            G.boundary(rb, [rb - 4, rb - 5], [10, 5, 5])                                    # OPEN, last value rb - 5 > any current_lb: undecided
        elif rb == 20:
            G.boundary(rb, [], [max_seg + 1])                                               # the first boundary cuts: current_lb >= 10 from here on
        elif rb % 30 == 0 or rb == G.n:
            G.boundary(rb, [8, 3], [10, 5, 5])                                              # OPEN, last value 3 <= current_lb: decided, joins
        else:
            G.boundary(rb, [], [max_seg + 1])
    return G


def _max_ge_m():
    """max_size[n - L] = m: the library merges nothing; complete lists without an excess give tau = 0 with the traceback."""
    G = Merge(120, 8, MG_M)
    for rb in range(10, 110, 10):
        G.boundary(rb, [rb - 6, 0], [10, 20, G.m - 30])
    G.boundary(G.n, [], [G.m])
    return G


def _large_S(S=5000):
    """S boundaries at hops of 4 to 6 columns with random short complete lists: thresholds of every value from a fixed seed, some of
    them exactly the boundary before."""
    rng = np.random.default_rng(4242)
    max_seg = 300
    hops = rng.integers(MG_L, MG_L + 3, size=S - 1)
    rbs = (8 + np.concatenate([[0], np.cumsum(hops[:-1])])).tolist()
    n = rbs[-1] + int(hops[-1]) + MG_L
    G = Merge(n, 4, max_seg)
    prev_rb = 0
    for rb in rbs + [n]:
        kind = int(rng.integers(0, 5))
        top = rb - MG_L
        if kind == 0:
            G.boundary(rb, [], [max_seg + 1 + int(rng.integers(0, 100))])                   # NEVER
        else:
            vs = {int(x) for x in rng.integers(0, top + 1, size=int(rng.integers(1, 4)))}
            if kind == 1 and prev_rb <= top:
                vs.add(prev_rb)
            vs = sorted(vs, reverse=True)
            cs = [int(rng.integers(100, max_seg))] + [int(rng.integers(1, 150)) for _ in vs]
            cs[-1] = G.m - sum(cs[:-1])
            G.boundary(rb, vs, cs, complete=True)
        prev_rb = rb
    return G


def _mg(name, build, listed_for):
    MG_CASES[name] = dict(build=build, listed_for=listed_for)


_mg("strips", _strips, dict(strips=1))
_mg("all_joins", functools.partial(_walk, "all_joins"), dict(segments=1, joins=14))
_mg("all_cuts", functools.partial(_walk, "all_cuts"), dict(cuts=14, joins=0))
_mg("alternating", functools.partial(_walk, "alternating"), dict(alternating=1))
_mg("tau_edges", functools.partial(_walk, "tau_edges"), dict(tau_eq_lb=2, tau_eq_lb_plus_1=1, keeps_dp_size=1, value_eq_lb=2, count_eq_max_seg=1))
_mg("open_decided", functools.partial(_cut_lists, None), dict(open_decided=4, overflow=0))
_mg("undecided_first", functools.partial(_cut_lists, 0), dict(overflow=1, undecided_at="first"))
_mg("undecided_middle", functools.partial(_cut_lists, 1), dict(overflow=1, undecided_at="middle"))
_mg("undecided_last", functools.partial(_cut_lists, 2), dict(overflow=1, undecided_at="last"))
_mg("max_ge_m", _max_ge_m, dict(no_merge=1))
_mg("large_S", _large_S, dict(S=5000, second_copy=1))


COUNT_STOPS = ((10, 130), (63, 130), (64, 130), (127, 130), (129, 130), (63, 64), (64, 65))


def _count_strips_case():
    """Pairs of a boundary that joins and one that cuts behind it, so that every join's count is a merged segment's size.  The join
    stands at current_lb = the boundary the cut in front of it moved it to, and its list -- 130 entries, 64 or 65 -- holds exactly
    that value at entry 10, 63, 64, 127 or at its last entry: k_seg_count counts the entries in front of it, not the entry itself,
    and leaves in the strip it stands in.  The first excess falls on the entry behind (tau = current_lb - 1), or nowhere on a cut
    list that ends in current_lb (OPEN, decided: every entry but the last is counted, no strip is left early)."""
    max_seg = 400
    G = Merge(150 + 145 * len(COUNT_STOPS) + 20, 134, max_seg)
    G.boundary(150, [], [G.m])
    G.boundary(155, [], [max_seg + 1])                                                      # cuts: current_lb = 150
    cur = 150
    for stop, nent in COUNT_STOPS:
        rb = cur + 140
        values = [cur + stop - 1 - i for i in range(nent - 1)]
        assert values[0] <= rb - MG_L and values[stop - 1] == cur and values[-1] >= 0
        counts = [5] + [2] * (nent - 1)
        if stop + 1 < nent:
            counts[stop + 1] = max_seg                                                      # the excess on the entry behind the value current_lb
        G.boundary(rb, values, counts)
        G.boundary(rb + 5, [], [max_seg + 1])                                               # cuts: current_lb = rb
        cur = rb
    G.boundary(G.n, [], [G.m])
    return G


_mg("count_strips", _count_strips_case, dict(count_stops=COUNT_STOPS))


@functools.lru_cache(maxsize=None)
def mg_case(name):
    """(G, lb, max_size, size) of a merge case."""
    G = MG_CASES[name]["build"]()
    lb, mx, sz = G.arrays(sum(map(ord, name)))
    return G, lb, mx, sz


@functools.lru_cache(maxsize=None)
def mg_expected(name):
    """(traceback, thresholds, segments, overflow, undecided boundary) of the model; max_size[n - L] >= m: the library's contract is
    that no segments come out (include/fseq_debug.h), the reference's loop is not asked."""
    G, lb, mx, sz = mg_case(name)
    tb = traceback(G.n, G.L, lb, mx, sz)
    tau = thresholds(tb, G.ent, G.hdr)
    if G.max_seg >= G.m:
        return tb, tau, np.zeros(0, dtype=SEGMENT), False, None
    seg, overflow, at = merge(G.m, tb, G.ent, G.hdr)
    return tb, tau, seg, overflow, at


def walk_steps(name):
    """'J' / 'C' per boundary 1 .. S - 1 as the model's walk takes them ('?' from the undecided one on), with current_lb at each."""
    G, lb, mx, sz = mg_case(name)
    tb, tau, _, _, _ = mg_expected(name)
    steps, lbs, current_lb, prev = [], [], 0, 0
    for j in range(1, len(tb)):
        lbs.append(current_lb)
        x, kind = int(tau[j, 0]), int(tau[j, 1])
        fits = kind != TAU_NEVER and current_lb >= x
        if not fits and kind == TAU_OPEN:
            steps.append("?")
            break
        steps.append("J" if fits else "C")
        if not fits:
            current_lb = int(tb[prev]["rb"])
        prev = j
    return "".join(steps), lbs


def split_layouts(name):
    """{layout: column splits} for a merge case: a boundary column equal to a split, one below a split, a range without a
    boundary, eight ranges."""
    G, lb, mx, sz = mg_case(name)
    cols = [rb - 1 for rb in G.rbs]
    mid = cols[len(cols) // 2]
    out = {"at_boundary": [mid], "one_above_boundary": [mid + 1], "empty_range": [mid + 1, mid + 2] if G.L > 2 else [mid + 1]}
    e = sorted({max(1, G.n * i // 8) for i in range(1, 8)} - {G.n})
    out["eight"] = e
    return out
