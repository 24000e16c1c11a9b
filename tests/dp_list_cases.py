"""Phase D (k_dp, csrc/fseq_dp.hpp) on constructed column lists: the model, the generators, the table.

The model is the oracle's own DP step and range-minimum structure (fso_dp_step, fso_rmq_update), driven over lists in the kernel's
format exactly as fso_segment_long drives them over the pBWT's counts: part 2 is m - cnt0, part 3 a dp_step on the list read
ascending with init = (0, k + 1, m, m), the final cell the step at text_pos = n - 1 written to entry n - L; the range-minimum handle
sits over the segment_max_size field of the DP_DTYPE array.  The per-cell measurements say what a list asks of the kernel: how many
entries a cell needs until the pruning bound cum > best is passed, where its lowest query begins, which sparse-table level a query
takes and where the kernel finds that level's samples.  Plain numpy over oracle/fso.py; no device.

The lists (SegmentationContext.debug_dp_on_lists): column k's list is ent[k] = {value, count} pairs, entry 0 the lump {k + 1, count
of the values >= thr = k + 2 - L}, then distinct values below thr descending; hdr[k] = {entries, count of value 0, complete,
cumulative count}.

The generators' columns, all valid by construction (test_dp_list_cases runs every case once under the oracle's debug build, whose
asserts certify them):
  level V, s   lump V, s single-count entries just below thr, the other m - V - s rows at value 0: holds M at V
  carry V      lump V and one entry {thr - 1, m - V}: M[t] = max(M[t - L], V), a value that travels until a level column ends it
  probe        lump 1 and `dense` single-count entries: gaps of 1 up to entry j, a fixed jump behind it, the rest at value 0: among
               level V columns its cell needs V + 1 entries, and from entry j on its queries begin jump x (i - j) entries back
  random       any valid complete list
Probes stand only where their whole list fits above value 0: a truncated probe drags the level down for everything behind it."""
import ctypes as C
import functools
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import fso  # noqa: E402
from proto_length_scan import cell_columns  # noqa: E402

DPW, DP_RL, PIPE_MIN_L, DP_TRN = 4096, 56, 96, 64      # csrc/fseq_dp.hpp, csrc/fseq_dpschedule.hpp
NONE = 0xFFFFFFFF


def stride_of(X):
    return (X + 3) & ~1


# ---- the round schedule (dp_schedule / dp_round, csrc/fseq_dpschedule.hpp) and what a round may read from the LDS ring (k_dp)
def schedule(L, n):
    pipe = L >= PIPE_MIN_L
    RL = (min(L // 2, 48) // 12) * 12 if pipe else min(L, DP_RL)
    nreg = (n - 2 * L) // RL + 1
    return dict(L=L, n=n, pipe=pipe, RL=RL, nreg=nreg, nrounds=nreg + (2 if pipe else 1))


def round_t0(S, r):
    """First entry of round r (the drain round and the final cell: the entry behind the last regular one, as k_dp's resume takes it)."""
    return r * S["RL"] if r < S["nreg"] else S["n"] - 2 * S["L"] + 1


def view_of(S, t):
    """(safe_lo, cb) of the round that computes entry t: entries >= safe_lo are read from the LDS ring, cb blocks are indexed."""
    L, n, RL = S["L"], S["n"], S["RL"]
    if t == n - L:
        filled = n - 2 * L + 1
    else:
        r = t // RL
        filled = r * RL if not S["pipe"] else (0 if r == 0 else (r - 1) * RL)
    inflight = 2 * RL if S["pipe"] else RL
    return max(0, filled + inflight + 128 - DPW), filled >> 6


def cut_rounds(S, residues=(), blocks=(), extra=()):
    """Rounds to cut at: for every residue the first regular round whose first entry T0 = residue (mod 64), for every block
    number the first with T0 // 64 = it, and the extra rounds; ascending, inside (0, rounds)."""
    out = set(int(x) for x in extra)
    for q in residues:
        out.add(next(r for r in range(1, S["nreg"]) if (r * S["RL"]) % 64 == q))
    for b in blocks:
        out.add(next(r for r in range(1, S["nreg"]) if (r * S["RL"]) // 64 == b))
    assert all(0 < r < S["nrounds"] for r in out)
    return tuple(sorted(out))


# ---- the model
def model(m, n, L, ent, hdr, debug=False):
    """(LB, M, SZ) of the DP over the lists, dp_size words each; the entries no cell writes read 0, as on the device."""
    lib = fso.lib(debug)
    dp_size = n - L + 1
    dp = np.zeros(dp_size, dtype=fso.DP_DTYPE)
    dp["segment_max_size"] = NONE
    dp["segment_size"] = NONE
    rmq = lib.fso_rmq_new(dp.ctypes.data + 16, 24, dp_size, 64)
    stride = ent.shape[1]
    # the lists read ascending: column k's is the last hdr[k][0] words of row k
    vals = np.ascontiguousarray(ent[:, ::-1, 0])
    cnts = np.ascontiguousarray(ent[:, ::-1, 1])
    nent = hdr[:, 0].astype(np.int64)
    cnt0 = hdr[:, 1].astype(np.int64)
    p2lim = min(2 * L, n - L) - 1
    arg = fso.DpArg()
    step, update = lib.fso_dp_step, lib.fso_rmq_update
    vbase, cbase, dpp = vals.ctypes.data, cnts.ctypes.data, dp.ctypes.data
    try:
        for k in cell_columns(n, L):
            final = k == n - 1
            t = n - L if final else k + 1 - L
            if not final and k < p2lim:
                s = m - int(cnt0[k])
                dp[t] = (0, k + 1, s, s)
            else:
                off = 4 * (k * stride + stride - int(nent[k]))
                arg.lb, arg.rb, arg.segment_max_size, arg.segment_size = 0, k + 1, m, m
                step(vbase + off, cbase + off, int(nent[k]), dpp, rmq, m, L, 0, k, C.byref(arg))
                dp[t] = (arg.lb, arg.rb, arg.segment_max_size, arg.segment_size)
            if not final:
                update(rmq, t)
    finally:
        lib.fso_rmq_free(rmq)
    written = np.zeros(dp_size, dtype=bool)
    written[:n - 2 * L + 1] = True
    written[n - L] = True
    out = []
    for f in ("lb", "segment_max_size", "segment_size"):
        a = dp[f].astype(np.uint32)
        a[~written] = 0
        out.append(a)
    return tuple(out)


def written_entries(n, L):
    return np.concatenate([np.arange(n - 2 * L + 1), [n - L]])


def unproven_cells(m, n, L, hdr, M):
    """proto_length_scan.unproven for every cell that reads its list (part 3 and the final cell): the columns left unproven."""
    p2lim = min(2 * L, n - L) - 1
    k = np.array([c for c in cell_columns(n, L) if c == n - 1 or c >= p2lim], dtype=np.int64)
    t = np.where(k == n - 1, n - L, k + 1 - L)
    bad = (hdr[k, 2] == 0) & (hdr[k, 3].astype(np.int64) <= M[t].astype(np.int64))
    return k[bad]


def _range_min(M, qb, qe):
    """min M[qb:qe) for arrays of ranges (a sparse table in numpy)."""
    T = [M.astype(np.int64)]
    while (1 << len(T)) <= len(M):
        h = 1 << (len(T) - 1)
        T.append(np.minimum(T[-1][:len(T[-1]) - h], T[-1][h:]))
    ln = np.maximum(qe - qb, 1)
    p = np.floor(np.log2(ln)).astype(np.int64)
    out = np.zeros(qb.shape, dtype=np.int64)
    for lev in np.unique(p):
        sel = p == lev
        out[sel] = np.minimum(T[lev][qb[sel]], T[lev][qe[sel] - (1 << lev)])
    return out


def measure(m, n, L, ent, hdr, M):
    """What the lists ask of k_dp, per cell that reads its list (arrays over those cells, in cell order) and per round:
    needed    list entries until the cumulative count passes the cell's value (the list's length where it ends first)
    back      how far behind the cell the lowest query of the strips the kernel evaluates begins (0: no query)
    far       that query begins below the round's safe_lo: the strip takes the memory path
    inside    the distance of the lowest query's begin above safe_lo (far cells: below, negative)
    level     the highest sparse-table level a query of those strips takes (-1: none), level_ring / level_mem: the highest with
              both samples in the LDS ring / with a sample from memory, on a strip that takes the memory path
    on_border the cell has an evaluated query over more than two blocks that ends on a block border
    ties      candidates of the evaluated strips that reach the cell's value, tie_strips: the strips they stand in
    mixed     a strip of the cell past the first holds queries on both sides of safe_lo
    hot       per regular round: more than half its cells need more than 32 entries (what drives pair_cool)"""
    S = schedule(L, n)
    p2lim = min(2 * L, n - L) - 1
    k = np.array([c for c in cell_columns(n, L) if c == n - 1 or c >= p2lim], dtype=np.int64)
    end = k + 1
    t = np.where(k == n - 1, n - L, end - L)
    best = M[t].astype(np.int64)
    E = ent[k].astype(np.int64)
    stride = E.shape[1]
    nent = hdr[k, 0].astype(np.int64)
    idx = np.arange(stride)[None, :]
    valid = idx < nent[:, None]
    v = E[:, :, 0]
    cc = np.where(valid & (v != 0), E[:, :, 1], 0)
    cum = np.cumsum(cc, axis=1)
    over = valid & (cum > best[:, None])
    needed = np.where(over.any(1), over.argmax(1) + 1, nent)
    # the strips: the pair step's 32 candidates, else 63 and then 64 a strip (dp_cell_pair, dp_cell_sequential)
    bound = np.where(needed <= 32, 32, 63 + 64 * ((np.maximum(needed, 63) - 63 + 63) // 64))
    vnext = np.concatenate([v[:, 1:], np.zeros((len(k), 1), dtype=np.int64)], axis=1)
    have_next = (idx + 1) < nent[:, None]
    ok = valid & (v != 0) & have_next & (vnext != 0)
    c_hi = np.minimum(v, (end + 1 - L)[:, None])
    lo = vnext.copy()
    low = lo < L
    ok &= ~(low & ~(L < c_hi))
    lo = np.where(low, L, lo)
    ok &= lo < c_hi
    ev = ok & (idx < bound[:, None])
    qb = np.where(ev, lo - L, 0)
    qe = np.where(ev, c_hi - L, 1)
    sl = np.array([view_of(S, int(x)) for x in t], dtype=np.int64)
    safe_lo, cb = sl[:, 0], sl[:, 1]
    qb_min = np.where(ev, qb, 1 << 40).min(1)
    has_q = ev.any(1)
    back = np.where(has_q, t - qb_min, 0)
    far = has_q & (qb_min < safe_lo)
    inside = np.where(has_q, qb_min - safe_lo, 1 << 40)
    beg_block, end_block = (qb >> 6) + 1, qe >> 6
    lev = np.where(ev & (beg_block < end_block), np.floor(np.log2(np.maximum(end_block - beg_block, 1))).astype(np.int64), -1)
    # a strip = the candidates the kernel evaluates together; the memory path is taken by the whole strip (the ballot)
    strip = np.where(idx < 63, 0, 1 + (idx - 63) // 64) * np.ones((len(k), 1), dtype=np.int64)
    strip = np.where((bound == 32)[:, None], 0, strip)
    lane_far = ev & (qb < safe_lo[:, None])
    nstrips = int(strip.max()) + 1
    strip_far = np.zeros((len(k), nstrips), dtype=bool)
    strip_near = np.zeros((len(k), nstrips), dtype=bool)
    for s in range(nstrips):
        strip_far[:, s] = (lane_far & (strip == s)).any(1)
        strip_near[:, s] = (ev & ~lane_far & (strip == s)).any(1)
    on_far_strip = np.take_along_axis(strip_far, strip, axis=1) & ev
    s1_ring = beg_block + (1 << np.maximum(lev, 0)) + DP_TRN > cb[:, None] + 2
    s2_ring = end_block + DP_TRN > cb[:, None] + 2
    level_ring = np.where(on_far_strip & (lev >= 0) & s1_ring & s2_ring, lev, -1).max(1)
    level_mem = np.where(on_far_strip & (lev >= 0) & ~(s1_ring & s2_ring), lev, -1).max(1)
    on_border = (ev & (lev >= 0) & ((qe & 63) == 0)).any(1)
    val = np.maximum(_range_min(M, qb, qe), cum)
    tie = ev & (val == best[:, None])
    ties = tie.sum(1)
    tie_strips = np.array([len(np.unique(strip[i][tie[i]])) for i in range(len(k))])
    mixed = (strip_far[:, 1:] & strip_near[:, 1:]).any(1) if nstrips > 1 else np.zeros(len(k), dtype=bool)
    # per regular round: cells past the pair step
    reg = k != n - 1
    rounds = t[reg] // S["RL"]
    deep = np.bincount(rounds[needed[reg] > 32], minlength=S["nreg"])
    hot = 2 * deep > S["RL"]
    return dict(k=k, t=t, needed=needed, back=back, far=far, inside=inside, level=lev.max(1), level_ring=level_ring, level_mem=level_mem,
                on_border=on_border, ties=ties, tie_strips=tie_strips, mixed=mixed, hot=hot, nent=nent)


def hot_stretches(hot):
    """Lengths of the runs of consecutive hot rounds."""
    out, run = [], 0
    for h in list(hot) + [False]:
        if h:
            run += 1
        elif run:
            out.append(run)
            run = 0
    return out


# ---- the generators
class Lists:
    def __init__(self, m, n, L, X):
        self.m, self.n, self.L, self.X = m, n, L, X
        self.ent = np.zeros((n, stride_of(X), 2), dtype=np.uint32)
        self.hdr = np.zeros((n, 4), dtype=np.uint32)
        for k in range(n):
            self.put(k, [k + 1], [m])                          # (columns no cell reads keep this)

    def thr(self, k):
        return k + 2 - self.L

    def put(self, k, values, counts):
        ne = len(values)
        assert 1 <= ne <= self.ent.shape[1], (k, ne)
        self.ent[k] = 0
        self.ent[k, :ne, 0] = values
        self.ent[k, :ne, 1] = counts
        s = int(np.sum(counts))
        assert s <= self.m
        self.hdr[k] = (ne, counts[-1] if values[-1] == 0 else 0, 1 if s == self.m else 0, s)

    def level(self, k, V, s=0):
        thr = self.thr(k)
        s = max(0, min(s, thr - 1))
        self.put(k, [k + 1] + [thr - 1 - i for i in range(s)] + [0], [V] + [1] * s + [self.m - V - s])

    def carry(self, k, V):
        self.put(k, [k + 1, self.thr(k) - 1], [V, self.m - V])

    def probe(self, k, offsets, lump=1, double=None):
        """Single-count entries at thr - offsets (ascending offsets, all below thr), the rest at value 0; double: the entry behind
        the lump whose count is 2."""
        thr = self.thr(k)
        vs = [thr - o for o in offsets]
        assert vs and vs[-1] >= 1 and all(a > b for a, b in zip(vs, vs[1:])) and vs[0] < thr, (k, vs[:3], vs[-3:])
        cs = [2 if i == double else 1 for i in range(len(vs))]
        self.put(k, [k + 1] + vs + [0], [lump] + cs + [self.m - lump - sum(cs)])


def offsets(dense, j, jump):
    """Gaps of 1 up to entry j, of `jump` behind it: the offsets below thr of a probe's `dense` entries."""
    return [i if i <= j else j + (i - j) * jump for i in range(1, dense + 1)]


def random_lists(m, n, L, X, seed, full_at=()):
    """Any valid complete lists: a random number of distinct values below thr (near thr, far from it, down to 1), random counts, the
    rest of the rows at value 0 or, without a value 0, on the last entry.  full_at: columns whose list has `stride` entries."""
    rng = np.random.default_rng(seed)
    G = Lists(m, n, L, X)
    stride = stride_of(X)
    for k in cell_columns(n, L):
        thr = G.thr(k)
        room = min(thr - 1, stride - 2, m // 4)                 # values 1 .. thr - 1
        want = stride - 2 if k in full_at else int(min(room, rng.choice([0, 1, 2, 5, 20, 40, stride - 2], p=[.1, .2, .2, .2, .15, .1, .05])))
        want = max(0, min(want, room))
        near = min(want, int(rng.integers(0, want + 1)))
        offs = list(range(1, near + 1))
        if want > near:
            pool = np.arange(near + 1, thr)
            offs += sorted(rng.choice(pool, size=want - near, replace=False).tolist())
        vs = [thr - o for o in offs]
        cs = rng.integers(1, 4, size=len(vs)).tolist()
        lump = int(rng.integers(0, 6))
        rest = m - lump - sum(cs)
        assert rest >= 1
        if rng.random() < 0.8 or not vs or k in full_at:
            G.put(k, [k + 1] + vs + [0], [lump] + cs + [rest])
        else:
            cs[-1] += rest
            G.put(k, [k + 1] + vs, [lump] + cs)
    return G


def cut_lists(ent, hdr, X):
    """The lists as k_columns leaves them at capacity X (proto_length_scan.column_list): behind the lump an entry is taken while
    the counts in front of it (the lump's not among them) do not exceed X; complete iff nothing was left out."""
    n, m_sum = ent.shape[0], hdr[:, 3].astype(np.int64)
    out_e = np.zeros((n, stride_of(X), 2), dtype=np.uint32)
    out_h = hdr.copy()
    for k in range(n):
        ne = int(hdr[k, 0])
        cc = ent[k, 1:ne, 1].astype(np.int64)
        before = np.concatenate([[0], np.cumsum(cc)[:-1]]) if len(cc) else np.zeros(0, dtype=np.int64)
        nt = int((before <= X).sum())
        out_e[k, :1 + nt] = ent[k, :1 + nt]
        cum = int(ent[k, 0, 1]) + int(cc[:nt].sum())
        out_h[k] = (1 + nt, hdr[k, 1], 1 if (hdr[k, 2] and cum == m_sum[k]) else 0, cum)
    return out_e, out_h


def proving_capacity(m, n, L, ent, hdr, M):
    """The smallest capacity at which the cut lists prove every cell of the model."""
    lo, hi = 0, ent.shape[1]
    while lo < hi:
        mid = (lo + hi) // 2
        if len(unproven_cells(m, n, L, cut_lists(ent, hdr, mid)[1], M)):
            lo = mid + 1
        else:
            hi = mid
    return lo


# ---- the families
def _levels(G, V, s_seed=1, lo=None, hi=None):
    rng = np.random.default_rng(s_seed)
    for k in cell_columns(G.n, G.L):
        if (lo is None or k >= lo) and (hi is None or k < hi):
            s = int(rng.integers(0, 4))
            G.level(k, V, 0 if k < 2 * G.L + 2 else s)         # (part 2 takes m - cnt0 = V + s: s = 0 there keeps M at V exactly)


def strips_lists(m, n, L, X, V, every=37, first=None, full_last=False, double=None):
    """Level V columns with a probe of gaps 1 every `every`-th column: the probes' cells need V + 1 entries (V with a count of 2
    among them: double)."""
    G = Lists(m, n, L, X)
    _levels(G, V)
    dense = min(stride_of(X) - 2, V + 30)
    first = dense + L + 2 if first is None else first
    for k in range(first, n - L, every):
        G.probe(k, offsets(dense, dense, 1), double=double)
    if full_last:
        # lists of exactly `stride` entries: a probe among the regular cells and the final cell's
        G.probe(first + 1, offsets(stride_of(X) - 2, stride_of(X), 1))
        G.probe(n - 1, offsets(stride_of(X) - 2, stride_of(X), 1))
    return G


def far_lists(m, n, L, X, V, dense, j, jump, every, first, edge=()):
    """Level V columns and far-reading probes from column `first` on.  edge: (column, delta) pairs: a short probe there whose lowest
    query begins exactly delta entries above its round's safe_lo (delta < 0: below, the memory path)."""
    G = Lists(m, n, L, X)
    _levels(G, V)
    offs = offsets(dense, j, jump)
    for k in range(first, n - L, every):
        G.probe(k, offs)
    S = schedule(L, n)
    for k, delta in edge:
        safe_lo = view_of(S, k + 1 - L)[0]
        assert safe_lo > 0
        v_low = safe_lo + delta + L                              # its query begins at v_low - L
        near = list(range(1, 9))
        G.probe(k, near + [G.thr(k) - v_low], lump=V)            # (lump V: its cell stays at the level)
    return G


def level_lists(m, n, L, X, V, spans, seed=3):
    """Level columns whose V wanders (so that range minima and their first places matter) and probes with one entry whose range
    spans the given numbers of entries: spans = (column, gap in front of the wide range, width, align): align makes the range end
    on a block border."""
    G = Lists(m, n, L, X)
    rng = np.random.default_rng(seed)
    for k in cell_columns(n, L):
        G.level(k, V + int(rng.integers(0, 5)), int(rng.integers(0, 4)))
    for k, gap, width, align in spans:
        thr = G.thr(k)
        top = thr - gap                                        # the wide range is [top - width, top)
        if align:
            top -= (top - L) & 63
        offs = list(range(1, 6)) + [thr - top, thr - top + width]
        offs = sorted(set(offs))
        G.probe(k, offs + [offs[-1] + 1 + i for i in range(V + 8)])
    return G


def cool_lists(m, n, L, X, V, stretches, gap_rounds=24):
    """Level V columns (short lists) with stretches of rounds whose every column is a probe needing V + 1 > 32 entries."""
    G = Lists(m, n, L, X)
    _levels(G, V)
    S = schedule(L, n)
    dense = V + 8
    r = (dense + 2 * L) // S["RL"] + 4
    for ln in stretches:
        for t in range(r * S["RL"], (r + ln) * S["RL"]):
            G.probe(t + L - 1, offsets(dense, dense, 1))
        r += ln + gap_rounds
    assert (r + 1) * S["RL"] < n - 2 * L
    return G


def spec_lists(m, n, L, X, border_rounds, levels, seed=5):
    """Stretches of carry and level columns with another V each, their borders at and beside the chunk borders of chunks of
    border_rounds rounds, and a few probes: M steps up and down there, and a carried value crosses chunk after chunk."""
    G = Lists(m, n, L, X)
    S = schedule(L, n)
    rng = np.random.default_rng(seed)
    cells = n - 2 * L + 1
    step = border_rounds * S["RL"]
    t, i = 0, 0
    while t < cells:
        shift = (-1, 0, 1, 0)[i % 4]
        t_hi = min(cells, max(t + 1, ((t // step) + 1 + int(rng.integers(0, 3))) * step + shift))
        V = levels[i % len(levels)]
        kind = i % 3
        for tt in range(t, t_hi):
            k = tt + L - 1
            if kind == 0 or G.thr(k) < 2:
                G.level(k, V, int(rng.integers(0, 4)))
            elif kind == 1:
                G.carry(k, V)
            else:
                G.carry(k, V) if rng.random() < 0.7 else G.level(k, V + 2, 1)
        t, i = t_hi, i + 1
    G.level(n - 1, levels[0], 2)
    for k in range(max(2 * L, 200), n - L, 173):
        if G.thr(k) > 120:
            G.probe(k, offsets(40, 6, 3))
    return G


# ---- the table: name -> (m, n, L, X, builder of the full lists, cut capacity or None, cuts, plans, listed_for)
# listed_for: predicate name -> argument, checked on the model's measurements by asks() (tests/test_dp_list_cases.py); the
# parameters were searched on the CPU until each fired.  plans: forced plans of the speculative sweeps for the case,
# (FSEQ_DP_SPEC_ROUNDS, FSEQ_DP_SPEC_WIN, FSEQ_DP_SPEC_MAX_SWEEPS), 0 = the library's own.
CASES = {}


def _case(name, m, n, L, X, build, listed_for, cuts=None, cut_to=None, plans=()):
    CASES[name] = dict(m=m, n=n, L=L, X=X, build=build, listed_for=listed_for, cuts=cuts, cut_to=cut_to, plans=tuple(plans))


M0 = 600
# strips: a cell decides on the last lane of a strip, on the first lane of the next, and past three strips
for _need in (32, 33, 63, 64, 65, 127, 128, 129):
    _case("strips_%d" % _need, M0, 1500, 20, 261, functools.partial(strips_lists, M0, 1500, 20, 261, _need - 1),
          dict(needed=_need, ties_across=(2 if _need > 64 else 1)))
_case("strips_250", M0, 2000, 20, 261, functools.partial(strips_lists, M0, 2000, 20, 261, 249, full_last=True), dict(needed=250, full_lists=2, ties_across=4))
_case("strips_pipe_130", M0, 2400, 100, 261, functools.partial(strips_lists, M0, 2400, 100, 261, 129), dict(needed=130, ties_across=3))
# far reads, classic (L = 20) and pipelined (L = 100): the lowest query just inside and just outside safe_lo, a strip on both
# sides of it, cells past the pair step that read behind the ring
_EDGE = ((9000, 0), (9037, -1), (9100, 1), (9161, -64), (12000, 0), (12001, -1))
_case("far_classic", M0, 20000, 20, 261, functools.partial(far_lists, M0, 20000, 20, 261, 249, 255, 40, 32, 211, 9300, _EDGE),
      dict(needed=250, inside=(0, -1), deep_far=20, mixed=1, back=6000))
_case("far_pipe", M0, 20000, 100, 261, functools.partial(far_lists, M0, 20000, 100, 261, 249, 255, 40, 32, 211, 9300, _EDGE),
      dict(needed=250, inside=(0, -1), deep_far=20, mixed=1, back=6000))
_case("far_two_strips", M0, 14000, 20, 133, functools.partial(far_lists, M0, 14000, 20, 133, 70, 100, 30, 100, 97, 9000), dict(needed=71, deep_far=20, mixed=1))
_case("far_pair_step", M0, 14000, 57, 69, functools.partial(far_lists, M0, 14000, 57, 69, 25, 48, 4, 180, 61, 9500), dict(needed=26, pair_far=20, back=5000))
# high levels of the sparse table: ranges over >= 128 and >= 256 blocks, ending on a block border or not.  Level 7 from memory (a
# range that begins 190 blocks or more behind the cell) and from the ring; level 8 from the ring only: its samples leave the ring
# 320 blocks behind the cell, more than n <= 20,000 has -- what the ring holds of levels 7 and 8 was pushed through the mailbox
_SPANS = tuple((k, gap, width, align) for k, gap, width, align in
               [(9000, 3, 8300, 0), (12000, 3, 8400, 1), (15000, 5000, 8256, 0), (15001, 5000, 8300, 1), (18500, 7, 16600, 0), (19000, 9, 16500, 1),
                (19500, 1500, 17000, 1), (19800, 40, 12000, 0)])
_case("levels_classic", M0, 20000, 20, 69, functools.partial(level_lists, M0, 20000, 20, 69, 30, _SPANS), dict(level_ring=8, level_mem=7, level=8, on_border=2))
_case("levels_pipe", M0, 20000, 96, 69, functools.partial(level_lists, M0, 20000, 96, 69, 30, _SPANS), dict(level_ring=8, level_mem=7, level=8, on_border=2))
# pair_cool: stretches of rounds past the pair step between stretches of short lists
_case("cool_classic", M0, 9000, 20, 69, functools.partial(cool_lists, M0, 9000, 20, 69, 40, (5, 16, 17, 18, 40, 1)), dict(hot=(1, 5, 16, 17, 18, 40)))
_case("cool_pipe", M0, 16000, 100, 69, functools.partial(cool_lists, M0, 16000, 100, 69, 40, (5, 16, 17, 18, 1)), dict(hot=(1, 5, 16, 17, 18)))


# schedule edges on random valid lists: the switch of schedules (L = 95, 96, 97), RL = L and RL = 56, rounds that end on the last
# regular cell, one cell over, one cell short; a block that completes on a round's last cell (RL = 16: every fourth round)
def _edge_n(L, rem):
    S = schedule(L, 2 * L)
    return 2 * L - 1 + 7 * S["RL"] + rem                       # n - 2L + 1 = 7 RL + rem


for _L in (1, 2, 55, 56, 57, 95, 96, 97, 192):
    _RL = schedule(_L, 2 * _L)["RL"]
    for _n in sorted({2 * _L, 2 * _L + 1, _edge_n(_L, 0), _edge_n(_L, 1), _edge_n(_L, _RL - 1)}):
        if _n >= 2 * _L:
            _case("edge_L%d_n%d" % (_L, _n), 90, _n, _L, 21, functools.partial(random_lists, 90, _n, _L, 21, 1000 * _L + _n, (_n - 1,)),
                  dict(rounds_mod=(_n - 2 * _L + 1) % _RL))
_case("edge_block_on_round_end", 300, 3000, 16, 69, functools.partial(random_lists, 300, 3000, 16, 69, 77, (1200, 2999)), dict(block_on_round_end=1, full_lists=2))
_case("edge_random_long", 300, 6000, 33, 133, functools.partial(random_lists, 300, 6000, 33, 133, 78), dict(needed=5))

# resume: the far-reading families cut where the ring restore depends on the 64-blocks and the power-of-two block counts
_SC, _SP = schedule(21, 20000), schedule(100, 20000)
_case("resume_classic", M0, 20000, 21, 261, functools.partial(far_lists, M0, 20000, 21, 261, 249, 255, 40, 32, 211, 9300),
      dict(deep_far=20, cut_residues=(0, 1, 63), cut_blocks=(63, 64, 65, 127, 128, 129), cut_single=1, cut_final=1),
      cuts=cut_rounds(_SC, (0, 1, 63), (63, 64, 65, 127, 128, 129), (500, 501, 700, _SC["nreg"])))
_case("resume_pipe", M0, 20000, 100, 261, functools.partial(far_lists, M0, 20000, 100, 261, 249, 255, 40, 32, 211, 9300),
      dict(deep_far=20, cut_residues=(0, 16, 48), cut_blocks=(63, 64, 65, 127, 128, 129), cut_single=1, cut_drain=1, cut_final=1),
      cuts=cut_rounds(_SP, (0, 16, 48), (63, 64, 65, 127, 128, 129), (300, 301, _SP["nreg"], _SP["nreg"] + 1)))
_case("resume_levels", M0, 20000, 20, 69, functools.partial(level_lists, M0, 20000, 20, 69, 30, _SPANS),
      dict(level_mem=7, level_ring=8, cut_blocks=(127, 128, 129, 255, 256, 257)), cuts=cut_rounds(schedule(20, 20000), (), (127, 128, 129, 255, 256, 257), (1,)))

# speculative: M steps at and beside the chunk borders of chunks of 1, 3, 7 and 40 rounds and of the library's own plan; tail
# windows of 1 and 5,000; sweep budgets of 1 and 2 (the serial take-over behind the first dirty chunk, a resumed launch)
_PLANS = ((1, 0, 0), (3, 0, 0), (7, 0, 0), (40, 0, 0), (7, 1, 0), (7, 5000, 0), (7, 0, 1), (7, 0, 2), (0, 0, 1), (0, 0, 2), (0, 1, 0))
_case("spec_classic", M0, 6000, 20, 69, functools.partial(spec_lists, M0, 6000, 20, 69, 7, (30, 50, 20, 64, 35)), dict(steps=8, carried=1), plans=_PLANS)
_case("spec_own_plan", M0, 20000, 20, 69, functools.partial(spec_lists, M0, 20000, 20, 69, 20, (30, 50, 20, 64, 35)), dict(steps=8, carried=1),
      plans=((0, 0, 1), (0, 0, 2), (0, 5000, 0), (40, 0, 0)))
_case("spec_pipe", M0, 12000, 100, 69, functools.partial(spec_lists, M0, 12000, 100, 69, 3, (30, 50, 20, 64, 35)), dict(steps=8, carried=1),
      plans=((1, 0, 0), (3, 0, 0), (7, 0, 0), (40, 0, 0), (3, 0, 1), (3, 0, 2), (3, 1, 0)))

# cut lists, in pairs: at the smallest capacity that proves every cell (the arrays are compared) and one below it (unproven and
# nothing else); the deciding entry at 31 / 32, 62 / 63, 63 / 64, 126 / 127.  cut_65_unproven is the case that found dp_strip
# counting the 64th entry of a list of exactly 64 entries twice: its cells then passed the bound and went unflagged
for _need in (32, 33, 63, 64, 65, 127, 128):
    for _below in (0, 1):
        _case("cut_%d_%s" % (_need, "unproven" if _below else "proven"), M0, 1500, 20, 261, functools.partial(strips_lists, M0, 1500, 20, 261, _need - 1),
              dict(deciding=_need - 1, unproven=_below), cut_to=-_below)


# the same at the default capacity: a count of 2 ends the list cut to capacity 63 on its 64th entry
for _below in (0, 1):
    _case("cut_counts2_%s" % ("unproven" if _below else "proven"), M0, 1500, 20, 261, functools.partial(strips_lists, M0, 1500, 20, 261, 65, double=5),
          dict(deciding=64, unproven=_below, cut_capacity=64 - _below, cut_entries=65 - _below), cut_to=-_below)


def _cnt0_lists():
    """Complete lists with cnt0 > 0 whose cells take w = m - cnt0, among level 40 columns: w equal to the best candidate (the
    reference visits w first and keeps it) and w below every candidate."""
    G = Lists(M0, 1500, 20, 21)
    _levels(G, 40)
    for k in range(100, 1480, 9):                                                       # (9: no such cell reads another's entry)
        thr = G.thr(k)
        G.put(k, [k + 1, thr - 1, 0], [10, 30, M0 - 40])                                # w = 40 = max(M, 10) of the one candidate
        G.put(k + 1, [k + 2, thr, thr - 1, 0], [10, 20, 1, M0 - 31])                    # w = 31 below every candidate
    return G


_case("cnt0_takes_w", M0, 1500, 20, 21, _cnt0_lists, dict(takes_w=100))


@functools.lru_cache(maxsize=None)
def full_lists(name):
    c = CASES[name]
    G = c["build"]()
    return G.ent, G.hdr


@functools.lru_cache(maxsize=None)
def reference(name, debug=True):
    """(LB, M, SZ) of the model on the case's uncut lists, under the oracle's debug build: its asserts certify the lists."""
    c = CASES[name]
    ent, hdr = full_lists(name)
    return model(c["m"], c["n"], c["L"], ent, hdr, debug=debug)


@functools.lru_cache(maxsize=None)
def device_lists(name):
    """(X, ent, hdr) as the device gets them: the case's lists, cut where the case says so (cut_to = 0: the smallest capacity that
    proves every cell, -1: one below it)."""
    c = CASES[name]
    ent, hdr = full_lists(name)
    if c["cut_to"] is None:
        return c["X"], ent, hdr
    X = proving_capacity(c["m"], c["n"], c["L"], ent, hdr, reference(name)[1]) + c["cut_to"]
    return (X,) + cut_lists(ent, hdr, X)


def expect_unproven(name):
    c = CASES[name]
    _, _, hdr = device_lists(name)
    return int(len(unproven_cells(c["m"], c["n"], c["L"], hdr, reference(name)[1])) > 0)


@functools.lru_cache(maxsize=None)
def measurements(name):
    c = CASES[name]
    _, ent, hdr = device_lists(name)
    return measure(c["m"], c["n"], c["L"], ent, hdr, reference(name)[1])


def asks(name):
    """{predicate: (holds, figure)} for what the case is listed for."""
    c = CASES[name]
    S = schedule(c["L"], c["n"])
    Q = measurements(name)
    LB, M, SZ = reference(name)
    out = {}
    for key, arg in c["listed_for"].items():
        if key == "needed":
            fig = int(Q["needed"].max())
            ok = fig == arg if arg >= 32 else fig >= arg
        elif key == "ties_across":
            fig = int(Q["tie_strips"][Q["ties"] >= 2].max(initial=0))
            ok = fig >= arg
        elif key == "full_lists":
            fig = int((Q["nent"] == stride_of(c["X"])).sum())
            ok = fig >= arg and bool(Q["nent"][Q["k"] == c["n"] - 1][0] == stride_of(c["X"]))
        elif key == "inside":
            fig = sorted(set(int(x) for x in Q["inside"] if -2 <= x <= 2))
            ok = all(a in fig for a in arg)
        elif key == "deep_far":
            fig = int((Q["far"] & (Q["needed"] > 32)).sum())
            ok = fig >= arg
        elif key == "pair_far":
            fig = int((Q["far"] & (Q["needed"] <= 32) & (Q["needed"] >= 20)).sum())
            ok = fig >= arg
        elif key == "mixed":
            fig = int(Q["mixed"].sum())
            ok = fig >= arg
        elif key == "back":
            fig = int(Q["back"].max())
            ok = fig >= arg
        elif key in ("level", "level_ring", "level_mem"):
            fig = int(Q[key].max())
            ok = fig >= arg
        elif key == "on_border":
            fig = int((Q["on_border"] & (Q["level"] >= 7)).sum())
            ok = fig >= arg
        elif key == "hot":
            fig = sorted(set(hot_stretches(Q["hot"])))
            ok = all(a in fig for a in arg)
        elif key == "rounds_mod":
            fig = (c["n"] - 2 * c["L"] + 1) % S["RL"]
            ok = fig == arg
        elif key == "block_on_round_end":
            fig = sum(1 for r in range(S["nreg"] - 1) if ((r + 1) * S["RL"]) % 64 == 0)
            ok = fig >= arg
        elif key == "cut_residues":
            fig = sorted(set(round_t0(S, r) % 64 for r in c["cuts"] if r < S["nreg"]))
            ok = all(a in fig for a in arg)
        elif key == "cut_blocks":
            fig = sorted(set(round_t0(S, r) // 64 for r in c["cuts"] if r < S["nreg"]))
            ok = all(a in fig for a in arg)
        elif key == "cut_single":
            fig = sum(1 for a, b in zip(c["cuts"], c["cuts"][1:]) if b == a + 1 and b < S["nreg"])
            ok = fig >= arg
        elif key == "cut_drain":
            fig = int(S["pipe"] and S["nreg"] in c["cuts"])
            ok = fig == arg
        elif key == "cut_final":
            fig = int(S["nrounds"] - 1 in c["cuts"])
            ok = fig == arg
        elif key == "steps":
            w = M[:c["n"] - 2 * c["L"] + 1].astype(np.int64)
            step_at = np.nonzero(np.abs(np.diff(w)) >= 5)[0] + 1
            fig = int(len(step_at))
            ok = fig >= arg and bool((np.diff(w) >= 5).any()) and bool((np.diff(w) <= -5).any())
        elif key == "carried":
            # a cell whose value is neither its list's lump nor w: it came from in front of it, more than L entries back
            fig = int((LB[Q["t"]] > 0).sum())
            ok = fig >= arg
        elif key == "deciding":
            # (on the uncut lists: the entry whose cumulative count passes the value of the cell that needs the most)
            ent, hdr = full_lists(name)
            fig = int(measure(c["m"], c["n"], c["L"], ent, hdr, M)["needed"].max()) - 1
            ok = fig == arg
        elif key == "unproven":
            fig = expect_unproven(name)
            ok = fig == arg
        elif key == "cut_capacity":
            fig = device_lists(name)[0]
            ok = fig == arg
        elif key == "cut_entries":
            fig = int(Q["nent"].max())
            ok = fig == arg
        elif key == "takes_w":
            k = Q["k"]
            _, ent, hdr = device_lists(name)
            fig = int(((LB[Q["t"]] == 0) & (hdr[k, 1] > 0) & (M[Q["t"]] == c["m"] - hdr[k, 1]) & (hdr[k, 0] > 2)).sum())
            ok = fig >= arg
        else:
            raise KeyError(key)
        out[key] = (bool(ok), fig)
    return out


def compared_by_arrays(name):
    return not CASES[name]["listed_for"].get("unproven")
