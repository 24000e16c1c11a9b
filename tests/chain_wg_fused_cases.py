"""A second table for phase B's chain-per-workgroup kernel (k_chain_wg, csrc/fseq_chainsort.hpp): what the sweeps in front of a run step
can get wrong where runs and the chunks of the waves meet, and tests/chain_wg_cases.py does not pin.  A sweep gives every wave a chunk
of whole 64-groups (chain_wg_cases.chunk); a wave numbers the runs that START in its chunk behind the runs of the chunks before; what
lies in front of its first start is the tail of a run of a chunk before (a carry-in: its maximum of d0 belongs to another wave's
run), and a run still open at the chunk's end goes on in the chunks behind.  However the sweeps are arranged -- one for the keys and
one for the runs' maxima, or one for both -- these are the places.  So the table holds, each on one step from a constructed state (an
expansion of one chain of one block, the last of all):
  * runs that span whole chunks, so that a wave's chunk holds no start at all and everything it sees is carry-in;
  * a start exactly at a chunk's first position, and one exactly at its last;
  * so few rows that waves have empty chunks (m = 700: waves 11 .. 15; m = 65: waves 2 .. 15, wave 1 one position);
  * spikes of d0 at the last position of a chunk and at the first of the next, inside one run, so that a lost carry-in or a lost open
    run changes the divergence of the head behind that run;
  * as many runs as the cap and one more, the cap's last run across a chunk border.
tests/test_chain_wg_fused_cases.py proves each on the inputs alone; tests/test_gpu_chain_wg_fused.py runs them through the kernel.
The model is tests/chain_step_cases.py's.  No GPU and no library in here.  TEST INFRASTRUCTURE."""
import numpy as np

import chain_step_cases as cs
import chain_wg_cases as cw

SPIKE = 1 << 24             # above every other divergence of a case (chain_step_cases.D_LIMIT is 2^25)


def keys_from_cuts(cuts, m, D):
    """By position: run j from cuts[j] up to cuts[j + 1] (m behind the last), of key j mod D."""
    cuts = np.asarray(cuts, dtype=np.int64)
    assert cuts[0] == 0 and np.all(np.diff(cuts) > 0) and cuts[-1] < m and (D >= 2 or len(cuts) == 1)
    return np.repeat(np.arange(len(cuts)) % D, np.diff(np.r_[cuts, m])).astype(np.int64), min(D, len(cuts))


def border_cuts(m, off=40):
    """Runs that cross every chunk border by `off` positions on either side, and the runs between them."""
    ch = cw.chunk(m)
    borders = np.arange(ch, m - off, ch)
    return np.r_[0, np.sort(np.r_[borders - off, borders + off])], borders


def fused_keys(spec, m, rng):
    """(keys by position, nkeys).  ("span", D): runs of 3 chunks + 5 positions; ("edges", D): a start at every chunk's first position
    and one at its last; ("borders", D): border_cuts; ("cap", R, D): exactly R runs, run 99 from 50 positions in front of the
    border of chunks 9 and 10 up to the next start (five positions behind the border of chunks 12 and 13, or m);
    else chain_wg_cases.keys_by_position's."""
    ch = cw.chunk(m)
    if spec[0] == "span":
        return keys_from_cuts(np.arange(0, m, 3 * ch + 5), m, spec[1])
    if spec[0] == "edges":
        firsts = np.arange(0, m, ch)
        lasts = firsts + ch - 1
        return keys_from_cuts(np.sort(np.r_[firsts, lasts[lasts < m]]), m, spec[1])
    if spec[0] == "borders":
        return keys_from_cuts(border_cuts(m)[0], m, spec[1])
    if spec[0] == "cap":
        R = spec[1]
        assert R in (100, 101) and 13 * ch + 5 < m
        cuts = np.r_[0, np.sort(rng.choice(np.arange(1, 8 * ch), size=98, replace=False)), 10 * ch - 50]
        if R == 101:
            cuts = np.r_[cuts, 13 * ch + 5]
        return keys_from_cuts(cuts, m, spec[2])
    return cw.keys_by_position(spec, m, rng)


def fused_d0(kind, m, rng):
    """"border-spikes": small random divergences, and inside the run across chunk border c a spike at the chunk's last position
    (c = 1 mod 3), at the next chunk's first (c = 2 mod 3) or at both, the second the higher (c = 0 mod 3)."""
    if kind != "border-spikes":
        return cs.make_d0(kind, m, rng)
    d = rng.integers(0, 1000, size=m).astype(np.int64)
    for c, b in enumerate(border_cuts(m)[1].tolist(), start=1):
        if c % 3 != 2:
            d[b - 1] = SPIKE + 2 * c
        if c % 3 != 1:
            d[b] = SPIKE + 2 * c + 1
    return d


def _f(name, m, spec, path, run_cap=cw.CW_RUN_CAP, runs=None, start="random"):
    return dict(name=name, m=m, blocks=(spec,), G=1, first=0, chains=1, own_start=True, states=True, keys=False, run_cap=run_cap, workgroups=1,
                paths=(path,), runs=runs, start=start)


def _table():
    T = []
    for m in (11265, 12288):
        ch = cw.chunk(m)
        T.append(_f("span", m, ("span", 3), "runs", runs=[-(-m // (3 * ch + 5))], start="spikes"))
        T.append(_f("edges", m, ("edges", 3), "runs", start="spikes"))
        T.append(_f("carry-spikes", m, ("borders", 2), "runs", start="border-spikes"))
    for m in (700, 65):
        T.append(_f("small-runs", m, ("runs", min(m // 3, 40), 3), "runs", start="spikes"))
        T.append(_f("small-one", m, ("one",), "runs", runs=[1]))
        T.append(_f("small-heads", m, ("perm",), "runs", runs=[m]))
        T.append(_f("small-sort", m, ("random", 5), "sort", run_cap=0))
    m = 12288
    T.append(_f("cap-crossing", m, ("cap", 100, 7), "runs", run_cap=100, runs=[100], start="spikes"))
    T.append(_f("cap+1-crossing", m, ("cap", 101, 7), "sort", run_cap=100, runs=[101], start="spikes"))
    for i, c in enumerate(T):
        c["seed"] = 9500 + i
        c["id"] = "%d-%s" % (c["m"], c["name"])
    return T


FUSED_CASES = _table()
SMALL_M = (700, 65)         # below the streamed regime's 11,265 rows: only the debug entry that hands keys over takes them


def build_fused(case):
    """chain_wg_cases.build_wg's dict for a case of this table (one block, a constructed state in front of it)."""
    rng = np.random.default_rng(case["seed"])
    m = case["m"]
    a0, d0 = cs.make_perm("random", m, rng), fused_d0(case["start"], m, rng)
    kp, nk = fused_keys(case["blocks"][0], m, rng)
    rank = cs.key_by_row(a0, kp)[None, :]
    keyd = rng.integers(0, cs.COLS + 1, size=(1, m))
    return dict(m=m, rank=rank, keyd=keyd, nkeys=np.array([nk], dtype=np.int64), a=a0, d=d0, kp=kp)
