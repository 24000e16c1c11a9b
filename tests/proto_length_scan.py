"""The model of the scan over segment lengths (fseq_scan_segment_lengths, k_relump_lists): the list of a column in the
kernel's format, built from the oracle's divergence-value counts at a capacity X and a segment length L, the folding of such a
list to a larger length, and the DP's "unproven" predicate on a folded list.  Plain numpy over oracle/fso.py; no device.

The list of column k (csrc/fseq_kernels.hpp, "emit the top of the histogram"): entry 0 is the lump {k + 1, count of the values
>= thr = max(0, k + 2 - L)}; behind it the distinct values below thr, descending, each taken while the counts of the values below
thr in front of it do not exceed X.  The header is {entries, count of value 0, complete, cumulative count}."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import fso  # noqa: E402
from helpers import founder_mosaic  # noqa: E402

UNCUT = 1 << 30


def mosaic(founders, m, n, seed, mu=0.0, brec=100, alphabet=b"ACGT"):
    """helpers.founder_mosaic with every cell replaced by a random symbol with probability mu."""
    msa = founder_mosaic(founders, m, n, brec=brec, seed=seed, alphabet=alphabet)
    if mu > 0:
        rng = np.random.default_rng(seed + 7919)
        hit = rng.random(msa.shape) < mu
        alpha = np.frombuffer(alphabet, dtype=np.uint8)
        msa[hit] = alpha[rng.integers(0, len(alpha), size=int(hit.sum()))]
    return np.ascontiguousarray(msa)


def column_counts(msa):
    """[(values ascending, counts)] of every column, from the oracle's pBWT."""
    p = fso.Pbwt(msa, debug=False)
    out = []
    for _ in range(msa.shape[1]):
        p.step()
        out.append(p.counts())
    return out


def column_list(v, c, k, L, X, stride=None):
    """The list of column k at segment length L and capacity X: (ent [stride][2], hdr [4]).  stride None: as long as the list."""
    m = int(c.sum())
    thr = max(0, k + 2 - L)
    rec = v >= thr
    R = int(c[rec].sum())
    cv, cc = v[~rec][::-1], c[~rec][::-1]
    before = np.concatenate([[0], np.cumsum(cc)[:-1]]) if len(cc) else np.zeros(0, dtype=np.int64)
    nt = int((before <= X).sum())
    cum = R + int(cc[:nt].sum())
    nent = 1 + nt
    ent = np.zeros((nent if stride is None else stride, 2), dtype=np.uint32)
    assert nent <= len(ent)
    ent[0] = (k + 1, R)
    ent[1:nent, 0], ent[1:nent, 1] = cv[:nt], cc[:nt]
    cnt0 = int(c[0]) if len(v) and v[0] == 0 else 0
    return ent, np.array([nent, cnt0, 1 if cum == m else 0, cum], dtype=np.uint32)


def relump(ent, hdr, k, L_to):
    """k_relump_lists on one column: the leading entries from index 1 on whose value is >= max(0, k + 2 - L_to) join the lump,
    the rest moves down, the entry count falls; the words behind the new end and the other header words stay."""
    ent, hdr = ent.copy(), hdr.copy()
    nent = int(hdr[0])
    thr = max(0, k + 2 - L_to)
    E = 0
    while 1 + E < nent and ent[1 + E, 0] >= thr:
        E += 1
    if E == 0:
        return ent, hdr
    ent[0, 1] += ent[1:1 + E, 1].sum(dtype=np.uint32)
    ent[1:nent - E] = ent[1 + E:nent].copy()
    hdr[0] = nent - E
    return ent, hdr


def ascending(ent, hdr):
    """A list as the oracle's dp_step takes it: values and counts ascending, the lump last."""
    nent = int(hdr[0])
    return ent[:nent, 0][::-1].copy(), ent[:nent, 1][::-1].copy()


def unproven(hdr, best):
    """The DP's verdict on a list (dp_cell_sequential): it ends incomplete before the cumulative count passes the cell's best
    value."""
    return not hdr[2] and int(hdr[3]) <= int(best)


def cell_columns(n, L):
    """The columns whose lists the DP's cells at segment length L read: column end - 1 of every cell end in [L, n - L] and n."""
    return list(range(L - 1, n - L)) + [n - 1]


def folded_unproven(counts, dp, n, L_from, L, X):
    """Columns whose list, built at (L_from, X) and folded to L, does not prove its cell (dp: the oracle's DP entries at L)."""
    bad = []
    for k in cell_columns(n, L):
        v, c = counts[k]
        ent, hdr = relump(*column_list(v, c, k, L_from, X), k, L)
        if unproven(hdr, dp["segment_max_size"][k + 1 - L]):
            bad.append(k)
    return bad


# The cases of tests/test_gpu_length_scan.py whose list capacity is fixed, with what each is listed for: `overflow`: some length
# behind the first is not proven by the lists folded from the length before it (the model's predicate; the parameters were
# searched on the CPU until it fired), else no folded list of the case is unproven.
CASES = {
    "lds_resident": dict(founders=6, m=60, n=3000, seed=11, mu=0.0, alphabet=b"ACGT", list_cap=63,
                         lengths=[5, 6, 7, 10, 20, 55, 56, 57, 95, 96, 97, 200, 1499, 1500, 1501, 4000], overflow=False),
    "overflow": dict(founders=24, m=150, n=3000, seed=5, mu=0.02, alphabet=b"ACGT", list_cap=3,
                     lengths=[8, 12, 16, 24, 40, 80, 150], overflow=True),
    "bits4": dict(founders=8, m=200, n=2400, seed=21, mu=0.002, alphabet=b"ACGTRYSWKMBDHVN-", list_cap=255,
                  lengths=[10, 30, 90, 300], overflow=False),
    "bits8": dict(founders=8, m=200, n=2400, seed=22, mu=0.002, alphabet=bytes(range(48, 48 + 40)), list_cap=255,
                  lengths=[10, 30, 90, 300], overflow=False),
}


def case_msa(name):
    c = CASES[name]
    return mosaic(c["founders"], c["m"], c["n"], c["seed"], mu=c["mu"], alphabet=c["alphabet"])


def simulate_scan(msa, lengths, X0):
    """The scan's order of work in the model: the lists built at the first long-path length (the capacity doubled until every
    cell is proven), folded to every further length, built again where a folded list leaves a cell unproven.  Returns
    [(L, built, X)] for the distinct long-path lengths ascending, and the retries."""
    m, n = msa.shape
    counts = column_counts(msa)
    out, retries = [], 0
    X, base = min(X0, m), None
    for L in sorted({int(x) for x in lengths if n >= 2 * int(x)}):
        dp = fso.segment_long(msa, L, keep_dp=True, threads=4)["dp"]
        built = base is None or bool(folded_unproven(counts, dp, n, base, L, X))
        if built:
            while folded_unproven(counts, dp, n, L, L, X):
                assert X < m
                X = min(m, 2 * X + 1)
                retries += 1
            base = L
        out.append((L, built, X))
    return out, retries
