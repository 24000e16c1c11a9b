"""The specification of the identity-column filters in numpy: what remove_identity_columns and insert_identity_columns
(founder-sequences_amd/host, the yardstick) do to an alignment, and the inputs the tests of the device path share.
tests/test_identity_abi.py pins this model to the two built host tools; tests/test_gpu_identity.py compares the device
path against it, integer for integer."""
import numpy as np

ALPHABETS = {2: b"AC", 4: b"ACGT", 16: b"ACGTRYSWKMBDHVN-", 40: bytes(range(48, 88))}


def identity_mask(msa):
    """mask[k] = every row equals row 0 in column k (m == 1: every column)."""
    return (msa == msa[0:1]).all(axis=0)


def reduce_rows(msa, mask):
    return np.ascontiguousarray(msa[:, ~mask])


def restore(founders, mask, row0):
    """insert_identity_columns with --reference = row 0: founders (K x kept) -> K x n."""
    out = np.repeat(np.asarray(row0, dtype=np.uint8)[None, :], founders.shape[0], axis=0)
    out[:, ~mask] = founders
    return out


def mask_text(mask):
    """The stdout of remove_identity_columns."""
    return (np.where(mask, ord("1"), ord("0")).astype(np.uint8).tobytes() + b"\n")


def lines_of(path):
    """A founders file (lines of equal length) as a K x n byte matrix."""
    data = open(path, "rb").read()
    n = data.index(b"\n")
    a = np.frombuffer(data, dtype=np.uint8).reshape(-1, n + 1)
    assert (a[:, n] == 10).all()
    return a[:, :n].copy()


def random_case(seed, m, n, sigma, identity_share=0.6, codes=False):
    """m x n symbols of the sigma-letter alphabet (or dense codes) of which about identity_share of the columns are
    identity columns and every other column has at least one row (m > 1) that differs from row 0."""
    rng = np.random.default_rng(seed)
    msa = rng.integers(0, sigma, size=(m, n), dtype=np.uint8)
    ident = rng.random(n) < identity_share
    msa[:, ident] = msa[0:1, ident]
    if m > 1:
        rows = rng.integers(1, m, size=n)
        cols = np.nonzero(~ident)[0]
        msa[rows[cols], cols] = (msa[0, cols] + 1 + rng.integers(0, sigma - 1, size=len(cols))) % sigma
    if not codes:
        msa = np.frombuffer(ALPHABETS[sigma], dtype=np.uint8)[msa]
    return np.ascontiguousarray(msa)


def needle_case(m, n, sigma, rows_at, seed=0, codes=False):
    """Every column an identity column except that in column k of rows_at = {k: r} exactly row r differs from the others."""
    rng = np.random.default_rng(seed)
    base = rng.integers(0, sigma, size=n, dtype=np.uint8)
    msa = np.repeat(base[None, :], m, axis=0)
    for k, r in rows_at.items():
        msa[r, k] = (msa[r, k] + 1 + (k % (sigma - 1))) % sigma
    if not codes:
        msa = np.frombuffer(ALPHABETS[sigma], dtype=np.uint8)[msa]
    return np.ascontiguousarray(msa)


def mosaic_with_identity(seed, m, n, L, founders=6, identity_share=0.6, extra_symbol=ord("N")):
    """A founder mosaic over ACGT with mutations, about identity_share of its columns overwritten with row 0's symbol, and
    one symbol (extra_symbol) that occurs in identity columns only: the kept alphabet is smaller than the code table."""
    rng = np.random.default_rng(seed)
    alpha = np.frombuffer(b"ACGT", dtype=np.uint8)
    F = alpha[rng.integers(0, 4, size=(founders, n))]
    blocks = (n + L - 1) // L
    pick = rng.integers(0, founders, size=(m, blocks))
    msa = np.empty((m, n), dtype=np.uint8)
    for b in range(blocks):
        msa[:, b * L:(b + 1) * L] = F[pick[:, b], b * L:(b + 1) * L]
    mut = rng.random((m, n)) < 0.002
    msa[mut] = alpha[rng.integers(0, 4, size=int(mut.sum()))]
    ident = rng.random(n) < identity_share
    msa[:, ident] = msa[0:1, ident]
    cols = np.nonzero(ident)[0]
    msa[:, cols[::7]] = extra_symbol
    return np.ascontiguousarray(msa)
