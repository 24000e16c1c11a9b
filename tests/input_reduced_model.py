"""Inputs and the numpy side of the chunked input that drops the identity columns on the way (include/fseq.h,
fseq_input_scan_identity .. fseq_input_end_kept): alignments with identity columns planted where the tests want them, the range
of a kept list inside a chunk as numpy states it, and the two ways to the reduced context that the GPU tests compare -- the
existing chain (set_sequences in chunks, then without_identity_columns) and the new entries.  The models of the two halves
are tests/identity_model.py and tests/input_model.py."""
import numpy as np

import identity_model as im


def pad16(x):
    return (x + 15) // 16 * 16


def staging_for(m, width):
    """two halves that hold exactly pad16(width) columns of m rows"""
    return 2 * m * pad16(width)


def kept_range(kept, c0, ncols):
    """(k0, k1): the entries of the ascending list kept with c0 <= kept[k] < c0 + ncols"""
    kept = np.asarray(kept, dtype=np.uint64)
    return int(np.searchsorted(kept, np.uint64(c0), side="left")), int(np.searchsorted(kept, np.uint64(c0 + ncols), side="left"))


def planted(seed, m, n, alphabet, identity, differ_rows=None):
    """A mosaic over `alphabet` (every byte of it occurs) in which exactly the columns of `identity` (a boolean mask, or a share
    in [0, 1]) are identity columns: they carry row 0's byte, and every other column differs from row 0 in at least one row (m > 1)
    -- in row differ_rows[k] alone where that dictionary names column k."""
    rng = np.random.default_rng(seed)
    alpha = np.frombuffer(bytes(alphabet), dtype=np.uint8)
    assert list(alpha) == sorted(set(alpha.tolist()))
    # input_model.mosaic's rows (blocks of 40 columns copied from 3 founders, one cell in a hundred changed); the alphabet is planted below
    F = alpha[rng.integers(0, len(alpha), size=(3, n))]
    msa = np.empty((m, n), dtype=np.uint8)
    for b0 in range(0, n, 40):
        msa[:, b0:b0 + 40] = F[rng.integers(0, 3, size=m), b0:b0 + 40]
    hit = rng.random((m, n)) < 0.01
    msa[hit] = alpha[rng.integers(0, len(alpha), size=int(hit.sum()))]
    ident = (rng.random(n) < identity) if np.isscalar(identity) else np.asarray(identity, dtype=bool).copy()
    if m == 1 or len(alpha) == 1:
        ident[:] = True
    msa[:, ident] = msa[0:1, ident]
    for k in np.nonzero(~ident)[0]:
        if differ_rows and int(k) in differ_rows:
            msa[:, k] = msa[0, k]
            r = differ_rows[int(k)]
            if r == 0:                                          # row 0 alone differs: every other row carries another byte
                msa[1:, k] = alpha[(np.searchsorted(alpha, msa[0, k]) + 1) % len(alpha)]
            else:
                msa[r, k] = alpha[(np.searchsorted(alpha, msa[0, k]) + 1) % len(alpha)]
        elif (msa[:, k] == msa[0, k]).all():
            msa[int(rng.integers(1, m)), k] = alpha[(np.searchsorted(alpha, msa[0, k]) + 1) % len(alpha)]
    # the identity columns took planted bytes with them: every byte of the alphabet occurs again, in identity columns where possible
    have = set(np.unique(msa).tolist())
    missing = [b for b in alpha if int(b) not in have]
    spots = np.nonzero(ident)[0]
    free = [int(k) for k in np.nonzero(~ident)[0] if not (differ_rows and int(k) in differ_rows)]
    assert len(missing) <= len(spots) + len(free), "no room to plant the alphabet"
    for i, b in enumerate(missing):
        if i < len(spots):
            msa[:, spots[i * (len(spots) // len(missing)) if len(missing) <= len(spots) else i]] = b
        else:
            msa[m - 1, free[i - len(spots)]] = b                # (a byte that occurs nowhere else: the column still differs from row 0)
    assert np.array_equal(im.identity_mask(msa), ident)
    return np.ascontiguousarray(msa)


def chain(pkg, msa, L, width, **kw):
    """the yardstick: the rows through the existing chunked input, then without_identity_columns.  Returns the new context."""
    m, n = msa.shape
    src = pkg.SegmentationContext(m, n, L)
    src.set_sequences(msa, staging_bytes=staging_for(m, width))
    new = src.without_identity_columns(L, **kw)
    src.close()
    return new


def feed(src, msa, width, L, alphabet=None, skip=True, **kw):
    """the new entries, chunk by chunk; a chunk without a kept column goes without rows when skip.  Returns the new context."""
    m, n = msa.shape
    src.input_begin(alphabet=alphabet, staging_bytes=staging_for(m, width))
    for c0 in range(0, n, width):
        src.input_scan_identity(c0, msa[:, c0:c0 + width])
    sm = src.input_reduce(L, **kw)
    assert sm["n"] == n and sm["identity"] + sm["kept"] == n
    skipped = 0
    for c0 in range(0, n, width):
        w = min(width, n - c0)
        if skip and src.input_kept_columns(c0, w) == 0:
            src.input_columns_kept(c0, w)
            skipped += 1
        else:
            src.input_columns_kept(c0, msa[:, c0:c0 + w])
    new = src.input_end_kept()
    new.skipped_chunks = skipped
    return new
