"""What the chunked input path (include/fseq.h, fseq_input_begin .. fseq_input_end) must leave on the device, restated in
numpy: the code table of consecutive_alphabet_as_builder (generate_context.cc:135-147: dense codes in ascending byte order) with
an optionally supplied alphabet, whose unused bytes keep their codes, and the packed column bytes with zeroed padding, through
the package's own pack_columns."""
import numpy as np


def code_table(msa, alphabet=None):
    """(table, sigma, bits): table[b] = code of byte b, -1 where b is not in the alphabet; bits per code as alloc_msa chooses."""
    present = np.zeros(256, dtype=bool)
    if alphabet is None:
        present[np.unique(msa)] = True
    else:
        alpha = np.frombuffer(bytes(alphabet), dtype=np.uint8)
        assert len(set(alpha.tolist())) == len(alpha)
        present[alpha] = True
    table = np.full(256, -1, dtype=np.int32)
    table[present] = np.arange(int(present.sum()))
    sigma = int(present.sum())
    return table, sigma, (2 if sigma <= 4 else 4 if sigma <= 16 else 8)


def outside(msa, alphabet):
    """the byte values of msa a supplied alphabet does not list (ascending)"""
    table, _, _ = code_table(msa, alphabet)
    return [int(b) for b in np.unique(msa) if table[b] < 0]


def packed_columns(pkg, msa, alphabet=None):
    """(bytes [n, ld], bits): every column as it is stored, padding bytes and padding fields zero."""
    table, _, bits = code_table(msa, alphabet)
    codes = table[msa]
    assert (codes >= 0).all()
    out, _ = pkg.pack_columns(codes.astype(np.uint8), bits)
    return out, bits


def alphabet_bytes(size, seed):
    """`size` distinct byte values, ascending, with values above 127 among them whenever size > 1"""
    rng = np.random.default_rng(1000 + seed)
    if size == 256:
        return bytes(range(256))
    low = rng.choice(128, size=(size + 1) // 2, replace=False)
    high = 128 + rng.choice(128, size=size // 2, replace=False)
    return bytes(sorted(int(x) for x in np.concatenate([low, high])))


def mosaic(seed, m, n, alphabet, founders=3, brec=40, flip=0.01):
    """Rows copied block by block from a few founders over `alphabet` with a few cells changed; every byte of the alphabet
    occurs (planted along the first rows where the draw missed it)."""
    rng = np.random.default_rng(seed)
    alpha = np.frombuffer(bytes(alphabet), dtype=np.uint8)
    F = alpha[rng.integers(0, len(alpha), size=(founders, n))]
    msa = np.empty((m, n), dtype=np.uint8)
    for b0 in range(0, n, brec):
        pick = rng.integers(0, founders, size=m)
        msa[:, b0:b0 + brec] = F[pick, b0:b0 + brec]
    hit = rng.random((m, n)) < flip
    msa[hit] = alpha[rng.integers(0, len(alpha), size=int(hit.sum()))]
    if m * n >= len(alpha):
        flat = msa.reshape(-1)
        missing = [b for b in alpha if b not in set(np.unique(msa).tolist())]
        at = rng.choice(m * n, size=len(missing), replace=False)
        flat[at] = missing
    return msa
