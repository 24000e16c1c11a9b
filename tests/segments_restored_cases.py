"""The model and the inputs of the segments file in source co-ordinates (fseq_get_segments_restored,
fseq_write_segments_restored): the bounds in numpy, alignments with identity columns planted at known places, and the expected
file made from the reduced writer's bytes.  Nothing here touches the library."""
import numpy as np

from helpers import founder_mosaic


def restored_bounds(kept, n_src, lb, rb):
    """(src_lb, src_rb) of the merged segments [lb[s], rb[s]) -- given in kept columns, tiling them -- in the source's
    co-ordinates.  kept[j] is the source column of kept column j.  A segment owns the source positions from its first kept column
    up to the next segment's first kept column; the first one those in front of kept[0] too, the last one those up to n_src."""
    kept = np.asarray(kept, dtype=np.int64)
    lb, rb = np.asarray(lb, dtype=np.int64), np.asarray(rb, dtype=np.int64)
    firsts = kept[lb]                                           # the source column of every segment's first kept column
    src_lb = np.concatenate([[0], firsts[1:]])
    src_rb = np.concatenate([firsts[1:], [n_src]])
    return src_lb.astype(np.uint64), src_rb.astype(np.uint64)


def without_own_identity(msa):
    """msa without the columns in which all its rows agree: an alignment that has no identity column."""
    return np.ascontiguousarray(msa[:, ~(msa == msa[0]).all(0)])


def mosaic_without_identity(X, m, n, **kw):
    """founder_mosaic(X, m, n, ...) with its own identity columns removed (about n columns: a few fewer)."""
    return without_own_identity(founder_mosaic(X, m, n, **kw))


def with_identity_runs(R, runs, byte_of=None):
    """R [m, n], without identity columns, with runs of identity columns inserted: runs maps a reduced position p in 0 .. n to a
    length, and the run stands in front of R's column p (p = n: behind the last).  byte_of(source position) gives an inserted
    column's byte (every row carries it); by default a byte of R's alphabet that changes along the run.  Returns (full, kept):
    the alignment [m, n + sum of the lengths] and the source column of every column of R."""
    m, n = R.shape
    assert not (R == R[0]).all(0).any(), "R has identity columns of its own"
    assert all(0 <= p <= n and k > 0 for p, k in runs.items())
    alphabet = np.unique(R)
    if byte_of is None:
        byte_of = lambda p: alphabet[(p * 7 + p // 5) % len(alphabet)]
    n_src = n + sum(runs.values())
    full = np.empty((m, n_src), dtype=np.uint8)
    kept = np.empty(n, dtype=np.int64)
    at = 0
    for p in range(n + 1):
        for _ in range(runs.get(p, 0)):
            full[:, at] = byte_of(at)
            at += 1
        if p < n:
            full[:, at] = R[:, p]
            kept[p] = at
            at += 1
    assert at == n_src
    return full, kept


def data_lines(blob):
    lines = blob.split(b"\n")
    assert lines[-1] == b""
    return lines[:-1]


BIPARTITE, RANDOM = 1, 2            # FSEQ_JOIN_BIPARTITE, FSEQ_JOIN_RANDOM


def restore_file(reduced_blob, full, kept, joining):
    """The file fseq_write_segments_restored must write, from the bytes fseq_write_segments_device wrote on the same context
    (reduced co-ordinates), the source alignment and the kept columns.  Every data line keeps its fields but LB / RB, which
    become the model's source bounds, and the substring, which becomes full[row, src_lb:src_rb] for the row whose bytes the line
    shows: the lowest row of the line's text (bipartite), the lowest row of the text named in COPIED_FROM (a placeholder), the
    line's substring index (random).  That the reduced substring is full[row, kept[lb:rb]] is asserted, so the choice of the row
    is checked too."""
    kept = np.asarray(kept, dtype=np.int64)
    lines = data_lines(reduced_blob)
    fields = [x.split(b"\t") for x in lines[1:]]
    if not fields:
        return reduced_blob                                     # (greedy: the header alone)
    assert all(len(f) == 7 for f in fields)
    # the segments as the file has them, in order
    segs = []
    for f in fields:
        s, lb, rb = int(f[0]), int(f[1]), int(f[2])
        if not segs or segs[-1][0] != s:
            assert s == len(segs)
            segs.append((s, lb, rb))
        assert segs[s] == (s, lb, rb)
    lbs, rbs = [x[1] for x in segs], [x[2] for x in segs]
    assert lbs[0] == 0 and rbs[-1] == len(kept) and lbs[1:] == rbs[:-1], "the reduced file's segments tile the kept columns"
    src_lb, src_rb = restored_bounds(kept, full.shape[1], lbs, rbs)
    first_of = {}                                               # (segment, index of a line inside it) -> the fields
    out = [lines[0]]
    count = {}
    for f in fields:
        s = int(f[0])
        j = count.get(s, 0)
        count[s] = j + 1
        first_of[(s, j)] = f
        if joining == BIPARTITE:
            if f[6] == b"-":
                row = int(f[5].split(b",")[0])                  # (the rows of a text ascend)
            else:
                assert f[5] == b""
                src = first_of[(s, int(f[6]))]                  # (a text stands in front of its placeholders)
                assert src[6] == b"-"
                row = int(src[5].split(b",")[0])
            text = 4
        else:
            row = int(f[4])
            text = 6
        lb, rb = lbs[s], rbs[s]
        assert f[text] == full[row, kept[lb:rb]].tobytes(), ("the reduced substring of segment %d, line %d is not row %d's" % (s, j, row))
        g = list(f)
        g[1], g[2] = b"%d" % int(src_lb[s]), b"%d" % int(src_rb[s])
        g[text] = full[row, int(src_lb[s]):int(src_rb[s])].tobytes()
        out.append(b"\t".join(g))
    return b"\n".join(out) + b"\n"
