"""Python model of pass 2's chain step BY RUNS (pass2_runs in csrc/fseq_chainsort.hpp).

A chain step takes the pBWT state (a0, d0) in front of a column block to the state (a1, d1) at a column c inside it, keyed by
the classes the rows form over the block's columns [k0, c) (classes numbered in co-lexicographic order of those substrings):
a1 = the stable sort of a0 by class; the first row of a class takes the class's divergence headd[class]; any other row takes
the maximum of d0 over the old positions behind its predecessor's up to its own.

Claim.  Cut the old order into runs, maximal stretches of consecutive positions of one class.  The stable sort by class is
the runs ordered by (class, start), each run copied whole.  A row that is not its run's first has its predecessor right in
front of it in the old order too, so its range is its own position and d1 = d0 there.  Only a run's first row needs more:
headd where the run is the first of its class, else the maximum of d0 from behind the end of the class's previous run up to
the run's start.  A boundary state is a pBWT order, in which rows that agree over the next columns already lie together: the
runs are few (about two a class) unless a recombination boundary of the founders lies between k0 and c.

chain_step_runs states that with a cap on the runs and the fallback to the sort of all rows; tests/test_proto_pass2_runs.py
proves it equal to chain_step_sorted and to the oracle's pBWT at the boundary.  TEST INFRASTRUCTURE (uses oracle/).
"""
import numpy as np


def block_classes(msa, k0, c, d_first):
    """(class of every row, headd) of the columns [k0, c): classes in co-lexicographic order of the rows' substrings, headd[q]
    = the divergence of class q's first row behind the step = one past the last column at which class q differs from class
    q - 1 (headd[0] = d_first: position 0 keeps the divergence the pBWT gives it)."""
    rev = np.ascontiguousarray(msa[:, k0:c][:, ::-1])
    uniq, key = np.unique(rev, axis=0, return_inverse=True)
    key = key.reshape(-1).astype(np.int64)
    headd = np.empty(len(uniq), dtype=np.int64)
    headd[0] = d_first
    for q in range(1, len(uniq)):
        headd[q] = c - int(np.flatnonzero(uniq[q] != uniq[q - 1])[0])
    return key, headd


def chain_step_sorted(a0, d0, key, headd):
    """The step as the stable sort of all rows by class plus range maxima (pass2_step)."""
    m = len(a0)
    k = key[a0]
    order = np.argsort(k, kind="stable")
    a1 = a0[order]
    d1 = np.empty(m, dtype=np.int64)
    for p in range(m):
        if p == 0 or k[order[p - 1]] != k[order[p]]:
            d1[p] = headd[k[order[p]]]
        else:
            d1[p] = d0[order[p - 1] + 1:order[p] + 1].max()
    return a1, d1


def run_starts(a0, key):
    k = key[a0]
    return np.flatnonzero(np.r_[True, k[1:] != k[:-1]])


def chain_step_runs(a0, d0, key, headd, cap):
    """The step by runs where the classes form at most `cap` of them (cap 0: never), else by the sort of all rows.
    Returns (a1, d1, runs, by_runs)."""
    m = len(a0)
    k = key[a0]
    starts = run_starts(a0, key)
    R = len(starts)
    if cap == 0 or R > cap:
        return chain_step_sorted(a0, d0, key, headd) + (R, False)
    ends = np.r_[starts[1:], m]
    order = np.lexsort((starts, k[starts]))                 # by (class, start)
    s, e, c = starts[order], ends[order], k[starts][order]
    off = np.r_[0, np.cumsum(e - s)]
    a1 = np.empty(m, dtype=a0.dtype)
    d1 = np.empty(m, dtype=np.int64)
    for j in range(R):
        p, n = off[j], e[j] - s[j]
        a1[p:p + n] = a0[s[j]:e[j]]
        d1[p + 1:p + n] = d0[s[j] + 1:e[j]]
        if j == 0 or c[j - 1] != c[j]:
            d1[p] = headd[c[j]]
        else:
            d1[p] = d0[e[j - 1]:s[j] + 1].max()
    return a1, d1, R, True
