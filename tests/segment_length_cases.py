"""Inputs for the sweep of the segment-length bound L: one table of mosaics for every L in 1..130 and for L around 512, 2,048,
4,096, 8,192 and 65,536, where L selects the code of the DP schedule, the DP's LDS rings, the speculative DP's plan, the
traceback windows and the reduced phase C (tests/test_gpu_segment_length.py names what each group reaches).

A case is (m, n, L, K, Brec, mu, seed, kind): the alignment is fso.synth_msa(fso.synth_spec(seed, K, Brec, mu, kind), m, n).
Recombination every ~3 L columns and a mutation rate of 0.02 / L keep the optimum at a handful of founders per segment
whatever L is, so that every long width has a traceback of several segments and a reduction (max_segment_size < m):
tests/test_segment_length_cases.py holds every case to that on the CPU, from the oracle alone.  numpy and the oracle's
generator only, no GPU."""
import numpy as np

import fso

DP_RL = 56              # cells of a classic DP round (csrc/fseq_dp.hpp)
DP_PIPE_MIN_L = 96      # from here on: the pipelined schedule, rounds of 48 cells


def round_length(L):
    """Cells of a regular DP round (dp_schedule, csrc/fseq_dp.hpp); tests/test_segment_length_cases.py holds it to the library's."""
    return L if L < DP_RL else DP_RL if L < DP_PIPE_MIN_L else 48


SMALL_L = tuple(range(1, 131))
LARGE_L = (511, 512, 513, 2047, 2048, 2049, 4095, 4096, 4097, 8191, 8192, 8193, 12289, 16385, 65535, 65536, 65537)
SPECULATIVE_L = (513, 2049, 4097, 8193)           # at 30 L columns the library's own plan has at least three chunks
FORCED_SPECULATIVE_L = (16385, 65537)             # at 6 L columns, chunks of a third of the regular rounds


def small_long(L):
    """40 rows, about fourteen segment lengths of columns, a width that moves against the rounds with L."""
    return (40, 14 * L + 211 + L % 7, L, 4, max(8, 3 * L), 0.02 / L, 500 + L, 0)


def small_short(L):
    """The same mosaic at n = 2 L + j: one to three regular rounds, the last one of 1, 2, RL - 1 or RL cells (the tail of the
    schedule); j goes through 0, 1, RL - 1, RL, RL + 1, 2 RL - 1 with L."""
    RL = round_length(L)
    j = (0, 1, RL - 1, RL, RL + 1, 2 * RL - 1)[L % 6]
    return (40, 2 * L + j, L, 4, max(8, 3 * L), 0.02 / L, 500 + L, 0)


def large(L, widths=6):
    """48 rows, 6 L columns (+ 37 + L mod 5): fewer than three chunks of 8 L entries, the serial DP kernel."""
    return (48, widths * L + 37 + L % 5, L, 5, 3 * L + 3, 0.02 / L, 900 + L, 0)


def speculative(L):
    """The generator of large() at 30 L + 37 columns: at least three chunks on the library's own plan."""
    return (48, 30 * L + 37, L, 5, 3 * L + 3, 0.02 / L, 900 + L, 0)


def forced_spec_rounds(L, n):
    """FSEQ_DP_SPEC_ROUNDS for the forced speculative cases: chunks of a third of the regular rounds."""
    nreg = (n - 2 * L) // round_length(L) + 1
    return max(1, nreg // 3)


# large L on larger row counts: name -> case.  By the row count alone the library keeps a block's order in LDS as 32-bit words
# (m <= 7,168), as 16-bit words (m <= 11,264) or streams it in tiles (tests/test_gpu_parity.py brackets these capacities in
# test_kernel_configuration_boundaries); sigma = 16 is stored at 4 bits per symbol.
ROW_CASES = {
    "rows_2504": (2504, 25000, 5000, 16, 9000, 2e-6, 5000 + 2504, 0),
    "rows_10000_sigma_16": (10000, 17500, 4200, 32, 8000, 1e-6, 4200 + 10000, 1),
    "rows_12000": (12000, 17000, 4100, 12, 7000, 1e-6, 4100 + 12000, 0),
}
ROW_CASE_BITS = {"rows_2504": 2, "rows_10000_sigma_16": 4, "rows_12000": 2}     # bits per stored symbol

# the sharded shapes (tests/test_gpu_segment_length.py): ranks that hold fewer columns than two segment lengths, and -- the
# second form -- leading ranks in front of column L, which own no DP round
SHARD_L_LONG = (513, 4097)
SHARD_L_SHORT = (100, 1000)


def shard_short(L):
    return (40, 2 * L + 3 * round_length(L), L, 4, max(8, 3 * L), 0.02 / L, 500 + L, 0)


def make(case):
    """The alignment of a case: C-contiguous uint8 (m, n), read-only."""
    m, n, L, K, Brec, mu, seed, kind = case
    msa = np.ascontiguousarray(fso.synth_msa(fso.synth_spec(seed, K, Brec, mu, kind), m, n))
    msa.setflags(write=False)
    return msa


def conditioned_cases():
    """Every case that must have a reduction, a traceback of at least three entries and at least two merged segments."""
    out = [("small_long_%d" % L, small_long(L)) for L in SMALL_L]
    out += [("large_%d" % L, large(L)) for L in LARGE_L]
    out += [("speculative_%d" % L, speculative(L)) for L in SPECULATIVE_L]
    out += list(ROW_CASES.items())
    return out
