"""[r7] The slim configuration of the reduced column kernel (512 threads x 15 rows, two workgroups per CU; csrc/fseq_kernels.hpp
`columns_slim`): the blocks it takes, its edges, and the blocks it refuses.

Every case builds an input whose number of representatives per block is known exactly: R pairwise different rows and
m - R exact copies of some of them, with a segment-length bound L so large that every block under test starts in front of
column L - 2.  Such a block is exact (vmin = 1: the rows left out are duplicates over all of [0, k1)), so it has exactly one
representative per distinct row prefix -- R of them once the rows differ.

Each case runs in a child process with FSEQ_DEBUG=1: the child runs the input reduced and again with FSEQ_NO_REDUCED (all
rows of every block), compares the per-column lists of the sampled columns and the results, and the parent reads the
library's plan report (`configuration of N rows: K blocks, ... (T threads x E rows, ...)`) from the child's stderr: a case
cannot pass without the configuration it is about having run.

 (a) blocks on the slim configuration, lists equal to the run on all rows;
 (b) a block whose representatives fit but whose distinct start values (> 4096) do not: the workgroup refuses, the block
     runs on 1024 x 7, the lists stay equal;
 (c) 6,719 / 6,720 / 6,721 representatives: the last two of the slim configuration's capacity and the first of the next."""
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
SLIM_ROWS = (512 - 64) * 15          # = (1024 - 64) * 7: the list wave holds no rows
SLIM_VALUES = 4096
SYMS = np.frombuffer(b"ACGT", dtype=np.uint8)


def distinct_rows_with_copies(R, m, n, seed):
    """R random rows (pairwise different within a few columns) and m - R exact copies, shuffled."""
    rng = np.random.default_rng(seed)
    base = SYMS[rng.integers(0, 4, size=(R, n), dtype=np.uint8)]
    # (the first columns spell the row number, so that the rows differ from column 7 on whatever the draw)
    idx = np.arange(R)
    for j in range(7):
        base[:, j] = SYMS[(idx >> (2 * j)) & 3]
    src = np.concatenate([idx, rng.integers(0, R, size=m - R)])
    rng.shuffle(src)
    return np.ascontiguousarray(base[src])


def chained_groups_with_copies(groups, g, m, n, cmax, seed):
    """groups x g rows: the rows of a group share one random sequence and differ from it in one column each, every one of the
    groups * g columns a different one below cmax.  Behind cmax the rows of a group are neighbours in the pBWT order and
    their divergences are the mutation columns: about groups * (g - 1) distinct values among groups * g rows."""
    rng = np.random.default_rng(seed)
    R = groups * g
    assert R <= cmax - 8
    seqs = SYMS[rng.integers(0, 4, size=(groups, n), dtype=np.uint8)]
    gi = np.arange(groups)
    for j in range(7):
        seqs[:, j] = SYMS[(gi >> (2 * j)) & 3]
    rows = np.repeat(seqs, g, axis=0)
    cols = 8 + rng.permutation(cmax - 8)[:R]
    r = np.arange(R)
    rows[r, cols] = SYMS[(np.searchsorted(SYMS, rows[r, cols]) + 1) & 3]
    src = np.concatenate([r, rng.integers(0, R, size=m - R)])
    rng.shuffle(src)
    return np.ascontiguousarray(rows[src])


CASES = {
    # name: (builder, arguments, L, block length, first column of the blocks under test)
    "slim": (distinct_rows_with_copies, dict(R=5600, m=8200, n=1300, seed=701), 640, 100, 100),
    "below": (distinct_rows_with_copies, dict(R=SLIM_ROWS - 1, m=9700, n=1300, seed=702), 640, 100, 100),
    "at": (distinct_rows_with_copies, dict(R=SLIM_ROWS, m=9700, n=1300, seed=703), 640, 100, 100),
    "above": (distinct_rows_with_copies, dict(R=SLIM_ROWS + 1, m=9700, n=1300, seed=704), 640, 100, 100),
    "values": (chained_groups_with_copies, dict(groups=800, g=8, m=9200, n=13500, cmax=6500, seed=705), 6700, 100, 4000),
}


def child(name):
    import importlib
    sys.path[:0] = [os.path.dirname(HERE), os.path.join(os.path.dirname(HERE), "oracle")]
    pkg = importlib.import_module("founder-sequences_amd")
    builder, kw, L, B, first = CASES[name]
    msa = builder(**kw)
    m, n = msa.shape

    def run(no_reduced):
        ctx = pkg.SegmentationContext(m, n, L, block_len=B)
        if no_reduced:
            ctx.set_tuning("FSEQ_NO_REDUCED", "1")
        ctx.set_sequences(msa)
        try:
            ctx.run()
        except pkg.NoReduction:
            pass
        return ctx

    red, full = run(False), run(True)
    # the columns of the exact blocks behind `first`: every 7th, and the first and last columns of every block
    cols = sorted({k for k in range(first, L - 2) if k % 7 == 0 or k % B in (0, 1, B - 1)})
    bad = []
    for k in cols:
        a, b = red.debug_column_list(k), full.debug_column_list(k)
        if not (np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[2:] == b[2:]):
            bad.append(k)
    t = red.timings()
    print(json.dumps({"columns": len(cols), "bad": bad[:10], "reduced_blocks": t["reduced_blocks"], "n_blocks": t["n_blocks"],
                      "full_reduced_blocks": full.timings()["reduced_blocks"],
                      "same_traceback": bool(np.array_equal(red.traceback(), full.traceback())),
                      "same_size": red.result.max_segment_size == full.result.max_segment_size}))


def run_case(name):
    env = dict(os.environ, FSEQ_DEBUG="1", FSEQ_REDUCED_ALWAYS="1")
    env.pop("FSEQ_NO_REDUCED", None)
    p = subprocess.run([sys.executable, os.path.abspath(__file__), name], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=900)
    assert p.returncode == 0, p.stderr[-4000:]
    out = json.loads([line for line in p.stdout.splitlines() if line.startswith("{")][-1])
    # the plans of the reduced context, in order: (rows, blocks, mean, threads, rows per thread, values, LDS, resident) per configuration in use
    plans, cur = [], None
    for line in p.stderr.splitlines():
        if "reduced phase C:" in line and "blocks on their representatives" in line:
            cur = []
            plans.append(cur)
        mm = re.search(r"configuration of (\d+) rows: (\d+) blocks, (\d+) representatives on average \((\d+) threads x (\d+) rows, (\d+) distinct values, (\d+) bytes of LDS, (\d+) workgroups per CU\)", line)
        if mm and cur is not None:
            cur.append(tuple(int(x) for x in mm.groups()))
    assert plans, p.stderr[-4000:]
    print(name, out, plans)
    assert out["columns"] > 50 and out["bad"] == [] and out["same_traceback"] and out["same_size"], out
    assert out["reduced_blocks"] > 0 and out["full_reduced_blocks"] == 0, out
    return out, plans, p.stderr


def slim_entries(plan):
    return [e for e in plan if (e[3], e[4]) == (512, 15)]


def test_blocks_on_the_slim_configuration_match_the_run_on_all_rows():
    """(a), (d): 5,600 representatives per block -- more than 1024 x 5 holds (4,800) -- run on 512 x 15, two workgroups per CU
    in at most 80 KB of LDS each, and give the lists of the run on all rows."""
    _, plans, _ = run_case("slim")
    slim = slim_entries(plans[0])
    assert slim and slim[0][1] >= 4, plans
    rows, blocks, mean, T, E, values, lds, resident = slim[0]
    assert rows == SLIM_ROWS and values == SLIM_VALUES and mean == 5600
    assert lds <= 80 * 1024 and resident == 2, slim
    assert len(plans) == 1, "no block was refused or redone"


@pytest.mark.parametrize("name,R", [("below", SLIM_ROWS - 1), ("at", SLIM_ROWS), ("above", SLIM_ROWS + 1)])
def test_edges_of_the_slim_capacity(name, R):
    """(c): one below and at the capacity the blocks run slim; one above they take the next configuration (1024 x 8)."""
    _, plans, _ = run_case(name)
    plan = plans[0]
    big = [e for e in plan if e[2] == R]            # the configuration that holds the blocks of R representatives
    assert len(big) == 1 and big[0][1] >= 4, plan
    if R <= SLIM_ROWS:
        assert big[0][3:5] == (512, 15) and big[0][0] == SLIM_ROWS, plan
    else:
        assert big[0][3] == 1024 and big[0][0] >= R, plan


def test_more_distinct_values_than_the_slim_table_fall_back_to_the_wide_configuration():
    """(b): 6,400 representatives (they fit) with ~5,600 distinct start values (they do not): the workgroups refuse, the
    blocks run on 1024 x 7 in the attempt that follows, and the lists are those of the run on all rows."""
    _, plans, err = run_case("values")
    assert "more distinct start values than the slim configuration" in err, err[-3000:]
    assert len(plans) >= 2, plans
    assert slim_entries(plans[0]), plans[0]
    wide = [e for e in plans[-1] if (e[3], e[4]) == (1024, 7) and e[0] == SLIM_ROWS]
    assert wide and wide[0][1] >= 1, plans[-1]


if __name__ == "__main__":
    child(sys.argv[1])
