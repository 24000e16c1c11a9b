"""The reduced column kernel k_columns_red<T, E, 4, PK, EW> (csrc/fseq_reduced.hpp) with R representatives on both sides of every
capacity of its 24 configurations, in phase C (the configurations with a list wave, (T - 64) x E rows, and the one-wave ones) and
in pass 2's class-table sweeps (the others, T x E rows), bit for bit against the CPU oracle.

tests/reduced_capacity_cases.py holds the inputs and the hand-written table of expected configurations;
tests/test_reduced_capacity_cases.py proves on the CPU that block 6 of every case has exactly R representatives (blocks 0 to 5:
R - 1), that the one boundary of the optimum lies inside it at column 687, and that its lists are not trivial.

A child process per group of cases, one after another, with FSEQ_DEBUG=1 FSEQ_REDUCED_ALWAYS=1.  For every case the child
  * holds the run to the oracle as test_gpu_parity.compare_long does: DP array, traceback, merged segments, the whole boundary
    state (a, d) at column 687 (and at n);
  * holds the lists of columns 595 to 699 to the oracle's pBWT (reduced_capacity_cases.lists_match);
  * runs the context again (the cached plan) and requires the same traceback and boundary state;
  * runs a fresh context from the default list capacity of 63, given explicitly -- by itself the library sizes the lists from
    the block boundary states, and no list of these inputs is open --: the list of column 686 is cut behind 63 rows' worth of
    entries (no cell of these inputs asks for more, so nothing is retried), and the result and the lists, as prefixes, are
    the oracle's again;
  * states the representatives of every block by the model of tests/proto_reduced.py over the oracle's pBWT (blocks 0 to 6:
    R - 1 six times, then R -- asserted; the blocks behind column L - 2 by choose_vmin at the list capacity in use).
The parent reads the library's reports from the child's stderr: the last plan of phase C (`configuration of N rows: K blocks,
M representatives on average (T threads x E rows, ...`) must be exactly the stated representatives sorted into the
hand-written configurations -- so the configuration of the table holds block 6, its rows are the table's capacity, and
blocks 0 to 5 sit in the configuration for R - 1 --, and pass 2's report (`reduced pass 2: configuration of N rows: W
workgroups, K tasks in blocks a to b (T threads x E rows)`) must show block 6's one task on the table's configuration, in
both runs.  R = 11,265 (more than the plan's cap) and R = 701 of 1,000 rows (more than 70 %) run block 6 on all rows beside
the reduced blocks 0 to 5: no line of the plan holds it.  A case cannot pass without its configuration having run.

Measured on an MI355X: the file takes 25 seconds (twelve child processes of 0.6 to 4.8 s, 62 cases)."""
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
CHILD_TIME_LIMIT = 300          # seconds; a group takes a tenth of it
FIRST_LIST_COLUMN, LAST_LIST_COLUMN = 595, 699


def representatives_per_block(msa, L, B, X):
    """k_reduce_prep's count for every block by the model of tests/proto_reduced.py: the rows with a divergence >= vmin behind
    the block; vmin = 1 for a block that starts in front of column L - 2, else choose_vmin over the state in front of it."""
    import fso
    from proto_reduced import choose_vmin
    m, n = msa.shape
    p = fso.Pbwt(msa, with_counts=False, debug=False)
    Xp = X + X // 4 + 8
    out = []
    d0 = p.d
    for k0 in range(0, n, B):
        k1 = min(n, k0 + B)
        for _ in range(k0, k1):
            p.step()
        d1 = p.d
        vmin = 1 if k0 + 2 <= L else max(1, choose_vmin(d0.astype(np.int64), k0, L, Xp, W=2048))
        out.append(int((d1 >= vmin).sum()))
        d0 = d1
    return out


def child(group):
    import importlib
    sys.path[:0] = [HERE, os.path.dirname(HERE), os.path.join(os.path.dirname(HERE), "oracle")]
    import reduced_capacity_cases as rcc
    from test_gpu_parity import check_long, compare_long, run_gpu
    pkg = importlib.import_module("founder-sequences_amd")

    def mark(text):
        sys.stderr.flush()
        sys.stderr.write("[case] %s\n" % text)
        sys.stderr.flush()

    for name in rcc.GROUPS[group]:
        case = rcc.CASES[name]
        msa = rcc.make(case)
        n, L, B = rcc.N, rcc.L, rcc.BLOCK
        mark(name + " first run")
        ctx, ref = compare_long(pkg, msa, L, check_dp=True, block_len=B)
        red = ctx.reduced_traceback()
        assert red["rb"].tolist() == [rcc.C, n] and len(ref["a"]) == 2, red
        lists = rcc.lists_match(ctx, msa, L, columns=range(FIRST_LIST_COLUMN, LAST_LIST_COLUMN + 1))
        t = ctx.timings()
        tb = ctx.traceback().copy()
        a, d = (x.copy() for x in ctx.boundary_state(0))
        mark(name + " second run")
        ctx.run()
        a2, d2 = ctx.boundary_state(0)
        t2 = ctx.timings()
        counts = representatives_per_block(msa, L, B, t["list_cap_used"])
        assert counts[:rcc.BLOCK_UNDER_TEST + 1] == [case.R - 1] * rcc.BLOCK_UNDER_TEST + [case.R], counts
        # a fresh context that starts at the default list capacity, given explicitly (by itself the library sizes the lists from the
        # block boundary states and no list of these inputs is open): the list of column 686 is cut
        mark(name + " from the default list capacity")
        low = run_gpu(pkg, msa, L, block_len=B, list_cap=rcc.DEFAULT_LIST_CAP)
        check_long(low, ref, n, L, check_dp=True)
        low_lists = rcc.lists_match(low, msa, L, columns=range(FIRST_LIST_COLUMN, LAST_LIST_COLUMN + 1))
        t3 = low.timings()
        low_complete = bool(low.debug_column_list(rcc.C - 1)[3])
        low.close()
        print(json.dumps({"name": name, "lists": lists, "bits": int(ctx.packed_columns(0, 1)[1]), "representatives": counts,
                          "low_lists": low_lists, "low_retries": t3["retries"], "low_list_cap_used": t3["list_cap_used"], "low_reduced_blocks": t3["reduced_blocks"],
                          "low_complete_at_686": low_complete,
                          "reduced_blocks": t["reduced_blocks"], "n_blocks": t["n_blocks"], "list_cap_used": t["list_cap_used"],
                          "retries": t["retries"], "redone": t["reduced_redone"], "second_reduced_blocks": t2["reduced_blocks"],
                          "second_list_cap_used": t2["list_cap_used"],
                          "same_traceback": bool(np.array_equal(ctx.traceback(), tb)),
                          "same_state": bool(np.array_equal(a, a2) and np.array_equal(d, d2)),
                          "state_is_the_oracles": bool(np.array_equal(a2, ref["a"][0]) and np.array_equal(d2, ref["d"][0]))}), flush=True)
        ctx.close()
    mark("end")


PLAN = re.compile(r"configuration of (\d+) rows: (\d+) blocks, (\d+) representatives on average \((\d+) threads x (\d+) rows, ")
PASS_2 = re.compile(r"reduced pass 2: configuration of (\d+) rows: (\d+) workgroups, (\d+) tasks in blocks (\d+) to (\d+) \((\d+) threads x (\d+) rows\)")


def reports(stderr):
    """{"<case> first run" | "<case> second run": (plans, pass-2 lines)} from a child's stderr: the plans of phase C in order, each
    [(rows, blocks, mean, T, E)], and pass 2's lines (rows, workgroups, tasks, first block, last block, T, E)."""
    out, cur, plans, p2 = {}, None, None, None
    for line in stderr.splitlines():
        if line.startswith("[case] "):
            plans, p2 = [], []
            cur = None
            out[line[len("[case] "):]] = (plans, p2)
            continue
        if plans is None:
            continue
        if "reduced phase C:" in line and "blocks on their representatives" in line:
            cur = []
            plans.append(cur)
        mm = PLAN.search(line)
        if mm and cur is not None:
            cur.append(tuple(int(x) for x in mm.groups()))
        mm = PASS_2.search(line)
        if mm:
            p2.append(tuple(int(x) for x in mm.groups()))
    return out


def expected_plan(rcc, counts, m):
    """The stated representatives of the blocks sorted into the hand-written configurations of phase C, {(rows, T, E): (blocks,
    mean)}, and the blocks that run on all rows: more representatives than the plan's cap or than 70 % of the rows."""
    bins, on_all_rows = {}, []
    for b, r in enumerate(counts):
        if r > rcc.RED_CAP or 10 * r > 7 * m:
            on_all_rows.append(b)
            continue
        T, E, rows = rcc.phase_c_of(r)
        bins.setdefault((rows, T, E), []).append(r)
    return {key: (len(v), sum(v) // len(v)) for key, v in bins.items()}, on_all_rows


@pytest.mark.parametrize("group", ["2b_192_to_961", "2b_1280_to_3137", "2b_3584_to_5121", "2b_6720_to_7681", "2b_8640_to_9217", "2b_9600_to_10241",
                                   "2b_10560_to_11265", "4b_448_to_2241", "4b_6720_to_8641", "8b_448_to_2241", "8b_6720_to_8641", "share_700_701"])
def test_both_sides_of_every_capacity(group):
    env = dict(os.environ, FSEQ_DEBUG="1", FSEQ_REDUCED_ALWAYS="1")
    for knob in ("FSEQ_NO_REDUCED", "FSEQ_REDUCED_CAP", "FSEQ_REDUCED_MARGIN"):
        env.pop(knob, None)
    p = subprocess.run([sys.executable, os.path.abspath(__file__), group], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=CHILD_TIME_LIMIT)
    assert p.returncode == 0, p.stderr[-6000:]
    check_group(group, p.stdout, p.stderr)


def check_group(group, stdout, stderr):
    """What a child printed and what the library reported while it ran, against the table."""
    import reduced_capacity_cases as rcc
    outs = {o["name"]: o for o in (json.loads(line) for line in stdout.splitlines() if line.startswith("{"))}
    rep = reports(stderr)
    assert list(outs) == rcc.GROUPS[group] and "end" in rep, (list(outs), stderr[-3000:])
    for name in rcc.GROUPS[group]:
        case, out = rcc.CASES[name], outs[name]
        plans, first_p2 = rep[name + " first run"]
        again, second_p2 = rep[name + " second run"]
        print(name, out, plans, first_p2, again, second_p2)
        blk = rcc.BLOCK_UNDER_TEST
        assert out["lists"] == LAST_LIST_COLUMN - FIRST_LIST_COLUMN + 1 and out["bits"] == case.bits, out
        assert out["same_traceback"] and out["same_state"] and out["state_is_the_oracles"], out
        # from the default capacity the list of column 686 is cut -- it has more than 63 distinct values below its threshold, and a
        # list takes entries only while the rows in front number at most the capacity -- unless the run went on to longer lists
        assert out["low_lists"] == out["lists"] and out["low_reduced_blocks"] > 0, out
        assert out["low_list_cap_used"] > rcc.DEFAULT_LIST_CAP or not out["low_complete_at_686"], out
        assert out["n_blocks"] == 13 and out["second_reduced_blocks"] == out["reduced_blocks"] and out["second_list_cap_used"] == out["list_cap_used"], out
        assert plans and again == [], (plans, again)         # (the second run launched by the first one's plan)
        got = {(rows, T, E): (blocks, mean) for rows, blocks, mean, T, E in plans[-1]}
        assert len(got) == len(plans[-1]), plans[-1]
        assert sum(blocks for blocks, _ in got.values()) == out["reduced_blocks"], (got, out)
        # the plan is the stated representatives in the hand-written configurations (a block whose lists reached below what its
        # representatives vouch for left the plan: then the assertions on blocks 0 to 6 below stand alone)
        want, on_all_rows = expected_plan(rcc, out["representatives"], case.m)
        assert (blk in on_all_rows) == case.on_all_rows, (case, on_all_rows)
        if out["redone"] == 0:
            assert got == want and out["reduced_blocks"] == out["n_blocks"] - len(on_all_rows), (got, want, out)
        if case.on_all_rows:
            # block 6 on all rows beside the reduced blocks 0 to 5: no line of the plan holds it
            assert 0 < out["reduced_blocks"] < out["n_blocks"], out
            T, E, rows = rcc.phase_c_of(case.R - 1)
            assert got[rows, T, E][0] >= blk, got
        else:
            T, E = case.phase_c
            rows = rcc.rows_of(T, E, T > 64)
            assert (rows, T, E) in got and rows >= case.R, (case, got)
            before = rcc.phase_c_of(case.R - 1)
            if before[:2] == case.phase_c:
                assert got[rows, T, E][0] >= blk + 1, got
            else:
                assert min(before[2], rcc.RED_CAP) == case.R - 1 and got[before[2], before[0], before[1]][0] >= blk and got[rows, T, E][0] >= 1, got
        # pass 2: block 6's one task on the configuration without a list wave, in both runs
        for p2 in (first_p2[-1:], second_p2):
            if case.pass_2 is None:
                assert p2 == [], p2
            else:
                T, E = case.pass_2
                assert p2 == [(T * E, 1, 1, blk, blk, T, E)] and T * E >= case.R, (case, p2)


if __name__ == "__main__":
    child(sys.argv[1])
