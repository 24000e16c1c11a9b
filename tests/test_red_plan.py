"""The plan of phase C on representative rows as a pure host function (plan_reduced, csrc/fseq_redplan.hpp) through its host entry
fseq_debug_red_plan: which block runs on which configuration, which on all rows, whether the representatives pay, and the layout of
the block list that goes to the device.  No GPU: the entry touches no device.

The expected configurations are named by (threads, rows per thread, list wave) and come from tests/reduced_capacity_cases.py, whose
table is written by hand; the library's own table (the `configs` the entry returns) is used only to turn such a name into an index.
The two deviations DESIGN.md records are pinned here: a block above 70 % of the rows is `full` and still has its `config_snap_of`
(pass 2 sweeps its representatives), and `config_snap_of` is set for every block with a count, `full` or not."""
import importlib
import os
import subprocess

import pytest

import reduced_capacity_cases as rcc


@pytest.fixture(scope="module")
def pkg():
    importlib.import_module("founder-sequences_amd.build").build()
    return importlib.import_module("founder-sequences_amd")


def index_of(plan, T, E, ew):
    """The index of the configuration of T threads x E rows with (ew) or without a list wave in the library's table."""
    hits = [i for i, (_, _, t, e, w, _) in enumerate(plan["configs"]) if (t, e, w) == (T, E, ew)]
    assert len(hits) == 1, (T, E, ew, plan["configs"])
    return hits[0]


def in_bin(plan, block):
    """The configurations whose stretch of `blocks` holds the block."""
    return [cf for cf, first, count in plan["bins"] if block in plan["blocks"][first:first + count].tolist()]


def all_rows_stretch(plan):
    return plan["blocks"][plan["full_at"]:plan["full_at"] + plan["nfull"]].tolist()


# ---- both sides of every capacity: the table of tests/reduced_capacity_cases.py

@pytest.mark.parametrize("name", sorted(rcc.CASES))
def test_capacity_case(pkg, name):
    """13 blocks as the case's run has them: blocks 0 to 5 with R - 1 representatives, block 6 with R (the prep writes RED_NONE above
    the plan's cap), planned as the GPU test runs them (FSEQ_REDUCED_ALWAYS, blocks of 100 columns, the case's rows and bits)."""
    case = rcc.CASES[name]
    count = lambda r: pkg.RED_NONE if r > rcc.RED_CAP else r
    cnt = [count(case.R - 1)] * 6 + [count(case.R)] + [count(case.R - 1)] * 6
    plan = pkg.red_plan_host(case.m, rcc.BLOCK, case.bits, case.m < rcc.STREAMED_FROM, cnt, reduced_always=True)
    assert plan["verdict"] == pkg.RED_USE and all(fits for *_, fits in plan["configs"])
    blk = rcc.BLOCK_UNDER_TEST
    if case.phase_c is None:
        assert plan["full"][blk] == 1 and blk in all_rows_stretch(plan) and in_bin(plan, blk) == []
    else:
        T, E = case.phase_c
        cf = index_of(plan, T, E, T > 64)
        assert plan["config_of"][blk] == cf and plan["full"][blk] == 0 and in_bin(plan, blk) == [cf]
        assert plan["configs"][cf][0] == rcc.rows_of(T, E, T > 64) >= min(case.R, rcc.RED_CAP)
    if case.pass_2 is None:
        assert plan["config_snap_of"][blk] == -1
    else:
        T, E = case.pass_2
        cs = index_of(plan, T, E, False)
        assert plan["config_snap_of"][blk] == cs and plan["configs"][cs][0] == T * E >= case.R
    # blocks 0 to 5 sit where the table's thresholds put R - 1
    T, E, rows = rcc.phase_c_of(case.R - 1)
    before = index_of(plan, T, E, T > 64)
    for b in range(blk):
        assert plan["config_of"][b] == before and plan["full"][b] == 0 and in_bin(plan, b) == [before], b
    T, E, _ = rcc.pass_2_of(case.R - 1)
    assert plan["config_snap_of"][:blk].tolist() == [index_of(plan, T, E, False)] * blk


# ---- the 70 % rule, the plan's cap, the force marks

def test_seventy_percent_rule(pkg):
    """10 r > 7 m: 700 of 1,000 rows run on the representatives, 701 on all rows -- and pass 2's configuration stays set at 701 (the
    recorded deviation: pass 2 sweeps the representatives of a block that phase C ran on all rows)."""
    at = pkg.red_plan_host(1000, 100, 2, True, [700] * 8, reduced_always=True)
    c256x5, c256x3 = index_of(at, 256, 5, True), index_of(at, 256, 3, False)
    assert at["full"].tolist() == [0] * 8 and at["config_of"].tolist() == [c256x5] * 8 and at["nfull"] == 0
    over = pkg.red_plan_host(1000, 100, 2, True, [700] * 7 + [701], reduced_always=True)
    assert over["full"].tolist() == [0] * 7 + [1] and all_rows_stretch(over) == [7] and in_bin(over, 7) == []
    assert over["config_snap_of"][7] == c256x3 and over["config_of"][7] == c256x5      # (known, not used: the block is full)
    assert over["listed"] == 8 and over["blocks"][:8].tolist() == list(range(8))        # (its representatives are still listed)
    assert over["reduced_blocks"] == 7 and over["rows_mean"] == 700 and over["max_rows"] == 701


def test_counts_above_the_plan_cap(pkg):
    """RED_NONE -- what the prep writes above the cap of 11,264 -- makes the block full and unlisted, with no configuration."""
    plan = pkg.red_plan_host(16100, 100, 2, False, [5000, pkg.RED_NONE, 5000, 5000, 5000, 5000], reduced_always=True)
    assert plan["full"].tolist() == [0, 1, 0, 0, 0, 0] and plan["config_of"][1] == -1 and plan["config_snap_of"][1] == -1
    assert plan["listed"] == 5 and plan["blocks"][:5].tolist() == [0, 2, 3, 4, 5] and all_rows_stretch(plan) == [1]
    assert plan["max_rows"] == 5000 and plan["verdict"] == pkg.RED_USE


def test_force_marks(pkg):
    """RED_FORCE_FULL sends a block to all rows; RED_FORCE_WIDE moves it past the slim configuration (values < rows: 512 x 15) to the
    next one with values >= rows, and to all rows where no such configuration fits."""
    cnt = [5000] * 6
    plain = pkg.red_plan_host(16100, 100, 2, False, cnt, reduced_always=True)
    slim, wide = index_of(plain, 512, 15, True), index_of(plain, 1024, 7, True)
    assert plain["configs"][slim][1] < plain["configs"][slim][0] and plain["configs"][wide][1] >= plain["configs"][wide][0]
    assert plain["config_of"].tolist() == [slim] * 6
    marked = pkg.red_plan_host(16100, 100, 2, False, cnt, force=[0, pkg.RED_FORCE_FULL, 0, pkg.RED_FORCE_WIDE, 0, 0], reduced_always=True)
    assert marked["full"].tolist() == [0, 1, 0, 0, 0, 0] and all_rows_stretch(marked) == [1]
    assert marked["config_of"].tolist() == [slim, slim, slim, wide, slim, slim]
    assert in_bin(marked, 3) == [wide] and in_bin(marked, 1) == [] and marked["listed"] == 6
    # the marks do not touch pass 2's configuration
    assert marked["config_snap_of"].tolist() == plain["config_snap_of"].tolist() == [index_of(plain, 1024, 5, False)] * 6
    # blocks of 32,000 columns of 8-bit symbols, LDS-resident rows: of the configurations that hold 5,000 rows only the slim one fits
    long_blocks = pkg.red_plan_host(11000, 32000, 8, True, cnt, reduced_always=True)
    assert [i for i, c in enumerate(long_blocks["configs"]) if c[5] and c[0] >= 5000] == [slim]
    assert long_blocks["config_of"].tolist() == [slim] * 6 and long_blocks["nfull"] == 0
    none_left = pkg.red_plan_host(11000, 32000, 8, True, cnt, force=[0, 0, pkg.RED_FORCE_WIDE, 0, 0, 0], reduced_always=True)
    assert none_left["config_of"][2] == -1 and none_left["full"].tolist() == [0, 0, 1, 0, 0, 0] and all_rows_stretch(none_left) == [2]


# ---- whether the representatives pay

def test_decline_rows(pkg):
    """rows_all * 5 > my_blocks * m, rows_all = the reduced blocks' representatives + 1.5 m per block on all rows.  20 blocks of 1,000
    rows: 4,000 representatives in all are used, 4,001 declined; with two blocks on all rows (3,000) 1,000 more are used, 1,001 not."""
    use = pkg.red_plan_host(1000, 100, 2, True, [200] * 20)
    assert use["verdict"] == pkg.RED_USE and use["reduced_blocks"] == 20 and use["rows_mean"] == 200
    assert pkg.red_plan_host(1000, 100, 2, True, [200] * 19 + [201])["verdict"] == pkg.RED_DECLINED
    full = [pkg.RED_NONE] * 2
    assert pkg.red_plan_host(1000, 100, 2, True, full + [56] * 10 + [55] * 8)["verdict"] == pkg.RED_USE          # 560 + 440 = 1,000
    assert pkg.red_plan_host(1000, 100, 2, True, full + [56] * 11 + [55] * 7)["verdict"] == pkg.RED_DECLINED     # 1,001


def test_decline_blocks_on_all_rows(pkg):
    """n_full * 4 > my_blocks.  A block on all rows counts 1.5 m rows, so n_full > my_blocks / 7.5 already meets the first clause: at
    20 blocks two on all rows are used, three declined, and on both sides of the second clause's own threshold (five | six of 20) the
    verdict is the first clause's.  FSEQ_REDUCED_ALWAYS overrides both clauses, but not a plan without a reduced block."""
    plan = lambda n_full, **kw: pkg.red_plan_host(1000, 100, 2, True, [pkg.RED_NONE] * n_full + [10] * (20 - n_full), **kw)
    assert [plan(k)["verdict"] for k in (2, 3, 5, 6)] == [pkg.RED_USE] + [pkg.RED_DECLINED] * 3
    for k in (3, 5, 6, 19):
        forced = plan(k, reduced_always=True)
        assert forced["verdict"] == pkg.RED_USE and forced["nfull"] == k and forced["reduced_blocks"] == 20 - k
    assert plan(20, reduced_always=True)["verdict"] == pkg.RED_DECLINED
    # reduced_always overrides the rows clause as well
    assert pkg.red_plan_host(1000, 100, 2, True, [600] * 20)["verdict"] == pkg.RED_DECLINED
    assert pkg.red_plan_host(1000, 100, 2, True, [600] * 20, reduced_always=True)["verdict"] == pkg.RED_USE


def test_no_block_list(pkg):
    """The first form of the streamed kernel takes no block list: with it in force a plan that sends a block to all rows is not used.
    Only then, and only with such a block; a declined plan stays declined."""
    cnt = [5000] * 19 + [pkg.RED_NONE]
    assert pkg.red_plan_host(100000, 800, 2, False, cnt, no_block_list=True)["verdict"] == pkg.RED_NO_BLOCK_LIST
    assert pkg.red_plan_host(100000, 800, 2, False, cnt, no_block_list=False)["verdict"] == pkg.RED_USE
    assert pkg.red_plan_host(100000, 800, 2, False, [5000] * 20, no_block_list=True)["verdict"] == pkg.RED_USE
    assert pkg.red_plan_host(100000, 800, 2, False, [90000] * 19 + [pkg.RED_NONE], no_block_list=True)["verdict"] == pkg.RED_DECLINED


# ---- a rank's range, the layout of the block list

def test_a_ranks_range(pkg):
    """b_lo > 0 and b_hi < nblocks: the blocks of the other ranks are neither listed nor full and have no configuration, whatever their
    counts say, and the verdict is over my blocks alone."""
    cnt = [900, pkg.RED_NONE, 100, 100, 100, 100, pkg.RED_NONE, 900]
    plan = pkg.red_plan_host(1000, 100, 2, True, cnt, b_lo=2, b_hi=6)
    assert plan["verdict"] == pkg.RED_USE and plan["reduced_blocks"] == 4 and plan["nfull"] == 0 and plan["listed"] == 4
    assert plan["blocks"].tolist() == [2, 3, 4, 5] * 2 and plan["bins"] == [(index_of(plan, 64, 3, False), 4, 4)]
    for b in (0, 1, 6, 7):
        assert plan["full"][b] == 0 and plan["config_of"][b] == -1 and plan["config_snap_of"][b] == -1
    # (all eight blocks mine: four of them on all rows -- declined)
    assert pkg.red_plan_host(1000, 100, 2, True, cnt)["verdict"] == pkg.RED_DECLINED


def test_layout_of_the_block_list(pkg):
    """`blocks`: every block with a count ascending, then each configuration in use in ascending index with its blocks ascending
    (`bins`), then the blocks on all rows ascending.  window_phase_c finds a window's blocks in every stretch by lower_bound."""
    rows = {"a": 100, "b": 300, "c": 2000, "d": 5000}
    kinds = "dacbX" "abcdF" "ccaXb" "dbaca" "abcdW"       # X: above the cap; F: forced to all rows; W: 5,000 rows, forced wide
    cnt = [pkg.RED_NONE if k == "X" else 5000 if k in "FW" else rows[k] for k in kinds]
    force = [pkg.RED_FORCE_FULL if k == "F" else pkg.RED_FORCE_WIDE if k == "W" else 0 for k in kinds]
    plan = pkg.red_plan_host(100000, 100, 2, False, cnt, force=force)
    assert plan["verdict"] == pkg.RED_USE
    where = lambda ks: [b for b, k in enumerate(kinds) if k in ks]
    by_config = [(index_of(plan, 64, 3, False), where("a")), (index_of(plan, 64, 5, False), where("b")), (index_of(plan, 512, 5, True), where("c")),
                 (index_of(plan, 512, 15, True), where("d")), (index_of(plan, 1024, 7, True), where("W"))]
    assert [cf for cf, _ in by_config] == sorted(cf for cf, _ in by_config) and len(by_config) >= 3
    listed, full = where("abcdFW"), where("XF")
    assert plan["blocks"].tolist() == listed + sum((blocks for _, blocks in by_config), []) + full
    assert plan["listed"] == len(listed) and plan["full_at"] == len(listed) + len(where("abcdW")) and plan["nfull"] == len(full) == 3
    at, want_bins = len(listed), []
    for cf, blocks in by_config:
        want_bins.append((cf, at, len(blocks)))
        at += len(blocks)
    assert plan["bins"] == want_bins
    for first, count in [(0, plan["listed"])] + [(f, n) for _, f, n in plan["bins"]] + [(plan["full_at"], plan["nfull"])]:
        stretch = plan["blocks"][first:first + count].tolist()
        assert stretch == sorted(set(stretch)), (first, count)
    assert plan["max_rows"] == 5000 and plan["reduced_blocks"] == len(kinds) - 3
    assert plan["rows_mean"] == sum(cnt[b] for b in where("abcdW")) // (len(kinds) - 3)


# ---- refusals: everything an index is formed from

@pytest.mark.parametrize("what, kw", [
    ("b_lo > b_hi", dict(b_lo=3, b_hi=2)),
    ("b_hi > nblocks", dict(b_hi=5)),
    ("a count above m", dict(cnt=[10, 10, 1001, 10])),
    ("a force mark above 2", dict(force=[0, 3, 0, 0])),
    ("no rows", dict(m=0)),
    ("no columns in a block", dict(B=0)),
    ("3 bits a symbol", dict(bits=3)),
])
def test_refusals(pkg, what, kw):
    args = dict(m=1000, B=100, bits=2, direct=True, cnt=[10, 10, 10, 10])
    assert pkg.red_plan_host(**args)["verdict"] == pkg.RED_USE      # (the call below differs from one that is taken in one thing)
    args.update(kw)
    with pytest.raises(pkg.FseqError) as e:
        pkg.red_plan_host(**args)
    assert e.value.code == pkg.FSEQ_E_ARG, what


def test_counts_at_the_bounds_are_taken(pkg):
    """... and the values on the permitted side of every rule: a count of m, RED_NONE, the marks 0 to 2, an empty range, no block."""
    plan = pkg.red_plan_host(1000, 100, 2, True, [1000, pkg.RED_NONE, 0, 10], force=[0, 1, 2, 0], b_lo=4, b_hi=4)
    assert plan["verdict"] == pkg.RED_DECLINED and len(plan["blocks"]) == 0      # (a rank without blocks has nothing to reduce)
    assert pkg.red_plan_host(1000, 100, 2, True, [])["verdict"] == pkg.RED_DECLINED


def test_planner_under_the_sanitizers(tmp_path):
    """The header is host-only: tests/red_plan_sanitized.cpp includes it alone and runs the decline rule, a rank's range and the layout
    as a program of its own under AddressSanitizer and UndefinedBehaviorSanitizer (nothing loaded into Python runs under either)."""
    here = os.path.dirname(os.path.abspath(__file__))
    exe = str(tmp_path / "red_plan_sanitized")
    subprocess.run(["g++", "-std=c++17", "-g", "-O1", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", os.path.join(os.path.dirname(here), "founder-sequences_amd", "csrc"), os.path.join(here, "red_plan_sanitized.cpp"), "-o", exe], check=True)
    p = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=60)
    assert p.returncode == 0, p.stderr[-3000:]
