"""The segments file in source co-ordinates (fseq_get_segments_restored, fseq_write_segments_restored; the restored forms of
k_segfile_lines / k_segfile_write, csrc/fseq_segfile.hpp).

The yardstick of every file is tests/segments_restored_cases.py's restore_file: the bytes fseq_write_segments_device wrote on the
same context -- which tests/test_gpu_segments_device.py pins to the host writer -- with LB / RB replaced by the numpy model's
source bounds and every substring by the source row's bytes over that range.  The inputs are alignments without identity columns
into which runs of identity columns are inserted at places chosen relative to the segment borders a plain run finds, so the kept
columns are known exactly and every test asserts that the library finds these."""
import importlib

import numpy as np
import pytest

import segments_restored_cases as cases
from test_gpu_input_stream import run_cli, write_list
from test_gpu_segments_device import packed

pytestmark = pytest.mark.gpu

HEADER_COPIES = b"SEGMENT\tLB\tRB\tSIZE\tSUBSEQUENCE_NUMBER\tCOPY_NUMBER\tSUBSEQUENCE\n"


@pytest.fixture(scope="module")
def pkg():
    return importlib.import_module("founder-sequences_amd")


def plain_segments(pkg, R, L):
    """(lb, rb, segment_size) of a plain context's run on R."""
    ctx = pkg.SegmentationContext(R.shape[0], R.shape[1], L)
    ctx.set_sequences(np.ascontiguousarray(R))
    ctx.run()
    red = ctx.reduced_traceback()
    ctx.close()
    assert len(red) > 1
    return red["lb"].astype(np.int64), red["rb"].astype(np.int64), red["segment_size"].copy()


def reduced_context(pkg, full, kept, L, tuning=(), **kw):
    """The context over the kept columns of `full`, run; the library must find exactly `kept`."""
    src = pkg.SegmentationContext(full.shape[0], full.shape[1], L)
    src.set_sequences(np.ascontiguousarray(full), **kw)
    ctx = src.without_identity_columns(L)
    src.close()
    assert ctx.source_n == full.shape[1] and np.array_equal(ctx.kept_columns().astype(np.int64), kept)
    for name, value in tuning:
        ctx.set_tuning(name, value)
    ctx.run()
    return ctx


def check_stats(ctx, blob):
    st = ctx.segments_file_stats()
    lines = cases.data_lines(blob)
    assert st["bytes"] == len(blob) and st["lines"] == len(lines) and st["longest_line"] == max(len(x) for x in lines) + 1, st
    return st


def same_bytes(got, want, what):
    if got != want:
        a, b = cases.data_lines(want), cases.data_lines(got)
        first = next((i for i in range(min(len(a), len(b))) if a[i] != b[i]), min(len(a), len(b)))
        raise AssertionError("%s: %d / %d lines, first difference at line %d:\n%r\n%r" % (what, len(a), len(b), first, a[first:first + 1], b[first:first + 1]))


def check_files(pkg, ctx, full, kept, tmp_path, tag="f", segments=None):
    """Both joinings: the restored file is restore_file of the reduced writer's; the stats fit it; segments_restored() is the
    model.  segments: (lb, rb) a plain run on the kept columns found, which this context must find too.  Returns
    ({joining: restored bytes}, src_lb, src_rb, kept widths)."""
    red = ctx.reduced_traceback()
    lb, rb = red["lb"].astype(np.int64), red["rb"].astype(np.int64)
    assert len(red) > 1
    if segments is not None:
        assert np.array_equal(lb, segments[0]) and np.array_equal(rb, segments[1])
    src_lb, src_rb = cases.restored_bounds(kept, full.shape[1], lb, rb)
    got_seg = ctx.segments_restored()
    assert np.array_equal(got_seg["lb"], src_lb) and np.array_equal(got_seg["rb"], src_rb)
    assert np.array_equal(got_seg["segment_size"], red["segment_size"])
    out = {}
    for joining in (pkg.JOIN_BIPARTITE, pkg.JOIN_RANDOM):
        d, r = str(tmp_path / ("%s_reduced%d.txt" % (tag, joining))), str(tmp_path / ("%s_restored%d.txt" % (tag, joining)))
        ctx.write_segments_device(joining, d)
        ctx.write_segments_restored(joining, r)
        got = open(r, "rb").read()
        want = cases.restore_file(open(d, "rb").read(), full, kept, joining)
        assert want.count(b"\n") > 1
        same_bytes(got, want, "%s, joining %d" % (tag, joining))
        check_stats(ctx, got)
        out[joining] = got
    return out, src_lb.astype(np.int64), src_rb.astype(np.int64), rb - lb


# ---- where a run stands

@pytest.fixture(scope="module")
def base(pkg):
    """m = 203, about 600 columns, X = 8, L = 20: R and the segments of a plain run on it."""
    R = cases.mosaic_without_identity(8, 203, 600, seed=21)
    lb, rb, _ = plain_segments(pkg, R, 20)
    return R, lb, rb


PLACEMENTS = ["leading", "trailing", "on a border", "behind a border's first kept column", "between every two kept columns", "none"]


@pytest.mark.parametrize("where", PLACEMENTS)
def test_run_placement(pkg, tmp_path, base, where):
    R, lb, rb = base
    n = R.shape[1]
    b = int(rb[0])                                              # the first kept column of segment 1
    runs = {"leading": {0: 37}, "trailing": {n: 41}, "on a border": {b: 30}, "behind a border's first kept column": {b + 1: 30},
            "between every two kept columns": {p: 1 for p in range(1, n)}, "none": {}}[where]
    full, kept = cases.with_identity_runs(R, runs)
    ctx = reduced_context(pkg, full, kept, 20)
    out, src_lb, src_rb, _ = check_files(pkg, ctx, full, kept, tmp_path, segments=(lb, rb))
    first = [x.split(b"\t") for x in cases.data_lines(out[pkg.JOIN_BIPARTITE])[1:]]
    if where == "leading":
        assert kept[0] == 37 and src_lb[0] == 0 and src_rb[0] == 37 + kept[b] - kept[0]
        assert all(f[4].startswith(full[0, :37].tobytes()) for f in first if f[0] == b"0")
    elif where == "trailing":
        assert kept[-1] == n - 1 and src_rb[-1] == n + 41
        assert all(f[4].endswith(full[0, n:].tobytes()) for f in first if int(f[0]) == len(lb) - 1)
    elif where == "on a border":
        # the run stands behind segment 0's last kept column: its columns show up in the left segment's lines
        assert src_rb[0] == b + 30 == src_lb[1] and kept[b] == b + 30
        assert all(f[4].endswith(full[0, b:b + 30].tobytes()) and len(f[4]) == b + 30 for f in first if f[0] == b"0")
        assert all(len(f[4]) == rb[1] - lb[1] for f in first if f[0] == b"1")
    elif where == "behind a border's first kept column":
        assert src_rb[0] == b == src_lb[1] and kept[b] == b and kept[b + 1] == b + 31
        assert all(f[4][1:31] == full[0, b + 1:b + 31].tobytes() and len(f[4]) == rb[1] - lb[1] + 30 for f in first if f[0] == b"1")
    elif where == "between every two kept columns":
        assert np.array_equal(kept, 2 * np.arange(n)) and full.shape[1] == 2 * n - 1
    else:
        # no identity column at all: the restored file is the reduced writer's, byte for byte
        assert full.shape[1] == n == ctx.n == ctx.source_n and np.array_equal(kept, np.arange(n))
        for joining in out:
            assert out[joining] == open(str(tmp_path / ("f_reduced%d.txt" % joining)), "rb").read()
    ctx.close()


# ---- widths around the 64 lanes of a wave

def test_source_widths_around_a_wave_and_both_orders_of_the_pass_lengths(pkg, tmp_path):
    """Segments of about 50 kept columns (blocks of 50), padded inside -- behind their first kept column -- to source widths
    below 64, exactly 64, 65 and exactly 128: the pass over the source positions ends inside its first round of 64 lanes, at its
    end, one lane into the second and at the end of the second.  In the padded segments the kept width is below 64 and the
    source width is 64 or above (the pass over the kept columns is the shorter one); the other order -- more than 64 kept columns,
    fewer than 64 identity columns to store -- is test_kept_width_above_a_wave's."""
    R = cases.mosaic_without_identity(8, 203, 600, brec=50, seed=21)
    lb, rb, _ = plain_segments(pkg, R, 20)
    w = rb - lb
    assert len(w) >= 5 and (w[1:5] < 64).all()
    targets = {1: 64, 2: 65, 3: 128}                            # segment -> source width; segment 4 stays below 64
    runs = {int(lb[s]) + 1: t - int(w[s]) for s, t in targets.items()}
    full, kept = cases.with_identity_runs(R, runs)
    ctx = reduced_context(pkg, full, kept, 20)
    _, src_lb, src_rb, kw = check_files(pkg, ctx, full, kept, tmp_path, segments=(lb, rb))
    sw = src_rb - src_lb
    assert [int(sw[s]) for s in (1, 2, 3)] == [64, 65, 128] and sw[4] < 64 and (sw < 64).any()
    assert kw[2] < 64 < sw[2] and kw[3] < 64 < sw[3]
    ctx.close()


def test_kept_width_above_a_wave(pkg, tmp_path, base):
    """About 100 kept columns a segment and 10 identity columns inside one: the pass over the kept columns takes two rounds of the
    wave, the identity columns fewer than 64 stores."""
    R, lb, rb = base
    full, kept = cases.with_identity_runs(R, {int(lb[2]) + 5: 10})
    ctx = reduced_context(pkg, full, kept, 20)
    _, src_lb, src_rb, kw = check_files(pkg, ctx, full, kept, tmp_path, segments=(lb, rb))
    assert kw[2] > 64 and src_rb[2] - src_lb[2] == kw[2] + 10
    ctx.close()


# ---- one long run, small batches

def test_one_long_run(pkg, tmp_path):
    """70,000 identity columns inside segment 2 of twelve.  With FSEQ_SEGFILE_BATCH = 4096 every line of that segment is a batch of
    its own and the batches of the other segments are cut inside segments; with the plain budget the file leaves in one batch."""
    R = cases.mosaic_without_identity(8, 203, 1200, seed=2)
    lb, rb, _ = plain_segments(pkg, R, 20)
    assert len(lb) >= 8
    full, kept = cases.with_identity_runs(R, {int(lb[2]) + 3: 70000})
    ctx = reduced_context(pkg, full, kept, 20)
    plain, src_lb, src_rb, _ = check_files(pkg, ctx, full, kept, tmp_path, tag="plain", segments=(lb, rb))
    assert src_rb[2] - src_lb[2] == rb[2] - lb[2] + 70000 and ctx.segments_file_stats()["batches"] == 1
    ctx.set_tuning("FSEQ_SEGFILE_BATCH", 4096)
    ctx.run()
    for joining in (pkg.JOIN_BIPARTITE, pkg.JOIN_RANDOM):
        path = str(tmp_path / ("small%d.txt" % joining))
        ctx.write_segments_restored(joining, path)
        got = open(path, "rb").read()
        same_bytes(got, plain[joining], "budget 4096, joining %d" % joining)
        st = check_stats(ctx, got)
        lines = cases.data_lines(got)[1:]
        lengths = [len(x) + 1 for x in lines]
        segment_of = [int(x.split(b"\t")[0]) for x in lines]
        expect = packed(lengths, 4096)
        assert st["batches"] == len(expect), (joining, st, len(expect))
        assert st["longest_line"] > 70000
        assert all(count == 1 for first, count in expect if segment_of[first] == 2) and sum(1 for s in segment_of if s == 2) >= 2
        assert any(first and segment_of[first] == segment_of[first - 1] != 2 for first, _ in expect)
        assert any(count > 1 for _, count in expect)
    ctx.close()


# ---- code widths, a partial last byte

ALPHABETS = {2: b"ACGT", 4: b"ACGTNRYKMSWBDHV-", 8: bytes(range(48, 88))}


@pytest.mark.parametrize("m", [5, 65, 203])
@pytest.mark.parametrize("bits", [2, 4, 8])
def test_code_widths_and_a_partial_last_byte(pkg, tmp_path, bits, m):
    """4, 16 and 40 symbols: 2, 4 and 8 bits a code; m = 5, 65 and 203 are no multiples of 4, so the last byte of a packed column
    is partial at 2 and 4 bits (203 and 5, 65 at 4 bits: odd)."""
    alphabet = ALPHABETS[bits]
    R = cases.mosaic_without_identity(2 if m == 5 else 8, m, 400, brec=50, seed=bits + m, alphabet=alphabet)
    assert len(np.unique(R)) == len(alphabet)
    n = R.shape[1]
    full, kept = cases.with_identity_runs(R, {0: 3, n // 3: 70, n // 2: 1, n: 9})
    assert len(np.unique(full)) == len(alphabet)
    ctx = reduced_context(pkg, full, kept, 20)
    check_files(pkg, ctx, full, kept, tmp_path)
    ctx.close()


def test_identity_columns_with_a_byte_of_their_own(pkg, tmp_path, base):
    """The identity columns carry '#', which no kept column has: the byte comes from the reference row alone, and it is the
    alphabet's fifth symbol (4 bits a code where the kept columns alone would take 2)."""
    R, lb, rb = base
    assert ord("#") not in np.unique(R)
    full, kept = cases.with_identity_runs(R, {0: 5, int(rb[1]): 66, int(lb[3]) + 7: 20, R.shape[1]: 2}, byte_of=lambda p: ord("#"))
    ctx = reduced_context(pkg, full, kept, 20)
    out, _, _, _ = check_files(pkg, ctx, full, kept, tmp_path, segments=(lb, rb))
    assert all(out[j].count(b"#") > 0 for j in out)
    ctx.close()


# ---- how full a segment is

def test_segment_fullness(pkg, tmp_path):
    """founder_mosaic's blocks use subsets of the founders: full segments and segments with fewer classes than slots both occur
    (placeholders and sorted texts in the bipartite file).  The smallest segments: a context made by
    without_identity_columns() has no segment of one class -- all rows equal over a segment's kept columns would make each of
    them an identity column, which is not kept -- so the smallest case there is runs on a context whose every segment has two."""
    R = cases.mosaic_without_identity(8, 203, 1200, seed=2)
    n = R.shape[1]
    full, kept = cases.with_identity_runs(R, {0: 11, n // 4: 80, n // 2: 130, n - 1: 7})
    ctx = reduced_context(pkg, full, kept, 20)
    sz = ctx.reduced_traceback()["segment_size"]
    assert ctx.result.max_segment_size == 8 and (sz == 8).any() and (sz < 8).any()
    out, _, _, _ = check_files(pkg, ctx, full, kept, tmp_path)
    copied = [x.split(b"\t")[6] for x in cases.data_lines(out[pkg.JOIN_BIPARTITE])[1:]]
    assert b"-" in copied and any(x != b"-" for x in copied)
    ctx.close()
    R = cases.mosaic_without_identity(2, 70, 600, seed=3)
    n = R.shape[1]
    full, kept = cases.with_identity_runs(R, {0: 4, n // 2: 90, n: 4})
    ctx = reduced_context(pkg, full, kept, 20)
    assert ctx.result.max_segment_size == 2 and (ctx.reduced_traceback()["segment_size"] == 2).all()
    check_files(pkg, ctx, full, kept, tmp_path, tag="two")
    ctx.close()


# ---- other ways to a context

def test_streamed_input(pkg, tmp_path):
    R = cases.mosaic_without_identity(16, 300, 3000, seed=4)
    n = R.shape[1]
    full, kept = cases.with_identity_runs(R, {0: 100, n // 3: 1500, 2 * n // 3: 63, n: 400})
    assert full.size > (1 << 20)                                # more than one chunk of staging
    ctx = reduced_context(pkg, full, kept, 20, staging_bytes=1 << 20)
    check_files(pkg, ctx, full, kept, tmp_path)
    ctx.close()


def test_held_out_context(pkg, tmp_path, base):
    """without_rows() then without_identity_columns(keep_held_out=True): the identity columns are those of the kept rows, in which
    the held-out rows may differ; the file describes the kept rows."""
    R, lb, rb = base
    full, kept = cases.with_identity_runs(R, {0: 9, int(rb[0]): 70, int(lb[3]) + 2: 33, R.shape[1]: 5})
    rng = np.random.default_rng(8)
    held = [0, 17, 205]
    everything = np.empty((full.shape[0] + len(held), full.shape[1]), dtype=np.uint8)
    mine = np.ones(len(everything), dtype=bool)
    mine[held] = False
    everything[mine] = full
    everything[~mine] = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, size=(len(held), full.shape[1]))]
    src = pkg.SegmentationContext(everything.shape[0], everything.shape[1], 20)
    src.set_sequences(everything)
    sub = src.without_rows(held, 20)
    src.close()
    ctx = sub.without_identity_columns(20, keep_held_out=True)
    sub.close()
    assert np.array_equal(ctx.kept_columns().astype(np.int64), kept) and ctx.m == full.shape[0]
    ctx.run()
    check_files(pkg, ctx, full, kept, tmp_path, segments=(lb, rb))
    ctx.close()


def test_set_segment_length(pkg, tmp_path, base):
    R, lb, rb = base
    full, kept = cases.with_identity_runs(R, {0: 9, int(rb[0]): 70, int(lb[3]) + 2: 33, R.shape[1]: 5})
    ctx = reduced_context(pkg, full, kept, 20)
    one, _, _, _ = check_files(pkg, ctx, full, kept, tmp_path, tag="L20", segments=(lb, rb))
    ctx.set_segment_length(150)
    with pytest.raises(pkg.FseqError) as err:
        ctx.write_segments_restored(pkg.JOIN_RANDOM, str(tmp_path / "stale.txt"))
    assert err.value.code == pkg.FSEQ_E_ARG and not (tmp_path / "stale.txt").exists()
    ctx.run()
    assert ctx.result.segment_count != len(lb)
    two, _, _, _ = check_files(pkg, ctx, full, kept, tmp_path, tag="L150")
    assert all(one[j] != two[j] for j in one)
    ctx.close()


def test_writers_in_a_row(pkg, tmp_path, base):
    """Reduced, restored, reduced again on one context: each file is what it is alone, and the stats follow the last call."""
    R, lb, rb = base
    full, kept = cases.with_identity_runs(R, {0: 9, int(rb[0]): 70, int(lb[3]) + 2: 33, R.shape[1]: 5})
    ctx = reduced_context(pkg, full, kept, 20)
    want, _, _, _ = check_files(pkg, ctx, full, kept, tmp_path, segments=(lb, rb))
    for joining in (pkg.JOIN_BIPARTITE, pkg.JOIN_RANDOM):
        reduced = open(str(tmp_path / ("f_reduced%d.txt" % joining)), "rb").read()
        for i, (writer, expect) in enumerate(((ctx.write_segments_device, reduced), (ctx.write_segments_restored, want[joining]),
                                              (ctx.write_segments_device, reduced))):
            path = str(tmp_path / ("row%d_%d.txt" % (joining, i)))
            writer(joining, path)
            got = open(path, "rb").read()
            same_bytes(got, expect, "joining %d, call %d" % (joining, i))
            assert check_stats(ctx, got)["bytes"] == len(expect)
        assert len(want[joining]) > len(reduced)
    ctx.close()


# ---- the two restored outputs fit each other

def test_restored_founders_are_the_restored_segments_rows(pkg, tmp_path, base):
    R, lb, rb = base
    full, kept = cases.with_identity_runs(R, {0: 9, int(rb[0]): 70, int(lb[3]) + 2: 33, R.shape[1]: 5})
    ctx = reduced_context(pkg, full, kept, 20)
    seg = ctx.segments_restored()
    assert seg["lb"][0] == 0 and seg["rb"][-1] == full.shape[1] and np.array_equal(seg["lb"][1:], seg["rb"][:-1])
    for name, perm in (("greedy", ctx.join_greedy()), ("bipartite", ctx.join_bipartite())):
        assert (perm < full.shape[0]).all()
        path = str(tmp_path / (name + ".txt"))
        ctx.write_founders_restored(perm, path)
        lines = cases.data_lines(open(path, "rb").read())
        assert len(lines) == ctx.result.max_segment_size
        for f, line in enumerate(lines):
            want = b"".join(full[perm[s][f], int(seg["lb"][s]):int(seg["rb"][s])].tobytes() for s in range(len(seg)))
            assert line == want, (name, f)
    ctx.close()


# ---- refusals

def test_refusals_leave_no_file_and_a_usable_context(pkg, tmp_path, base):
    R, lb, rb = base
    full, kept = cases.with_identity_runs(R, {0: 9, int(rb[0]): 70, R.shape[1]: 5})
    path = tmp_path / "s.txt"

    def refused(ctx, code, joining, where=None, word=None):
        with pytest.raises(pkg.FseqError) as err:
            ctx.write_segments_restored(joining, str(where or path))
        assert err.value.code == code and str(err.value) and (word is None or word in str(err.value)), str(err.value)
        assert not path.exists()

    # a plain context, before and after its run: the message of the other restored entries
    plain = pkg.SegmentationContext(full.shape[0], full.shape[1], 20)
    plain.set_sequences(full)
    for after_run in (False, True):
        if after_run:
            plain.run()
        for joining in (pkg.JOIN_GREEDY, pkg.JOIN_BIPARTITE, pkg.JOIN_RANDOM):
            refused(plain, pkg.FSEQ_E_ARG, joining, word="not a context made by fseq_create_without_identity_columns")
        with pytest.raises(pkg.FseqError) as err:
            plain.segments_restored()
        assert err.value.code == pkg.FSEQ_E_ARG and "not a context made by fseq_create_without_identity_columns" in str(err.value)
    ctx = plain.without_identity_columns(20)
    plain.close()
    # before a run
    for joining in (pkg.JOIN_GREEDY, pkg.JOIN_BIPARTITE, pkg.JOIN_RANDOM):
        refused(ctx, pkg.FSEQ_E_ARG, joining)
    with pytest.raises(pkg.FseqError) as err:
        ctx.segments_restored()
    assert err.value.code == pkg.FSEQ_E_ARG
    ctx.run()
    refused(ctx, pkg.FSEQ_E_ARG, 3)                             # an unknown joining
    refused(ctx, pkg.FSEQ_E_ARG, -1)
    for joining in (pkg.JOIN_GREEDY, pkg.JOIN_BIPARTITE, pkg.JOIN_RANDOM):
        refused(ctx, pkg.FSEQ_E_ARG, joining, where=tmp_path / "no" / "such" / "dir.txt")      # a path that cannot be opened
    check_files(pkg, ctx, full, kept, tmp_path, segments=(lb, rb))
    ctx.write_segments_restored(pkg.JOIN_GREEDY, str(tmp_path / "g.txt"))
    assert (tmp_path / "g.txt").read_bytes() == HEADER_COPIES
    st = ctx.segments_file_stats()
    assert st["batches"] == 0 and st["lines"] == 1 and st["bytes"] == len(HEADER_COPIES)
    ctx.close()
    # a short-path result: fewer than 2 L kept columns
    few, kept_few = cases.with_identity_runs(np.ascontiguousarray(R[:, 85:115]), {0: 9, 15: 70, 30: 5})      # (across a block border)
    short = reduced_context(pkg, few, kept_few, 20)
    assert short.result.short_path
    for joining in (pkg.JOIN_GREEDY, pkg.JOIN_BIPARTITE, pkg.JOIN_RANDOM):
        refused(short, pkg.FSEQ_E_ARG, joining, word="short path")
    with pytest.raises(pkg.FseqError) as err:
        short.segments_restored()
    assert err.value.code == pkg.FSEQ_E_ARG
    # ... and the same context writes a correct file after a long-path run
    short.set_segment_length(10)
    short.run()
    assert not short.result.short_path
    check_files(pkg, short, few, kept_few, tmp_path, tag="after")
    short.close()


# ---- the front end, in child processes

@pytest.fixture(scope="module")
def front_end_input(tmp_path_factory):
    R = cases.mosaic_without_identity(6, 65, 2300, brec=150, seed=31)
    n = R.shape[1]
    full, kept = cases.with_identity_runs(R, {0: 13, n // 2: 700, n // 2 + 200: 64, n: 21})
    tmp = tmp_path_factory.mktemp("restored")
    return tmp, write_list(tmp, full), full, kept


@pytest.mark.parametrize("joining", ["greedy", "bipartite-matching", "random"])
def test_front_end(pkg, front_end_input, joining):
    """--output-restored-segments beside --output-segments, which stays in reduced co-ordinates: the restored file is
    restore_file of the run's own reduced file and the input.  Greedy joining: the header alone.  Bipartite-matching joining
    under --upload-memory, where --output-segments is refused and no row is on the host: the same restored file."""
    cli = importlib.import_module("founder-sequences_amd.build").build_cli()
    tmp, lst, full, kept = front_end_input
    how = {"greedy": pkg.JOIN_GREEDY, "bipartite-matching": pkg.JOIN_BIPARTITE, "random": pkg.JOIN_RANDOM}[joining]
    base = ["--input", lst, "--segment-length-bound", "40", "--segment-joining", joining, "--random-seed", "7", "--remove-identity-columns"]
    got = run_cli(cli, tmp, joining, base, ["segments", "restored-segments", "identity-columns"])
    assert got["identity-columns"] == bytes(np.where(np.isin(np.arange(full.shape[1]), kept), ord("0"), ord("1")).astype(np.uint8)) + b"\n"
    assert len(cases.data_lines(got["founders"])[0]) == full.shape[1]
    if joining == "greedy":
        assert got["segments"] == got["restored-segments"] == HEADER_COPIES
        return
    want = cases.restore_file(got["segments"], full, kept, how)
    assert want.count(b"\n") > 1
    same_bytes(got["restored-segments"], want, joining)
    if joining == "bipartite-matching":
        chunks = run_cli(cli, tmp, joining + "-chunks", base + ["--upload-memory=1"], ["restored-segments"])
        same_bytes(chunks["restored-segments"], want, joining + ", --upload-memory")
        assert chunks["founders"] == got["founders"]
