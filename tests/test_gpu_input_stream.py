"""The input in column chunks (fseq_input_begin .. fseq_set_rows_streamed, csrc/fseq_input.hpp) against its specification
(tests/input_model.py) and against fseq_set_rows on the same rows.  Integer work: every comparison is exact.  Shapes sit at the
edges of k_input_encode's tiles (128 columns x 64 packed bytes = 256 / 128 / 64 rows), not at the workload's."""
import ctypes as C
import importlib
import os
import subprocess

import numpy as np
import pytest

import input_model as model

pytestmark = pytest.mark.gpu

ROWS = [1, 3, 15, 16, 17, 31, 33, 63, 64, 65, 127, 129, 257]
WIDTHS = [1, 15, 16, 17, 63, 64, 65, 100]
ALPHABETS = [1, 2, 4, 5, 16, 17, 256]
N, L = 300, 20
E_ARG, E_UNSUPPORTED = 1, 5


@pytest.fixture(scope="module")
def pkg():
    return importlib.import_module("founder-sequences_amd")


@pytest.fixture(scope="module")
def build():
    return importlib.import_module("founder-sequences_amd.build")


def pad16(x):
    return (x + 15) // 16 * 16


def staging_for(m, width):
    """two halves that hold exactly pad16(width) columns of m rows"""
    return 2 * m * pad16(width)


def outcome(pkg, ctx):
    """everything a run on the context's input gives, as comparable values"""
    try:
        res = ctx.run()
    except pkg.NoReduction:
        return ("no reduction",)
    if res.short_path:
        first, runs = ctx.short_path_runs()
        return ("short", res.max_segment_size, first.tolist(), runs.tolist())
    states = [tuple(x.tobytes() for x in ctx.boundary_state(i)) for i in range(res.segment_count)]
    return ("long", res.max_segment_size, ctx.traceback().tobytes(), ctx.reduced_traceback().tobytes(), states, ctx.join_greedy().tobytes())


def check_resident(pkg, ctx, msa, alphabet=None):
    assert np.array_equal(ctx.get_sequences(), msa)
    want, bits = model.packed_columns(pkg, msa, alphabet)
    got, got_bits = ctx.packed_columns()
    assert got_bits == bits and got.shape == want.shape
    assert np.array_equal(got, want)                          # (padding bytes and padding fields included: zero)


def feed(ctx, msa, width, scan=True):
    n = msa.shape[1]
    for c0 in range(0, n, width) if scan else []:
        ctx.input_scan(c0, msa[:, c0:c0 + width])
    for c0 in range(0, n, width):
        ctx.input_columns(c0, msa[:, c0:c0 + width])
    ctx.input_end()


_reference = {}


def reference(pkg, m, size, n=N):
    """the rows of a case and what fseq_set_rows gives on them: computed once, shared, not changed"""
    key = (m, size, n)
    if key not in _reference:
        msa = model.mosaic(7 * m + size, m, n, model.alphabet_bytes(size, m))
        msa.setflags(write=False)
        ctx = pkg.SegmentationContext(m, n, L)
        ctx.set_sequences(msa)
        _reference[key] = (msa, outcome(pkg, ctx))
        ctx.close()
    return _reference[key]


CASES = [(m, size, WIDTHS[(i + j) % len(WIDTHS)]) for i, m in enumerate(ROWS) for j, size in enumerate(ALPHABETS)]


def test_the_cases_cover_what_they_claim():
    assert {c[0] for c in CASES} == set(ROWS) and {c[1] for c in CASES} == set(ALPHABETS) and {c[2] for c in CASES} == set(WIDTHS)
    assert 1 in WIDTHS and any(N % w not in (0, 1) for w in WIDTHS)     # ragged last chunks, and a last chunk of a single column
    for size in ALPHABETS:
        assert size == 1 or max(model.alphabet_bytes(size, 3)) > 127


@pytest.mark.parametrize("m,size,width", CASES, ids=["m%d-s%d-w%d" % c for c in CASES])
def test_explicit_chunks(pkg, m, size, width):
    msa, want = reference(pkg, m, size)
    ctx = pkg.SegmentationContext(m, N, L)
    assert ctx.input_chunk_columns() == 0
    ctx.input_begin(staging_bytes=staging_for(m, width))
    assert ctx.input_chunk_columns() == pad16(width)         # floor(staging / 2 / m) in whole 16-byte pieces of a staged row
    feed(ctx, msa, width)
    assert ctx.input_chunk_columns() == 0
    check_resident(pkg, ctx, msa)
    assert outcome(pkg, ctx) == want
    ctx.close()


STREAMED = [(320, 1), (192, 2), (48, 7)]                      # chunk width of fseq_set_rows_streamed at the staging given, chunks of N columns


@pytest.mark.parametrize("m,size", [(m, ALPHABETS[i % len(ALPHABETS)]) for i, m in enumerate(ROWS)] + [(257, 2), (65, 16), (129, 256)])
def test_set_rows_streamed(pkg, m, size):
    msa, want = reference(pkg, m, size)
    for width, chunks in STREAMED:
        assert -(-N // width) == chunks
        ctx = pkg.SegmentationContext(m, N, L)
        ctx.set_sequences(msa, staging_bytes=staging_for(m, width))
        check_resident(pkg, ctx, msa)
        assert outcome(pkg, ctx) == want
        ctx.close()


def test_rows_that_are_not_one_matrix(pkg):
    """separately allocated rows (no constant step between them) go up row by row"""
    m, size = 65, 5
    msa, want = reference(pkg, m, size)
    rows = [np.array(msa[r]) for r in range(m)]
    rows[3], rows[40] = np.array(msa[3]), np.array(msa[40])   # (out of allocation order)
    ctx = pkg.SegmentationContext(m, N, L)
    ptrs = (C.c_void_p * m)(*[r.ctypes.data for r in rows])
    assert ctx.L.fseq_set_rows_streamed(ctx.h, ptrs, staging_for(m, 64)) == 0
    check_resident(pkg, ctx, msa)
    assert outcome(pkg, ctx) == want
    ctx.close()


def test_short_path(pkg):
    m, n = 33, 30
    msa, want = reference(pkg, m, 4, n)
    assert want[0] == "short"
    ctx = pkg.SegmentationContext(m, n, L)
    ctx.input_begin(staging_bytes=staging_for(m, 17))
    feed(ctx, msa, 17)
    check_resident(pkg, ctx, msa)
    assert outcome(pkg, ctx) == want
    ctx.close()


def test_supplied_alphabet_keeps_the_code_of_an_unused_byte(pkg):
    m = 65
    msa, want = reference(pkg, m, 4)
    used = bytes(np.unique(msa).tolist())
    unused = bytes([b for b in range(256) if b not in used and min(used) < b < max(used)][:1])
    alphabet = used[2:] + unused + used[:2]                  # any order
    assert model.code_table(msa, alphabet)[1:] == (5, 4) and model.code_table(msa)[1:] == (4, 2)
    ctx = pkg.SegmentationContext(m, N, L)
    ctx.input_begin(alphabet=alphabet, staging_bytes=staging_for(m, 100))
    feed(ctx, msa, 100, scan=False)
    check_resident(pkg, ctx, msa, alphabet)
    assert outcome(pkg, ctx) == want
    ctx.close()


def refused(pkg, call, code=E_ARG):
    with pytest.raises(pkg.FseqError) as ei:
        call()
    assert ei.value.code == code, ei.value
    return str(ei.value)


def test_call_order_refusals(pkg):
    m, width = 17, 64
    msa, want = reference(pkg, m, 4)
    ctx = pkg.SegmentationContext(m, N, L)
    chunk = lambda c0, w=width: msa[:, c0:c0 + w]
    # without a begin
    refused(pkg, lambda: ctx.input_scan(0, chunk(0)))
    refused(pkg, lambda: ctx.input_columns(0, chunk(0)))
    refused(pkg, lambda: ctx.input_end())
    # a staging too small for one column names the bytes needed; a duplicate in the alphabet
    assert "%d bytes needed" % (32 * m) in refused(pkg, lambda: ctx.input_begin(staging_bytes=32 * m - 1))
    refused(pkg, lambda: ctx.input_begin(alphabet=b"ACGA"))
    ctx.input_begin(staging_bytes=staging_for(m, width))
    refused(pkg, lambda: ctx.run())                           # (no input between begin and end)
    refused(pkg, lambda: ctx.input_columns(0, chunk(0)))      # before the scans have covered [0, n)
    refused(pkg, lambda: ctx.input_scan(64, chunk(64)))       # out of order
    refused(pkg, lambda: ctx.input_scan(0, chunk(0, 65)))     # wider than fseq_input_chunk_columns
    ctx.input_scan(0, chunk(0))
    refused(pkg, lambda: ctx.input_scan(0, chunk(0)))         # again
    refused(pkg, lambda: ctx.input_scan(32, chunk(32)))       # overlapping
    refused(pkg, lambda: ctx.input_scan(128, chunk(128)))     # gapped
    refused(pkg, lambda: ctx.input_columns(0, chunk(0)))      # scans incomplete
    refused(pkg, lambda: ctx.input_end())
    for c0 in range(64, N, width):
        ctx.input_scan(c0, chunk(c0))
    refused(pkg, lambda: ctx.input_scan(N - 1, chunk(N - 1)))  # behind the end
    refused(pkg, lambda: ctx.input_columns(64, chunk(64)))
    ctx.input_columns(0, chunk(0))
    refused(pkg, lambda: ctx.input_scan(0, chunk(0)))         # the code table is fixed
    refused(pkg, lambda: ctx.input_columns(0, chunk(0)))
    refused(pkg, lambda: ctx.input_columns(128, chunk(128)))
    refused(pkg, lambda: ctx.input_columns(64, msa[:, 64:]))  # wider than a chunk
    refused(pkg, lambda: ctx.input_end())                     # before column n has arrived
    refused(pkg, lambda: ctx.run())
    for c0 in range(64, N, width):
        ctx.input_columns(c0, chunk(c0))
    refused(pkg, lambda: ctx.input_columns(N - 1, chunk(N - 1)))
    ctx.input_end()
    refused(pkg, lambda: ctx.input_end())
    # every refusal left the pass where it was
    check_resident(pkg, ctx, msa)
    assert outcome(pkg, ctx) == want
    # a scan after an explicit alphabet; a begin on a context that holds an input and a result discards them
    ctx.input_begin(alphabet=bytes(np.unique(msa).tolist()), staging_bytes=staging_for(m, width))
    refused(pkg, lambda: ctx.input_scan(0, chunk(0)))
    refused(pkg, lambda: ctx.run())
    feed(ctx, msa, width, scan=False)
    assert outcome(pkg, ctx) == want
    ctx.close()


def test_byte_outside_a_supplied_alphabet(pkg):
    m = 33
    msa, want = reference(pkg, m, 4)
    alphabet = bytes(np.unique(msa).tolist())
    bad = np.array(msa)
    stray = [b for b in range(200, 256) if b not in alphabet][0]
    bad[m - 1, N - 1] = stray                                # the last cell of the last, ragged chunk
    ctx = pkg.SegmentationContext(m, N, L)
    ctx.input_begin(alphabet=alphabet, staging_bytes=staging_for(m, 64))
    for c0 in range(0, N, 64):
        ctx.input_columns(c0, bad[:, c0:c0 + 64])             # (no round trip per chunk: the chunks are accepted)
    message = refused(pkg, lambda: ctx.input_end())
    assert "0x%02X" % stray in message and "(%d)" % stray in message
    assert model.outside(bad, alphabet) == [stray]
    refused(pkg, lambda: ctx.run())                           # the context has no input
    assert ctx.device_bytes()[0] == 0
    ctx.set_sequences(msa)                                    # ... and takes a plain upload
    assert outcome(pkg, ctx) == want
    ctx.close()


def test_sharded_context_is_unsupported(pkg):
    import torch
    m, n = 300, 5000
    rows = np.zeros((m, 64), dtype=np.uint8)
    a = pkg.SegmentationContext(m, n, 10)
    words = int(a.L.fseq_shard_xbuf_words(a.h, 2))
    xbuf = torch.zeros(words + 64, dtype=torch.int32, device="cuda:0")
    a.set_shard(0, 2, xbuf.data_ptr(), xbuf.numel(), lambda off, cnt, op: 0)
    refused(pkg, lambda: a.input_begin(), E_UNSUPPORTED)
    refused(pkg, lambda: a.set_sequences(np.zeros((m, n), dtype=np.uint8), staging_bytes=1 << 20), E_UNSUPPORTED)
    b = pkg.SegmentationContext(m, n, 10)
    b.input_begin(staging_bytes=staging_for(m, 64))
    b.set_shard(0, 2, xbuf.data_ptr(), xbuf.numel(), lambda off, cnt, op: 0)      # (no input yet: the shard is accepted)
    refused(pkg, lambda: b.input_scan(0, rows), E_UNSUPPORTED)
    refused(pkg, lambda: b.input_columns(0, rows), E_UNSUPPORTED)
    refused(pkg, lambda: b.input_end(), E_UNSUPPORTED)
    a.close()
    b.close()


def test_device_memory_stays_within_the_packed_alignment_and_the_staging(pkg):
    MiB = 1 << 20
    m, n = 2048, 65536                                       # 128 MiB raw, 32 MiB packed at 2 bits
    rng = np.random.default_rng(5)
    msa = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, size=(m, n), dtype=np.uint8)]
    ctx = pkg.SegmentationContext(m, n, 50)
    assert ctx.device_bytes() == (0, 0)
    ctx.set_sequences(msa, staging_bytes=8 * MiB)
    now, peak = ctx.device_bytes(reset_peak=True)
    print("streamed: %.2f MiB held, peak %.2f MiB" % (now / MiB, peak / MiB))
    assert peak <= (32 + 8 + 1) * MiB
    assert 32 * MiB <= now <= 32 * MiB + 4096                 # after the end the staging is released
    got, bits = ctx.packed_columns(n - 70, n)
    assert bits == 2 and np.array_equal(got, model.packed_columns(pkg, msa[:, n - 70:], b"ACGT")[0])
    assert np.array_equal(ctx.get_sequences(12345, 12500), msa[:, 12345:12500])
    ctx.close()
    # the accessor sees the difference: the same rows through fseq_set_rows hold the raw bytes beside the packed ones
    ctx = pkg.SegmentationContext(m, n, 50)
    ctx.set_sequences(msa)
    now, peak = ctx.device_bytes()
    print("fseq_set_rows: %.2f MiB held, peak %.2f MiB" % (now / MiB, peak / MiB))
    assert peak >= 128 * MiB and now <= 32 * MiB + 4096
    ctx.close()


# ---- the front end
def write_list(tmp_path, msa):
    src = tmp_path / "in"
    src.mkdir()
    names = []
    for i, row in enumerate(msa):
        (src / ("s%d" % i)).write_bytes(row.tobytes())
        names.append(str(src / ("s%d" % i)))
    (tmp_path / "list.txt").write_text("\n".join(names) + "\n")
    return str(tmp_path / "list.txt")


def run_cli(cli, tmp_path, tag, args, outputs):
    out = tmp_path / tag
    out.mkdir()
    cmd = [cli] + args + ["--output-founders", str(out / "founders")]
    for name in outputs:
        cmd += ["--output-" + name, str(out / name)]
    r = subprocess.run(cmd, capture_output=True, timeout=300)
    assert r.returncode == 0, r.stderr.decode()
    return {name: (out / name).read_bytes() for name in ["founders"] + list(outputs)}


@pytest.fixture(scope="module")
def front_end_input(tmp_path_factory):
    m, n = 65, 5000
    msa = np.array(model.mosaic(11, m, n, b"ACGT", founders=4, brec=150))
    msa[:, 1200:1900] = msa[0, 1200:1900]                    # a planted run of identity columns
    tmp = tmp_path_factory.mktemp("upload")
    return tmp, write_list(tmp, msa)


@pytest.mark.parametrize("joining", ["greedy", "bipartite-matching", "random"])
def test_front_end_writes_the_same_founders(build, front_end_input, joining):
    cli = build.build_cli()
    tmp, lst = front_end_input
    base = ["--input", lst, "--segment-length-bound", "40", "--segment-joining", joining, "--random-seed", "7"]
    variants = [("identity", ["--remove-identity-columns"], ["identity-columns", "restored-matches"]), ("matches", [], ["matches"])]
    for tag, extra, outputs in variants:
        want = run_cli(cli, tmp, "%s-%s-whole" % (joining, tag), base + extra, outputs)
        got = run_cli(cli, tmp, "%s-%s-chunks" % (joining, tag), base + extra + ["--upload-memory=1"], outputs)
        assert len(want["founders"]) > 5000 and got == want, tag


def test_front_end_segments_header_with_greedy_joining(build, front_end_input):
    cli = build.build_cli()
    tmp, lst = front_end_input
    base = ["--input", lst, "--segment-length-bound", "40", "--segment-joining", "greedy"]
    want = run_cli(cli, tmp, "seg-whole", base, ["segments"])
    got = run_cli(cli, tmp, "seg-chunks", base + ["--upload-memory", "1"], ["segments"])
    assert got == want and want["segments"]


def test_front_end_short_path(build, tmp_path):
    cli = build.build_cli()
    msa = model.mosaic(3, 65, 70, b"ACGT", founders=3, brec=70, flip=0.0)
    lst = write_list(tmp_path, msa)
    base = ["--input", lst, "--segment-length-bound", "40"]
    want = run_cli(cli, tmp_path, "whole", base, ["matches"])
    got = run_cli(cli, tmp_path, "chunks", base + ["--upload-memory", "1"], ["matches"])
    assert got == want and want["founders"].count(b"\n") == 3
