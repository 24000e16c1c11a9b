"""Identity columns on the device (fseq_identity_columns .. fseq_write_founders_restored, csrc/fseq_identity.hpp) against
their specification (tests/identity_model.py, pinned to the host tools by tests/test_identity_abi.py).  Integer work: every
comparison is exact."""
import importlib
import os
import subprocess

import numpy as np
import pytest

import identity_model as im
from helpers import founder_mosaic

pytestmark = pytest.mark.gpu

BITS = {2: 2, 4: 2, 16: 4, 40: 8}                                 # 2-, 2-, 4- and 8-bit packing
TILE = 2048                                                       # ID_TILE of csrc/fseq_identity.hpp: columns per workgroup of the scan


@pytest.fixture(scope="module")
def pkg():
    return importlib.import_module("founder-sequences_amd")


@pytest.fixture(scope="module")
def build():
    return importlib.import_module("founder-sequences_amd.build")


def lane_class(m, sigma):
    """id_shape of csrc/fseq_identity.hpp: lanes per column by the column's 16-byte chunks"""
    per = 8 // BITS[sigma]
    chunks = ((m + per - 1) // per + 15) // 16
    if chunks > 1024:
        return "workgroup"
    if chunks > 64:
        return "wave"
    g = 1
    while g < chunks:
        g *= 2
    return "G%d" % g


def borrowed_packed(pkg, codes, sigma, L=5, pad=0, garbage=False):
    """A context over codes handed over as packed device columns (the code width is the caller's, not the alphabet's)."""
    import torch
    m, n = codes.shape
    bits = BITS[sigma]
    packed, ld = pkg.pack_columns(codes, bits)
    if pad or garbage:
        per = 8 // bits
        col_bytes = (m + per - 1) // per
        wide = np.zeros((n, ld + pad), dtype=np.uint8)
        wide[:, :ld] = packed
        if garbage:
            wide[:, col_bytes:] = 0xFF
            tail = m % per
            if tail:
                wide[:, col_bytes - 1] |= (0xFF << (tail * bits)) & 0xFF
        packed, ld = wide, ld + pad
    dev = torch.from_numpy(np.ascontiguousarray(packed)).to("cuda")
    ctx = pkg.SegmentationContext(m, n, L)
    ctx.set_device_columns_packed(dev.data_ptr(), ld, sigma, bits, keepalive=dev)
    return ctx


SIGMAS = [2, 4, 16, 40]
# 1 .. 16385: around rows per byte, per 16-byte load, per wave iteration, per workgroup iteration; 129 .. 1025 and (with 8-bit codes)
# 17, 33, 65, 16385: one above every boundary of the mapping of lanes to columns (1, 2, 4 .. 64 lanes, a wave, a workgroup);
# 65537 and 262145: a workgroup per column at 4 and 2 bits
ROWS = [1, 2, 3, 4, 5, 15, 16, 17, 31, 33, 63, 64, 65, 4095, 4096, 4097, 16385, 129, 257, 513, 1025, 65537, 262145]
COLUMNS = [1, 2, 63, 64, 65, 1003, TILE - 1, TILE, TILE + 1, 3 * TILE + 5]


def differential_cases():
    """Every (lane class, n) pair once; within a class the (m, sigma) that fall into it take turns, so that every listed m and
    sigma occurs.  A pair of more than 40 M cells is left to a smaller m of its class (host time, not device time)."""
    by_class = {}
    for m in ROWS:
        for sigma in SIGMAS:
            by_class.setdefault(lane_class(m, sigma), []).append((m, sigma))
    cases = []
    for cls in sorted(by_class):
        members = by_class[cls]
        # the rows not seen in another class yet first, widest codes first (they put the boundaries of the mapping at the listed rows)
        turn = 0
        for n in COLUMNS:
            seen = {c[1] for c in cases}
            order = sorted(members, key=lambda ms: (ms[0] in seen, -BITS[ms[1]], members.index(ms)))
            fit = [ms for ms in order if ms[0] * n <= 40e6] or [min(members)]
            m, sigma = fit[0] if fit[0][0] not in seen else fit[turn % len(fit)]
            turn += 1
            cases.append((cls, m, sigma, n))
    return cases


CASES = differential_cases()


def test_the_cases_cover_what_they_claim():
    classes = ["G1", "G2", "G4", "G8", "G16", "G32", "G64", "wave", "workgroup"]
    assert sorted({(c[0], c[3]) for c in CASES}) == sorted((k, n) for k in classes for n in COLUMNS) and len(CASES) == len(classes) * len(COLUMNS)
    assert {c[1] for c in CASES} == set(ROWS) and {c[2] for c in CASES} == set(SIGMAS)
    for cls, m, sigma, n in CASES:
        assert lane_class(m, sigma) == cls
    # one row count just above every boundary of the mapping, at the code width that puts the boundary there
    above = {(m, sigma) for _, m, sigma, _ in CASES}
    for m in (17, 33, 65, 129, 257, 513, 1025, 16385):
        assert (m, 40) in above, m


@pytest.mark.parametrize("cls,m,sigma,n", CASES, ids=["%s-m%d-s%d-n%d" % c for c in CASES])
def test_mask_differential(pkg, cls, m, sigma, n):
    codes = im.random_case(m * 31 + n, m, n, sigma, 0.6, codes=True)
    want = im.identity_mask(codes)
    ctx = borrowed_packed(pkg, codes, sigma)
    mask, s = ctx.identity_columns()
    print("%s m=%d sigma=%d n=%d: %d identity columns (model %d), %.3f ms" % (cls, m, sigma, n, s["identity"], want.sum(), s["ms_device"]))
    assert np.array_equal(mask, want)
    assert (s["n"], s["identity"], s["kept"]) == (n, int(want.sum()), n - int(want.sum()))
    if not want.all() and m * n <= 4e6:
        red = ctx.without_identity_columns(5)
        ctx.close()                                               # (the new context stands alone)
        assert np.array_equal(red.kept_columns(), np.flatnonzero(~want))
        assert np.array_equal(red.identity_mask(), want)
        assert np.array_equal(red.get_sequences(), codes[:, ~want])
        red.close()
    else:
        ctx.close()


NEEDLES = [(2, 70), (4, 37), (16, 100), (40, 100), (4, 4101), (16, 2500), (40, 1100), (40, 16500), (2, 70001)]


@pytest.mark.parametrize("sigma,m", NEEDLES)
def test_needle(pkg, sigma, m):
    """All columns identity columns except that in chosen columns exactly one row differs: row 0, 1, m - 1 and every row that
    is the last of its byte, its 16-byte load, its wave iteration (1 KiB) or its workgroup iteration (4 KiB), and the row behind."""
    per = 8 // BITS[sigma]
    rows = {0, 1, m - 1, m - 2}
    for unit in (per, 16 * per, 1024 * per, 4096 * per):
        for k in (1, 2, (m - 1) // unit):
            rows |= {k * unit - 1, k * unit}
    rows = sorted(r for r in rows if 0 <= r < m)
    n = 3 * len(rows) + 2
    at = {3 * i + 1: r for i, r in enumerate(rows)}
    codes = im.needle_case(m, n, sigma, at, seed=m, codes=True)
    want = np.ones(n, dtype=bool)
    want[list(at)] = False
    assert np.array_equal(im.identity_mask(codes), want)
    ctx = borrowed_packed(pkg, codes, sigma)
    mask, s = ctx.identity_columns()
    assert np.array_equal(mask, want), [at[k] for k in np.flatnonzero(mask != want)]
    assert s["kept"] == len(rows)
    red = ctx.without_identity_columns(2)
    ctx.close()
    assert np.array_equal(red.get_sequences(), codes[:, ~want])
    red.close()


@pytest.mark.parametrize("sigma,m", [(4, 37), (2, 4101), (4, 70001), (16, 2501), (16, 33)])
def test_garbage_padding_packed(pkg, sigma, m):
    """Borrowed packed columns, ld 32 bytes larger than a column needs, the padding fields of the last byte and every byte up to
    ld set to 0xFF: the same mask as the clean buffer's, and a reduced alignment without the garbage."""
    assert m % (8 // BITS[sigma])
    n = 301
    codes = im.random_case(m, m, n, sigma, 0.6, codes=True)
    want = im.identity_mask(codes)
    clean = borrowed_packed(pkg, codes, sigma)
    dirty = borrowed_packed(pkg, codes, sigma, pad=32, garbage=True)
    a, _ = clean.identity_columns()
    b, _ = dirty.identity_columns()
    assert np.array_equal(a, want) and np.array_equal(b, want)
    ra, rb = clean.without_identity_columns(5), dirty.without_identity_columns(5)
    clean.close()
    dirty.close()
    assert np.array_equal(ra.get_sequences(), codes[:, ~want]) and np.array_equal(rb.get_sequences(), codes[:, ~want])
    ra.close()
    rb.close()


@pytest.mark.parametrize("sigma,m", [(4, 37), (40, 1030), (16, 16411)])
def test_garbage_padding_one_code_per_byte(pkg, sigma, m):
    """The same for columns borrowed one code per byte: the code width stays 8 bits whatever sigma is."""
    import torch
    n = 301
    codes = im.random_case(m + 1, m, n, sigma, 0.6, codes=True)
    want = im.identity_mask(codes)
    ld = (m + 15) // 16 * 16 + 32
    cols = np.full((n, ld), 0xFF, dtype=np.uint8)
    cols[:, :m] = codes.T
    dev = torch.from_numpy(cols).to("cuda")
    ctx = pkg.SegmentationContext(m, n, 5)
    ctx.set_device_columns(dev.data_ptr(), ld, sigma, keepalive=dev)
    mask, s = ctx.identity_columns()
    assert np.array_equal(mask, want)
    red = ctx.without_identity_columns(5)
    ctx.close()
    del dev
    assert np.array_equal(red.get_sequences(), codes[:, ~want])     # (bytes are codes on a borrowed context: the width was kept)
    red.close()


def test_gather_corners(pkg):
    # no identity column: a plain copy
    msa = im.random_case(1, 9, 500, 4, 0.0)
    ctx = pkg.SegmentationContext(9, 500, 10)
    ctx.set_sequences(msa)
    red = ctx.without_identity_columns(10)
    assert red.n == 500 and red.identity_summary["identity"] == 0
    assert np.array_equal(red.get_sequences(), ctx.get_sequences()) and np.array_equal(red.get_sequences(), msa)
    assert np.array_equal(red.kept_columns(), np.arange(500))
    red.close()
    ctx.close()
    # every column an identity column (one row; all rows equal): refused, nothing made, and the source still runs
    for rows in (msa[:1], np.repeat(msa[:1], 6, axis=0)):
        rows = np.ascontiguousarray(rows)
        ctx = pkg.SegmentationContext(rows.shape[0], 500, 10)
        ctx.set_sequences(rows)
        mask, s = ctx.identity_columns()
        assert mask.all() and s["kept"] == 0
        with pytest.raises(pkg.FseqError) as e:
            ctx.without_identity_columns(10)
        assert e.value.code == pkg.FSEQ_E_ARG and "every column is an identity column" in str(e.value)
        if rows.shape[0] == 1:
            with pytest.raises(pkg.NoReduction):
                ctx.run()
        else:
            assert ctx.run().max_segment_size == 1
        ctx.close()
    # ill-formed parameters on a live context
    ctx = pkg.SegmentationContext(9, 500, 10)
    ctx.set_sequences(msa)
    h = pkg.C.c_void_p()
    for p in (pkg.Params(0, 7, 10, 0, 0, 0, 0), pkg.Params(8, 0, 10, 0, 0, 0, 0), pkg.Params(0, 0, 0, 0, 0, 0, 0), pkg.Params(0, 0, 10, 0, 0, 0, 99)):
        assert ctx.L.fseq_create_without_identity_columns(ctx.h, pkg.C.byref(p), pkg.C.byref(h), None) == pkg.FSEQ_E_ARG
        assert h.value is None
    # the calls of a reduced context on a plain one
    with pytest.raises(pkg.FseqError) as e:
        ctx.kept_columns()
    assert e.value.code == pkg.FSEQ_E_ARG
    with pytest.raises(pkg.FseqError) as e:
        ctx.write_identity_columns("/dev/null")
    assert e.value.code == pkg.FSEQ_E_ARG
    ctx.close()


def results_of(ctx):
    res = ctx.run()
    out = {"max": res.max_segment_size, "traceback": ctx.traceback(), "segments": ctx.reduced_traceback()}
    out["states"] = [ctx.boundary_state(i) for i in range(len(out["segments"]))]
    out["greedy"], out["bipartite"], out["random"] = ctx.join_greedy(), ctx.join_bipartite(), ctx.join_random(5)
    return out


def mosaic_with_identity(seed, m, n, share=0.6):
    """A founder mosaic over ACGT of which about `share` of the columns are overwritten with row 0's symbol, every seventh of
    those with 'N': a symbol that occurs in identity columns only, so the kept alphabet is smaller than the code table."""
    msa = founder_mosaic(6, m, n, brec=250, seed=seed)
    ident = np.random.default_rng(seed).random(n) < share
    msa[:, ident] = msa[0:1, ident]
    msa[:, np.flatnonzero(ident)[::7]] = ord("N")
    return np.ascontiguousarray(msa)


@pytest.mark.parametrize("m,n", [(50, 3000), (12000, 600)])
def test_same_results_as_a_fresh_upload(pkg, tmp_path, m, n):
    """Segments, traceback, boundary states and the three joiners' permutations of the compacted context are those of a plain
    context given msa[:, ~mask] -- although the compacted one keeps the source's five codes at four bits and the fresh upload
    packs its four at two.  m = 12,000: streamed rows, and the gather's columns of several chunks."""
    L = 20
    msa = mosaic_with_identity(m, m, n)
    mask = im.identity_mask(msa)
    assert 0.5 * n < mask.sum() < 0.9 * n and ord("N") not in msa[:, ~mask] and ord("N") in msa
    src = pkg.SegmentationContext(m, n, L)
    src.set_sequences(msa)
    red = src.without_identity_columns(L)
    src.close()
    reduced = im.reduce_rows(msa, mask)
    assert red.n == reduced.shape[1] and np.array_equal(red.get_sequences(), reduced)
    fresh = pkg.SegmentationContext(m, reduced.shape[1], L)
    fresh.set_sequences(reduced)
    a, b = results_of(red), results_of(fresh)
    assert a["max"] == b["max"] < m
    for f in ("traceback", "segments", "greedy", "bipartite", "random"):
        assert np.array_equal(a[f], b[f]), f
    for (a1, d1), (a2, d2) in zip(a["states"], b["states"]):
        assert np.array_equal(a1, a2) and np.array_equal(d1, d2)
    # the restored founders: the model's restore of what write_founders_device writes.  The bipartite joiner's permutations a second
    # time with slots that have no row (join_context.cc:348-349, m_permutation_max; this library's joiners fill every slot, so they
    # are put in as tests/test_join.py does): '-' over those segments, at the kept columns only
    holes = a["bipartite"].copy()
    holes[0, 0] = holes[len(holes) // 2, -1] = holes[-1, a["max"] // 2] = (1 << int(m).bit_length()) - 1
    for name, perm in (("greedy", a["greedy"]), ("bipartite", a["bipartite"]), ("bipartite_holes", holes)):
        plain, restored = str(tmp_path / ("plain_" + name)), str(tmp_path / ("restored_" + name))
        red.write_founders_device(perm, plain)
        red.write_founders_restored(perm, restored)
        want = im.restore(im.lines_of(plain), mask, msa[0])
        got = im.lines_of(restored)
        assert got.shape == (a["max"], n) and np.array_equal(got, want)
        if name == "bipartite_holes":
            seg = a["segments"]
            assert (perm >= m).sum() == 3 and len(seg) >= 3
            kept = np.flatnonzero(~mask)
            for s_, r in ((0, 0), (len(holes) // 2, a["max"] - 1), (len(holes) - 1, a["max"] // 2)):
                cols = kept[int(seg["lb"][s_]):int(seg["rb"][s_])]
                assert (got[r, cols] == ord("-")).all()
                lo, hi = cols[0], cols[-1]
                inside = np.flatnonzero(mask[lo:hi]) + lo        # identity columns inside the segment keep row 0's byte
                assert np.array_equal(got[r, inside], msa[0, inside])
    red.write_identity_columns(str(tmp_path / "mask"))
    assert open(str(tmp_path / "mask"), "rb").read() == im.mask_text(mask)
    fresh.close()
    red.close()


def test_restored_founders_refusals(pkg, tmp_path):
    msa = mosaic_with_identity(3, 30, 1500)
    ctx = pkg.SegmentationContext(30, 1500, 20)
    ctx.set_sequences(msa)
    ctx.run()
    perm = ctx.join_greedy()
    with pytest.raises(pkg.FseqError) as e:                       # a plain context
        ctx.write_founders_restored(perm, str(tmp_path / "f"))
    assert e.value.code == pkg.FSEQ_E_ARG
    red = ctx.without_identity_columns(20)
    with pytest.raises(pkg.FseqError) as e:                       # before a run
        red.write_founders_restored(perm, str(tmp_path / "f"))
    assert e.value.code == pkg.FSEQ_E_ARG
    red.close()
    short = ctx.without_identity_columns(red.n)                   # n < 2 L: the short path
    ctx.close()
    try:
        short.run()
    except pkg.NoReduction:                                      # (the rows may all differ over the whole length)
        pass
    assert short.result.short_path
    with pytest.raises(pkg.FseqError) as e:
        short.write_founders_restored(perm, str(tmp_path / "f"))
    assert e.value.code == pkg.FSEQ_E_ARG
    short.close()


@pytest.mark.parametrize("joining", ["greedy", "bipartite-matching"])
def test_cli_against_the_chain_of_tools(build, tmp_path, joining):
    """founder_sequences --remove-identity-columns against remove_identity_columns -> founder_sequences -> insert_identity_columns
    -r <row 0's file> with the project's own host tools: the same mask, founders and segments files."""
    cli = build.build_cli()
    tools = dict(zip(build.AUX_TOOLS, build.build_aux()))
    m, n, L = 20, 5000, 20
    msa = mosaic_with_identity(11, m, n)
    src = tmp_path / "in"
    src.mkdir()
    names = []
    for i, row in enumerate(msa):
        (src / ("s%02d" % i)).write_bytes(row.tobytes())
        names.append(str(src / ("s%02d" % i)))
    (tmp_path / "list.txt").write_text("\n".join(names) + "\n")
    common = ["--segment-length-bound", str(L), "--segment-joining", joining]
    r = subprocess.run([cli, "--input", str(tmp_path / "list.txt"), "--remove-identity-columns", "--output-identity-columns=" + str(tmp_path / "M"),
                        "--output-founders=" + str(tmp_path / "F"), "--output-segments=" + str(tmp_path / "E")] + common, capture_output=True, timeout=120)
    assert r.returncode == 0, r.stderr
    mask = im.identity_mask(msa)
    assert ("Removed %d of %d columns in which all sequences agree." % (mask.sum(), n)).encode() in r.stderr
    # the chain
    red = tmp_path / "reduced"
    red.mkdir()
    r = subprocess.run([tools["remove_identity_columns"], "--input", str(tmp_path / "list.txt")], capture_output=True, cwd=str(red), timeout=120)
    assert r.returncode == 0, r.stderr
    (tmp_path / "M2").write_bytes(r.stdout)
    (tmp_path / "list2.txt").write_text("\n".join(str(red / ("s%02d" % i)) for i in range(m)) + "\n")
    r = subprocess.run([cli, "--input", str(tmp_path / "list2.txt"), "--output-founders=" + str(tmp_path / "F2"), "--output-segments=" + str(tmp_path / "E2")] + common,
                       capture_output=True, timeout=120)
    assert r.returncode == 0, r.stderr
    back = tmp_path / "back"
    back.mkdir()
    r = subprocess.run([tools["insert_identity_columns"], "--input", str(tmp_path / "F2"), "--reference", names[0], "--identity-columns", str(tmp_path / "M2")],
                       capture_output=True, cwd=str(back), timeout=120)
    assert r.returncode == 0, r.stderr
    K = len(os.listdir(str(back)))
    chain = b"".join((back / str(i + 1)).read_bytes() + b"\n" for i in range(K))
    assert (tmp_path / "M").read_bytes() == (tmp_path / "M2").read_bytes() == im.mask_text(mask)
    assert (tmp_path / "F").read_bytes() == chain and K >= 2
    assert (tmp_path / "E").read_bytes() == (tmp_path / "E2").read_bytes()


def test_cli_every_column_an_identity_column(build, tmp_path):
    cli = build.build_cli()
    (tmp_path / "in.fa").write_text(">a\nACGTACGTAC\n>b\nACGTACGTAC\n")
    r = subprocess.run([cli, "--input", str(tmp_path / "in.fa"), "--input-format", "FASTA", "--segment-length-bound", "2", "--remove-identity-columns",
                        "--output-founders=" + str(tmp_path / "F")], capture_output=True, timeout=120)
    assert r.returncode != 0 and b"every column is an identity column" in r.stderr
