"""CPU checks of the restored match (include/fseq.h, fseq_match_founders_restored): the symbol, the refusal that must not
touch a device, the front end's option -- and the plain-Python gap step (tests/match_restored_model.py) the kernel follows,
pinned to match_model.match_row on the full-length rows and the full-length restored founders.  match_row is pinned to the
built host tool by tests/test_match_abi.py, and identity_model.restore to insert_identity_columns by
tests/test_identity_abi.py, so the closed form hangs on the two yardsticks."""
import ctypes as C
import importlib
import subprocess

import numpy as np
import pytest

import identity_model as im
import match_model as mm
import match_restored_model as mr


@pytest.fixture(scope="module")
def build():
    return importlib.import_module("founder-sequences_amd.build")


@pytest.fixture(scope="module")
def pkg(build):
    build.build()
    return importlib.import_module("founder-sequences_amd")


def test_library_exports_the_entry_point(pkg):
    lib = pkg.load_library()
    assert hasattr(lib, "fseq_match_founders_restored")
    assert "fseq_match_founders_restored" in pkg.EXPORTS and "fseq_match_founders_restored" not in pkg.DEBUG_EXPORTS
    assert lib.fseq_abi_version() == 5                       # (detected by symbol: no struct of the boundary changed)
    assert hasattr(pkg.SegmentationContext, "match_founders_restored")


def test_null_arguments_fail_without_touching_a_device(pkg):
    lib = pkg.load_library()
    sm = pkg.MatchSummary()
    perm = (C.c_uint32 * 4)()
    assert lib.fseq_match_founders_restored(None, perm, 0, C.byref(sm)) == pkg.FSEQ_E_ARG


def test_front_end_names_the_option_and_requires_the_identity_columns_removed(build, tmp_path):
    cli = build.build_cli()
    r = subprocess.run([cli, "--help"], capture_output=True, timeout=60)
    assert r.returncode == 0 and b"--output-restored-matches" in r.stdout
    # refused before any input is read: the input does not exist, and the message is the option's
    r = subprocess.run([cli, "--input", str(tmp_path / "missing.txt"), "--segment-length-bound", "5", "--output-founders", str(tmp_path / "f"),
                        "--output-restored-matches", str(tmp_path / "m")], capture_output=True, timeout=60)
    assert r.returncode != 0
    assert b"--output-restored-matches" in r.stderr and b"--remove-identity-columns" in r.stderr
    assert b"Loading the input" not in r.stderr and b"Unable to open" not in r.stderr
    assert not (tmp_path / "m").exists() and not (tmp_path / "f").exists()


MIN_LENS = [0, 1, 2, 7]
N_CASES = 320


def gap_case(i):
    """Case i: a source laid out as gap, kept column, gap, ..., kept column, gap with gap lengths drawn from 0, 1, a few and
    several times min_len, the lengths of the first and the last gap and the place of the uncovered cells going through
    their combinations with i.  -> (msa, reduced founders, kept, mask, min_len)"""
    rng = np.random.default_rng(9000 + i)
    min_len = MIN_LENS[i % 4]
    long_gap = 3 * max(min_len, 1) + int(rng.integers(1, 4))
    n_kept = int(rng.integers(1, 8))
    if i % 8 == 4:
        gaps = [0] * (n_kept + 1)                             # no identity column at all
    else:
        gaps = [int(rng.choice([0, 0, 1, 2, long_gap])) for _ in range(n_kept + 1)]
        gaps[0] = [0, 1, long_gap][(i // 4) % 3]
        gaps[-1] = [0, 1, long_gap, 0][(i // 12) % 4]
    mask = np.concatenate([np.r_[np.ones(g, dtype=bool), False] for g in gaps[:-1]] + [np.ones(gaps[-1], dtype=bool)])
    m, K, sigma = int(rng.integers(2, 5)), int(rng.integers(1, 6)), int(rng.integers(2, 5))
    uncovered = []
    if (i // 2) % 3 == 0:
        uncovered.append((int(rng.integers(m)), n_kept - 1))
    if (i // 5) % 3 == 0:
        uncovered.append((int(rng.integers(m)), 0))
    if n_kept > 2 and i % 7 == 0:
        uncovered.append((int(rng.integers(m)), int(rng.integers(1, n_kept - 1))))
    msa, founders, kept = mr.planted_case(rng, m, len(mask), K, sigma, mask, uncovered)
    assert np.array_equal(im.identity_mask(msa), mask) and len(kept) == n_kept
    return msa, founders, kept, mask, min_len


def gap_lengths(mask):
    """(leading, [inner ...], trailing) runs of identity columns"""
    kept = np.flatnonzero(~mask)
    inner = np.diff(kept) - 1
    return int(kept[0]), inner[inner > 0].tolist(), int(len(mask) - 1 - kept[-1])


def test_gap_step_is_the_host_loop_on_the_full_length_data():
    """match_row_restored on (reduced row, reduced founders, kept columns) against match_row on (full row, restored
    founders): pieces, founder lists, uncovered cells and short pieces, row by row.  The restored founders are
    identity_model.restore of the reduced ones, the construction tests/test_identity_abi.py pins to insert_identity_columns."""
    seen = set()
    for i in range(N_CASES):
        msa, founders, kept, mask, min_len = gap_case(i)
        n_src = msa.shape[1]
        full = im.restore(founders, mask, msa[0])
        assert full.shape == (len(founders), n_src) and np.array_equal(full[:, kept], founders)
        red = im.reduce_rows(msa, mask)
        fb, rb = [bytes(f) for f in full], [bytes(f) for f in founders]
        lead, inner, trail = gap_lengths(mask)
        for r in range(len(msa)):
            want = mm.match_row(bytes(msa[r]), fb, min_len)
            got = mr.match_row_restored(bytes(red[r]), rb, kept, n_src, min_len)
            assert got == want, (i, r, min_len, mask.astype(int).tolist())
            # what this row of this case reaches
            unc_last = not (founders[:, -1] == red[r, -1]).any()
            unc_first = not (founders[:, 0] == red[r, 0]).any()
            seen.add(("min_len", min_len))
            if unc_last:
                seen.add("uncovered in the last kept column, trailing gap" if trail else "uncovered in the last kept column, no trailing gap")
                if trail and not min_len:                    # the one-column piece and a last piece of every founder
                    assert want[0][-2:] == [(n_src - trail - 1, n_src - trail, []), (want[0][-1][0], n_src, list(range(len(founders))))]
            if unc_first and lead == 0:
                seen.add("uncovered in source column 0")
                assert want[0][0] == (0, 0, list(range(len(founders))))
            if unc_first and lead:
                seen.add("uncovered in the first kept column behind a gap")
                assert min_len or want[0][0] == (0, lead, list(range(len(founders))))
            if min_len and any(rb_ > lb and mask[lb:rb_].all() for lb, rb_, _ in want[0]):
                seen.add("a piece inside a gap")
        seen.add("leading gap" if lead else "no leading gap")
        seen.add("trailing gap" if trail else "no trailing gap")
        if not mask.any():
            seen.add("no gap at all")
        if 1 in [lead, trail] + inner:
            seen.add("gap of length 1")
        if min_len and max([lead, trail] + inner) >= 3 * min_len:
            seen.add(("gap several times min_len", min_len))
    wanted = {"leading gap", "no leading gap", "trailing gap", "no trailing gap", "no gap at all", "gap of length 1",
              "uncovered in the last kept column, trailing gap", "uncovered in the last kept column, no trailing gap",
              "uncovered in source column 0", "uncovered in the first kept column behind a gap", "a piece inside a gap"}
    wanted |= {("min_len", v) for v in MIN_LENS} | {("gap several times min_len", v) for v in MIN_LENS if v}
    assert wanted <= seen, wanted - seen


def test_mapping_the_reduced_pieces_back_is_not_the_restored_match():
    """Why the walk carries source positions: the reduced match with its boundaries sent through kept_columns differs from the
    restored match wherever a piece starts behind an uncovered cell that an identity column follows."""
    mask = np.array([0, 1, 0, 1, 1, 0, 1], dtype=bool)
    rng = np.random.default_rng(5)
    msa, founders, kept = mr.planted_case(rng, 3, len(mask), 2, 3, mask, [(1, 1)])
    red = im.reduce_rows(msa, mask)
    reduced = mm.match_row(bytes(red[1]), [bytes(f) for f in founders], 0)
    to_src = np.r_[kept, len(mask)]
    mapped = [(int(to_src[lb]), int(to_src[rb]), idx) for lb, rb, idx in reduced[0]]
    restored = mr.match_row_restored(bytes(red[1]), [bytes(f) for f in founders], kept, len(mask), 0)
    assert restored == mm.match_row(bytes(msa[1]), [bytes(f) for f in im.restore(founders, mask, msa[0])], 0)
    assert (2, 3, []) in restored[0] and (2, 5, []) in mapped and mapped != restored[0]
