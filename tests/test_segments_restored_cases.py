"""The bounds of merged segments in source co-ordinates, without a device: the numpy model of tests/segments_restored_cases.py on
an example written out by hand, the library's pure host function (restored_segment_bounds, csrc/fseq_restored_bounds.hpp, through
fseq_debug_restored_bounds) against the model, its refusals, and the same function as a program under the host sanitizers."""
import importlib
import os
import subprocess

import numpy as np
import pytest

import segments_restored_cases as cases


@pytest.fixture(scope="module")
def pkg():
    importlib.import_module("founder-sequences_amd.build").build()
    return importlib.import_module("founder-sequences_amd")


def test_model_on_an_example_by_hand():
    """Source of 16 columns, I = identity, digits = kept columns:
         position  0 1 2 3 4 5 6 7 8 9 10 11 12 13 14 15
                   I I 0 1 I I 2 3 I 4 5  I  I  6  I  I
       kept = 2 3 6 7 9 10 13; segments [0, 2) [2, 5) [5, 7) in kept columns.  A leading run (0, 1), a run on the border between
       segments 0 and 1 (4, 5: segment 0's, they stand behind its last kept column), runs inside segments 1 and 2 (8; 11, 12) and a
       trailing run (14, 15: the last segment's)."""
    kept = [2, 3, 6, 7, 9, 10, 13]
    lb, rb = [0, 2, 5], [2, 5, 7]
    src_lb, src_rb = cases.restored_bounds(kept, 16, lb, rb)
    assert src_lb.tolist() == [0, 6, 10] and src_rb.tolist() == [6, 10, 16]
    # position by position: the owner of a source column is the segment of the last kept column at or in front of it
    owner = [0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 2, 2]
    for p, s in enumerate(owner):
        assert src_lb[s] <= p < src_rb[s]
    # the same example through with_identity_runs
    R = np.array([[65, 67, 65, 67, 65, 67, 65], [67, 65, 67, 65, 67, 65, 67]], dtype=np.uint8)
    full, k = cases.with_identity_runs(R, {0: 2, 2: 2, 4: 1, 6: 2, 7: 2})
    assert k.tolist() == kept and full.shape == (2, 16)
    assert np.array_equal(full[:, kept], R) and ((full == full[0]).all(0) == ~np.isin(np.arange(16), kept)).all()


def random_case(rng):
    n_src = int(rng.integers(1, 400))
    n = int(rng.integers(1, n_src + 1))
    kept = np.sort(rng.choice(n_src, size=n, replace=False))
    S = int(rng.integers(1, min(n, 12) + 1))
    cuts = np.sort(rng.choice(np.arange(1, n), size=S - 1, replace=False)) if S > 1 else np.zeros(0, dtype=np.int64)
    lb = np.concatenate([[0], cuts]).astype(np.uint64)
    rb = np.concatenate([cuts, [n]]).astype(np.uint64)
    return kept, n_src, lb, rb


def test_host_function_equals_the_model(pkg):
    rng = np.random.default_rng(2024)
    shapes = set()
    for _ in range(200):
        kept, n_src, lb, rb = random_case(rng)
        want = cases.restored_bounds(kept, n_src, lb, rb)
        got = pkg.restored_bounds_host(kept, n_src, lb, rb)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), (kept, n_src, lb, rb)
        assert got[0][0] == 0 and got[1][-1] == n_src and np.array_equal(got[0][1:], got[1][:-1]) and (got[0] < got[1]).all()
        shapes.add((kept[0] > 0, kept[-1] < n_src - 1, len(lb) == 1, len(kept) == n_src))
    # leading and trailing runs present and absent, one segment, no identity column at all: all among the 200
    assert {x[0] for x in shapes} == {x[1] for x in shapes} == {x[2] for x in shapes} == {True, False} and any(x[3] for x in shapes)


def test_host_function_refuses_malformed_inputs(pkg):
    kept, lb, rb = [1, 4, 5, 9], [0, 2], [2, 4]
    pkg.restored_bounds_host(kept, 10, lb, rb)
    malformed = {
        "kept with an entry twice": ([1, 4, 4, 9], 10, lb, rb),
        "kept descending": ([1, 5, 4, 9], 10, lb, rb),
        "a kept column at n_src": ([1, 4, 5, 10], 10, lb, rb),
        "a kept column far behind n_src": ([1, 4, 5, 2 ** 64 - 1], 10, lb, rb),
        "no segments": (kept, 10, [], []),
        "the first segment does not begin at 0": (kept, 10, [1, 2], [2, 4]),
        "a hole between two segments": (kept, 10, [0, 3], [2, 4]),
        "two segments overlap": (kept, 10, [0, 1], [2, 4]),
        "the last segment ends in front of n": (kept, 10, [0, 2], [2, 3]),
        "the last segment ends behind n": (kept, 10, [0, 2], [2, 5]),
        "a border behind n": (kept, 10, [0, 5], [5, 4]),
        "a border that wraps": (kept, 10, [0, 2 ** 64 - 1], [2 ** 64 - 1, 4]),
    }
    for what, (k, n_src, l, r) in malformed.items():
        with pytest.raises(pkg.FseqError) as err:
            pkg.restored_bounds_host(np.array(k, dtype=np.uint64), n_src, np.array(l, dtype=np.uint64), np.array(r, dtype=np.uint64))
        assert err.value.code == pkg.FSEQ_E_ARG, what


def test_bounds_under_the_sanitizers(tmp_path):
    """The header is host-only: tests/restored_bounds_sanitized.cpp includes it alone and runs random tilings and every refusal on
    arrays of exactly the lengths given, as a program of its own under AddressSanitizer and UndefinedBehaviorSanitizer (nothing
    loaded into Python runs under either)."""
    here = os.path.dirname(os.path.abspath(__file__))
    exe = str(tmp_path / "restored_bounds_sanitized")
    subprocess.run(["g++", "-std=c++17", "-g", "-O1", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", os.path.join(os.path.dirname(here), "founder-sequences_amd", "csrc"), os.path.join(here, "restored_bounds_sanitized.cpp"), "-o", exe], check=True)
    p = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120)
    assert p.returncode == 0 and p.stdout.strip() == "ok", p.stderr[-3000:]
