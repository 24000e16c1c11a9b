"""CPU checks of the segment length entry points: the symbols, the refusals that need no device, the scan's order of work
(plan_length_scan, csrc/fseq_scanplan.hpp, through fseq_debug_scan_plan), the argument checks of fseq_debug_relump_lists, and
the front end's validation of --scan-segment-lengths, --output-scan and --max-founders."""
import ctypes as C
import importlib
import subprocess

import numpy as np
import pytest

NEW = ["fseq_set_segment_length", "fseq_scan_segment_lengths"]
NEW_DEBUG = ["fseq_debug_scan_plan", "fseq_debug_relump_lists"]


@pytest.fixture(scope="module")
def pkg():
    build = importlib.import_module("founder-sequences_amd.build")
    build.build()
    return importlib.import_module("founder-sequences_amd")


@pytest.fixture(scope="module")
def cli():
    return importlib.import_module("founder-sequences_amd.build").build_cli()


def test_symbols_and_layouts(pkg):
    lib = pkg.load_library()
    for name in NEW + NEW_DEBUG:
        assert hasattr(lib, name), name
        assert name in pkg.EXPORTS and (name in pkg.DEBUG_EXPORTS) == (name in NEW_DEBUG), name
    assert lib.fseq_abi_version() == 5
    assert pkg.LENGTH_SCAN_DTYPE.itemsize == 40 and C.sizeof(pkg.LengthScanSummary) == 40
    assert (pkg.SCAN_LISTS_BUILT, pkg.SCAN_LISTS_FOLDED, pkg.SCAN_LISTS_NONE) == (0, 1, 2)


def test_refusals_that_need_no_device(pkg):
    lib = pkg.load_library()
    entries = np.zeros(2, dtype=pkg.LENGTH_SCAN_DTYPE)
    sm = pkg.LengthScanSummary()
    assert lib.fseq_scan_segment_lengths(None, entries.ctypes.data, 2, C.byref(sm)) == pkg.FSEQ_E_ARG
    assert lib.fseq_scan_segment_lengths(None, None, 2, C.byref(sm)) == pkg.FSEQ_E_ARG
    assert lib.fseq_scan_segment_lengths(None, entries.ctypes.data, 0, C.byref(sm)) == pkg.FSEQ_E_ARG
    assert lib.fseq_set_segment_length(None, 5) == pkg.FSEQ_E_ARG
    assert lib.fseq_set_segment_length(None, 0) == pkg.FSEQ_E_ARG


def test_scan_plan_orders_and_splits(pkg):
    n = 3000
    lengths = [200, 5, 1501, 20, 5, 4000, 1500, 20, 1499, 200]
    long_lengths, slot, n_short = pkg.scan_plan_host(n, lengths)
    assert list(long_lengths) == [5, 20, 200, 1499, 1500]                # distinct, ascending, n >= 2L
    assert n_short == 2
    assert list(slot) == [2, 0, -1, 1, 0, -1, 4, 1, 3, 2]
    # the split at n = 2L - 1 | 2L, for odd and even n
    for n in (9, 10, 11, 2999, 3000):
        for L in range(1, n + 3):
            ll, sl, ns = pkg.scan_plan_host(n, [L])
            assert (ns == 1) == (n < 2 * L) and (len(ll) == 0) == (n < 2 * L) and sl[0] == (-1 if n < 2 * L else 0), (n, L)
    # a length of any size does not overflow the comparison
    assert pkg.scan_plan_host(10, [2 ** 63, 2 ** 64 - 1, 5])[2] == 2
    for bad in ([], [0], [5, 0]):
        with pytest.raises(pkg.FseqError) as e:
            pkg.scan_plan_host(100, bad)
        assert e.value.code == pkg.FSEQ_E_ARG
    with pytest.raises(pkg.FseqError):
        pkg.scan_plan_host(0, [5])
    lib = pkg.load_library()
    one = np.array([5], dtype=np.uint64)
    assert lib.fseq_debug_scan_plan(100, None, 1, one.ctypes.data, None, None, None) == pkg.FSEQ_E_ARG


def test_relump_lists_refuses_bad_arrays_before_a_device(pkg):
    """There is no device here: a call that got past the argument checks would return FSEQ_E_HIP, not FSEQ_E_ARG."""
    lib = pkg.load_library()
    ent = np.zeros((2, 8, 2), dtype=np.uint32)
    hdr = np.array([[3, 0, 1, 5], [8, 0, 1, 5]], dtype=np.uint32)
    call = lambda k0, ncols, stride, L_from, L_to, e=ent, h=hdr: lib.fseq_debug_relump_lists(
        0, k0, ncols, stride, L_from, L_to, None if e is None else e.ctypes.data, None if h is None else h.ctypes.data)
    assert call(100, 2, 8, 4, 9, e=None) == pkg.FSEQ_E_ARG
    assert call(100, 2, 8, 4, 9, h=None) == pkg.FSEQ_E_ARG
    assert call(100, 0, 8, 4, 9) == pkg.FSEQ_E_ARG
    assert call(100, 2, 0, 4, 9) == pkg.FSEQ_E_ARG
    assert call(100, 2, 8, 4, 3) == pkg.FSEQ_E_ARG                       # L_to < L_from
    assert call(100, 2, 8, 0, 3) == pkg.FSEQ_E_ARG
    assert call(2 ** 32 - 1, 2, 8, 4, 9) == pkg.FSEQ_E_ARG
    for bad in (0, 9, 0xFFFFFFFF):                                       # n_entries == 0 or > stride
        h = hdr.copy()
        h[1, 0] = bad
        assert call(100, 2, 8, 4, 9, h=h) == pkg.FSEQ_E_ARG
    with pytest.raises(pkg.FseqError) as e:
        pkg.relump_lists(np.zeros((2, 8, 3), dtype=np.uint32), hdr, 100, 4, 9)
    assert e.value.code == pkg.FSEQ_E_ARG
    assert call(100, 2, 8, 4, 9) != pkg.FSEQ_E_ARG                       # in order: it goes on to the device


@pytest.mark.parametrize("args,message", [
    (["--scan-segment-lengths=5,,7"], "segment lengths to scan"),
    (["--scan-segment-lengths=0,7"], "segment lengths to scan"),
    (["--scan-segment-lengths=9:3:1"], "segment lengths to scan"),
    (["--scan-segment-lengths=3:9:0"], "segment lengths to scan"),
    (["--scan-segment-lengths=3:9"], "segment lengths to scan"),
    (["--scan-segment-lengths=5x"], "segment lengths to scan"),
    (["--max-founders=4"], "--max-founders requires --scan-segment-lengths"),
    (["--output-scan=t.tsv", "-s", "5"], "--output-scan requires --scan-segment-lengths"),
    (["--scan-segment-lengths=5,7", "--max-founders=4", "-s", "5"], "--max-founders is not supported together with --segment-length-bound"),
    (["--scan-segment-lengths=5,7", "--max-founders=0"], "maximum number of founders"),
    (["--scan-segment-lengths=5,7", "--gpus=2"], "--scan-segment-lengths is not supported together with --gpus > 1"),
])
def test_front_end_option_validation(cli, tmp_path, args, message):
    """Every refusal comes before the input is read (the list file names no sequences)."""
    lst = tmp_path / "in.txt"
    lst.write_text("")
    r = subprocess.run([cli, "--input=" + str(lst)] + args, capture_output=True, text=True)
    assert r.returncode != 0 and message in r.stderr, r.stderr


def test_front_end_help_and_invocation(cli, tmp_path):
    out = subprocess.run([cli, "--help"], capture_output=True, text=True).stdout
    for opt in ("--scan-segment-lengths=SPEC", "--output-scan=PATH", "--max-founders=K"):
        assert opt in out
    lst = tmp_path / "in.txt"
    lst.write_text("")
    r = subprocess.run([cli, "--input=" + str(lst), "--print-invocation", "--scan-segment-lengths=4:12:4", "--max-founders=3"], capture_output=True, text=True)
    assert "--scan-segment-lengths=4:12:4" in r.stderr and "--max-founders=3" in r.stderr
    # an empty input is no error; the scan alone needs no segment length bound
    assert r.returncode == 0 and "contained no sequences" in r.stderr
