"""An input whose per-column lists do not fit the device fails LOUDLY (FSEQ_E_OOM with the sizes in the message), and the failure
stays with that call: found with C4's shape at mu = 1e-3 (profiles/r05_diversity_C4.txt: the lists would take 758 GB), where
the HIP runtime kept the failed hipMalloc as its last error and the next context of the process -- a different input -- failed
in the check behind its first kernel launch with "hipGetLastError(): out of memory"."""
import ctypes as C
import gc
import importlib

import numpy as np
import pytest

import fso
from test_gpu_parity import check_long, compare_long

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def pkg():
    return importlib.import_module("founder-sequences_amd")


def test_lists_beyond_the_device_fail_with_oom_and_leave_no_error_behind(pkg):
    m, n, L = 20_000, 2_500_000, 100                                 # (a list holds at most m entries: the rows make the size)
    ctx = pkg.SegmentationContext(m, n, L, list_cap=m)               # 2,500,000 x 20,002 x 8 bytes = 400 GB of lists
    ctx.generate_synthetic(7, 8, 1000, 1e-4, 0)
    with pytest.raises(pkg.FseqError) as ei:
        ctx.run()
    assert ei.value.code == pkg.FSEQ_E_OOM
    assert "hipMalloc of" in str(ei.value) and "bytes free on the device" in str(ei.value)
    ctx.close()
    # the next context of the process (same thread) sees nothing of it
    msa = fso.synth_msa(fso.synth_spec(5, 6, 400, 1e-3, 0), 300, 2500)
    compare_long(pkg, msa, 20)
    # and neither does a context that was open while the other one failed
    a = pkg.SegmentationContext(300, 2500, 20)
    a.set_sequences(msa)
    b = pkg.SegmentationContext(m, n, L, list_cap=m)
    b.generate_synthetic(7, 8, 1000, 1e-4, 0)
    with pytest.raises(pkg.FseqError):
        b.run()
    b.close()
    a.run()
    ref = fso.segment_long(msa, 20, keep_dp=False, threads=2)
    assert a.result.max_segment_size == ref["max_segment_size"]
    assert np.array_equal(a.traceback()["lb"], ref["traceback"]["lb"])
    a.close()


# A run that failed with FSEQ_E_OOM leaves a context that runs correctly once the memory is there: no buffer of the context
# remembers a size it no longer has.  The card is filled up to a fraction of what the run takes, so that the failure lands in
# another allocation each time; the last case retries with a run that needs less than the one that failed.
RETRY_M, RETRY_N, RETRY_L = 600, 60_000, 30
# (fractions of the run's need, measured as the drop in free memory around a run, that the ballast leaves free: each less than
# the whole, in steps that stop the run at different allocations -- the lists, a per-block array, small per-column arrays)
RETRY_MARGINS = (0.5, 0.2, 0.1, 0.02)


@pytest.fixture(scope="module")
def retry_input(pkg):
    import torch
    msa = fso.synth_msa(fso.synth_spec(21, 8, 500, 2e-3, 0), RETRY_M, RETRY_N)
    ref = fso.segment_long(msa, RETRY_L, keep_dp=True, threads=4)
    # what a run takes on top of the input: the free memory around a run with nothing in its way (the second of the process:
    # the first also loads the kernels and sets up the runtime's own memory, which the retries do not pay again)
    gc.collect()
    for _ in range(2):
        ctx = pkg.SegmentationContext(RETRY_M, RETRY_N, RETRY_L)
        ctx.set_sequences(msa)
        free0 = torch.cuda.mem_get_info()[0]
        ctx.run()
        need = free0 - torch.cuda.mem_get_info()[0]
        check_long(ctx, ref, RETRY_N, RETRY_L)
        ctx.close()
    print("retry input: a run takes %d bytes of device memory" % need)
    assert need > (8 << 20)
    return msa, ref, need


_hip = None


def _hip_runtime():
    global _hip
    if _hip is None:
        _hip = C.CDLL("libamdhip64.so")
        _hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
        _hip.hipFree.argtypes = [C.c_void_p]
    return _hip


def fill_device(leave, step=1 << 20):
    """Takes the device's memory down to about `leave` bytes.  The bulk is one torch tensor sized from mem_get_info; that figure
    lags behind what the runtime can hand out (memory that contexts freed a moment ago, contexts of earlier tests the collector
    has not reached), so the rest is taken in 1 MiB hipMallocs until the device refuses one, and `leave` bytes of them go back."""
    import torch
    gc.collect()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    ballast = []
    spare = torch.cuda.mem_get_info()[0] - leave
    if spare > 0:
        ballast.append(torch.empty(spare, dtype=torch.uint8, device="cuda"))
    hip, blocks = _hip_runtime(), []
    while len(blocks) < 65536:
        p = C.c_void_p()
        if hip.hipMalloc(C.byref(p), step) != 0:
            hip.hipGetLastError()                                     # (the runtime remembers the failure)
            break
        blocks.append(p)
    else:
        raise AssertionError("the ballast did not fill the device")
    for _ in range(min(len(blocks), -(-leave // step))):
        hip.hipFree(blocks.pop())
    return ballast, blocks


def release_device(ballast, blocks):
    import torch
    while blocks:
        _hip_runtime().hipFree(blocks.pop())
    ballast.clear()
    torch.cuda.empty_cache()


def oom_then_retry(pkg, retry_input, margin, first_knobs=(), retry_knobs=()):
    import torch
    msa, ref, need = retry_input
    ctx = pkg.SegmentationContext(RETRY_M, RETRY_N, RETRY_L)
    ctx.set_sequences(msa)
    for name, value in first_knobs:
        ctx.set_tuning(name, value)
    leave = int(need * margin)
    ballast, blocks = fill_device(leave)
    try:
        print("margin %.2f: %d bytes left free of the %d a run takes" % (margin, torch.cuda.mem_get_info()[0], need))
        with pytest.raises(pkg.FseqError) as ei:
            ctx.run()
        print("  ->", ei.value)
        assert ei.value.code == pkg.FSEQ_E_OOM
        assert "hipMalloc of" in str(ei.value) and "bytes free on the device" in str(ei.value)
    finally:
        release_device(ballast, blocks)
    for name, value in retry_knobs:
        ctx.set_tuning(name, value)
    ctx.run()
    check_long(ctx, ref, RETRY_N, RETRY_L)
    ctx.close()


@pytest.mark.parametrize("margin", RETRY_MARGINS)
def test_context_runs_correctly_after_oom(pkg, retry_input, margin):
    oom_then_retry(pkg, retry_input, margin)


def test_context_runs_a_smaller_run_after_oom(pkg, retry_input):
    # the run that fails goes through the representatives (their buffers on top of everything else); the retry does not
    oom_then_retry(pkg, retry_input, 0.2, first_knobs=(("FSEQ_REDUCED_ALWAYS", "1"),), retry_knobs=(("FSEQ_REDUCED_ALWAYS", None), ("FSEQ_NO_REDUCED", "1")))
