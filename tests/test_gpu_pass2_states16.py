"""[r16] Whole runs through the reduced stride states as two 16-bit arrays: phase C drops them, pass 2's sweeps start from them, and
EVERY boundary state of the run must be the oracle's -- at two strides beside the library's own (FSEQ_RED_SS_STRIDE = 4 and 32; 8 and
16 are what tests/test_gpu_reduced.py runs), 2 and 4 bits a symbol, LDS-resident and streamed rows."""
import importlib

import numpy as np
import pytest

import fso
from test_gpu_parity import check_long, run_gpu

pytestmark = pytest.mark.gpu

SHAPES = {
    # m, n, L, K, Brec, mu, seed, kind, block_len
    "2bit": (600, 3000, 30, 8, 600, 5e-4, 62, 0, 128),
    "4bit": (900, 3000, 40, 10, 500, 5e-4, 63, 1, 100),
    "2bit_streamed": (12000, 1200, 20, 12, 300, 3e-4, 65, 0, 100),
    "4bit_streamed": (13000, 1200, 20, 12, 300, 3e-4, 69, 1, 100),
}
REF = {}


def reference(name):
    if name not in REF:
        m, n, L, K, Brec, mu, seed, kind, B = SHAPES[name]
        msa = fso.synth_msa(fso.synth_spec(seed, K, Brec, mu, kind), m, n)
        REF[name] = (msa, fso.segment_long(msa, L, keep_dp=False, threads=4))
    return REF[name]


@pytest.fixture(scope="module")
def pkg():
    return importlib.import_module("founder-sequences_amd")


@pytest.mark.parametrize("name", sorted(SHAPES))
@pytest.mark.parametrize("stride", [4, 32])
def test_every_boundary_state_is_the_oracles(pkg, monkeypatch, name, stride):
    monkeypatch.setenv("FSEQ_REDUCED_ALWAYS", "1")
    monkeypatch.setenv("FSEQ_RED_SS_STRIDE", str(stride))
    msa, ref = reference(name)
    L, B = SHAPES[name][2], SHAPES[name][8]
    ctx = run_gpu(pkg, msa, L, block_len=B)
    assert ctx.timings()["reduced_blocks"] > 0
    check_long(ctx, ref, msa.shape[1], L, check_dp=False)
    S = len(ctx.reduced_traceback())
    assert S == len(ref["a"]) and S > 4
    inside = 0
    for i in range(S):
        a, d = ctx.boundary_state(i)
        assert np.array_equal(a, ref["a"][i]) and np.array_equal(d, ref["d"][i]), i
        inside += int(ctx.reduced_traceback()["rb"][i]) % B != 0
    assert inside > 0                                    # (boundaries strictly inside blocks: the ones the sweeps serve)
