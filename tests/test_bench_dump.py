"""bench.py --dump-outputs on the host: the arrays it writes from a context's last run stay within 64 MB, and when the
boundary states do not all fit, the same seeded sample of them is written every time.  A stand-in context gives C4's
shape (m = 100,000, 24,000 segments); bench.py is imported in a child process so that its environment defaults stay
out of this one."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CHILD = r'''
import os, sys, types
import numpy as np
sys.path.insert(0, sys.argv[1])
import bench
SEG = np.dtype([("lb", "<u8"), ("rb", "<u8"), ("segment_size", "<u4"), ("reserved", "<u4")])
DPA = np.dtype([("lb", "<u8"), ("rb", "<u8"), ("segment_max_size", "<u4"), ("segment_size", "<u4")])

class Ctx:
    m, S = 100000, 24000
    result = types.SimpleNamespace(max_segment_size=37)
    def reduced_traceback(self):
        r = np.zeros(self.S, SEG)
        r["lb"] = np.arange(self.S) * 200
        r["rb"] = r["lb"] + 200
        r["segment_size"] = 5
        return r
    def traceback(self):
        return np.zeros(self.S, DPA)
    def boundary_state(self, i):
        return np.arange(self.m, dtype=np.uint32)[::-1].copy(), np.full(self.m, i, np.uint32)

for d in sys.argv[2:]:
    bench.dump_outputs(Ctx(), d)
'''


def test_dump_outputs_budget_and_seeded_sample(tmp_path):
    import numpy as np
    dirs = [tmp_path / "a", tmp_path / "b"]
    p = subprocess.run([sys.executable, "-c", CHILD, ROOT] + [str(d) for d in dirs], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    for d in dirs:
        assert sum(os.path.getsize(d / f) for f in os.listdir(d)) <= 64 * 10**6
    idx = np.load(dirs[0] / "boundary_index.npy")
    assert 0 < len(idx) < 24000 and np.all(np.diff(idx) > 0) and idx[-1] < 24000
    assert np.array_equal(idx, np.load(dirs[1] / "boundary_index.npy"))
    bd = np.load(dirs[0] / "boundary_d.npy")
    assert bd.dtype == np.float64 and bd.shape == (len(idx), 100000) and np.array_equal(bd[:, 0], idx)
    assert np.array_equal(np.load(dirs[0] / "segments_rb.npy"), np.arange(1, 24001) * 200.0)
