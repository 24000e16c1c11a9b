"""world_size-2 gloo tests (CPU) of the N > 1 path.

The real shard arithmetic -- block range per rank, hyper key block exchange, sharded speculative DP with its
per-sweep key exchange, threshold merge, pass 2 on the owners -- runs here as its Python model
(tests/proto_shard.py, the statement of what the path's units, csrc/fseq_path_*.hip, do with sh.on) in two processes whose ONLY
connection is torch.distributed all_reduce over gloo, the same primitive (fseq_allreduce_fn) the library asks
bench.py's ShardTransport for on the GPUs.  Every rank's result must equal the oracle's serial walk.  Also the
launcher logic bench.py uses: env ranks, barrier + max-over-ranks timing."""
import importlib
import os
import socket
import sys

import numpy as np
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

HERE = os.path.dirname(os.path.abspath(__file__))


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, world, port, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), LOCAL_RANK=str(rank), WORLD_SIZE=str(world))
    for p in (HERE, os.path.dirname(HERE), os.path.join(os.path.dirname(HERE), "oracle")):
        if p not in sys.path:
            sys.path.insert(0, p)
    import fso
    import proto_shard as ps
    d = importlib.import_module("founder-sequences_amd.dist")
    dist.init_process_group(backend="gloo", rank=rank, world_size=world)
    try:
        assert d.env_rank() == (rank, rank, world)
        calls = []

        def allreduce(arr, op):
            t = torch.from_numpy(np.ascontiguousarray(arr, dtype=np.int64).copy())
            dist.all_reduce(t, op=dist.ReduceOp.SUM if op == 0 else dist.ReduceOp.MAX)
            calls.append(t.numel())
            return t.numpy()

        m, n, L, B, X = 14, 900, 8, 20, 2                      # X = 2: the ranks find the lists too short together and retry
        msa = fso.synth_msa(fso.synth_spec(31, 3, 70, 5e-3, 0), m, n)
        codes = np.searchsorted(np.unique(msa), msa).astype(np.int64)
        out = {}

        def step():
            out["r"] = ps.segment_sharded(codes, L, B, X, rank, world, allreduce, forced_rounds=3)

        dt = d.timed_steps(step, steps=1, warmup=0, dist=dist, device_sync=None,
                           tensor_factory=lambda v: torch.tensor(v, dtype=torch.float64))
        r = out["r"]
        ref = fso.segment_long(msa, L, keep_dp=True, threads=1)
        w = np.ones(n - L + 1, dtype=bool)
        w[n - 2 * L + 1:n - L] = False
        ok = (r["max_segment_size"] == ref["max_segment_size"]
              and np.array_equal(r["M"][w], ref["dp"]["segment_max_size"][w])
              and np.array_equal(r["LB"][w], ref["dp"]["lb"][w].astype(np.int64))
              and np.array_equal(r["SZ"][w], ref["dp"]["segment_size"][w])
              and [tuple(x) for x in r["reduced"]] == [(int(x["lb"]), int(x["rb"]), int(x["segment_size"])) for x in ref["reduced"]]
              and all(np.array_equal(sa, ref["a"][i]) and np.array_equal(sd, ref["d"][i]) for i, (sa, sd) in r["snaps"].items()))
        g = r["geometry"]
        q.put((rank, ok, sorted(r["snaps"]), len(ref["reduced"]), (g["c_lo"], g["c_hi"], g["c_end"]), len(calls), dt, r["X"]))
    finally:
        dist.destroy_process_group()


def test_two_ranks_shard_one_alignment_over_gloo():
    world = 2
    port = _free_port()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    out = sorted(q.get(timeout=300) for _ in range(world))
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    (r0, ok0, snaps0, S, cols0, calls0, t0, x0), (r1, ok1, snaps1, _, cols1, calls1, t1, x1) = out
    assert ok0 and ok1                                      # both ranks hold the oracle's result
    assert snaps0 and snaps1 and not set(snaps0) & set(snaps1)
    assert sorted(snaps0 + snaps1) == list(range(S))        # every boundary state on exactly one rank
    assert cols0[0] == 0 and cols0[1] == cols1[0] and cols1[1] == 900      # contiguous shares of the columns
    assert cols0[2] > cols0[1]                              # rank 0 reads a halo of the next rank's columns
    assert calls0 == calls1 and calls0 >= 8                 # the same exchanges on both sides
    assert abs(t0 - t1) < 1e-9                              # both ranks report the max over ranks
    assert x0 == x1 and x0 > 2                              # the retry with longer lists happened on both


def _rowshard_worker(rank, world, port, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), LOCAL_RANK=str(rank), WORLD_SIZE=str(world))
    for p in (HERE, os.path.dirname(HERE), os.path.join(os.path.dirname(HERE), "oracle")):
        if p not in sys.path:
            sys.path.insert(0, p)
    import fso
    import proto_shard as ps
    dist.init_process_group(backend="gloo", rank=rank, world_size=world)
    try:
        def allreduce(arr, op):
            t = torch.from_numpy(np.ascontiguousarray(arr, dtype=np.int64).copy())
            dist.all_reduce(t, op=dist.ReduceOp.SUM if op == 0 else dist.ReduceOp.MAX)
            return t.numpy()

        ok = True
        calls = []
        for (m, n, K, B, mu, seed, kind) in [(41, 60, 4, 20, 2e-2, 71, 0), (30, 25, 5, 10, 3e-2, 72, 1)]:
            msa = fso.synth_msa(fso.synth_spec(seed, K, B, mu, kind), m, n)
            al = np.unique(msa)
            codes = np.searchsorted(al, msa).astype(np.int64)
            a, d, c = ps.rowshard_pbwt(codes, n, rank, world, allreduce, sigma=len(al))
            p = fso.Pbwt(msa)
            while p.idx < n:
                p.step()
            ok = ok and np.array_equal(a, p.a) and np.array_equal(d, p.d)
            calls.append(c)
        q.put((rank, bool(ok), calls))
    finally:
        dist.destroy_process_group()


def test_two_ranks_row_shard_the_pbwt_over_gloo():
    """The north-star partition (positions of the order over the ranks; per column the column, one summary per rank,
    the scatter -- csrc/fseq_rowshard.hpp) as its Python model in two processes joined by gloo all-reduces only."""
    world = 2
    port = _free_port()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_rowshard_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    out = sorted(q.get(timeout=300) for _ in range(world))
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    assert out[0][1] and out[1][1]
    assert out[0][2] == out[1][2] == [1 + 2 * 60, 1 + 2 * 2 * 25]      # two exchanges per column and 2-bit digit


def test_assignment_covers_everything_once():
    d = importlib.import_module("founder-sequences_amd.dist")
    for n in (0, 1, 7, 22, 64):
        for world in (1, 2, 3, 8):
            got = sum((d.alignments_for_rank(n, r, world) for r in range(world)), [])
            assert got == list(range(n))
    assert d.aggregate_cells_per_second(10, 3, 2, 2.0) == 30.0
