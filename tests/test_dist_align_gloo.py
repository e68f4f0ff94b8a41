"""CPU, 2 processes over gloo: the PLUMBING of the edge-sharded aligner -- shard bounds from parallel.shard_rows, one flat additive
buffer, exactly one all_reduce(SUM) per iteration (parallel.GradientAllReduce driven by parallel.sharded_step, the same two pieces
aligner.ShardedAlignEngine's group= form uses), replicated state identical on both ranks and equal to a one-process run.

The HIP kernels are NOT exercised here: the partial step is a CPU stand-in, oracle/align_ref.c evaluated on each rank's edge rows
with norm_pw_scale=False and images of one size -- there the loss and every gradient are additive over edges (the oracle
normalises by the edge count of what it is given, so a shard's results are rescaled by E_shard / E).  The kernels and the
post-reduction scale coupling are covered on the GPU by tests/test_gpu_align_sharded.py."""
import ctypes as C
import os
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from conftest import rel_err
from align3r_amd.parallel import GradientAllReduce, shard_rows, sharded_step

KEYS = ("pw_poses", "depth", "im_poses", "im_focals")
NITER, LR = 6, 0.05


def _problem(N=4, H=8, W=12, seed=2):
    rng = np.random.default_rng(seed)
    edges = [(i, j) for i in range(N) for j in range(N) if i != j]
    E, P = len(edges), H * W
    p1 = rng.standard_normal((E, P, 3)).astype(np.float32)
    p2 = rng.standard_normal((E, P, 3)).astype(np.float32)
    w1 = np.log(1 + 9 * rng.random((E, P))).astype(np.float32)
    w2 = np.log(1 + 9 * rng.random((E, P))).astype(np.float32)
    init = dict(pw_poses=rng.standard_normal((E, 8)).astype(np.float32), depth=(0.1 * rng.standard_normal((N, P)) - 3).astype(np.float32),
                im_poses=rng.standard_normal((N, 7)).astype(np.float32), im_focals=np.full(N, 20 * np.log(max(H, W)), np.float32))
    return edges, p1, p2, w1, w2, [(H, W)] * N, init


def _lrs():
    from oracle.align_ref import schedule_lr
    return [float(schedule_lr("cosine", it / NITER, LR, 1e-6)) for it in range(NITER)]


class _ShardStandIn:
    """partial / apply of one rank: `sub` evaluates the rank's edge rows, `full` holds the replicated state and runs the oracle's Adam."""

    def __init__(self, rank, world):
        from oracle.align_ref import AlignOracle
        edges, p1, p2, w1, w2, shapes, init = _problem()
        self.E = E = len(edges)
        self.e0, self.e1, _ = shard_rows(E, rank, world)
        sl = slice(self.e0, self.e1)
        ei, ej = [i for i, j in edges], [j for i, j in edges]
        self.full = AlignOracle(ei, ej, p1, p2, w1, w2, shapes, norm_pw_scale=False)
        self.sub = AlignOracle(ei[sl], ej[sl], p1[sl], p2[sl], w1[sl], w2[sl], shapes, norm_pw_scale=False)
        self.full.set_params(**init)
        self.sizes = [self.full.params[k].size for k in KEYS]
        self.losses = []

    def partial(self):
        p = self.full.params
        self.sub.set_params(p["pw_poses"][self.e0:self.e1], p["depth"], p["im_poses"], p["im_focals"])
        loss, g = self.sub.loss_grad()
        scale = (self.e1 - self.e0) / self.E
        g_pw = np.zeros_like(p["pw_poses"])
        g_pw[self.e0:self.e1] = g["pw_poses"]                       # rows outside the shard are zero
        parts = [np.float32([loss])] + [np.asarray(a, np.float32).ravel() for a in (g_pw, g["depth"], g["im_poses"], g["im_focals"])]
        return torch.from_numpy(np.concatenate(parts) * np.float32(scale))

    def apply(self, buf, lr):
        flat = buf.numpy()
        loss, off, g = float(flat[0]), 1, {}
        for k, n in zip(KEYS, self.sizes):
            g[k] = flat[off:off + n].reshape(self.full.params[k].shape).copy()
            off += n
        self.full.loss_grad = lambda epoch=9999: (loss, g)          # the oracle's own Adam on the REDUCED gradients
        self.losses.append(self.full.step(lr))


def _worker(rank, world, port, out_dir):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    s = _ShardStandIn(rank, world)
    reduce = GradientAllReduce(dist.group.WORLD)
    for lr in _lrs():
        sharded_step(s.partial, reduce, s.apply, lr)
    torch.save(dict(params={k: s.full.params[k].copy() for k in KEYS}, losses=s.losses, calls=reduce.calls, rows=(s.e0, s.e1)),
               os.path.join(out_dir, f"rank{rank}.pt"))
    dist.destroy_process_group()


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def test_two_ranks_one_collective_per_iteration(tmp_path):
    from oracle.align_ref import AlignOracle
    world = 2
    mp.spawn(_worker, args=(world, _free_port(), str(tmp_path)), nprocs=world, join=True)
    got = [torch.load(os.path.join(tmp_path, f"rank{r}.pt"), weights_only=False) for r in range(world)]
    edges, p1, p2, w1, w2, shapes, init = _problem()
    assert [g["rows"] for g in got] == [(0, 6), (6, 12)]
    assert all(g["calls"] == NITER for g in got)                     # exactly one all-reduce per iteration
    for k in KEYS:                                                   # the replicas never diverge
        assert np.array_equal(got[0]["params"][k], got[1]["params"][k]), k
    assert got[0]["losses"] == got[1]["losses"]
    one = AlignOracle([i for i, j in edges], [j for i, j in edges], p1, p2, w1, w2, shapes, norm_pw_scale=False)
    one.set_params(**init)
    ref = [one.step(lr) for lr in _lrs()]
    # the same sums in another order (per shard, then across ranks, in fp32): equal to rounding, not bit for bit
    assert rel_err(got[0]["losses"], ref) < 1e-5
    for k in KEYS:
        assert rel_err(got[0]["params"][k], one.params[k]) < 1e-4, k


def test_shard_creation_refusals_need_no_gpu():
    from align3r_amd import _lib
    lib = _lib.load()
    d, h = _lib.AlignDesc(), C.c_void_p()
    d.E, d.N, d.P = 12, 4, 96
    for e0, e1, msg in ((4, 4, b"empty shard"), (7, 3, b"empty shard"), (-2, 3, b"out of range"), (6, 13, b"out of range")):
        assert lib.a3r_align_shard_create(C.byref(d), e0, e1, C.byref(h), None) != 0
        assert msg in lib.a3r_last_error()
    assert lib.a3r_align_shard_reduce_floats(12, 4, 96) == 4 * 96 + 16 * 4 + 16 * 12
    assert lib.a3r_align_shard_reduce_floats(2, 3, 1517) == 4552 + 16 * 3 + 16 * 2      # N*P rounded up to a multiple of four
    assert 0 < lib.a3r_align_shard_workspace_bytes(4032, 504, 64, 147456) < lib.a3r_align_workspace_bytes(4032, 64, 147456)
    assert lib.a3r_align_shard_workspace_bytes(84, 84, 16, 196608) == lib.a3r_align_workspace_bytes(84, 16, 196608)


def test_sharded_engine_refuses_cpu_and_flow_variant():
    from align3r_amd.aligner import ShardedAlignEngine
    args = ([0, 1], [1, 0], np.zeros((2, 4, 3)), np.zeros((2, 4, 3)), np.zeros((2, 4)), np.zeros((2, 4)), [(2, 2)] * 2)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ShardedAlignEngine(*args, device="cpu", local_shards=2)
    with pytest.raises(NotImplementedError, match="flow variant"):
        ShardedAlignEngine(*args, device="cpu", local_shards=2, temporal_smoothing_weight=0.1)
    from align3r_amd.dust3r.cloud_opt_flow.optimizer import PointCloudOptimizer as FlowOptimizer
    with pytest.raises(NotImplementedError, match="edge_shards"):
        FlowOptimizer(dict(idx=[0, 1]), dict(idx=[1, 0]), {}, {}, edge_shards=2)
