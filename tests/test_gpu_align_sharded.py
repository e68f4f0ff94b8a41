"""GPU: the edge-sharded aligner (a3r_align_shard_*, aligner.ShardedAlignEngine) -- K shard handles on one device, each walking
its own rows of the observations, one flat reduce buffer summed in a fixed order, every replica applying the same update.

The reference of every numeric check is the WHOLE graph: oracle/align_ref.c (AlignOracle) with the bounds tests/test_gpu_align.py
asserts for the monolithic handle (loss 1e-6, gradients 1e-5, loss curve 1e-5, states 1e-4, relative to the tensor max), never the
sharded code itself.  The three cases of tests/golden/alignx.npz (mixed image shapes, trainable pw_adaptors) are checked against
the reference's own goldens with the bounds of tests/test_gpu_alignx.py instead: the C oracle has no pw_adaptors gradient, and
those goldens are what the monolithic engine is pinned to.  K = 7 leaves uneven and, on the small graphs, empty trailing shards
(parallel.shard_rows), which the engine skips."""
import ctypes as C
import functools
import json
import os
import socket

import numpy as np
import pytest
import torch

from conftest import GOLDEN, REPO, record_margin, rel_err
from test_oracle_align import META, NAMES, build

pytestmark = pytest.mark.gpu
KS = (1, 2, 3, 7)


def host(t):
    return t.detach().cpu().numpy()


def Sharded(K, **kw):
    from align3r_amd.aligner import ShardedAlignEngine
    return functools.partial(ShardedAlignEngine, local_shards=K, **kw)


def _scene(edges, N, H, W, seed, mono):                    # the random problem of tests/test_gpu_align.py
    from test_gpu_align import _scene as scene
    return scene(edges, N, H, W, seed, mono)


def _margins_vs_oracle(o, a, nsteps, lr=0.05, schedule="cosine", lr_min=1e-6, total=None):
    lo, go = o.loss_grad()
    la, ga = a.loss_grad()
    m = dict(loss0=abs(lo - la) / lo)
    assert set(go) == set(ga), (sorted(go), sorted(ga))
    for k in go:
        m[f"grad_{k}"] = rel_err(host(ga[k]).reshape(go[k].shape), go[k])
    lo = np.asarray(o.run(nsteps, lr, schedule, lr_min, total_iters=total))
    la = a.run(nsteps, lr, schedule, lr_min, total_iters=total)
    m["losses"] = rel_err(la, lo)
    for k in o.trainable():
        m[f"state_{k}"] = rel_err(host(a.params[k]).reshape(o.params[k].shape), o.params[k])
    return m, la


def _assert_bounds(m, state=1e-4):
    assert m["loss0"] < 1e-6, m
    assert all(v < 1e-5 for k, v in m.items() if k.startswith("grad_")), m
    assert m["losses"] < 1e-5, m
    assert all(v < state for k, v in m.items() if k.startswith("state_")), m


def _replicas_identical(a):
    r0 = a.replicas[0]
    for r in a.replicas[1:]:
        for k in r0.params:
            assert torch.equal(r0.params[k], r.params[k]), k
        for k in r0.adam:
            assert torch.equal(r0.adam[k], r.adam[k]), k
        assert torch.equal(r0.loss_history, r.loss_history)


@pytest.fixture(scope="module")
def g():
    return np.load(os.path.join(GOLDEN, "align.npz"))


@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("case", META["cases"], ids=[c["tag"] for c in META["cases"]])
def test_golden_cases_vs_whole_graph_oracle(case, K, g):
    o = build(case, g)
    a = build(case, g, cls=Sharded(K))
    assert len(a.replicas) == len([1 for r in range(K) if r * -(-len(case["edges"]) // K) < len(case["edges"])])
    eM, iR = a.pose_matrices()
    tag = case["tag"]
    assert rel_err(host(eM), g[tag + "_pw_poses_4x4"][:, :3]) < 1e-6
    assert rel_err(host(iR), g[tag + "_im_poses_4x4"][:, :3]) < 1e-6
    assert abs(float(a.loss().item()) - g[tag + "_loss0"]) / g[tag + "_loss0"] < 1e-6
    m, _ = _margins_vs_oracle(o, a, 20, case["lr"], case["schedule"], case["lr_min"], total=case["niter"])
    record_margin(f"align_sharded_{tag}_K{K}", **m)
    _assert_bounds(m)
    _replicas_identical(a)
    assert a.steps_done == 20


# ------------------------------------------------------------------------------------------------- alignx goldens through the mirror API
XMETA = json.load(open(os.path.join(GOLDEN, "alignx.json")))
ENGINE_KEY = dict(pw_poses="pw_poses", pw_adaptors="pw_adaptors", im_depthmaps="depth", scalemaps="depth", shifts="shifts",
                  im_poses="im_poses", im_focals="im_focals")


@pytest.fixture(scope="module")
def gx():
    return np.load(os.path.join(GOLDEN, "alignx.npz"))


@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("case", XMETA["cases"], ids=[c["tag"] for c in XMETA["cases"]])
def test_mixed_shapes_and_adaptors_through_global_aligner(case, K, gx):
    import align3r_amd
    from align3r_amd.aligner import ShardedAlignEngine
    align3r_amd.install_as_dust3r()
    from dust3r.cloud_opt import global_aligner, GlobalAlignerMode
    tag, edges = case["tag"], [tuple(e) for e in case["edges"]]
    E, N = len(edges), len(case["shapes"])
    tt = lambda key: [torch.from_numpy(gx[f"{tag}_{key}_{e}"]) for e in range(E)]
    out = dict(view1=dict(idx=[i for i, j in edges]), view2=dict(idx=[j for i, j in edges]),
               pred1=dict(pts3d=tt("p1"), conf=tt("c1")), pred2=dict(pts3d_in_other_view=tt("p2"), conf=tt("c2")))
    mono = [torch.from_numpy(gx[f"{tag}_mono_{n}"]) for n in range(N)] if case["use_mono"] else []
    torch.manual_seed(17)
    scene = global_aligner(out, case["use_mono"], mono, "cuda", mode=GlobalAlignerMode.PointCloudOptimizer, verbose=False,
                           min_conf_thr=3, allow_pw_adaptors=case["allow_pw_adaptors"], edge_shards=K)
    eng = scene.engine
    assert isinstance(eng, ShardedAlignEngine)
    init = {ENGINE_KEY[n]: torch.from_numpy(gx[f"{tag}_init_{n}"]) for n in case["trainable"]}
    init["pw_adaptors"] = torch.from_numpy(gx[f"{tag}_init_pw_adaptors"])
    eng.set_params(**{k: v.reshape(eng.params[k].shape) for k, v in init.items()})
    m = {}
    m["pw_poses_4x4"] = rel_err(scene.get_pw_poses().cpu().numpy(), gx[f"{tag}_pw_poses_4x4"])
    m["pts3d0"] = rel_err(scene.get_pts3d(raw=True).cpu().numpy(), gx[f"{tag}_pts3d0"])
    loss, gr = eng.loss_grad()
    m["loss0"] = abs(loss - gx[f"{tag}_loss0"]) / gx[f"{tag}_loss0"]
    assert set(ENGINE_KEY[n] for n in case["trainable"]) == set(gr), (case["trainable"], list(gr))
    for n in case["trainable"]:
        ref = gx[f"{tag}_grad_{n}"]
        m[f"grad_{n}"] = rel_err(gr[ENGINE_KEY[n]].cpu().numpy().reshape(ref.shape), ref)
    losses, done = [], 0
    for k in (1, 5, 50):
        losses += list(eng.run(k - done, case["lr"], case["schedule"], case["lr_min"], first_iter=done, total_iters=case["niter"]))
        done = k
        for n in case["trainable"]:
            ref = gx[f"{tag}_k{k}_{n}"]
            m[f"k{k}_{n}"] = rel_err(eng.params[ENGINE_KEY[n]].cpu().numpy().reshape(ref.shape), ref)
    m["losses"] = rel_err(np.asarray(losses), gx[f"{tag}_losses"])
    record_margin(f"alignx_sharded_{tag}_K{K}", **m)
    assert m["pw_poses_4x4"] < 1e-6 and m["pts3d0"] < 1e-6 and m["loss0"] < 1e-6, m
    assert all(v < 1e-5 for k, v in m.items() if k.startswith("grad_")), m
    assert all(v < 1e-4 for k, v in m.items() if k.startswith("k")), m
    assert m["losses"] < 1e-5, m
    _replicas_identical(eng)


# ------------------------------------------------------------------------------------------------- other graphs
def _other_graph(N, H, W, mono, seed=3):
    from align3r_amd.dust3r.image_pairs import make_pairs
    if N == 16:
        pairs = make_pairs([dict(idx=i) for i in range(N)], "swin-3-noncyclic", symmetrize=True)
        edges = [(a["idx"], b["idx"]) for a, b in pairs]
    else:
        edges = [(i, j) for i in range(N) for j in range(N) if i != j]
    edges, p1, p2, w1, w2, m, init = _scene(edges, N, H, W, seed, mono)
    return ([i for i, j in edges], [j for i, j in edges], p1, p2, w1, w2, [(H, W)] * N), m, init


@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("name,N,H,W,mono,dist", [
    ("ragged_chunk", 3, 37, 41, False, "l1"),       # P = 1517: ragged pixel path, N*P not a multiple of four (buffer padding)
    ("swin16", 16, 24, 32, True, "l1"),             # config-2 graph (84 edges) at reduced resolution
    ("l2", 4, 16, 16, False, "l2"),
])
def test_other_graphs_vs_whole_graph_oracle(name, N, H, W, mono, dist, K):
    from oracle.align_ref import AlignOracle
    args, m, init = _other_graph(N, H, W, mono)
    o = AlignOracle(*args, mono=m, dist=dist)
    a = Sharded(K)(*args, mono=m, dist=dist)
    for eng in (o, a):
        eng.set_params(**init)
    mg, _ = _margins_vs_oracle(o, a, 20)
    record_margin(f"align_sharded_{name}_K{K}", **mg)
    _assert_bounds(mg)
    _replicas_identical(a)


def test_config2_full_size_four_shards_vs_oracle():
    """BASELINE config 2 at full size (N = 16, E = 84, P = 384 x 512) in K = 4 shards of 21 edges, bounds and step count of
    test_gpu_align.py::test_config2_full_size_vs_oracle."""
    from oracle.align_ref import AlignOracle
    args, m, init = _other_graph(16, 384, 512, False, seed=21)
    assert len(args[0]) == 84
    o = AlignOracle(*args)
    a = Sharded(4)(*args)
    assert a.bounds == [(0, 21), (21, 42), (42, 63), (63, 84)]
    for eng in (o, a):
        eng.set_params(**init)
    mg, la = _margins_vs_oracle(o, a, 8)
    record_margin("align_sharded_config2_full_size_K4", **mg)
    _assert_bounds(mg)
    assert la[-1] < la[0]
    _replicas_identical(a)


@pytest.mark.parametrize("K", (2, 3))
def test_norm_pw_scale_coupling_across_shards(K):
    """norm_pw_scale=True couples every edge's log-scale gradient through the mean log-scale: g_e -= (1/E) sum_e' S_e'.  Here the
    log-scales of the first rows are near +2 and those of the last rows near -2, so each shard's own mean differs from the
    graph's by ~2 and a coupling taken per shard (before the reduction) is far outside the bounds."""
    from oracle.align_ref import AlignOracle
    args, m, init = _other_graph(5, 24, 32, False, seed=13)
    E = len(args[0])
    init = dict(init)
    init["pw_poses"] = init["pw_poses"].copy()
    init["pw_poses"][:, 7] = np.where(np.arange(E) < E // 2, 2.0, -2.0) + 0.1 * init["pw_poses"][:, 7]
    o = AlignOracle(*args, norm_pw_scale=True)
    a = Sharded(K)(*args, norm_pw_scale=True)
    for eng in (o, a):
        eng.set_params(**init)
    mg, _ = _margins_vs_oracle(o, a, 20)
    record_margin(f"align_sharded_norm_coupling_K{K}", **mg)
    _assert_bounds(mg)


def test_frozen_parameters_and_no_norm():
    """preset_pose semantics (train_poses / train_focals off, norm_pw_scale off) and train_pp on, against the oracle."""
    from oracle.align_ref import AlignOracle
    args, m, init = _other_graph(4, 16, 24, False, seed=5)
    kw = dict(train_poses=False, train_focals=False, train_pp=True, norm_pw_scale=False)
    o = AlignOracle(*args, **kw)
    a = Sharded(3)(*args, **kw)
    for eng in (o, a):
        eng.set_params(**init)
    before = host(a.params["im_poses"]).copy(), host(a.params["im_focals"]).copy()
    mg, _ = _margins_vs_oracle(o, a, 20)
    _assert_bounds(mg)
    assert "im_pp" in a.trainable() and "im_poses" not in a.trainable()
    assert np.array_equal(before[0], host(a.params["im_poses"])) and np.array_equal(before[1], host(a.params["im_focals"]))


def test_bitwise_reproducible():
    args, m, init = _other_graph(6, 40, 52, False, seed=9)
    outs = []
    for _ in range(2):
        a = Sharded(3)(*args)
        a.set_params(**init)
        losses = a.run(10, 0.05)
        outs.append((losses, {k: host(v).copy() for k, v in a.params.items()}, host(a.replicas[0].buf).copy()))
    assert np.array_equal(outs[0][0], outs[1][0])
    for k in outs[0][1]:
        assert np.array_equal(outs[0][1][k], outs[1][1][k]), k
    assert np.array_equal(outs[0][2], outs[1][2])          # the reduce buffer of the last iteration


def test_record_k1_vs_monolithic_margins():
    """Recorded, not asserted: K = 1 differs from the monolithic handle only in where the per-edge sums are rounded to fp32 (once
    more, in the reduce buffer) -- the largest differences after 20 steps go to profiles/r04_align_sharded_margins.json."""
    from align3r_amd.aligner import AlignEngine
    res = {}
    for name, (N, H, W, mono) in dict(swin16=(16, 24, 32, True), complete6=(6, 72, 96, False)).items():
        args, m, init = _other_graph(N, H, W, mono, seed=11)
        a, b = AlignEngine(*args, mono=m), Sharded(1)(*args, mono=m)
        for eng in (a, b):
            eng.set_params(**init)
        la, lb = a.run(20, 0.05), b.run(20, 0.05)
        r = dict(losses=rel_err(lb, la))
        for k in a.trainable():
            r[f"state_{k}"] = rel_err(host(b.params[k]), host(a.params[k]))
        res[name] = r
        record_margin(f"align_sharded_K1_vs_monolithic_{name}", **r)
    doc = dict(what="max |sharded(K=1) - monolithic| / max |monolithic| after 20 Adam steps (lr 0.05, cosine), same inputs", cases=res)
    try:
        os.makedirs(os.path.join(REPO, "profiles"), exist_ok=True)
        with open(os.path.join(REPO, "profiles", "r04_align_sharded_margins.json"), "w") as f:
            json.dump(doc, f, indent=1, sort_keys=True)
    except OSError:
        pass
    assert all(np.isfinite(v) for r in res.values() for v in r.values())


def test_refusals():
    from align3r_amd import _lib
    from align3r_amd._lib import check
    from align3r_amd.aligner import ShardedAlignEngine
    args, m, init = _other_graph(4, 16, 16, False)
    a = Sharded(2)(*args)
    lib, r = a.lib, a.replicas[0]
    E, N, P = a.E, a.N, a.P
    assert a.n_floats == N * P + 16 * N + 16 * E == lib.a3r_align_shard_reduce_floats(E, N, P)
    short = torch.zeros(a.n_floats - 4, device="cuda")
    with pytest.raises(RuntimeError, match="wrong length"):
        check(lib.a3r_align_shard_partial(r.handle, short.data_ptr(), short.numel(), None))
    with pytest.raises(RuntimeError, match="wrong length"):
        check(lib.a3r_align_shard_apply(r.handle, short.data_ptr(), short.numel(), 0.01, None))
    f = _lib.AlignFlowDesc()
    with pytest.raises(RuntimeError, match="no flow variant"):
        check(lib.a3r_align_set_flow(r.handle, C.byref(f), None))
    with pytest.raises(RuntimeError, match="no depth prior"):
        check(lib.a3r_align_set_depth_prior(r.handle, 1.0, r.params["depth"].data_ptr(), None, r.params["depth"].data_ptr(), 16, None))
    with pytest.raises(RuntimeError, match="edge-shard handle"):
        check(lib.a3r_align_step(r.handle, 0.01, None))
    with pytest.raises(RuntimeError, match="edge-shard handle"):
        check(lib.a3r_align_loss(r.handle, short.data_ptr(), None))
    # creation: empty shard, rows out of range
    h = C.c_void_p()
    d = _lib.AlignDesc()
    d.E, d.N, d.P = E, N, P
    for e0, e1, msg in ((3, 3, "empty shard"), (5, 2, "empty shard"), (-1, 2, "out of range"), (0, E + 1, "out of range")):
        with pytest.raises(RuntimeError, match=msg):
            check(lib.a3r_align_shard_create(C.byref(d), e0, e1, C.byref(h), None))
    # a monolithic handle is not a shard
    from align3r_amd.aligner import AlignEngine
    mono_h = AlignEngine(*args)
    with pytest.raises(RuntimeError, match="not an edge-shard handle"):
        check(lib.a3r_align_shard_partial(mono_h.handle, r.buf.data_ptr(), a.n_floats, None))
    # Python layer
    with pytest.raises(NotImplementedError, match="flow variant"):
        ShardedAlignEngine(*args, local_shards=2, shared_focal=True)
    with pytest.raises(ValueError, match="exactly one"):
        ShardedAlignEngine(*args)
    a.set_params(**init)
    assert np.isfinite(a.run(2, 0.05)).all()              # the handle is still usable after the refused calls


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def test_process_group_of_one_rank_equals_local_shard():
    """The group= branch with a real RCCL process group of world size 1 (one GPU cannot host two ranks): one all_reduce per
    iteration, and bit for bit the results of local_shards=1."""
    import torch.distributed as dist
    from align3r_amd.aligner import ShardedAlignEngine
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ["MASTER_PORT"] = str(_free_port())
    dev = torch.device("cuda", 0)
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=dev)
    try:
        args, m, init = _other_graph(5, 40, 52, False, seed=7)
        a = ShardedAlignEngine(*args, group=dist.group.WORLD)
        b = ShardedAlignEngine(*args, local_shards=1)
        for eng in (a, b):
            eng.set_params(**init)
        la, lb = a.run(12, 0.05), b.run(12, 0.05)
        torch.cuda.synchronize()
        assert a.collectives == 12 and b.collectives == 0
        assert np.array_equal(la, lb)
        for k in a.params:
            assert torch.equal(a.params[k], b.params[k]), k
        ga, gb = a.loss_grad(), b.loss_grad()
        assert a.collectives == 13
        assert ga[0] == gb[0]
        for k in ga[1]:
            assert torch.equal(ga[1][k], gb[1][k]), k
    finally:
        dist.destroy_process_group()
