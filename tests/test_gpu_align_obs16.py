"""GPU: packed fp16 pair observations of the aligner (AlignEngine(obs_dtype='fp16'), csrc/obs.hip, the packed kernels of align.hip).

The mode is DEFINED as the fp32 aligner run on the decoded observations (align3r_amd/obs16.py), so every comparison here is made
on engine.decoded_observations(): against the float64 oracle built from them, with the bounds of tests/test_gpu_align_paths.py
(first loss 1e-6, gradients 1e-5 of the tensor maximum, trajectory losses 1e-5, states 1e-4), and against the fp32 engine fed the
same arrays (same bounds; whether the two are bitwise equal is recorded, not required: the compiler may contract differently
around the decode).  The packer itself is compared bit for bit with the numpy definition.

Problems are those of tests/align_cases.py / tests/test_align_cases_cpu.py and _scene of tests/test_gpu_align.py: at most 15 frames
of 2080 pixels, one oracle evaluation well under a second."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import align_cases as ac
from conftest import GOLDEN, record_margin, rel_err
from test_align_cases_cpu import flow_case, prior_case
from test_align_obs16_cpu import row_kinds
from test_gpu_align import _scene, host

pytestmark = pytest.mark.gpu

TOL = dict(loss=1e-6, grad=1e-5, losses=1e-5, state=1e-4)


def _engines():
    from align3r_amd.aligner import AlignEngine, ShardedAlignEngine
    return AlignEngine, ShardedAlignEngine


def _check(case, margins, **info):
    record_margin("align_obs16_" + case, **margins, **info)
    for k, v in margins.items():
        assert np.isfinite(v) and v < TOL[k.split("_")[0]], (case, k, v, margins)


# ------------------------------------------------------------------------------------------------- 1. the packer
def _pack_on_device(pred, w, rows=None):
    """a3r_align_pack_obs on the rows [r0, r1) of device copies of pred / w, into buffers pre-filled with a marker."""
    from align3r_amd import _lib
    lib = _lib.load()
    R, P = w.shape
    r0, r1 = rows or (0, R)
    dp, dw = torch.from_numpy(pred).cuda(), torch.from_numpy(w).cuda()
    obs = torch.full((R, P, 4), 0x7B7B, dtype=torch.int16, device="cuda")
    exps = torch.full((R,), -777, dtype=torch.int32, device="cuda")
    _lib.check(lib.a3r_align_pack_obs(_lib.ptr(dp[r0:r1]), _lib.ptr(dw[r0:r1]), r1 - r0, P, _lib.ptr(obs[r0:r1]), _lib.ptr(exps[r0:r1]),
                                      _lib.stream_ptr()), "a3r_align_pack_obs")
    torch.cuda.synchronize()
    return obs.cpu().numpy().view(np.uint16), exps.cpu().numpy()


@pytest.mark.parametrize("P", [1028, 1030], ids=["vec_1028", "scalar_tail_1030"])
def test_packer_bitwise_vs_numpy(P):
    """Seven row kinds (N(0,1), x 1e6, x 1e-30, max exactly 8, max nextafter(8, 0), all zero, inf / nan); P = 1028 is one quad past a
    1024-thread pass of the 16-byte path, P = 1030 takes the scalar path.  Records and exponents equal pack_reference exactly; a
    row range from the middle of the buffers (rows 2..5) leaves its neighbours untouched and gives what the whole call gives."""
    from align3r_amd import obs16
    pred, w = row_kinds(P)
    rec, k = obs16.pack_reference(pred, w)
    want = rec.view(np.uint16)
    got, gk = _pack_on_device(pred, w)
    assert np.array_equal(gk, k), (gk, k)
    diff = got != want
    assert not diff.any(), (int(diff.sum()), np.argwhere(diff)[:5], got[diff][:5], want[diff][:5])
    part, pk = _pack_on_device(pred, w, rows=(2, 5))
    assert np.array_equal(pk[2:5], k[2:5]) and np.array_equal(part[2:5], want[2:5])
    assert (pk[:2] == -777).all() and (pk[5:] == -777).all()
    assert (part[:2] == 0x7B7B).all() and (part[5:] == 0x7B7B).all()


# ------------------------------------------------------------------------------------------------- 2. + 3. engine vs oracle and vs fp32
def _first_eval(ref, a, epoch, tag, zero_rows=None):
    lo, go = ref.loss_grad(epoch)
    la, ga = a.loss_grad(epoch)
    assert set(go) == set(ga)
    m = {f"loss_{tag}": abs(lo - la) / abs(lo)}
    equal = True
    for k in go:
        want = np.array(host(go[k]) if torch.is_tensor(go[k]) else go[k], dtype=np.float64)
        got = host(ga[k]).reshape(want.shape)
        for key, rows in (zero_rows or {}).items():
            if key == k:
                assert np.all(got[rows] == 0), (k, "a frozen group's gradient rows are exact zeros")
                want[rows] = 0
        m[f"grad_{tag}_{k}"] = rel_err(got, want)
        equal = equal and np.array_equal(got.astype(np.float32), want.astype(np.float32))
    return m, equal and float(lo) == float(la)


def _trajectory(ref, a, steps, lr, schedule, total, tag):
    lo = np.asarray(ref.run(steps, lr, schedule, total_iters=total))
    la = a.run(steps, lr, schedule, total_iters=total)
    m = {f"losses_{tag}": rel_err(la, lo)}
    equal = np.array_equal(np.asarray(la, np.float32), np.asarray(lo, np.float32))
    for k in a.trainable():
        want = host(ref.params[k]) if torch.is_tensor(ref.params[k]) else ref.params[k]
        got = host(a.params[k]).reshape(want.shape)
        m[f"state_{tag}_{k}"] = rel_err(got, want)
        equal = equal and np.array_equal(got, np.asarray(want, np.float32))
    return m, equal


def _run_case(case, args, kw, init, steps, lr, schedule, total=None, epoch=9999, prior=None, make_a=None, masks=None, zero_rows=None,
              loss_only=True):
    """fp16 engine `a` against (o) the oracle and (b) the fp32 engine, both built from a.decoded_observations()."""
    from oracle.align_ref import AlignOracle
    Engine, _ = _engines()
    a = make_a(*args, obs_dtype="fp16", **kw) if make_a else Engine(*args, obs_dtype="fp16", **kw)
    dec = [host(t) for t in a.decoded_observations()]
    E, P = dec[2].shape
    assert dec[0].shape == (E, P, 3) and all(d.dtype == np.float32 for d in dec)
    assert a.observation_bytes == 16 * E * P + 8 * E
    args_dec = (args[0], args[1], *dec, args[6])
    o, b = AlignOracle(*args_dec, **kw), Engine(*args_dec, obs_dtype="fp32", **kw)
    for eng in (o, a, b):
        eng.set_params(**init)
        if prior is not None:
            eng.set_depth_prior(**prior)
    if masks is not None:
        a.set_train_masks(**masks)
        b.set_train_masks(**masks)
    m, _ = _first_eval(o, a, epoch, "o", zero_rows)
    mb, eq_first = _first_eval(b, a, epoch, "f")
    m.update(mb)
    if loss_only:
        m["loss_only_o"] = abs(float(a.loss().item()) - o.loss_grad(epoch)[0]) / abs(o.loss_grad(epoch)[0])
    frozen = None
    if masks is not None:
        frozen = {k: v.clone() for k, v in a.params.items()}, {k: v.clone() for k, v in a.adam.items()}
        lb = b.run(steps, lr, schedule, total_iters=total)          # the oracle has no per-image masks: the trajectory is b's
        la = a.run(steps, lr, schedule, total_iters=total)
        m["losses_f"] = rel_err(la, lb)
        eq_run = np.array_equal(la, lb)
        for k in a.trainable():
            m[f"state_f_{k}"] = rel_err(host(a.params[k]), host(b.params[k]))
            eq_run = eq_run and torch.equal(a.params[k], b.params[k])
    else:
        mo, _ = _trajectory(o, a, steps, lr, schedule, total, "o")
        m.update(mo)
        lb = b.run(steps, lr, schedule, total_iters=total)
        m["losses_f"] = rel_err(a.loss_history[:steps].cpu().numpy(), lb)
        eq_run = torch.equal(a.loss_history[:steps], b.loss_history[:steps])
        for k in a.trainable():
            m[f"state_f_{k}"] = rel_err(host(a.params[k]), host(b.params[k]))
            eq_run = eq_run and torch.equal(a.params[k], b.params[k])
    _check(case, m, bitwise_equal_to_fp32_first=float(eq_first), bitwise_equal_to_fp32_run=float(eq_run))
    return a, b, frozen


CONFIGS = [(False, "l1"), (True, "l1"), (False, "l2"), (True, "l2")]


@pytest.mark.parametrize("mono,dist", CONFIGS, ids=[("mono_" if m else "") + d for m, d in CONFIGS])
def test_complete_graph_vs_oracle(mono, dist):
    """Complete graph of 4 images at 36 x 44 (P = 1584: two chunks, a ragged last one): loss(), loss_grad(), 20 cosine steps in
    the four (mono, dist) instantiations of the packed kernels, modes 0 / 1 / 2."""
    N, H, W = 4, 36, 44
    edges, p1, p2, w1, w2, m, init = _scene(ac.complete_graph(N), N, H, W, 3, mono)
    args = ([i for i, j in edges], [j for i, j in edges], p1, p2, w1, w2, [(H, W)] * N)
    _run_case(f"complete_{'mono_' if mono else ''}{dist}", args, dict(mono=m, dist=dist), init, 20, 0.05, "cosine")


def _degree_problem(H, W, seed=3):
    edges, N = ac.degree_class_graph()
    edges, p1, p2, w1, w2, _, init = _scene(edges, N, H, W, seed, False)
    init.pop("shifts")
    return edges, N, ([i for i, j in edges], [j for i, j in edges], p1, p2, w1, w2, [(H, W)] * N), init


def test_degree_classes_train_pp_vs_oracle():
    """1 to 17 incident edge sides per image (batch rollover, the 2-deep prefetch with odd and even counts) at 40 x 52, train_pp."""
    edges, N, args, init = _degree_problem(40, 52)
    init["im_pp"] = (0.05 * np.random.default_rng(17).standard_normal((N, 2))).astype(np.float32)
    _run_case("degree_train_pp", args, dict(train_pp=True), init, 20, 0.05, "cosine")


def test_exponents_twenty_apart_vs_oracle():
    """Two edges' predictions multiplied by 2^10 and 2^-10, their log-scales offset by -/+ 10 ln 2 to compensate: the rows'
    exponents move by exactly -/+ 10 (20 apart), the per-edge factor is what keeps the result within the same bounds."""
    from align3r_amd import obs16
    edges, N, args, init = _degree_problem(36, 44)
    e_up, e_dn = 10, 11
    k0_i, k0_j = obs16.row_exponents(args[2]), obs16.row_exponents(args[3])
    p1, p2 = args[2].copy(), args[3].copy()
    for p in (p1, p2):
        p[e_up] *= np.float32(2.0 ** 10)
        p[e_dn] *= np.float32(2.0 ** -10)
    init["pw_poses"] = init["pw_poses"].copy()
    init["pw_poses"][e_up, 7] -= np.float32(10 * np.log(2))
    init["pw_poses"][e_dn, 7] += np.float32(10 * np.log(2))
    args = (args[0], args[1], p1, p2) + args[4:]
    a, _, _ = _run_case("exponents_20_apart", args, {}, init, 20, 0.05, "cosine")
    shift = np.zeros(len(edges), np.int32)
    shift[e_up], shift[e_dn] = -10, 10
    assert np.array_equal(host(a.exp_i), k0_i + shift) and np.array_equal(host(a.exp_j), k0_j + shift)
    assert host(a.exp_i)[e_dn] - host(a.exp_i)[e_up] == 20 + k0_i[e_dn] - k0_i[e_up]
    for k0 in (k0_i, k0_j):
        assert abs(int(k0[e_dn]) - int(k0[e_up])) <= 1          # N(0,1) rows of 4752 values: maxima within one binade of each other


def test_flow_variant_vs_oracle():
    """flow_case('v36x44_deg_sf', loose): first evaluation with the ego-flow term on, then 10 linear steps across its start gate."""
    prob = flow_case("v36x44_deg_sf", False)
    a, _, _ = _run_case("flow_v36x44_deg_sf", prob["args"], prob["kw"], prob["init"], 10, 0.01, "linear", total=50)
    assert not a.flow_dropped


def test_depth_prior_with_flow_vs_oracle():
    """prior_case('p40x52_flow'): the depth prior and the ego-flow pass in front of the packed main kernel, first evaluation, 10 steps."""
    prob = prior_case("p40x52_flow")
    _run_case("prior_p40x52_flow", prob["args"], prob["kw"], prob["init"], 10, 0.01, "linear", total=50, prior=prob["prior"])


def test_sharded_three_local_shards_vs_whole_graph_oracle():
    """ShardedAlignEngine(local_shards=3, obs_dtype='fp16') on the degree-class graph: each shard walks its rows of the packed
    buffers and of the exponent tables; against the whole-graph oracle, replicas identical bit for bit."""
    import functools
    _, Sharded = _engines()
    edges, N, args, init = _degree_problem(36, 44)
    a, _, _ = _run_case("sharded_K3", args, {}, init, 20, 0.05, "cosine", make_a=functools.partial(Sharded, local_shards=3),
                        loss_only=False)
    assert len(a.replicas) == 3
    r0 = a.replicas[0]
    for r in a.replicas[1:]:
        for k in r0.params:
            assert torch.equal(r0.params[k], r.params[k]), k
        for k in r0.adam:
            assert torch.equal(r0.adam[k], r.adam[k]), k
        assert torch.equal(r0.loss_history, r.loss_history)


def test_sharded_group_form_equals_local_shard():
    """ShardedAlignEngine(group=..., obs_dtype='fp16') with a real process group of world size 1 (one GPU cannot host two ranks):
    the rank packs its own rows, one all-reduce per iteration, and bit for bit the results of local_shards=1 with packed rows."""
    import socket
    import torch.distributed as dist
    _, Sharded = _engines()
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda", 0))
    try:
        edges, N, args, init = _degree_problem(36, 44)
        a = Sharded(*args, group=dist.group.WORLD, obs_dtype="fp16")
        b = Sharded(*args, local_shards=1, obs_dtype="fp16")
        assert a.obs_dtype == "fp16" and a.pred_i is None and torch.equal(a.exp_i, b.exp_i)
        assert torch.equal(a.obs_i.view(torch.int16), b.obs_i.view(torch.int16))
        for eng in (a, b):
            eng.set_params(**init)
        la, lb = a.run(8, 0.05), b.run(8, 0.05)
        torch.cuda.synchronize()
        assert a.collectives == 8 and np.array_equal(la, lb) and np.isfinite(la).all()
        for k in a.params:
            assert torch.equal(a.params[k], b.params[k]), k
    finally:
        dist.destroy_process_group()


def test_train_masks_keep_frozen_bits():
    """One frozen pose (image 2) and one frozen depth map (image 3): over 5 steps their parameters and Adam moments keep their
    bits; the gradients against the oracle have exact zeros in the frozen rows, the rest and the trajectory (against the fp32
    engine with the same masks: the oracle has none) meet the bounds."""
    edges, N, args, init = _degree_problem(36, 44)
    pose, depth = np.ones(N, bool), np.ones(N, bool)
    pose[2], depth[3] = False, False
    a, _, (p0, m0) = _run_case("train_masks", args, {}, init, 5, 0.05, "cosine", masks=dict(pose=pose, depth=depth),
                               zero_rows=dict(im_poses=2, depth=3))
    assert a.steps_done == 5
    assert torch.equal(a.params["im_poses"][2], p0["im_poses"][2]) and torch.equal(a.adam["small"][:, 2, :7], m0["small"][:, 2, :7])
    assert torch.equal(a.params["depth"][3], p0["depth"][3]) and torch.equal(a.adam["depth"][:, 3], m0["depth"][:, 3])
    assert not torch.equal(a.params["im_poses"][1], p0["im_poses"][1]) and not torch.equal(a.params["depth"][2], p0["depth"][2])


# ------------------------------------------------------------------------------------------------- accuracy: AbsRel on the defined function
def test_absrel_within_1e4_of_oracle_on_decoded_observations():
    """The north-star bound of test_adam_trajectory_vs_reference (AbsRel within 1e-4, same synthetic ground truth and LAD rule),
    applied to the function the mode defines: 300 cosine iterations on the config-2 graph (16 frames, 84 edges) at 24 x 32, the
    fp16 engine against the oracle on the decoded observations.  (What fp16 storage costs against fp32 storage is measured by
    tools/bench_align_obs.py at config-2 size and written down in DESIGN.md 6.8; no threshold is put on it.)"""
    from oracle.align_ref import AlignOracle
    from align3r_amd.dust3r.image_pairs import make_pairs
    from align3r_amd.tool.depth_metrics import evaluate_depth
    Engine, _ = _engines()
    N, H, W = 16, 24, 32
    pairs = make_pairs([dict(idx=i) for i in range(N)], "swin-3-noncyclic", symmetrize=True)
    edges, p1, p2, w1, w2, _, init = _scene([(x["idx"], y["idx"]) for x, y in pairs], N, H, W, 3, False)
    init.pop("shifts")
    args = ([i for i, j in edges], [j for i, j in edges], p1, p2, w1, w2, [(H, W)] * N)
    a = Engine(*args, obs_dtype="fp16")
    o = AlignOracle(args[0], args[1], *[host(t) for t in a.decoded_observations()], args[6])
    for eng in (o, a):
        eng.set_params(**init)
    o.run(300, 0.05, "cosine")
    a.run(300, 0.05, "cosine")
    d_ref = np.exp(o.params["depth"].astype(np.float64)).reshape(N, -1)
    d_hip = np.exp(host(a.params["depth"]).astype(np.float64)).reshape(N, -1)
    yy = np.linspace(0, 1, d_ref[0].size).reshape(1, -1)
    gt = (2.0 * d_ref + 0.1) * (1 + 0.2 * np.sin(7 * yy + np.arange(N)[:, None]))
    m_ref = evaluate_depth(d_ref.reshape(N, 1, -1), gt.reshape(N, 1, -1), depth_max=1e9, mode="lad")
    m_hip = evaluate_depth(d_hip.reshape(N, 1, -1), gt.reshape(N, 1, -1), depth_max=1e9, mode="lad")
    record_margin("align_obs16_absrel", abs_rel_oracle=m_ref["abs_rel"], abs_rel_fp16=m_hip["abs_rel"],
                  diff=abs(m_hip["abs_rel"] - m_ref["abs_rel"]))
    assert m_ref["abs_rel"] > 0.01
    assert abs(m_hip["abs_rel"] - m_ref["abs_rel"]) < 1e-4, (m_hip, m_ref)


# ------------------------------------------------------------------------------------------------- 4. memory
def test_observation_bytes_and_device_memory():
    """Degree-class graph at 40 x 52 (E = 57, P = 2080): observation_bytes is 16 E P + 8 E packed and 32 E P in fp32.  The caching
    allocator hands out buffers of this size in 2 MiB granules, and an engine holds 4 (fp32) or 4 (packed: 2 record buffers, 2
    exponent tables) observation buffers, 6 granules of slack in all: the allocated bytes after construction must differ by at
    least 16 E P minus 6 x 2 MiB.  (At this size that bound is below zero -- it is stated for the rule, observation_bytes is the
    check that bites -- and the measured difference is recorded.)"""
    Engine, _ = _engines()
    edges, N, args, init = _degree_problem(40, 52)
    E, P = len(edges), 40 * 52
    assert (E, P) == (57, 2080)
    torch.cuda.synchronize()
    used = {}
    for dt in ("fp32", "fp16"):
        before = torch.cuda.memory_allocated()
        a = Engine(*args, obs_dtype=dt)
        torch.cuda.synchronize()
        used[dt] = torch.cuda.memory_allocated() - before
        assert a.observation_bytes == (32 * E * P if dt == "fp32" else 16 * E * P + 8 * E)
        if dt == "fp16":
            assert a.pred_i is None and a.w_i is None and a.obs_i.dtype == torch.float16 and tuple(a.obs_i.shape) == (E, P, 4)
        del a
    record_margin("align_obs16_memory", allocated_fp32=float(used["fp32"]), allocated_fp16=float(used["fp16"]),
                  saved=float(used["fp32"] - used["fp16"]), algorithmic=float(16 * E * P))
    assert used["fp32"] - used["fp16"] >= 16 * E * P - 6 * (2 << 20)


def test_pack_budget_chunks_give_the_same_records():
    """A byte budget of three fp32 rows packs the 57 rows in 19 calls: same records and exponents as one call."""
    Engine, _ = _engines()
    edges, N, args, init = _degree_problem(36, 44)
    a = Engine(*args, obs_dtype="fp16")
    b = Engine(*args, obs_dtype="fp16", pack_budget_bytes=3 * 16 * 36 * 44)
    for k in ("obs_i", "obs_j", "exp_i", "exp_j"):
        assert torch.equal(getattr(a, k).view(torch.int16) if k.startswith("obs") else getattr(a, k),
                           getattr(b, k).view(torch.int16) if k.startswith("obs") else getattr(b, k)), k


# ------------------------------------------------------------------------------------------------- 5. refusals
def test_refusals_leave_a_valid_engine_usable():
    from align3r_amd import _lib
    Engine, Sharded = _engines()
    edges, N, args, init = _degree_problem(36, 44)
    good = Engine(*args, obs_dtype="fp16")
    good.set_params(**init)
    lib = good.lib

    def create(mutate, shard=None):
        d = good._fill_desc(good.params, good.adam, good.workspace, good.loss_history, slice(None))
        mutate(d)
        h = C.c_void_p()
        if shard:
            return lib.a3r_align_shard_create(C.byref(d), shard[0], shard[1], C.byref(h), _lib.stream_ptr())
        return lib.a3r_align_create(C.byref(d), C.byref(h), _lib.stream_ptr())

    # P % 4 != 0 with packed observations (37 x 41)
    e2, N2, args2, _ = _degree_problem(37, 41)
    with pytest.raises(RuntimeError, match=r"P % 4 == 0"):
        Engine(*args2, obs_dtype="fp16")
    with pytest.raises(RuntimeError, match=r"P % 4 == 0"):
        Sharded(*args2, obs_dtype="fp16", local_shards=2)
    # fp32 and packed pointers together
    fp32 = torch.zeros(16, device="cuda")
    with pytest.raises(RuntimeError, match="w_j must be null"):
        _lib.check(create(lambda d: setattr(d, "w_j", fp32.data_ptr())))
    with pytest.raises(RuntimeError, match="pred_i must be null"):
        _lib.check(create(lambda d: setattr(d, "pred_i", fp32.data_ptr())))

    def packed_next_to_fp32(d):
        d.obs_format = 0
        d.pred_i = d.pred_j = d.w_i = d.w_j = fp32.data_ptr()
    with pytest.raises(RuntimeError, match="must be null with fp32 observations"):
        _lib.check(create(packed_next_to_fp32))
    # a missing exponent table, on a fused and on a shard handle
    with pytest.raises(RuntimeError, match="obs_exp_j is missing"):
        _lib.check(create(lambda d: setattr(d, "obs_exp_j", None)))
    with pytest.raises(RuntimeError, match="obs_exp_i is missing"):
        _lib.check(create(lambda d: setattr(d, "obs_exp_i", None), shard=(0, 20)))
    with pytest.raises(RuntimeError, match="obs_format must be"):
        _lib.check(create(lambda d: setattr(d, "obs_format", 2)))
    losses = good.run(2, 0.05)
    assert good.steps_done == 2 and np.isfinite(losses).all()


# ------------------------------------------------------------------------------------------------- 6. through the mirror API
def _depth_reach(d16, d32, lrs):
    """What 'within the format's reach' means here, fixed before anything was measured (the largest difference is recorded
    beside it, without a bound: an Adam step is at most its learning rate, so 2 sum(lr_t) holds whatever the inputs and says
    nothing).  Typical pixel: the normalised step is homogeneous of degree 0 in the gradient history, so a relative gradient perturbation
    delta changes it by about 2 delta; the decoded observations differ from the fp32 ones by 2^-11 relative, which turns the unit
    residual directions of the l1 loss by 2^-11 |pred| / |residual|, and |pred| / |residual| is allowed up to 4 at the median:
    median |log d16 - log d32| <= 2 * 4 * 2^-11 * sum(lr_t)."""
    dl = np.abs(np.log(d16.astype(np.float64)) - np.log(d32.astype(np.float64)))
    return dict(max_dlog=float(dl.max()), median_dlog=float(np.median(dl)), typical=8 * 2.0 ** -11 * float(np.sum(lrs)))


def _assert_reach(name, r):
    record_margin("align_obs16_mirror_" + name, **r)
    assert np.isfinite(r["max_dlog"]) and r["median_dlog"] <= r["typical"], r


def test_mirror_cloud_opt_global_aligner():
    """cloud_opt.global_aligner(..., obs_dtype='fp16') on the uniform-shape case of tests/golden/alignx.npz, 10 iterations."""
    import json
    import align3r_amd
    from align3r_amd.aligner import schedule_lr
    align3r_amd.install_as_dust3r()
    from dust3r.cloud_opt import global_aligner, GlobalAlignerMode
    g = np.load(os.path.join(GOLDEN, "alignx.npz"))
    case = [c for c in json.load(open(os.path.join(GOLDEN, "alignx.json")))["cases"] if len({tuple(s) for s in c["shapes"]}) == 1][0]
    tag, edges = case["tag"], [tuple(e) for e in case["edges"]]
    E = len(edges)
    tt = lambda key: torch.stack([torch.from_numpy(g[f"{tag}_{key}_{e}"]) for e in range(E)])
    out = dict(view1=dict(idx=[i for i, j in edges]), view2=dict(idx=[j for i, j in edges]),
               pred1=dict(pts3d=tt("p1"), conf=tt("c1")), pred2=dict(pts3d_in_other_view=tt("p2"), conf=tt("c2")))
    depths = {}
    for dt in ("fp32", "fp16"):
        torch.manual_seed(17)
        scene = global_aligner(out, False, [], "cuda", mode=GlobalAlignerMode.PointCloudOptimizer, verbose=False, min_conf_thr=3,
                               allow_pw_adaptors=case["allow_pw_adaptors"], obs_dtype=dt)
        assert scene.engine.obs_dtype == dt
        loss = scene.compute_global_alignment(init=None, niter=10, schedule="cosine", lr=0.05)
        assert np.isfinite(loss) and np.isfinite(scene.engine.loss_history[:10].cpu().numpy()).all()
        depths[dt] = torch.stack(scene.get_depthmaps()).cpu().numpy()
    with pytest.raises(ValueError, match="obs_dtype"):
        global_aligner(out, False, [], "cuda", verbose=False, obs_dtype="bf16")
    lrs = [schedule_lr("cosine", t / 10, 0.05, 1e-6) for t in range(10)]
    _assert_reach("cloud_opt_" + tag, _depth_reach(depths["fp16"], depths["fp32"], lrs))


def test_mirror_scene_keeps_no_fp32_stack_on_the_device():
    """Device memory through cloud_opt.global_aligner, which is how the mode is used: with obs_dtype='fp16' the scene holds the
    packed records and no fp32 predictions on the device -- after construction, and again after init='mst' (which stages them
    while it runs) and two iterations.  A consistent scene of 5 images at 256 x 320 (E = 20, P = 81920): 32 E P = 52 MB in fp32,
    16 E P = 26 MB packed.  Everything else the two scenes hold is the same, so their allocated bytes must differ by at least
    16 E P minus the allocator's slack, one 2 MiB granule for each of the 6 observation buffers involved (13.6 MB here); and the
    packed scene's predictions must be host tensors."""
    import align3r_amd
    align3r_amd.install_as_dust3r()
    from dust3r.cloud_opt import global_aligner
    from test_gpu_api import _geom_scene
    N, H, W = 5, 256, 320
    edges, p1, p2, c, _, _, _ = _geom_scene(N, H, W)
    E, P = len(edges), H * W
    out = dict(view1=dict(idx=[i for i, j in edges]), view2=dict(idx=[j for i, j in edges]),
               pred1=dict(pts3d=torch.from_numpy(p1), conf=torch.from_numpy(c)),
               pred2=dict(pts3d_in_other_view=torch.from_numpy(p2), conf=torch.from_numpy(c)))
    used, losses = {}, {}
    for dt in ("fp32", "fp16"):
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        before = torch.cuda.memory_allocated()
        torch.manual_seed(0)
        scene = global_aligner(out, False, [], "cuda", verbose=False, min_conf_thr=1.5, obs_dtype=dt)
        torch.cuda.synchronize()
        built = torch.cuda.memory_allocated() - before
        losses[dt] = scene.compute_global_alignment(init="mst", niter=2, schedule="cosine", lr=0.01)
        torch.cuda.synchronize()
        used[dt] = (built, torch.cuda.memory_allocated() - before)
        assert scene.engine.observation_bytes == (32 * E * P if dt == "fp32" else 16 * E * P + 8 * E)
        assert scene._pred_i.device.type == ("cuda" if dt == "fp32" else "cpu")
        del scene
    slack = 6 * (2 << 20)
    record_margin("align_obs16_mirror_memory", built_fp32=float(used["fp32"][0]), built_fp16=float(used["fp16"][0]),
                  after_init_fp32=float(used["fp32"][1]), after_init_fp16=float(used["fp16"][1]), algorithmic=float(16 * E * P),
                  loss_fp32=float(losses["fp32"]), loss_fp16=float(losses["fp16"]))
    assert np.isfinite(losses["fp16"]) and np.isfinite(losses["fp32"])
    for stage in (0, 1):
        assert used["fp32"][stage] - used["fp16"][stage] >= 16 * E * P - slack, (stage, used)


def test_mirror_cloud_opt_flow_global_aligner():
    """cloud_opt_flow.global_aligner(..., obs_dtype='fp16') on the first case of tests/golden/alignflow.npz, 10 iterations."""
    import json
    import align3r_amd
    from align3r_amd.aligner import schedule_lr
    align3r_amd.install_as_dust3r()
    from dust3r.cloud_opt_flow import global_aligner, GlobalAlignerMode
    g = np.load(os.path.join(GOLDEN, "alignflow.npz"))
    case = json.load(open(os.path.join(GOLDEN, "alignflow.json")))["cases"][0]
    tag, N, edges = case["tag"], case["N"], case["edges"]
    dyn = torch.from_numpy(g[tag + "_dyn"])
    out = dict(view1=dict(idx=[i for i, j in edges], dynamic_mask=[dyn[i] for i, j in edges]),
               view2=dict(idx=[j for i, j in edges], dynamic_mask=[dyn[j] for i, j in edges]),
               pred1=dict(pts3d=torch.from_numpy(g[tag + "_p1"]), conf=torch.from_numpy(g[tag + "_c1"])),
               pred2=dict(pts3d_in_other_view=torch.from_numpy(g[tag + "_p2"]), conf=torch.from_numpy(g[tag + "_c2"])))
    depths = {}
    for dt in ("fp32", "fp16"):
        scene = global_aligner(out, "cuda", mode=GlobalAlignerMode.PointCloudOptimizer, verbose=False, min_conf_thr=3,
                               shared_focal=case["shared_focal"], temporal_smoothing_weight=case["temporal_smoothing_weight"],
                               translation_weight=case["translation_weight"], flow_loss_weight=case["flow_loss_weight"],
                               flow_loss_start_epoch=0.0, flow_loss_thre=case["flow_loss_thre"], num_total_iter=10,
                               pxl_thre=case["pxl_thre"], flow=(g[tag + "_flow_ij"], g[tag + "_flow_ji"]), obs_dtype=dt)
        assert scene.engine.obs_dtype == dt and scene.engine.flow is not None
        scene.engine.set_params(pw_poses=g[tag + "_init_pw_poses"], depth=g[tag + "_init_im_depthmaps"],
                                im_poses=g[tag + "_init_im_poses"], im_focals=g[tag + "_init_im_focals"])
        loss = scene.compute_global_alignment(init=None, niter=10, schedule=case["schedule"], lr=case["lr"], lr_min=case["lr_min"])
        assert np.isfinite(loss) and np.isfinite(scene.engine.loss_history[:10].cpu().numpy()).all()
        depths[dt] = torch.stack(scene.get_depthmaps()).cpu().numpy()
    lrs = [schedule_lr(case["schedule"], t / 10, case["lr"], case["lr_min"]) for t in range(10)]
    _assert_reach("cloud_opt_flow_" + tag, _depth_reach(depths["fp16"], depths["fp32"], lrs))
