"""GPU: ModularPointCloudOptimizer (partial preset_pose / preset_focal / preset_principal_point / preset_intrinsics) through
global_aligner(mode=ModularPointCloudOptimizer), and the per-image train masks of the engine underneath.

Checkers: goldens captured from the reference's own ModularPointCloudOptimizer + autograd + Adam (tests/golden/alignmod.npz,
make_goldens_modular.py); a float64 torch restatement of the stacked loss for the frozen depth map (no reference counterpart);
the unchanged C oracle at full size (masks change which parameters move, not the gradient, and the first Adam step of a free
parameter depends on nothing but its own gradient).
Bounds are those of the other aligner goldens (test_gpu_alignx.py): derived matrices / world points / loss0 1e-6, gradients
1e-5, 1 / 5 / 50-step trajectories 1e-4, loss curve 1e-5, all relative to the tensor maximum (conftest.rel_err); the full-size
test uses test_config2_full_size_vs_oracle's (1e-6 loss, 1e-5 gradients, 1e-4 state)."""
import json
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN, record_margin, rel_err

pytestmark = pytest.mark.gpu
META = json.load(open(os.path.join(GOLDEN, "alignmod.json")))
CASES = {c["tag"]: c for c in META["cases"]}
KEYS = ("pw_poses", "pw_adaptors", "depth", "im_poses", "im_focals", "im_pp")


@pytest.fixture(scope="module")
def g():
    return np.load(os.path.join(GOLDEN, "alignmod.npz"))


def host(t):
    return t.detach().cpu().numpy()


def _mask(m):
    if isinstance(m, str):
        kind, vals = m.split(":")
        vals = [int(v) for v in vals.split(",")]
        return np.asarray(vals, dtype=np.int64) if kind == "int64" else np.asarray(vals, dtype=bool)
    return m


def _output(case, g):
    edges, name = [tuple(e) for e in case["edges"]], case["inputs"]
    tt = lambda key: [torch.from_numpy(g[f"{name}_{key}_{e}"]) for e in range(len(edges))]
    return dict(view1=dict(idx=[i for i, j in edges]), view2=dict(idx=[j for i, j in edges]),
                pred1=dict(pts3d=tt("p1"), conf=tt("c1")), pred2=dict(pts3d_in_other_view=tt("p2"), conf=tt("c2")))


def _scene(case, g, package="cloud_opt", presets=True, **kw):
    import align3r_amd
    align3r_amd.install_as_dust3r()
    torch.manual_seed(META["seed"])
    common = dict(verbose=False, min_conf_thr=3, dist=case["dist"], **case["kw"], **kw)
    if package == "cloud_opt":
        from dust3r.cloud_opt import global_aligner, GlobalAlignerMode
        scene = global_aligner(_output(case, g), False, [], "cuda", mode=GlobalAlignerMode.ModularPointCloudOptimizer, **common)
    else:
        from dust3r.cloud_opt_flow import global_aligner, GlobalAlignerMode
        scene = global_aligner(_output(case, g), "cuda", mode=GlobalAlignerMode.ModularPointCloudOptimizer, **common)
    if presets:
        _apply_presets(scene, case, g)
    return scene


def _apply_presets(scene, case, g):
    tag = case["tag"]
    poses, focals, pps = g[f"{tag}_known_poses"], g[f"{tag}_known_focals"], g[f"{tag}_known_pp"]
    for p in case["presets"]:
        idx, msk = p["indices"], _mask(p["mask"])
        if p["kind"] == "pose":
            scene.preset_pose([torch.from_numpy(poses[i]) for i in idx], msk)
        elif p["kind"] == "focal":
            scene.preset_focal([float(focals[i]) for i in idx], msk)
        elif p["kind"] == "pp":
            scene.preset_principal_point([pps[i] for i in idx], msk)
        else:
            Ks = []
            for i in idx:
                K = torch.eye(3)
                K[0, 0] = K[1, 1] = float(focals[i])
                K[0, 2], K[1, 2] = float(pps[i][0]), float(pps[i][1])
                Ks.append(K)
            scene.preset_intrinsics(Ks, msk)


def _start(scene, case, g):
    """The generator's start state, exactly (the presets went through the API already; this removes the last-ulp difference of
    the two closed-form rotmat -> quaternion stand-ins and installs the perturbed adaptors)."""
    tag = case["tag"]
    state = {k: torch.from_numpy(g[f"{tag}_start_{k}"]) for k in KEYS if k != "depth"}
    scene.engine.set_params(depth=torch.from_numpy(g[f"{tag}_init_depth"]), **state)


def _frozen_rows(case):
    fz = case["frozen"]
    return dict(im_poses=np.asarray(fz["pose"]), im_focals=np.asarray(fz["focal"]), im_pp=np.asarray(fz["pp"]))


def _check_case(case, g, package, margin_name):
    tag = case["tag"]
    scene = _scene(case, g, package, presets=False)
    eng = scene.engine
    from align3r_amd.dust3r.cloud_opt.modular_optimizer import ModularPointCloudOptimizer
    assert type(scene) is ModularPointCloudOptimizer
    # same torch seed -> the reference's random initial state bit for bit (parameters drawn in its order)
    for k in KEYS:
        assert np.array_equal(host(eng.params[k]).reshape(g[f"{tag}_init_{k}"].shape), g[f"{tag}_init_{k}"]), k
    _apply_presets(scene, case, g)
    eng = scene.engine
    assert scene.norm_pw_scale == case["norm_pw_scale"] and eng.flags["norm_pw_scale"] == case["norm_pw_scale"]
    fz = _frozen_rows(case)
    assert np.array_equal(scene.get_known_focal_mask().numpy(), fz["im_focals"])
    assert np.array_equal(scene._frozen["pose"], fz["im_poses"])
    assert np.array_equal(scene._frozen["pp"] | (not eng.flags["train_pp"]), fz["im_pp"])
    m = {}
    for k in ("im_poses", "im_focals", "im_pp"):        # what the presets wrote, before the exact start state goes in
        m[f"preset_{k}"] = rel_err(host(eng.params[k]).reshape(g[f"{tag}_start_{k}"].shape), g[f"{tag}_start_{k}"])
    _start(scene, case, g)
    start = {k: host(eng.params[k]).copy() for k in KEYS}
    m["pw_poses_4x4"] = rel_err(host(scene.get_pw_poses()), g[f"{tag}_pw_poses_4x4"])
    m["adaptors"] = rel_err(host(scene.get_adaptors()), g[f"{tag}_adaptors"])
    m["im_poses_4x4"] = rel_err(host(scene.get_im_poses()), g[f"{tag}_im_poses_4x4"])
    m["focals"] = rel_err(host(scene.get_focals()).reshape(-1), g[f"{tag}_focals"].reshape(-1))
    m["pp"] = rel_err(host(scene.get_principal_points()), g[f"{tag}_pp"])
    pts = host(scene.get_pts3d(raw=True)).copy()
    for n, (h, w) in enumerate(case["shapes"]):
        pts[n, h * w:] = 0                               # the golden is zero-filled behind each image's own area
    m["pts3d0"] = rel_err(pts, g[f"{tag}_pts3d0"])
    m["loss0"] = abs(float(scene()) - g[f"{tag}_loss0"]) / g[f"{tag}_loss0"]
    loss, gr = eng.loss_grad()
    m["loss0_grad_call"] = abs(loss - g[f"{tag}_loss0"]) / g[f"{tag}_loss0"]
    want = {"pw_poses", "depth", "im_poses", "im_focals"} | ({"im_pp"} if case["kw"].get("optimize_pp") else set()) \
        | ({"pw_adaptors"} if case["kw"].get("allow_pw_adaptors") else set())
    assert set(gr) == want, (sorted(gr), sorted(want))
    for k, v in gr.items():
        ref = g[f"{tag}_grad_{k}"]
        got = host(v).reshape(ref.shape)
        m[f"grad_{k}"] = rel_err(got, ref)
        if k in fz:                                       # rows of frozen images: exact zeros
            assert np.all(got[fz[k]] == 0), k
            assert fz[k].all() or np.abs(got[~fz[k]]).max() > 0, k
    losses, done = [], 0
    for n in (1, 5, 50):
        losses += list(eng.run(n - done, case["lr"], case["schedule"], case["lr_min"], first_iter=done, total_iters=case["niter"]))
        done = n
        for k in KEYS:
            ref = g[f"{tag}_k{n}_{k}"]
            m[f"k{n}_{k}"] = rel_err(host(eng.params[k]).reshape(ref.shape), ref)
    m["losses"] = rel_err(np.asarray(losses), g[f"{tag}_losses"])
    record_margin(margin_name, **m)
    # frozen parameters: bitwise unchanged after 50 steps; the free ones moved
    for k, rows in fz.items():
        now = host(eng.params[k])
        assert np.array_equal(now[rows], start[k][rows]), k
        if (~rows).any() and (k != "im_pp" or eng.flags["train_pp"]):
            assert not np.array_equal(now[~rows], start[k][~rows]), k
    if not case["kw"].get("allow_pw_adaptors"):
        assert np.array_equal(host(eng.params["pw_adaptors"]), start["pw_adaptors"])
    assert all(v < 1e-6 for k, v in m.items() if k.startswith("preset_")), m
    assert all(m[k] < 1e-6 for k in ("pw_poses_4x4", "adaptors", "im_poses_4x4", "focals", "pp", "pts3d0", "loss0", "loss0_grad_call")), m
    assert all(v < 1e-5 for k, v in m.items() if k.startswith("grad_")), m
    assert all(v < 1e-4 for k, v in m.items() if k[0] == "k" and k[1].isdigit()), m
    assert m["losses"] < 1e-5, m
    for d, p, (h, w) in zip(scene.get_depthmaps(), scene.get_pts3d(), case["shapes"]):
        assert tuple(d.shape) == (h, w) and tuple(p.shape) == (h, w, 3)


# ------------------------------------------------------------------------------------------------ 1. reference goldens
@pytest.mark.parametrize("tag", list(CASES))
def test_modular_vs_reference(tag, g):
    _check_case(CASES[tag], g, "cloud_opt", f"alignmod_{tag}")


# ------------------------------------------------------------------------------------------------ 2. identities
def _run20(scene):
    losses = scene.engine.run(20, 0.05, "cosine")
    return losses, {k: host(v).copy() for k, v in scene.engine.params.items()}


def _stacked(case, g):
    from dust3r.cloud_opt import global_aligner, GlobalAlignerMode
    torch.manual_seed(META["seed"])
    return global_aligner(_output(case, g), False, [], "cuda", mode=GlobalAlignerMode.PointCloudOptimizer, verbose=False, min_conf_thr=3)


def test_no_mask_is_the_stacked_optimizer_bitwise(g):
    case = CASES["none"]
    a, b = _scene(case, g), _stacked(case, g)
    for k in a.engine.params:
        assert torch.equal(a.engine.params[k], b.engine.params[k]), k
    (la, pa), (lb, pb) = _run20(a), _run20(b)
    assert np.array_equal(la, lb)
    for k in pa:
        assert np.array_equal(pa[k], pb[k]), k


def test_all_poses_frozen_is_preset_pose_bitwise(g):
    case = CASES["none"]
    poses = [torch.from_numpy(p) for p in g["none_known_poses"]]
    a, b = _scene(case, g), _stacked(case, g)
    a.preset_pose(poses, None)
    b.preset_pose(poses)
    assert a.engine.flags["train_poses"] and not b.engine.flags["train_poses"]      # per-image masks against the handle-wide switch
    assert not a.norm_pw_scale and not b.norm_pw_scale
    before = host(a.engine.params["im_poses"]).copy()
    (la, pa), (lb, pb) = _run20(a), _run20(b)
    assert np.array_equal(la, lb)
    for k in pa:
        assert np.array_equal(pa[k], pb[k]), k
    assert np.array_equal(pa["im_poses"], before)


# ------------------------------------------------------------------------------------------------ 3. both tails
def test_fused_tail_honours_the_masks_bitwise(g, monkeypatch):
    case, res = CASES["pose2"], {}
    for mode in ("launch", "fused"):
        monkeypatch.setenv("A3R_ALIGN_TAIL", mode)       # read when the handle is created
        scene = _scene(case, g)
        _start(scene, case, g)
        losses = scene.engine.run(50, case["lr"], case["schedule"], case["lr_min"])
        res[mode] = (losses, {k: host(v).copy() for k, v in scene.engine.params.items()}, scene.engine.loss_grad())
    assert np.array_equal(res["launch"][0], res["fused"][0])
    for k in res["launch"][1]:
        assert np.array_equal(res["launch"][1][k], res["fused"][1][k]), k
    rows = np.asarray(case["frozen"]["pose"])
    assert np.array_equal(res["fused"][1]["im_poses"][rows], g["pose2_start_im_poses"][rows])
    assert res["launch"][2][0] == res["fused"][2][0]
    for k, v in res["launch"][2][1].items():
        assert torch.equal(v, res["fused"][2][1][k]), k
    assert torch.all(res["fused"][2][1]["im_poses"][torch.from_numpy(rows)] == 0)


# ------------------------------------------------------------------------------------------------ 4. frozen depth maps
def _random_problem(edges, N, H, W, seed):
    rng = np.random.default_rng(seed)
    E, P = len(edges), H * W
    p1 = rng.standard_normal((E, P, 3)).astype(np.float32)
    p2 = rng.standard_normal((E, P, 3)).astype(np.float32)
    w1 = np.log(1 + 9 * rng.random((E, P))).astype(np.float32)
    w2 = np.log(1 + 9 * rng.random((E, P))).astype(np.float32)
    init = dict(pw_poses=rng.standard_normal((E, 8)).astype(np.float32), depth=(0.1 * rng.standard_normal((N, P)) - 3).astype(np.float32),
                im_poses=rng.standard_normal((N, 7)).astype(np.float32), im_focals=np.full(N, 20 * np.log(max(H, W)), np.float32))
    return p1, p2, w1, w2, init


def _loss_f64(edges, p1, p2, w1, w2, H, W, params, base_scale=0.5, pw_break=20.0, focal_break=20.0):
    """float64 restatement of the stacked l1 loss (uniform shapes, norm_pw_scale on, adaptors at zero): every edge side's
    weighted distances between the image's world points and the pairwise prediction moved by the edge's similarity, summed
    and divided by the total area of that side."""
    sexpm1 = lambda x: torch.sign(x) * torch.expm1(torch.abs(x))

    def rot(q):
        x, y, z, w = (q / q.norm(dim=-1, keepdim=True)).unbind(-1)
        return torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w),
                            2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w),
                            2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)], -1).reshape(-1, 3, 3)
    pw, depth, im, foc = params["pw_poses"], params["depth"], params["im_poses"], params["im_focals"]
    N, P = depth.shape
    ys, xs = torch.meshgrid(torch.arange(H, dtype=torch.float64), torch.arange(W, dtype=torch.float64), indexing="ij")
    grid = torch.stack((xs, ys), -1).reshape(P, 2)
    d = depth.exp()
    f = (foc / focal_break).exp()
    rel = torch.cat((d[..., None] * (grid[None] - torch.tensor([W / 2, H / 2], dtype=torch.float64)) / f[:, None, None], d[..., None]), -1)
    pts = torch.einsum("nij,npj->npi", rot(im[:, :4]), rel) + sexpm1(im[:, 4:7])[:, None]
    s = pw[:, 7].exp() * (np.log(base_scale) - pw[:, 7].mean()).exp()
    Rp, Tp = rot(pw[:, :4]) * s[:, None, None], sexpm1(pw[:, 4:7]) * s[:, None]
    ei, ej = [i for i, j in edges], [j for i, j in edges]
    ai = torch.einsum("eij,epj->epi", Rp, torch.from_numpy(p1).double()) + Tp[:, None]
    aj = torch.einsum("eij,epj->epi", Rp, torch.from_numpy(p2).double()) + Tp[:, None]
    li = ((pts[ei] - ai).norm(dim=-1) * torch.from_numpy(w1).double()).sum() / (len(edges) * P)
    lj = ((pts[ej] - aj).norm(dim=-1) * torch.from_numpy(w2).double()).sum() / (len(edges) * P)
    return li + lj


@pytest.mark.parametrize("H,W", [(40, 52), (37, 41)], ids=["vec", "ragged"])
def test_frozen_depth_maps(H, W):
    from align3r_amd.aligner import AlignEngine
    N = 4
    edges = [(i, j) for i in range(N) for j in range(N) if i != j]
    p1, p2, w1, w2, init = _random_problem(edges, N, H, W, 31)
    a = AlignEngine([i for i, j in edges], [j for i, j in edges], p1, p2, w1, w2, [(H, W)] * N)
    a.set_params(**init)
    a.run(3, 0.05)                                        # non-zero Adam moments everywhere before anything is frozen
    frozen = np.asarray([False, True, False, True])
    a.set_train_masks(depth=~frozen)
    assert a.steps_done == 3                              # setting masks neither re-creates the handle nor resets Adam
    depth0, adam0 = host(a.params["depth"]).copy(), host(a.adam["depth"]).copy()
    assert np.abs(adam0[:, frozen]).min() > 0
    # gradients: frozen rows exact zeros, free rows against float64 autograd
    params = {k: a.params[k].detach().cpu().double().requires_grad_(True) for k in ("pw_poses", "depth", "im_poses", "im_focals")}
    ref = _loss_f64(edges, p1, p2, w1, w2, H, W, params)
    ref.backward()
    loss, gr = a.loss_grad()
    m = dict(loss=abs(loss - ref.item()) / ref.item())
    for k in params:
        got, want = host(gr[k]).reshape(params[k].shape), params[k].grad.numpy()
        if k == "depth":
            assert np.all(got[frozen] == 0)
            got, want = got[~frozen], want[~frozen]
        m[f"grad_{k}"] = rel_err(got, want)
    record_margin(f"alignmod_frozen_depth_{H}x{W}", **m)
    assert m["loss"] < 1e-5 and all(v < 1e-5 for v in m.values()), m
    a.run(10, 0.05)
    depth1, adam1 = host(a.params["depth"]), host(a.adam["depth"])
    assert np.array_equal(depth1[frozen], depth0[frozen])
    assert np.array_equal(adam1[:, frozen], adam0[:, frozen])
    assert np.all(depth1[~frozen] != depth0[~frozen]) and not np.array_equal(adam1[:, ~frozen], adam0[:, ~frozen])
    a.set_train_masks()                                   # masks off again: every map moves
    a.run(1, 0.05)
    assert np.all(host(a.params["depth"])[frozen] != depth0[frozen])


# ------------------------------------------------------------------------------------------------ 5. realistic size
def test_config2_full_size_with_masks_vs_oracle():
    """N = 16, E = 84, 512 x 384 (the problem bench.py times) with four frozen poses, focals and depth maps."""
    from align3r_amd.aligner import AlignEngine
    from align3r_amd.dust3r.image_pairs import make_pairs
    from oracle.align_ref import AlignOracle
    from test_gpu_align import _scene as oracle_scene
    N, H, W = 16, 384, 512
    pairs = make_pairs([dict(idx=i) for i in range(N)], "swin-3-noncyclic", symmetrize=True)
    edges = [(a["idx"], b["idx"]) for a, b in pairs]
    assert len(edges) == 84
    edges, p1, p2, w1, w2, _, init = oracle_scene(edges, N, H, W, 21, False)
    args = ([i for i, j in edges], [j for i, j in edges], p1, p2, w1, w2, [(H, W)] * N)
    o, a = AlignOracle(*args), AlignEngine(*args)
    for eng in (o, a):
        eng.set_params(**init)
    frozen = np.zeros(N, bool)
    frozen[[0, 5, 10, 15]] = True
    a.set_train_masks(pose=~frozen, focal=~frozen, depth=~frozen)
    lo, go = o.loss_grad()
    la, ga = a.loss_grad()
    m = dict(loss0=abs(lo - la) / lo)
    for k in go:
        got, want = host(ga[k]).reshape(go[k].shape), go[k]
        if k != "pw_poses":
            assert np.all(got[frozen] == 0), k
            got, want = got[~frozen], want[~frozen]
        m[f"grad_{k}"] = rel_err(got, want)
    o.run(1, 0.05, "cosine")
    a.run(1, 0.05, "cosine")
    for k in o.trainable():
        got, want = host(a.params[k]).reshape(o.params[k].shape), o.params[k]
        if k != "pw_poses":
            got, want = got[~frozen], want[~frozen]
        m[f"state_{k}"] = rel_err(got, want)
    record_margin("alignmod_config2_full_size_vs_oracle", **m)
    a.run(1, 0.05, "cosine")
    for k in ("im_poses", "im_focals", "depth"):
        now, was = host(a.params[k]).reshape(N, -1), np.asarray(init[k]).reshape(N, -1)
        assert np.array_equal(now[frozen], was[frozen]), k
        assert not np.array_equal(now[~frozen], was[~frozen]), k
    assert np.all(host(a.adam["depth"])[:, frozen] == 0) and np.all(host(a.adam["small"])[:, frozen, :8] == 0)
    assert m["loss0"] < 1e-6, m
    assert all(v < 1e-5 for k, v in m.items() if k.startswith("grad_")), m
    assert all(v < 1e-4 for k, v in m.items() if k.startswith("state_")), m


# ------------------------------------------------------------------------------------------------ 6. init='mst'
def _geom_modular(N=4, H=32, W=48):
    import align3r_amd
    align3r_amd.install_as_dust3r()
    from dust3r.cloud_opt import global_aligner, GlobalAlignerMode
    from test_gpu_api import _geom_scene
    edges, p1, p2, c, cams, depths, f = _geom_scene(N, H, W)
    out = dict(view1=dict(idx=[i for i, j in edges]), view2=dict(idx=[j for i, j in edges]),
               pred1=dict(pts3d=torch.from_numpy(p1), conf=torch.from_numpy(c)),
               pred2=dict(pts3d_in_other_view=torch.from_numpy(p2), conf=torch.from_numpy(c)))
    torch.manual_seed(0)
    scene = global_aligner(out, False, [], "cuda", mode=GlobalAlignerMode.ModularPointCloudOptimizer, verbose=False, min_conf_thr=1.5)
    poses = []
    for R, t in cams:
        T = np.eye(4, dtype=np.float32)
        T[:3, :3], T[:3, 3] = R, t
        poses.append(torch.from_numpy(T))
    return scene, poses, f


def test_mst_init_with_two_frozen_poses():
    scene, poses, f = _geom_modular()
    loss_random = float(scene())
    scene.preset_pose([poses[0], poses[3]], [0, 3])
    scene.preset_focal([f], 1)
    scene.preset_principal_point([(25.0, 15.0)], 2)
    eng = scene.engine
    before = {k: host(eng.params[k]).copy() for k in ("im_poses", "im_focals", "im_pp")}
    scene.compute_global_alignment(init="mst", niter=0)
    after = {k: host(eng.params[k]) for k in before}
    assert np.array_equal(after["im_poses"][[0, 3]], before["im_poses"][[0, 3]])
    assert not np.array_equal(after["im_poses"][[1, 2]], before["im_poses"][[1, 2]])
    assert after["im_focals"][1] == before["im_focals"][1] and np.all(after["im_focals"][[0, 2, 3]] != before["im_focals"][[0, 2, 3]])
    assert np.array_equal(after["im_pp"], before["im_pp"])
    loss_init = float(scene())
    assert np.isfinite(loss_init) and loss_init < loss_random, (loss_init, loss_random)
    final = scene.compute_global_alignment(init=None, niter=20, lr=0.01)
    assert np.isfinite(final)
    assert np.array_equal(host(eng.params["im_poses"])[[0, 3]], before["im_poses"][[0, 3]])


def test_mst_init_with_one_frozen_pose_is_refused():
    scene, poses, f = _geom_modular()
    scene.preset_pose(poses[2], 2)
    assert scene.norm_pw_scale
    with pytest.raises(NotImplementedError, match="single known pose"):
        scene.compute_global_alignment(init="mst", niter=0)


# ------------------------------------------------------------------------------------------------ 7. refusals
def test_refusals(g):
    case = CASES["none"]
    with pytest.raises(NotImplementedError, match="fx_and_fy"):
        _scene(case, g, fx_and_fy=True)
    with pytest.raises(NotImplementedError, match="edge-sharded"):
        _scene(case, g, edge_shards=2)
    from align3r_amd.aligner import AlignEngine
    N, H, W = 3, 16, 16
    edges = [(i, j) for i in range(N) for j in range(N) if i != j]
    p1, p2, w1, w2, init = _random_problem(edges, N, H, W, 5)
    a = AlignEngine([i for i, j in edges], [j for i, j in edges], p1, p2, w1, w2, [(H, W)] * N, shared_focal=True)
    with pytest.raises(ValueError, match="shared_focal"):
        a.set_train_masks(focal=[True, False, True])
    msk = np.ones(N, np.uint8)
    rc = a.lib.a3r_align_set_train_masks(a.handle, None, msk.ctypes.data, None, None, None)      # the C entry point refuses it too
    assert rc != 0 and b"shared_focal" in a.lib.a3r_last_error()
    a.set_train_masks(pose=[True, False, True])           # the other masks work next to shared_focal
    with pytest.raises(ValueError, match="expected 3 entries"):
        a.set_train_masks(pose=[True, False])
    import align3r_amd
    align3r_amd.install_as_dust3r()
    from dust3r.cloud_opt_flow import global_aligner, GlobalAlignerMode
    with pytest.raises(NotImplementedError):
        global_aligner(_output(case, g), "cuda", mode=GlobalAlignerMode.PairViewer)


# ------------------------------------------------------------------------------------------------ 8. cloud_opt_flow
def test_cloud_opt_flow_modular_reproduces_pose2(g):
    _check_case(CASES["pose2"], g, "cloud_opt_flow", "alignmod_flow_pose2")
