"""GPU: the hierarchical pose pipeline (tool/pose_test.py --mode eval_pose_h) -- keyframes, then every clip, through the
flow-regularised aligner -- and the init_priors branch of the device MST initialisation it rests on.

1. init_priors on the device path: the priors cases of mst.npz and the three of hier_flow.npz (make_goldens_hier_flow.py) with
   the inputs on the device.  The generic minimum_spanning_tree must not run; tree and PnP hand-offs exact; every quantity of
   test_gpu_mst_parity.py within that file's rule (fp32 expectations: mst.json's fallback_bound).
2..6. The driver on the scene of test_gpu_hier.py (N = 8, 32x48, clip size 3: clips of 3, 3, 2 frames) with a faked pair forward
   and the scene's exact ego flow injected through flow_fn, a rectangle of displaced flow moving through the frames.
"""
import json
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN, record_margin, rel_err

pytestmark = pytest.mark.gpu
MST = json.load(open(os.path.join(GOLDEN, "mst.json")))
HF = json.load(open(os.path.join(GOLDEN, "hier_flow.json")))
PRIOR_CASES = [("mst", t) for t in ("priors_i", "priors_j")] + [("hier_flow", c["tag"]) for c in HF["cases"]]


# ------------------------------------------------------------------------------------------------ 1. priors on the device path
@pytest.fixture(scope="module")
def fixtures():
    return dict(mst=(MST, np.load(os.path.join(GOLDEN, "mst.npz"))), hier_flow=(HF, np.load(os.path.join(GOLDEN, "hier_flow.npz"))))


def _device_scene(meta, g, case):
    """test_gpu_mst_parity._scene with every input on the device, so that the scene is _fast."""
    import align3r_amd
    align3r_amd.install_as_dust3r()
    sc, name = meta["scenes"][case["scene"]], case["scene"]
    edges = [tuple(e) for e in sc["edges"]]
    fac = [np.float32(f) for f in case["factors"]]
    get = lambda key: [g[f"{name}_{key}_{e}"] for e in range(len(edges))]
    c1, c2 = [c * f for c, f in zip(get("c1"), fac)], [c * f for c, f in zip(get("c2"), fac)]
    assert all(c.dtype == np.float32 for c in c1 + c2)
    pack = lambda lst: torch.from_numpy(np.stack(lst)).to("cuda")
    out = dict(view1=dict(idx=[i for i, j in edges]), view2=dict(idx=[j for i, j in edges]),
               pred1=dict(pts3d=pack(get("p1")), conf=pack(c1)), pred2=dict(pts3d_in_other_view=pack(get("p2")), conf=pack(c2)))
    torch.manual_seed(meta["seed"])
    kw = dict(verbose=True, min_conf_thr=meta["min_conf_thr"])
    if case["cls"] == "flow":
        from dust3r.cloud_opt_flow import global_aligner, GlobalAlignerMode
        dyn = torch.from_numpy(g[f"{name}_dyn"])
        out["view1"]["dynamic_mask"], out["view2"]["dynamic_mask"] = [dyn[i] for i, j in edges], [dyn[j] for i, j in edges]
        return global_aligner(out, "cuda", mode=GlobalAlignerMode.PointCloudOptimizer, translation_weight=1.0, flow_loss_weight=0.0,
                              flow_loss_start_epoch=0.1, flow_loss_thre=20.0, num_total_iter=30, pxl_thre=50, **case["kw"], **kw)
    from dust3r.cloud_opt import global_aligner, GlobalAlignerMode
    return global_aligner(out, False, [], "cuda", mode=GlobalAlignerMode.PointCloudOptimizer, **kw)


@pytest.mark.parametrize("which,tag", PRIOR_CASES)
def test_init_priors_take_the_device_path(fixtures, which, tag, monkeypatch, capsys):
    from align3r_amd.dust3r.cloud_opt import init_im_poses as mod
    from test_gpu_mst_parity import Checker, _tree, _which_image, host
    meta, g = fixtures[which]
    case = {c["tag"]: c for c in meta["cases"]}[tag]
    assert case["priors"] and not case["float64_expectations"]           # fp32 expectations: Checker takes mst.json's fallback_bound
    sc = meta["scenes"][case["scene"]]
    shapes, edges = [tuple(s) for s in sc["shapes"]], [tuple(e) for e in sc["edges"]]
    N = len(shapes)
    scene = _device_scene(meta, g, case)
    assert scene._fast
    seen = dict(pnp=[], generic=0)

    def recorder(items, iterations=10):
        seen["pnp"] += [(host(pts), focal, int(msk.sum())) for pts, focal, msk, pp in items]
        return [None] * len(items)

    def no_generic(*a, **k):
        seen["generic"] += 1
        raise AssertionError("init_priors went to the generic minimum_spanning_tree")
    monkeypatch.setattr(mod, "linear_pnp_many", recorder)
    monkeypatch.setattr(mod, "minimum_spanning_tree", no_generic)
    name = case["scene"]
    priors = [g[f"{name}_key_pose"].tolist(), g[f"{name}_key_depth"], [float(sc["key_focal"])]]
    capsys.readouterr()
    scene.compute_global_alignment(init="mst", init_priors=priors, niter=0)
    tree = _tree(capsys.readouterr().out)
    assert seen["generic"] == 0
    want = lambda key: g[f"{tag}_{key}"]
    spread = case["spread"]
    check = Checker(case)
    # ---- exact: the walk over the tree (root found by the pop-and-reinsert loop), who goes to PnP, the mask counts
    assert tree == case["tree"], (tree, case["tree"])
    calls = [(_which_image(pts, want("mst_pts3d"), shapes), pts, focal, n_msk) for pts, focal, n_msk in seen["pnp"]]
    assert [c[0] for c in calls] == [c["index"] for c in case["pnp"]]
    assert [c[3] for c in calls] == [c["msk_sum"] for c in case["pnp"]]
    for (idx, pts, focal, _), rec in zip(calls, case["pnp"]):
        h, w = shapes[idx]
        check(f"pnp{idx}_pts3d", pts.reshape(-1, 3), want("mst_pts3d")[idx, :h * w], rec["spread_pts"])
        check(f"pnp{idx}_focal", focal, rec["focal"], rec["spread_focal"])
    if scene._edge_conf_mean is not None:
        m = host(scene._edge_conf_mean).astype(np.float32)
        check("scores", m[0::2] * m[1::2], want("scores"), spread["scores"])
    # ---- the written state, through the getters
    check("pw_poses_4x4", host(scene.get_pw_poses()), want("pw_poses_4x4"), spread["pw_poses_4x4"])
    check("im_poses_4x4", host(scene.get_im_poses()), want("im_poses_4x4"), spread["im_poses_4x4"])
    check("focals", host(scene.get_focals()).reshape(N), want("focals"), spread["focals"])
    check("depth", host(scene.get_depthmaps(raw=True)), want("depth"), spread["depth"])
    check("s_factor", float(scene.get_pw_norm_scale_factor()), want("s_factor"), spread["s_factor"])
    check("loss", float(scene()), want("loss"), spread["loss"])
    if case["cls"] == "flow":                                            # _mst_state_written captured the depth maps for the prior
        assert rel_err(host(torch.stack(list(scene.get_init_depthmaps(raw=True)))), host(scene.get_depthmaps(raw=True))) < 1e-6
        assert (scene.engine.prior is not None) == (case["kw"]["depth_regularize_weight"] > 0)
    record_margin(f"mst_priors_device_{tag}", **check.margins)
    assert not check.misses, check.misses


# ------------------------------------------------------------------------------------------------ 2..6: the driver
N_FRAMES, H, W, CLIP = 8, 32, 48, 3
RECT = dict(y0=10, y1=20, w=8, x0=6, dx=3, shift=(9.0, 4.0))            # rows, width, first column, columns per frame, flow offset
DRIVE = dict(clip_size=CLIP, schedule="linear", lr=0.01, min_conf_thr=1.5)
_CACHE = {}


def _rect(n):
    x0 = RECT["x0"] + RECT["dx"] * n
    return slice(RECT["y0"], RECT["y1"]), slice(x0, x0 + RECT["w"])


def _world(H=H, W=W):
    from test_gpu_hier import _scene
    return _scene(N_FRAMES, H, W)


def _fake_inference(cams, world, H, W, frames=None, accepts_device=False):
    """The pair forward of tests/test_gpu_hier.py: consistent point maps at scale 0.7 + noise, random confidences (one generator,
    consumed in call order).  accepts_device: the keep_on_device keyword exists and puts the outputs on the device."""
    rng = np.random.default_rng(0)

    def run(pairs, model, device, batch_size=1, verbose=False, keep_on_device=False):
        gi = [int(a["instance"]) for a, b in pairs]
        gj = [int(b["instance"]) for a, b in pairs]
        p1 = np.stack([0.7 * ((world[i] - cams[i][1]) @ cams[i][0]) for i in gi]).astype(np.float32)
        p2 = np.stack([0.7 * ((world[j] - cams[i][1]) @ cams[i][0]) for i, j in zip(gi, gj)]).astype(np.float32)
        p1 += 0.001 * rng.standard_normal(p1.shape).astype(np.float32)
        p2 += 0.001 * rng.standard_normal(p2.shape).astype(np.float32)
        c = (2 + 8 * rng.random((len(pairs), H, W))).astype(np.float32)
        t = (lambda a: torch.from_numpy(a).to("cuda")) if keep_on_device else torch.from_numpy
        v1 = dict(idx=[a["idx"] for a, b in pairs], instance=[a["instance"] for a, b in pairs])
        v2 = dict(idx=[b["idx"] for a, b in pairs], instance=[b["instance"] for a, b in pairs])
        if frames is not None:
            v1["img"], v2["img"] = torch.stack([frames[i] for i in gi]), torch.stack([frames[j] for j in gj])
        return dict(view1=v1, view2=v2, pred1=dict(pts3d=t(p1), conf=t(c)), pred2=dict(pts3d_in_other_view=t(p2), conf=t(c.copy())))

    if accepts_device:
        return run
    return lambda pairs, model, device, batch_size=1, verbose=False: run(pairs, model, device, batch_size, verbose)


def _flow_fn(cams, world, f):
    """The exact ego flow of the scene for every edge, both directions, with the rectangle of the source frame displaced."""
    xs, ys = np.meshgrid(np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64))

    def ego(src, tgt):
        R, t = cams[tgt]
        Y = (world[src] - t) @ R
        fl = np.stack([f * Y[..., 0] / Y[..., 2] + W / 2 - xs, f * Y[..., 1] / Y[..., 2] + H / 2 - ys], 0)
        ry, rx = _rect(src)
        fl[0, ry, rx] += RECT["shift"][0]
        fl[1, ry, rx] += RECT["shift"][1]
        return fl.astype(np.float32)

    def fn(edges, views):
        gi, gj = [int(s) for s in views[0]["instance"]], [int(s) for s in views[1]["instance"]]
        assert len(edges) == len(gi)
        return (torch.from_numpy(np.stack([ego(i, j) for i, j in zip(gi, gj)])), torch.from_numpy(np.stack([ego(j, i) for i, j in zip(gi, gj)])))
    return fn


def _imgs():
    return [dict(idx=i, instance=str(i), true_shape=np.int32([[H, W]])) for i in range(N_FRAMES)]


def _drive(tmp_path_factory, device_resident, niter, obs_dtype="fp32"):
    """One run of the driver on the scene (cached: tests 2, 3, 4 and 6 share them).  Host-resident runs replace inference() by a
    function WITHOUT the keep_on_device keyword, as tests/test_gpu_hier.py does."""
    key = (device_resident, niter, obs_dtype)
    if key in _CACHE:
        return _CACHE[key]
    import align3r_amd.dust3r.inference as inf_mod
    from align3r_amd.dust3r.cloud_opt import init_im_poses as init_mod
    from align3r_amd.tool import hierarchical as hz
    cams, world, f = _world()
    out_dir = tmp_path_factory.mktemp(f"hf_{int(device_resident)}_{niter}_{obs_dtype}")
    real, real_mst = inf_mod.inference, init_mod.minimum_spanning_tree
    generic = []                                  # one entry per scene that went through the generic minimum_spanning_tree

    def spy_mst(*a, **k):
        generic.append(k.get("init_priors") is not None)
        return real_mst(*a, **k)
    inf_mod.inference = _fake_inference(cams, world, H, W, accepts_device=device_resident)
    init_mod.minimum_spanning_tree = spy_mst
    try:
        torch.manual_seed(0)
        res = hz.hierarchical_alignment(_imgs(), None, "cuda", niter=niter, output_dir=str(out_dir), obs_dtype=obs_dtype,
                                        flow=dict(flow_fn=_flow_fn(cams, world, f)), device_resident=device_resident, **DRIVE)
    finally:
        inf_mod.inference, init_mod.minimum_spanning_tree = real, real_mst
    res["generic_mst_calls"] = generic
    _CACHE[key] = (res, out_dir, cams)
    return _CACHE[key]


def _hand_chain(niter):
    """The same two stages written out with what exists without the driver: cloud_opt_flow.global_aligner and
    compute_global_alignment(init='mst', init_priors=...), same seeds, same order of draws."""
    if ("hand", niter) in _CACHE:
        return _CACHE[("hand", niter)]
    from align3r_amd.dust3r.cloud_opt_flow import GlobalAlignerMode, global_aligner
    from align3r_amd.tool import hierarchical as hz
    cams, world, f = _world()
    inference, flow_fn = _fake_inference(cams, world, H, W), _flow_fn(cams, world, f)
    coarse, kf, clips, _ = hz.my_make_pairs_pose(_imgs(), hz.choose_clip_size(N_FRAMES, CLIP))

    def align(pairs, priors):
        out = inference(pairs, None, "cuda")                              # confidences as predicted: the pose pipeline has no clamp
        edges = list(zip(out["view1"]["idx"], out["view2"]["idx"]))
        scene = global_aligner(out, "cuda", mode=GlobalAlignerMode.PointCloudOptimizer, verbose=False, min_conf_thr=1.5, num_total_iter=niter,
                               obs_dtype="fp32", flow_loss_weight=0.01, temporal_smoothing_weight=0.01, translation_weight=1.0,
                               flow_loss_start_epoch=0.1, flow_loss_thre=40, pxl_thre=50, motion_mask_thre=0.35,
                               depth_regularize_weight=0, shared_focal=True, use_self_mask=True, flow=flow_fn(edges, (out["view1"], out["view2"])))
        scene.compute_global_alignment(init="mst", init_priors=priors, niter=niter, schedule="linear", lr=0.01)
        return scene
    torch.manual_seed(0)
    key = align(coarse, None)
    kp = key.get_im_poses().detach().cpu().numpy().tolist()
    kd = [d.detach().cpu().numpy() for d in key.get_depthmaps()]
    kfoc = key.get_focals().detach().cpu().numpy().tolist()
    got = dict(depths=[], poses_raw=[], focals=[], dynamic_masks=[], key_poses=kp)
    for c, pairs in enumerate(clips):
        s = align(pairs, [kp[c], kd[c], kfoc[c]])
        got["depths"] += [d.detach().cpu().numpy() for d in s.get_depthmaps()]
        got["poses_raw"] += list(s.get_im_poses().detach().cpu().numpy())
        got["focals"] += s.get_focals().detach().cpu().numpy().reshape(-1).tolist()
        got["dynamic_masks"] += [np.asarray(m.cpu()).astype(bool) for m in s.dynamic_masks]
    _CACHE[("hand", niter)] = got
    return got


def _purpose(poses, cams, keyframes_id, clip_size):
    """The purpose measures of tests/test_gpu_hier.py: worst rotation entry against frame 0, worst in-clip baseline cosine, worst
    in-clip ratio of baseline scales."""
    poses = np.asarray(poses, np.float64)

    def truth(a, b):
        Ta, Tb = np.eye(4), np.eye(4)
        Ta[:3, :3], Ta[:3, 3] = cams[a]
        Tb[:3, :3], Tb[:3, 3] = cams[b]
        return np.linalg.inv(Ta) @ Tb
    rot = max(np.abs((np.linalg.inv(poses[0]) @ poses[n])[:3, :3] - truth(0, n)[:3, :3]).max() for n in range(1, len(poses)))
    cos, ratio = 1.0, 1.0
    for k in keyframes_id:
        rs = []
        for n in range(k + 1, min(k + clip_size, len(poses))):
            rel, gt = np.linalg.inv(poses[k]) @ poses[n], truth(k, n)
            cos = min(cos, float(rel[:3, 3] @ gt[:3, 3] / (np.linalg.norm(rel[:3, 3]) * np.linalg.norm(gt[:3, 3]))))
            rs.append(np.linalg.norm(rel[:3, 3]) / np.linalg.norm(gt[:3, 3]))
        if len(rs) > 1:
            ratio = max(ratio, max(rs) / min(rs))
    return dict(rot=float(rot), cos=cos, ratio=float(ratio))


def test_driver_adds_sequencing_only(tmp_path_factory):
    """Host-resident driver == the hand-written chain, bitwise; every clip re-anchored on its keyframe exactly; the files."""
    res, out_dir, cams = _drive(tmp_path_factory, False, 30)
    hand = _hand_chain(30)
    assert res["clip_size"] == 3 and res["keyframes_id"] == [0, 3, 6] and res["all_clips_id"] == [[0, 1, 2], [3, 4, 5], [6, 7]]
    for q in ("depths", "poses_raw", "dynamic_masks"):
        assert len(res[q]) == N_FRAMES == len(hand[q])
        for n in range(N_FRAMES):
            assert np.array_equal(res[q][n], hand[q][n]), (q, n)
    assert res["focals"] == hand["focals"] and len(res["focals"]) == N_FRAMES
    assert all(np.isfinite(d).all() and d.shape == (H, W) for d in res["depths"])
    kp = res["key_scene"].get_im_poses().detach().cpu().numpy()
    assert np.array_equal(kp, np.asarray(hand["key_poses"], np.float32))
    for c, k in enumerate(res["keyframes_id"]):
        assert np.array_equal(res["poses"][k], kp[c])                                     # frame 0 of a clip IS the keyframe pose
        assert res["poses"][k].dtype == np.float32
        rel = kp[c].astype(np.float64) @ np.linalg.inv(res["poses_raw"][k].astype(np.float64))
        for n in range(k + 1, min(k + 3, N_FRAMES)):                                      # the rest moved by one rigid transform
            assert np.allclose(res["poses"][n], rel @ res["poses_raw"][n], atol=1e-5)
    # ---- files, with running offsets
    names = lambda pat: sorted(p.name for p in out_dir.glob(pat))
    assert names("frame_*.npy") == [f"frame_{i:04d}.npy" for i in range(N_FRAMES)]
    for pat in ("conf_{}.npy", "init_conf_{}.npy", "dynamic_mask_{}.png", "enlarged_dynamic_mask_{}.png"):
        assert all((out_dir / pat.format(i)).exists() for i in range(N_FRAMES)), pat
    assert len(names("conf_*.npy")) == N_FRAMES and len(names("init_conf_*.npy")) == N_FRAMES
    assert len(names("dynamic_mask_*.png")) == N_FRAMES and len(names("enlarged_dynamic_mask_*.png")) == N_FRAMES
    for i in (0, 4, 7):
        assert np.array_equal(np.load(out_dir / f"frame_{i:04d}.npy"), res["depths"][i])
        assert np.array_equal(np.load(out_dir / f"conf_{i}.npy"), res["confs"][i])
        assert np.array_equal(np.load(out_dir / f"init_conf_{i}.npy"), res["init_confs"][i])
    lines = (out_dir / "pred_traj.txt").read_text().splitlines()
    assert [ln.split()[0] for ln in lines] == [str(float(i)) for i in range(N_FRAMES)] and all(len(ln.split()) == 8 for ln in lines)
    xyz = np.array([[float(x) for x in ln.split()[1:4]] for ln in lines])
    assert np.allclose(xyz, np.stack(res["poses"])[:, :3, 3], atol=1e-6)                 # the re-anchored poses are the written ones
    assert len((out_dir / "pred_intrinsics.txt").read_text().splitlines()) == N_FRAMES
    assert np.allclose(np.loadtxt(out_dir / "pred_focal.txt"), res["focals"], atol=1e-5)


def test_device_resident_matches_host_resident(tmp_path_factory):
    bound = MST["fallback_bound"]
    host0, _, cams = _drive(tmp_path_factory, False, 0)
    dev0, _, _ = _drive(tmp_path_factory, True, 0)
    # the device-resident run took the device routes: every scene _fast, no scene through the generic minimum_spanning_tree
    assert dev0["key_scene"]._fast and not host0["key_scene"]._fast
    assert dev0["generic_mst_calls"] == [] and host0["generic_mst_calls"] == [False, True, True, True]
    assert all(float(c.std()) > 0.1 for c in host0["confs"])                   # the confidences are the predicted ones, not one constant
    margins, misses = {}, []
    for c, ids in enumerate(host0["all_clips_id"]):
        sl = slice(ids[0], ids[-1] + 1)
        for q in ("depths", "poses_raw", "focals", "intrinsics", "init_confs", "confs"):       # confs: log() on the host | the device
            err = rel_err(np.stack(dev0[q][sl]), np.stack(host0[q][sl]))
            margins[f"clip{c}_{q}"] = err
            if not err < bound:
                misses.append((c, q, err))
    record_margin("hier_flow_device_vs_host_niter0", bound=bound, **margins)
    assert not misses, misses
    # ---- after 30 iterations both modes serve the purpose (bounds of tests/test_gpu_hier.py)
    hand = _purpose(_reanchored(_hand_chain(30)), cams, [0, 3, 6], 3)
    record_margin("hier_flow_hand_chain_purpose", **hand)
    for resident in (False, True):
        res, _, _ = _drive(tmp_path_factory, resident, 30)
        assert res["generic_mst_calls"] == ([] if resident else [False, True, True, True])
        m = _purpose(res["poses"], cams, res["keyframes_id"], res["clip_size"])
        record_margin(f"hier_flow_purpose_{'device' if resident else 'host'}", **m)
        assert m["rot"] < 0.03 and m["cos"] > 0.96 and m["ratio"] < 1.5, (resident, m)


def _reanchored(hand):
    poses = []
    for c, k in enumerate((0, 3, 6)):
        raw = np.stack(hand["poses_raw"][k:k + 3])
        key = np.array(hand["key_poses"][c])
        rel = key @ np.linalg.inv(raw[0])
        poses += [key.astype(np.float32)] + [rel @ p for p in raw[1:]]
    return poses


def test_motion_masks_reach_the_output(tmp_path_factory):
    import PIL.Image
    res, out_dir, _ = _drive(tmp_path_factory, False, 30)
    for n in range(N_FRAMES):
        m = res["dynamic_masks"][n]
        ry, rx = _rect(n)
        assert m.dtype == bool and m.shape == (H, W)
        assert m[ry, rx].all(), (n, float(m[ry, rx].mean()))                              # the moving rectangle is flagged ...
        far = np.ones((H, W), bool)
        far[max(ry.start - 3, 0):ry.stop + 3, max(rx.start - 3, 0):rx.stop + 3] = False
        assert m[far].mean() < 0.05, (n, float(m[far].mean()))                           # ... and the static scene is not
        png = np.array(PIL.Image.open(out_dir / f"dynamic_mask_{n}.png").convert("L"))
        assert np.array_equal(png, m.astype(np.uint8) * 255)
        big = np.array(PIL.Image.open(out_dir / f"enlarged_dynamic_mask_{n}.png").convert("L"))
        pad = np.zeros((H + 2, W + 2), np.uint8)
        pad[1:-1, 1:-1] = png
        want = np.max([pad[dy:dy + H, dx:dx + W] for dy in range(3) for dx in range(3)], axis=0)       # 3x3 dilation (self masks)
        assert np.array_equal(big, want)


def test_own_flow_builds_the_flow_engine_once(monkeypatch):
    import align3r_amd.dust3r.inference as inf_mod
    import align3r_amd.raft as raft_mod
    from align3r_amd.raft_weights import RAFT_TINY, synthetic_raft_frames, synthetic_raft_state_dict
    from align3r_amd.tool import hierarchical as hz
    S = 128
    cams, world, f = _world(S, S)
    a, _ = synthetic_raft_frames(N_FRAMES, S, S, 21)
    frames = [torch.from_numpy(a[n] / 255.0 * 2 - 1) for n in range(N_FRAMES)]          # view['img'] is normalised to [-1, 1]
    built = []
    real_init = raft_mod.RaftEngine.__init__

    def spy(self, *args, **kw):
        built.append(1)
        return real_init(self, *args, **kw)
    monkeypatch.setattr(raft_mod.RaftEngine, "__init__", spy)
    monkeypatch.setattr(inf_mod, "inference", _fake_inference(cams, world, S, S, frames=frames))
    net = raft_mod.RAFT2(RAFT_TINY, synthetic_raft_state_dict(RAFT_TINY, 0))
    imgs = [dict(idx=i, instance=str(i), true_shape=np.int32([[S, S]])) for i in range(N_FRAMES)]
    torch.manual_seed(0)
    res = hz.hierarchical_alignment(imgs, None, "cuda", niter=10, flow=dict(flow_net=net), **DRIVE)
    assert len(built) == 1, len(built)                                  # one engine for the keyframe scene and all three clips
    assert len(res["depths"]) == N_FRAMES and all(np.isfinite(d).all() and d.shape == (S, S) for d in res["depths"])
    assert np.isfinite(np.stack(res["poses"])).all() and np.isfinite(res["focals"]).all()
    assert all(m is not None and m.shape == (S, S) for m in res["dynamic_masks"])


def test_fp16_observations_through_the_flow_driver(tmp_path_factory):
    h32, _, _ = _drive(tmp_path_factory, False, 0)
    h16, _, _ = _drive(tmp_path_factory, False, 0, "fp16")
    for q in ("depths", "poses_raw", "poses", "intrinsics", "dynamic_masks"):           # the initialisation reads the fp32 predictions
        assert all(np.array_equal(a, b) for a, b in zip(h16[q], h32[q])), q
    assert h16["focals"] == h32["focals"]
    run, _, _ = _drive(tmp_path_factory, False, 5, "fp16")
    assert all(np.isfinite(d).all() for d in run["depths"]) and np.isfinite(np.stack(run["poses"])).all()


def test_two_keyframes_and_refusals(monkeypatch):
    """Five frames at clip size 3: a keyframe stage of exactly two keyframes (a scene of N = 2) and a last clip of two frames."""
    import align3r_amd.dust3r.inference as inf_mod
    from align3r_amd.tool import hierarchical as hz
    cams, world, f = _world()
    monkeypatch.setattr(inf_mod, "inference", _fake_inference(cams, world, H, W, accepts_device=True))
    torch.manual_seed(0)
    res = hz.hierarchical_alignment(_imgs()[:5], None, "cuda", niter=10, flow=dict(flow_fn=_flow_fn(cams, world, f)), device_resident=True,
                                    **DRIVE)
    assert res["keyframes_id"] == [0, 3] and res["all_clips_id"] == [[0, 1, 2], [3, 4]] and res["key_scene"].n_imgs == 2
    assert len(res["depths"]) == 5 and all(np.isfinite(d).all() for d in res["depths"]) and np.isfinite(np.stack(res["poses"])).all()
    kp = res["key_scene"].get_im_poses().detach().cpu().numpy()
    assert np.array_equal(res["poses"][0], kp[0]) and np.array_equal(res["poses"][3], kp[1])
    with pytest.raises(ValueError, match="3 frames"):                    # the clip-size rule has no answer for three frames
        hz.hierarchical_alignment(_imgs()[:3], None, "cuda", flow=dict(flow_fn=_flow_fn(cams, world, f)), **DRIVE)
