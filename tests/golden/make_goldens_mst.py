"""Goldens of init='mst' (dust3r/cloud_opt/init_im_poses.py:69-252, cloud_opt_flow/init_im_poses.py:88-284) -> tests/golden/mst.npz / .json.

    python tests/golden/make_goldens_mst.py [--out tests/golden]

Drives the reference's own init_minimum_spanning_tree + init_from_pts3d on the CPU with the stand-ins that make_goldens.py
installs (this file imports its helpers and does not edit it).  Three more stand-ins, all named in the metadata:
  * roma.rigid_points_registration: weighted Kabsch / Umeyama in closed form with the determinant fix, computed in float64 and
    returned in the input dtype (tests/test_mst_golden_cpu.py checks it on its own);
  * roma.rotmat_to_unitquat: the closed form of make_goldens_modular.py (largest-component branch, XYZW), returned in the input
    dtype so that the float64 run keeps its precision;
  * fast_pnp of the module under test (cv2's RANSAC-PnP): a recorder that stores what it was handed and returns None, so the
    reference falls through to the identity pose.  The PnP solve itself is therefore NOT pinned.
Everything else -- edge scores, the spanning tree and the walk over it, estimate_focal (with its stale-`i_j` quirk), the chain
of registrations, init_from_pts3d, get_pw_norm_scale_factor, _set_pose / _set_depthmap / _set_focal -- is the reference's code.

Every case runs twice through the same code: in fp32 (as the reference runs) and in float64 (float64 inputs, float64 default
dtype, parameters cast to float64).  The float64 results are the expected values; `spread[q]` = rel_err(fp32 run, float64 run)
is the reference's own rounding noise on quantity q and is what the GPU test scales its bounds from.  A case whose float64 run
does not stay in float64 (init_priors: the reference casts the key pose to np.float32 and geotrf follows the pose's dtype) stores
its fp32 values and says so.

Layout: inputs per scene (`<scene>_p1_<e>` ..., shared by the cases that name the scene; a case's confidences are the scene's
base maps times its per-edge `factors`, a float32 product), per case `tag`: the seed-11 state before the init, edge scores,
what minimum_spanning_tree returned (focals, point maps, poses), and the state after init_from_pts3d through the getters.
"""
from __future__ import annotations

import argparse
import contextlib
import io
import json
import os
import re
import sys
import zipfile

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import numpy as np
import torch

SEED = 11
MIN_SCORE_GAP = 1e-3
SHAPE4 = (12, 16)
MIXED = [(12, 16), (12, 16), (10, 12), (14, 10)]
COMPLETE4 = [(i, j) for i in range(4) for j in range(4) if i != j]
# tag, scene, class, boosted edges (their factors, best first; every other edge draws one of 1 + 0.03 k), extras
CASES = [
    dict(tag="swin", scene="s5", cls="pco", boost={}),
    dict(tag="complete", scene="c4", cls="pco", boost={(0, 1): 2.0, (2, 3): 1.8, (1, 2): 1.6}, want_retry=True),
    dict(tag="ragged", scene="r4", cls="pco", boost={}),
    dict(tag="priors_i", scene="c4", cls="pco", boost={(1, 3): 2.0, (0, 2): 1.8, (2, 1): 1.6}, priors=True, want_init=(0, 2)),
    dict(tag="priors_j", scene="c4", cls="pco", boost={(1, 2): 2.0, (3, 0): 1.8, (0, 1): 1.6}, priors=True, want_init=(3, 0)),
    dict(tag="preset2", scene="c4", cls="modular", boost={}, preset=[1, 3]),
    dict(tag="flow", scene="f4", cls="flow", boost={}, kw=dict(shared_focal=False, temporal_smoothing_weight=0.0,
                                                                depth_regularize_weight=50.0)),
    dict(tag="flow_shared", scene="f4", cls="flow", boost={}, kw=dict(shared_focal=True, temporal_smoothing_weight=0.01,
                                                                       depth_regularize_weight=5.0)),
]
QUANTITIES = ("scores", "mst_focals", "mst_pts3d", "mst_poses", "pw_poses_4x4", "im_poses_4x4", "focals", "depth", "s_factor", "loss")


# ----------------------------------------------------------------------------- stand-ins (the project's own code)
def rigid_points_registration(x, y, weights=None, compute_scaling=False):
    """roma.rigid_points_registration for x, y [P,3]: (R, T, s) minimising sum_p w_p |s R x_p + T - y_p|^2 over rotations R
    (det R = +1: the determinant fix flips the weakest singular direction rather than return a reflection), translations T and,
    with compute_scaling, scales s (else s = 1).  Weighted Kabsch / Umeyama in closed form, float64 inside, input dtype outside."""
    dt = x.dtype
    X, Y = x.reshape(-1, 3).double(), y.reshape(-1, 3).double()
    w = torch.ones(len(X), dtype=torch.float64) if weights is None else weights.reshape(-1).double()
    w = w / w.sum()
    xm, ym = (w[:, None] * X).sum(0), (w[:, None] * Y).sum(0)
    Xc, Yc = X - xm, Y - ym
    cov = (w[:, None] * Yc).T @ Xc                                      # sum_p w_p y_p x_p^T
    U, S, Vt = torch.linalg.svd(cov)
    d = torch.ones(3, dtype=torch.float64)
    d[2] = torch.sign(torch.det(U @ Vt))
    R = (U * d[None, :]) @ Vt
    s = (S * d).sum() / (w * Xc.square().sum(-1)).sum() if compute_scaling else torch.ones((), dtype=torch.float64)
    T = ym - s * (R @ xm)
    return R.to(dt), T.to(dt), s.to(dt)


def rotmat_to_unitquat(R):
    """Rotation matrix -> XYZW unit quaternion: the closed form of make_goldens_modular.py (largest-component branch selection,
    float64 inside), returned in R's dtype."""
    m00, m01, m02, m10, m11, m12, m20, m21, m22 = R.detach().double().reshape(9).tolist()
    tr = m00 + m11 + m22
    if tr > 0:
        s = np.sqrt(tr + 1.0) * 2
        q = ((m21 - m12) / s, (m02 - m20) / s, (m10 - m01) / s, 0.25 * s)
    elif m00 > m11 and m00 > m22:
        s = np.sqrt(1.0 + m00 - m11 - m22) * 2
        q = (0.25 * s, (m01 + m10) / s, (m02 + m20) / s, (m21 - m12) / s)
    elif m11 > m22:
        s = np.sqrt(1.0 + m11 - m00 - m22) * 2
        q = ((m01 + m10) / s, 0.25 * s, (m12 + m21) / s, (m02 - m20) / s)
    else:
        s = np.sqrt(1.0 + m22 - m00 - m11) * 2
        q = ((m02 + m20) / s, (m12 + m21) / s, 0.25 * s, (m10 - m01) / s)
    return torch.tensor(q, dtype=R.dtype)


# ----------------------------------------------------------------------------- scenes
def camera(n, N):
    a = 0.15 * (n - (N - 1) / 2)
    R = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])
    return R, np.array([0.6 * np.sin(a) * 3, 0.05 * n, 3 - 3 * np.cos(a)])


def geom_scene(shapes, edges, seed):
    """The 'geom' idea of make_goldens._align_scene -- a bumpy surface seen from a small arc, pairwise point maps = the true points
    in the first camera's frame + noise of sigma 0.01 (1 % of the unit) -- with what the MST initialisation is sensitive to: every
    camera has its OWN focal 1.2 S (1 + 0.1 n), S the largest image side, and possibly its own shape, and the two sides' confidences are independent."""
    N = len(shapes)
    rng = np.random.default_rng(seed)
    cams = [camera(n, N) for n in range(N)]
    S = max(max(s) for s in shapes)                     # one base for all images, so that the focals stay 10 % apart on mixed shapes
    focals = [1.2 * S * (1 + 0.1 * n) for n in range(N)]
    world = []
    for n, (H, W) in enumerate(shapes):
        u, v = np.meshgrid(np.arange(W) - W / 2 + 0.5, np.arange(H) - H / 2 + 0.5)
        d = 3 + 0.5 * np.sin(u / W * 6 + n) * np.cos(v / H * 4) + 0.2 * rng.random((H, W))
        pc = np.stack([u / focals[n] * d, v / focals[n] * d, d], -1)
        world.append(pc @ cams[n][0].T + cams[n][1])
    p1, p2, c1, c2 = [], [], [], []
    for i, j in edges:
        R, t = cams[i]
        p1.append(((world[i] - t) @ R + 0.01 * rng.standard_normal(shapes[i] + (3,))).astype(np.float32))
        p2.append(((world[j] - t) @ R + 0.01 * rng.standard_normal(shapes[j] + (3,))).astype(np.float32))
    for i, j in edges:
        c1.append((1 + 9 * rng.random(shapes[i])).astype(np.float32))
        c2.append((1 + 9 * rng.random(shapes[j])).astype(np.float32))
    poses = np.zeros((N, 4, 4), np.float32)
    for n, (R, t) in enumerate(cams):
        poses[n, :3, :3], poses[n, :3, 3], poses[n, 3, 3] = R, t, 1
    return dict(shapes=shapes, edges=edges, p1=p1, p2=p2, c1=c1, c2=c2, cam_poses=poses, cam_focals=focals)


def edge_factors(edges, boost, seed):
    """One confidence factor per edge: the boosted edges as written, every other edge a distinct 1 + 0.03 k in a seeded order."""
    rest = [e for e in edges if e not in boost]
    order = np.random.default_rng(seed).permutation(len(rest))
    low = {e: 1 + 0.03 * int(k) for e, k in zip(rest, order)}
    return [float(boost.get(e, low.get(e))) for e in edges]


def rel_err(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30))


# ----------------------------------------------------------------------------- one run of the reference
def run_reference(case, scene, factors, f64):
    """The reference's init='mst' on one case in fp32 or float64.  Returns (dict of arrays, dict of discrete facts)."""
    dt = torch.float64 if f64 else torch.float32
    torch.set_default_dtype(dt)
    try:
        return _run(case, scene, factors, dt)
    finally:
        torch.set_default_dtype(torch.float32)


def _run(case, scene, factors, dt):
    shapes, edges = scene["shapes"], scene["edges"]
    N, E, P = len(shapes), len(edges), max(h * w for h, w in shapes)
    uniform = all(s == shapes[0] for s in shapes)
    tt = lambda lst: [torch.from_numpy(a).to(dt) for a in lst]
    c1 = [c * np.float32(f) for c, f in zip(scene["c1"], factors)]          # float32 products: the test rebuilds the same values
    c2 = [c * np.float32(f) for c, f in zip(scene["c2"], factors)]
    assert all(c.dtype == np.float32 for c in c1 + c2)
    p1, p2, c1, c2 = tt(scene["p1"]), tt(scene["p2"]), tt(c1), tt(c2)
    if uniform and case["cls"] != "modular":
        p1, p2, c1, c2 = (torch.stack(x) for x in (p1, p2, c1, c2))
    view1, view2 = dict(idx=[i for i, j in edges]), dict(idx=[j for i, j in edges])
    pred1, pred2 = dict(pts3d=p1, conf=c1), dict(pts3d_in_other_view=p2, conf=c2)
    torch.manual_seed(SEED)
    log = io.StringIO()
    with contextlib.redirect_stdout(log):
        if case["cls"] == "pco":
            from dust3r.cloud_opt import global_aligner, GlobalAlignerMode
            import dust3r.cloud_opt.init_im_poses as init_fun
            net = global_aligner(dict(view1=view1, view2=view2, pred1=pred1, pred2=pred2), False, [], "cpu",
                                 mode=GlobalAlignerMode.PointCloudOptimizer, verbose=True, min_conf_thr=3)
        elif case["cls"] == "modular":       # the reference's global_aligner() cannot build this class (make_goldens_modular.py)
            from dust3r.cloud_opt.modular_optimizer import ModularPointCloudOptimizer
            import dust3r.cloud_opt.init_im_poses as init_fun
            net = ModularPointCloudOptimizer(view1, view2, pred1, pred2, False, [], verbose=True, min_conf_thr=3)
        else:
            from dust3r.cloud_opt_flow import global_aligner, GlobalAlignerMode
            import dust3r.cloud_opt_flow.init_im_poses as init_fun
            dyn = torch.from_numpy(scene["dyn"])
            view1["dynamic_mask"], view2["dynamic_mask"] = [dyn[i] for i, j in edges], [dyn[j] for i, j in edges]
            net = global_aligner(dict(view1=view1, view2=view2, pred1=pred1, pred2=pred2), "cpu", mode=GlobalAlignerMode.PointCloudOptimizer,
                                 verbose=True, min_conf_thr=3, translation_weight=1.0, flow_loss_weight=0.0, flow_loss_start_epoch=0.1,
                                 flow_loss_thre=20.0, num_total_iter=30, pxl_thre=50, **case["kw"])
        if dt == torch.float64:
            net.double()                       # im_focals is a torch.FloatTensor whatever the default dtype
    rav = lambda t: torch.cat((t.reshape(-1, *t.shape[2:]), t.new_zeros((P - t.shape[0] * t.shape[1],) + tuple(t.shape[2:]))))
    out, facts = {}, {}
    depth_params = list(net.im_depthmaps)
    out["init_pw_poses"] = net.pw_poses.detach().numpy().copy()
    out["init_im_poses"] = torch.stack(list(net.im_poses)).detach().numpy().copy()
    out["init_depth"] = torch.stack([rav(d.reshape(h, w)) if d.numel() == h * w else d for d, (h, w) in zip(depth_params, shapes)]).detach().numpy().copy()
    if case.get("preset"):
        with contextlib.redirect_stdout(log):
            net.preset_pose([torch.from_numpy(scene["cam_poses"][i]).to(dt) for i in case["preset"]], case["preset"])
    init_priors = None
    if case.get("priors"):                     # [pose, depth, [focal]] of the key image, nested lists as tool/hierarchical.py passes them
        init_priors = [scene["key_pose"].tolist(), scene["key_depth"], [float(scene["key_focal"])]]
    # ---- recorders: fast_pnp -> None, and a copy of what minimum_spanning_tree returns (init_from_pts3d works in place on it)
    calls, got = [], {}
    real_mst = init_fun.minimum_spanning_tree

    def fake_pnp(pts3d, focal, msk, device, pp=None, niter_PnP=10):
        calls.append(dict(pts=pts3d, focal=focal, msk_sum=int(msk.sum())))
        return None

    def spy_mst(*a, **k):
        pts3d, msp_edges, im_focals, im_poses = real_mst(*a, **k)
        got.update(pts3d=[p.clone() for p in pts3d], focals=list(im_focals), poses=im_poses.clone(), objects=pts3d)
        return pts3d, msp_edges, im_focals, im_poses
    real_pnp = init_fun.fast_pnp
    init_fun.fast_pnp, init_fun.minimum_spanning_tree = fake_pnp, spy_mst
    try:
        with contextlib.redirect_stdout(log):
            init_fun.init_minimum_spanning_tree(net, init_priors=init_priors, niter_PnP=10)
    finally:
        init_fun.fast_pnp, init_fun.minimum_spanning_tree = real_pnp, real_mst
    facts["all_float64"] = bool(dt == torch.float64 and all(p.dtype == torch.float64 for p in got["pts3d"]) and got["poses"].dtype == torch.float64)
    # ---- discrete facts: the walk over the tree as printed, the PnP calls
    tree = [[int(i), int(j), bool(si), bool(sj)] for i, si, j, sj in re.findall(r" init edge \((\d+)(\*?),(\d+)(\*?)\)", log.getvalue())]
    facts["tree"] = tree
    scores = init_fun.compute_edge_scores(map(init_fun.i_j_ij, edges), net.conf_i, net.conf_j)
    out["scores"] = np.asarray([scores[e] for e in edges], np.float64)
    pnp = []
    for c in calls:
        idx = [n for n, p in enumerate(got["objects"]) if p is c["pts"]]
        assert len(idx) == 1
        pnp.append(dict(index=idx[0], msk_sum=c["msk_sum"], focal=float(c["focal"])))
    facts["pnp"] = pnp
    out["mst_focals"] = np.asarray([np.nan if f is None else float(f) for f in got["focals"]], np.float64)
    out["mst_pts3d"] = torch.stack([rav(p) for p in got["pts3d"]]).numpy()
    out["mst_poses"] = got["poses"].numpy()
    with torch.no_grad(), contextlib.redirect_stdout(log):
        out["pw_poses_4x4"] = net.get_pw_poses().numpy()
        out["im_poses_4x4"] = net.get_im_poses().numpy()
        out["focals"] = net.get_focals().reshape(N).numpy()
        if case["cls"] == "modular":
            out["depth"] = torch.stack([rav(d) for d in net.get_depthmaps()]).numpy()
        else:
            out["depth"] = torch.stack(list(net.get_depthmaps(raw=True))).numpy()
        out["s_factor"] = np.asarray(float(net.get_pw_norm_scale_factor()))
        out["loss"] = np.asarray(float(net()))
    facts["norm_pw_scale"] = bool(net.norm_pw_scale)
    facts["known_poses"] = [not p.requires_grad for p in net.im_poses]
    return out, facts


def write_npz(path, arrays):
    """np.savez_compressed with fixed zip timestamps and a sorted member order: the same arrays give the same bytes."""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for name in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asarray(arrays[name], order="C"), allow_pickle=False)
            info = zipfile.ZipInfo(name + ".npy", (1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            z.writestr(info, buf.getvalue())


def generate(out_dir):
    sys.dont_write_bytecode = True              # the reference tree is read-only
    import make_goldens as mg
    mg.import_reference(aligner=True)
    sys.modules["roma"].rigid_points_registration = rigid_points_registration
    sys.modules["roma"].rotmat_to_unitquat = rotmat_to_unitquat
    torch.set_num_threads(1)
    from dust3r.image_pairs import make_pairs
    with contextlib.redirect_stdout(io.StringIO()):
        swin = [(a["idx"], b["idx"]) for a, b in make_pairs([dict(idx=i) for i in range(5)], scene_graph="swin-2", prefilter=None, symmetrize=True)]
    scenes = dict(s5=geom_scene([(16, 24)] * 5, swin, seed=31), c4=geom_scene([SHAPE4] * 4, COMPLETE4, seed=32),
                  r4=geom_scene(MIXED, COMPLETE4, seed=33))
    c4 = scenes["c4"]                                     # the key image's priors: a pose away from the identity, its own focal
    c4["key_pose"] = scenes["s5"]["cam_poses"][4].astype(np.float64)
    c4["key_depth"] = (3 + 0.1 * np.arange(SHAPE4[0] * SHAPE4[1], dtype=np.float32).reshape(SHAPE4) / 192)
    c4["key_focal"] = 1.3 * max(SHAPE4)
    fs = mg._flow_scene(4, 12, 16, seed=5)
    scenes["f4"] = dict(shapes=[(12, 16)] * 4, edges=[tuple(e) for e in fs["edges"]], p1=list(fs["p1"]), p2=list(fs["p2"]),
                        c1=list(fs["c1"]), c2=list(fs["c2"]), dyn=fs["dyn"])
    g = {}
    meta = dict(note="reference init_minimum_spanning_tree + init_from_pts3d on the CPU; stand-ins: roma of make_goldens.py (unit quaternion "
                     "-> 4x4) plus rigid_points_registration (weighted Kabsch/Umeyama, determinant fix, float64 inside) and rotmat_to_unitquat "
                     "(closed form, largest-component branch, XYZW) of make_goldens_mst.py; cv2 stubbed; fast_pnp replaced by a recorder "
                     "returning None (identity pose fallback): the PnP solve is not pinned",
                seed=SEED, min_conf_thr=3, min_score_gap=MIN_SCORE_GAP, fallback_bound=2e-4, scenes={}, cases=[])
    for name, sc in scenes.items():
        for e in range(len(sc["edges"])):
            g[f"{name}_p1_{e}"], g[f"{name}_p2_{e}"], g[f"{name}_c1_{e}"], g[f"{name}_c2_{e}"] = sc["p1"][e], sc["p2"][e], sc["c1"][e], sc["c2"][e]
        if "dyn" in sc:
            g[f"{name}_dyn"] = sc["dyn"]
        if "cam_poses" in sc:
            g[f"{name}_cam_poses"] = sc["cam_poses"]
        if "key_pose" in sc:
            g[f"{name}_key_pose"], g[f"{name}_key_depth"] = sc["key_pose"], sc["key_depth"]
        meta["scenes"][name] = dict(shapes=[list(s) for s in sc["shapes"]], edges=[list(e) for e in sc["edges"]],
                                    cam_focals=sc.get("cam_focals"), key_focal=sc.get("key_focal"))
    for k, case in enumerate(CASES):
        tag, sc = case["tag"], scenes[case["scene"]]
        factors = edge_factors(sc["edges"], case["boost"], seed=100 + k)
        r32, f32 = run_reference(case, sc, factors, f64=False)
        r64, f64 = run_reference(case, sc, factors, f64=True)
        for key in ("tree", "pnp", "norm_pw_scale", "known_poses"):
            a, b = f32[key], f64[key]
            if key == "pnp":
                a, b = [(c["index"], c["msk_sum"]) for c in a], [(c["index"], c["msk_sum"]) for c in b]
            assert a == b, (tag, key, a, b)
        use64 = f64["all_float64"]
        want = r64 if use64 else r32
        s = np.sort(want["scores"])
        gap = float(((s[1:] - s[:-1]) / s[1:]).min())
        assert gap >= MIN_SCORE_GAP, (tag, gap)
        tree = f32["tree"]
        # 'let's try again later': an edge of the tree was popped while neither of its images was placed
        order = sorted(((r64["scores"][sc["edges"].index((i, j))], i, j) for i, j, _, _ in tree), reverse=True)
        retry = [(i, j) for _, i, j in order] != [(i, j) for i, j, _, _ in tree]
        if case.get("want_retry"):
            assert retry, (tag, tree)
        if case.get("want_init"):
            assert tuple(tree[0][:2]) == case["want_init"], (tag, tree)
        assert len(f32["pnp"]) >= 1, tag
        for key, v in want.items():
            g[f"{tag}_{key}"] = v if key.startswith("init_") else np.asarray(v, np.float64)
        for key in ("init_pw_poses", "init_im_poses", "init_depth"):
            g[f"{tag}_{key}"] = r32[key]
        spread = {q: rel_err(r32[q], r64[q]) for q in QUANTITIES}
        spread["mst_focals"] = rel_err(np.nan_to_num(r32["mst_focals"]), np.nan_to_num(r64["mst_focals"]))
        pnp = [dict(c, spread_pts=rel_err(r32["mst_pts3d"][c["index"]], r64["mst_pts3d"][c["index"]]),
                    spread_focal=rel_err(c["focal"], d["focal"]), focal=(d if use64 else c)["focal"]) for c, d in zip(f32["pnp"], f64["pnp"])]
        meta["cases"].append(dict(tag=tag, scene=case["scene"], cls=case["cls"], kw=case.get("kw", {}), factors=factors,
                                  priors=bool(case.get("priors")), preset=case.get("preset"), tree=tree, retry_triggered=bool(retry),
                                  pnp=pnp, score_gap=gap, float64_expectations=bool(use64), spread=spread,
                                  norm_pw_scale=f32["norm_pw_scale"], known_poses=f32["known_poses"]))
        print("mst", tag, "tree", [f"({i}{'*' * a},{j}{'*' * b})" for i, j, a, b in tree], "retry", retry, "pnp", [c["index"] for c in pnp],
              "gap %.2e" % gap, "f64", use64, "loss", float(want["loss"]), "s_factor", float(want["s_factor"]))
        print("    focals", np.round(want["mst_focals"], 5).tolist())
        print("    spread", {q: float("%.2e" % v) for q, v in spread.items()})
    write_npz(os.path.join(out_dir, "mst.npz"), g)
    with open(os.path.join(out_dir, "mst.json"), "w") as f:
        json.dump(meta, f, sort_keys=True)
    print("mst.npz", os.path.getsize(os.path.join(out_dir, "mst.npz")), "bytes")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=HERE)
    generate(ap.parse_args().out)
