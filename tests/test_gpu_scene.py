"""GPU: scene out (csrc/scene.hip) -- the aligned scene of an aligner handle as dense world points and as a compacted point cloud.

Every case is compared with a float64 numpy restatement built only from the scene's own getters after the fact (get_depthmaps(raw),
get_focals, get_principal_points, get_im_poses, im_conf, dynamic_masks, imgs):
  * the kept set is exact: index (values and order), count and gathered colours equal the restatement's -- the threshold compare
    is an fp32 compare on caller-given numbers, there is nothing to round;
  * coordinates: |delta| <= 1e-5 * max|xyz| of the case, the project's bound for aligner tensors; measured margins
    are recorded as scene_<case>.
Shapes: 2x3 (fewer pixels than a wave), 37x41 (P % 4 != 0: scalar form, ragged last chunk), 36x44 (vector form, two chunks, ragged
tail), 32x48 mixed with 24x40 (padding).  Problems come from tests/align_cases.py.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import align_cases as ac
from conftest import record_margin

pytestmark = pytest.mark.gpu

BOUND = 1e-5                 # of the case's max |xyz| ("1e-5 of the tensor max")


# ------------------------------------------------------------------------------------------------- scenes
def _views(edges, imgs, dyn=None):
    v1 = dict(idx=[i for i, j in edges], img=[imgs[i] for i, j in edges])
    v2 = dict(idx=[j for i, j in edges], img=[imgs[j] for i, j in edges])
    if dyn is not None:
        v1["dynamic_mask"] = [dyn[i] for i, j in edges]
        v2["dynamic_mask"] = [dyn[j] for i, j in edges]
    return v1, v2


def _problem(N, H, W, seed, shared_focal=False):
    # 30 % dynamic pixels, the LAST image fully dynamic
    return ac.flow_problem(N, H, W, ac.window_graph(N, 2), seed, dyn_frac=0.3, pxl_thre=1e9, thre=1e9, shared_focal=shared_focal,
                           train_pp=False, full_dynamic=True, guard=False)


def make_scene(kind, N, H, W, seed=5):
    """(scene, dyn [N,P] bool).  kind: plain | mono | flow (cloud_opt_flow class, shared_focal=True, dynamic masks in the views)."""
    prob = _problem(N, H, W, seed, shared_focal=(kind == "flow"))
    edges, P = prob["edges"], H * W
    ei, ej, p1, p2, w1, w2, _ = prob["args"]
    rng = np.random.default_rng(seed + 77)
    imgs = [torch.from_numpy(rng.uniform(-1.1, 1.1, (3, H, W)).astype(np.float32)) for _ in range(N)]     # beyond [-1, 1]: clipped
    dyn = prob["flow"]["dyn"].reshape(N, H, W)
    v1, v2 = _views(edges, imgs, [torch.from_numpy(d) for d in dyn] if kind == "flow" else None)
    t = lambda a, *s: torch.from_numpy(np.ascontiguousarray(a)).reshape(len(edges), *s)
    out = dict(view1=v1, view2=v2, pred1=dict(pts3d=t(p1, H, W, 3), conf=t(np.exp(w1), H, W)),
               pred2=dict(pts3d_in_other_view=t(p2, H, W, 3), conf=t(np.exp(w2), H, W)))
    torch.manual_seed(3)
    init = dict(prob["init"])
    if kind == "flow":
        from align3r_amd.dust3r.cloud_opt_flow import GlobalAlignerMode, global_aligner
        scene = global_aligner(out, "cuda", mode=GlobalAlignerMode.PointCloudOptimizer, verbose=False, min_conf_thr=3, shared_focal=True,
                               temporal_smoothing_weight=0.01)
    else:
        from align3r_amd.dust3r.cloud_opt import GlobalAlignerMode, global_aligner
        mono = [torch.from_numpy((1 + rng.random((H, W))).astype(np.float32)) for _ in range(N)] if kind == "mono" else []
        scene = global_aligner(out, kind == "mono", mono, "cuda", mode=GlobalAlignerMode.PointCloudOptimizer, verbose=False, min_conf_thr=3)
        if kind == "mono":
            init["shifts"] = (0.05 * rng.standard_normal(N)).astype(np.float32)
    scene.engine.set_params(**init)
    return scene, dyn.reshape(N, P)


def make_mixed_scene(seed=9):
    """Four images, 32x48 and 24x40 alternating, per-edge prediction lists (max_area = 1536, 960 real pixels in the small ones)."""
    shapes = [(32, 48), (24, 40), (32, 48), (24, 40)]
    N, edges = len(shapes), ac.window_graph(4, 2)
    rng = np.random.default_rng(seed)
    imgs = [torch.from_numpy(rng.uniform(-1, 1, (3, h, w)).astype(np.float32)) for h, w in shapes]
    rnd = lambda n: [torch.from_numpy(rng.standard_normal(shapes[n] + (3,)).astype(np.float32))]
    cnf = lambda n: [torch.from_numpy((1 + 9 * rng.random(shapes[n])).astype(np.float32))]
    p1, p2, c1, c2 = [], [], [], []
    for i, j in edges:
        p1 += rnd(i); p2 += rnd(j); c1 += cnf(i); c2 += cnf(j)
    v1, v2 = _views(edges, imgs)
    out = dict(view1=v1, view2=v2, pred1=dict(pts3d=p1, conf=c1), pred2=dict(pts3d_in_other_view=p2, conf=c2))
    from align3r_amd.dust3r.cloud_opt import GlobalAlignerMode, global_aligner
    torch.manual_seed(4)
    scene = global_aligner(out, False, [], "cuda", mode=GlobalAlignerMode.PointCloudOptimizer, verbose=False, min_conf_thr=3)
    P = scene.max_area
    im = (0.05 * rng.standard_normal((N, 7))).astype(np.float32)
    im[:, 3] += 1
    scene.engine.set_params(depth=(0.1 * rng.standard_normal((N, P))).astype(np.float32), im_poses=im)
    dyn = rng.random((N, P)) < 0.3
    return scene, dyn


# ------------------------------------------------------------------------------------------------- restatement
def restate(depth, focals, pp, RT, imshapes, P):
    """float64 world points [N,P,3] (zeros at padding) from fp32 depths [N,P], focals [N], principal points [N,2], poses [N,>=3,4]."""
    N = len(imshapes)
    depth, focals, pp, RT = (np.asarray(a).astype(np.float64) for a in (depth, focals, pp, RT))
    xyz = np.zeros((N, P, 3))
    with np.errstate(all="ignore"):
        for n, (h, w) in enumerate(imshapes):
            p = np.arange(h * w)
            x, y, d = (p % w).astype(np.float64), (p // w).astype(np.float64), depth[n, :h * w]
            rel = np.stack([d * (x - pp[n, 0]) / focals[n], d * (y - pp[n, 1]) / focals[n], d], 1)
            xyz[n, :h * w] = rel @ RT[n, :3, :3].T + RT[n, :3, 3]
    return xyz


def scene_points_np(scene):
    host = lambda t: t.detach().cpu().numpy()
    return restate(host(scene.get_depthmaps(raw=True)), host(scene.get_focals()).reshape(-1), host(scene.get_principal_points()),
                   host(scene.get_im_poses()), scene.imshapes, scene.max_area)


def stacked(maps, imshapes, P, dtype):
    """per-image [h,w,...] maps -> [N,P,...], zero-filled"""
    out = np.zeros((len(maps), P) + tuple(np.asarray(maps[0]).shape[2:]), dtype)
    for n, (m, (h, w)) in enumerate(zip(maps, imshapes)):
        m = m.detach().cpu().numpy() if torch.is_tensor(m) else np.asarray(m)
        out[n, :h * w] = m.reshape((h * w,) + m.shape[2:])
    return out


def scene_inputs(scene):
    """(conf [N,P] float32 from the scene's CURRENT im_conf, rgb [N,P,3] uint8 from its frames)"""
    conf = stacked(scene.im_conf, scene.imshapes, scene.max_area, np.float32)
    rgb = stacked([np.clip(np.rint(255 * im), 0, 255).astype(np.uint8) for im in scene.imgs], scene.imshapes, scene.max_area, np.uint8)
    return conf, rgb


def kept_np(xyz, conf, thr, dyn, imshapes):
    """the numpy index list (n * P + p, image-major, row-major) of the kept pixels"""
    N, P = conf.shape
    inside = np.arange(P)[None, :] < np.asarray([h * w for h, w in imshapes])[:, None]
    keep = inside & (conf > np.float32(thr)) & np.isfinite(xyz).all(-1)
    if dyn is not None:
        keep &= ~np.asarray(dyn, bool)
    return np.flatnonzero(keep.reshape(-1))


def check_export(got, xyz, conf, thr, dyn, rgb, imshapes):
    """Exact kept set + colours, bounded coordinates.  Returns (M, max |delta| / max |xyz| or 0.0 for an empty cloud)."""
    idx = kept_np(xyz, conf, thr, dyn, imshapes)
    M = len(idx)
    assert got["xyz"].shape == (M, 3) and got["xyz"].dtype == torch.float32
    assert got["index"].dtype == torch.int32 and np.array_equal(got["index"].cpu().numpy(), idx)
    if rgb is not None:
        assert got["rgb"].dtype == torch.uint8 and np.array_equal(got["rgb"].cpu().numpy(), rgb.reshape(-1, 3)[idx])
    if M == 0:
        return 0, 0.0
    ref = xyz.reshape(-1, 3)[idx]
    scale = np.abs(ref).max()
    return M, float(np.abs(got["xyz"].cpu().numpy().astype(np.float64) - ref).max() / scale)


CASES = {                     # name: (kind, N, H, W)
    "plain_2x3": ("plain", 3, 2, 3),
    "plain_37x41": ("plain", 4, 37, 41),
    "plain_36x44": ("plain", 4, 36, 44),
    "mono_37x41": ("mono", 3, 37, 41),
    "mono_36x44": ("mono", 3, 36, 44),
    "flow_sf_37x41": ("flow", 5, 37, 41),
    "flow_sf_36x44": ("flow", 4, 36, 44),
    "mixed_32x48_24x40": ("mixed", 4, 0, 0),
}


def _build(name):
    kind, N, H, W = CASES[name]
    return make_mixed_scene() if kind == "mixed" else make_scene(kind, N, H, W)


@pytest.mark.parametrize("name", list(CASES))
def test_export_vs_numpy_restatement(name):
    """Thresholds keeping about half / nothing / everything, with and without the 30 % dynamic mask (one image fully masked)."""
    scene, dyn = _build(name)
    eng, shapes = scene.engine, scene.imshapes
    xyz = scene_points_np(scene)
    conf, rgb = scene_inputs(scene)
    real = np.concatenate([conf[n, :h * w] for n, (h, w) in enumerate(shapes)])
    total = sum(h * w for h, w in shapes)
    worst, counts = 0.0, {}
    for tag, thr in (("half", float(np.median(real))), ("none", float(real.max()) + 1.0), ("all", float(real.min()) - 1.0)):
        for dtag, d in (("", None), ("_dyn", dyn)):
            got = eng.export_points(conf, thr, dyn=d, rgb=rgb, with_index=True)
            M, err = check_export(got, xyz, conf, thr, d, rgb, shapes)
            counts[tag + dtag] = M
            worst = max(worst, err)
            total_c, per_img = eng.count_points(conf, thr, dyn=d)
            assert total_c == M and int(per_img.sum()) == M
            if d is not None and name != "mixed_32x48_24x40":
                assert int(per_img[-1]) == 0                     # the fully masked image contributes nothing
    assert counts["none"] == 0 and counts["none_dyn"] == 0
    assert counts["all"] == total
    assert 0.3 * total < counts["half"] < 0.7 * total
    assert 0 < counts["all_dyn"] < counts["all"]
    # the threshold is strict: a threshold equal to a confidence value drops exactly the pixels holding it
    v = float(np.sort(real)[len(real) // 3])
    got = eng.export_points(conf, v, with_index=True)
    assert got["index"].numel() == int((real > np.float32(v)).sum())
    record_margin(f"scene_{name}", xyz_err_over_max=worst, kept_half=counts["half"], pixels=total)
    assert worst <= BOUND, (name, worst)


@pytest.mark.parametrize("name", ["plain_36x44", "mono_37x41", "flow_sf_36x44"])
def test_export_reads_the_current_state_after_run(name):
    scene, dyn = _build(name)
    before = scene.engine.points().clone()
    scene.engine.run(20, 0.01)
    xyz = scene_points_np(scene)
    assert np.abs(xyz - before.cpu().numpy()).max() > 1e-3 * np.abs(xyz).max()           # the state did move
    conf, rgb = scene_inputs(scene)
    if name.startswith("flow"):
        got = scene.get_pointcloud(min_conf_thr=5.0, mask_dynamic=True, with_index=True)   # the scene's own dynamic masks
        d = stacked(scene.dynamic_masks, scene.imshapes, scene.max_area, bool)
        assert np.array_equal(d, dyn)
    else:
        got, d = scene.engine.export_points(conf, 5.0, dyn=dyn, rgb=rgb, with_index=True), dyn
    M, err = check_export(got, xyz, conf, 5.0, d, rgb, scene.imshapes)
    record_margin(f"scene_{name}_after_run20", xyz_err_over_max=err, kept=M)
    assert M > 0 and err <= BOUND, (name, err)


@pytest.mark.parametrize("name", ["plain_37x41", "plain_36x44", "mono_36x44"])
def test_overflowing_depths_are_dropped_by_the_finite_test(name):
    """A few log-depths (scale maps) at +100: exp overflows to inf in fp32, the pixel's point is not finite and is not exported."""
    scene, _ = _build(name)
    eng, P = scene.engine, scene.max_area
    depth = eng.params["depth"].clone()
    hot = [(0, 0), (0, 5), (1, 63), (1, 64), (1, 1023), (2, 1024), (2, P - 1)]
    for n, p in hot:
        depth[n, p] = 100.0
    eng.set_params(depth=depth, reset_optimizer=False)
    xyz = scene_points_np(scene)
    assert all(not np.isfinite(xyz[n, p]).all() for n, p in hot)
    conf, rgb = scene_inputs(scene)
    got = eng.export_points(conf, 0.0, rgb=rgb, with_index=True)
    M, err = check_export(got, xyz, conf, 0.0, None, rgb, scene.imshapes)
    assert M == scene.n_imgs * P - len(hot)
    assert not set(got["index"].cpu().tolist()) & {n * P + p for n, p in hot}
    assert torch.isfinite(got["xyz"]).all() and err <= BOUND


@pytest.mark.parametrize("name", ["plain_36x44", "plain_37x41"])
def test_capacity_and_sentinels_through_the_c_entry(name):
    """capacity = M + 64: the tail keeps its sentinel.  capacity = M - 1: an error with the needed count, and not one element of
    any output was written."""
    from align3r_amd._lib import check, ptr, stream_ptr
    scene, dyn = _build(name)
    eng, lib, dev = scene.engine, scene.engine.lib, scene.engine.device
    N, P = eng.N, eng.P
    conf_np, rgb_np = scene_inputs(scene)
    conf, rgb = torch.from_numpy(conf_np).to(dev), torch.from_numpy(rgb_np).to(dev)
    dyn_t = torch.from_numpy(dyn.astype(np.uint8)).to(dev)
    thr = float(np.median(conf_np))
    want = eng.export_points(conf, thr, dyn=dyn_t, rgb=rgb, with_index=True)
    M = want["xyz"].shape[0]
    assert M > 64
    ws = torch.empty(int(lib.a3r_align_scene_workspace_bytes(N, P)), dtype=torch.uint8, device=dev)
    counts, total = torch.empty(N, dtype=torch.int32, device=dev), C.c_longlong(-1)
    check(lib.a3r_align_scene_count(eng.handle, ptr(conf), thr, ptr(dyn_t), ptr(ws), ws.numel(), ptr(counts), C.byref(total), stream_ptr()))
    assert total.value == M and int(counts.sum()) == M
    assert np.array_equal(counts.cpu().numpy(), np.bincount(want["index"].cpu().numpy() // P, minlength=N))

    def buffers(cap):
        return (torch.full((cap, 3), -12345.5, device=dev), torch.full((cap, 3), 0xAB, dtype=torch.uint8, device=dev),
                torch.full((cap,), -7, dtype=torch.int32, device=dev))

    cap = M + 64
    xyz, col, idx = buffers(cap)
    n = C.c_longlong(-1)
    check(lib.a3r_align_scene_export(eng.handle, ptr(conf), thr, ptr(dyn_t), ptr(rgb), ptr(ws), ws.numel(), cap, ptr(xyz), ptr(col), ptr(idx),
                                     C.byref(n), stream_ptr()))
    torch.cuda.synchronize()
    assert n.value == M
    assert torch.equal(xyz[:M], want["xyz"]) and torch.equal(col[:M], want["rgb"]) and torch.equal(idx[:M], want["index"])
    assert (xyz[M:] == -12345.5).all() and (col[M:] == 0xAB).all() and (idx[M:] == -7).all()
    # optional outputs left out: xyz alone
    xyz2, _, _ = buffers(cap)
    check(lib.a3r_align_scene_export(eng.handle, ptr(conf), thr, ptr(dyn_t), None, ptr(ws), ws.numel(), cap, ptr(xyz2), None, None,
                                     C.byref(n), stream_ptr()))
    torch.cuda.synchronize()
    assert n.value == M and torch.equal(xyz2, xyz)
    # one point short
    xyz, col, idx = buffers(M - 1)
    n = C.c_longlong(-1)
    rc = lib.a3r_align_scene_export(eng.handle, ptr(conf), thr, ptr(dyn_t), ptr(rgb), ptr(ws), ws.numel(), M - 1, ptr(xyz), ptr(col), ptr(idx),
                                    C.byref(n), stream_ptr())
    torch.cuda.synchronize()
    assert rc != 0 and n.value == M
    msg = lib.a3r_last_error().decode()
    assert "capacity" in msg and str(M) in msg, msg
    assert (xyz == -12345.5).all() and (col == 0xAB).all() and (idx == -7).all()
    # a workspace that is too small is refused as well
    assert lib.a3r_align_scene_count(eng.handle, ptr(conf), thr, None, ptr(ws), 4, None, C.byref(total), stream_ptr()) != 0
    assert "workspace too small" in lib.a3r_last_error().decode()


@pytest.mark.parametrize("name", ["plain_2x3", "plain_37x41", "mono_36x44", "flow_sf_36x44", "mixed_32x48_24x40"])
def test_points_match_depth_to_pts3d(name):
    scene, _ = _build(name)
    got = scene.engine.points()
    ref = scene.depth_to_pts3d()
    assert got.shape == ref.shape == (scene.n_imgs, scene.max_area, 3)
    xyz = scene_points_np(scene)
    scale = np.abs(xyz).max()
    err_np = float(np.abs(got.cpu().numpy() - xyz).max() / scale)
    err_t = 0.0
    for n, (h, w) in enumerate(scene.imshapes):               # padding pixels: exact zeros here (the torch getter projects them too)
        assert (got[n, h * w:] == 0).all()
        err_t = max(err_t, float((got[n, :h * w] - ref[n, :h * w]).abs().max().item() / scale))
    record_margin(f"scene_points_{name}", vs_numpy=err_np, vs_depth_to_pts3d=err_t)
    assert err_np <= BOUND and err_t <= BOUND, (name, err_np, err_t)


def test_sharded_engine_exports_replica_0():
    """export_points / points of a ShardedAlignEngine(local_shards=2) against the restatement of that engine's own state."""
    from align3r_amd.aligner import ShardedAlignEngine
    N, H, W = 4, 36, 44
    prob = _problem(N, H, W, 11)
    eng = ShardedAlignEngine(*prob["args"], device="cuda:0", local_shards=2)
    eng.set_params(**prob["init"])
    eng.run(5, 0.01)
    host = lambda t: t.detach().cpu().numpy()
    par = eng.params
    focals = np.exp(host(par["im_focals"]) / np.float32(eng.focal_break)).astype(np.float32)
    pp = host(eng.pp0) + np.float32(10) * host(par["im_pp"])
    xyz = restate(np.exp(host(par["depth"])), focals, pp, ac._pose_rt(host(par["im_poses"])), [(H, W)] * N, H * W)
    rng = np.random.default_rng(2)
    conf = (1 + 9 * rng.random((N, H * W))).astype(np.float32)
    rgb = rng.integers(0, 256, (N, H * W, 3), dtype=np.uint8)
    dyn = prob["flow"]["dyn"].reshape(N, -1)
    got = eng.export_points(conf, 5.0, dyn=dyn, rgb=rgb, with_index=True)
    M, err = check_export(got, xyz, conf, 5.0, dyn, rgb, [(H, W)] * N)
    dense = float(np.abs(host(eng.points()) - xyz).max() / np.abs(xyz).max())
    record_margin("scene_sharded_k2_36x44", xyz_err_over_max=err, dense=dense, kept=M)
    assert M > 0 and err <= BOUND and dense <= BOUND


def test_get_pointcloud_is_get_masks_and_survives_clean_pointcloud(tmp_path):
    from align3r_amd.tool.pointcloud import read_ply
    scene, _ = make_scene("plain", 4, 36, 44)
    P = scene.max_area

    def masks_index():
        return torch.nonzero(torch.cat([m.flatten() for m in scene.get_masks()])).flatten().cpu().numpy()

    pc = scene.get_pointcloud(with_index=True)
    assert set(pc) == {"xyz", "rgb", "index"}
    first = masks_index()
    assert 0 < len(first) < scene.n_imgs * P and np.array_equal(pc["index"].cpu().numpy(), first)
    assert set(scene.get_pointcloud()) == {"xyz", "rgb"}
    # clean_pointcloud lowers confidences in place: the next export honours them
    scene.clean_pointcloud()
    pc2 = scene.get_pointcloud(with_index=True)
    second = masks_index()
    assert np.array_equal(pc2["index"].cpu().numpy(), second) and len(second) <= len(first)
    conf, rgb = scene_inputs(scene)
    M, err = check_export(pc2, scene_points_np(scene), conf, scene.min_conf_thr, None, rgb, scene.imshapes)
    assert err <= BOUND
    # the file holds exactly what get_pointcloud returns
    saved = scene.save_pointcloud(tmp_path / "scene.ply")
    xyz, col = read_ply(tmp_path / "scene.ply")
    assert xyz.tobytes() == saved["xyz"].cpu().numpy().tobytes() == pc2["xyz"].cpu().numpy().tobytes()
    assert np.array_equal(col, pc2["rgb"].cpu().numpy())
    with pytest.raises(RuntimeError, match="no dynamic masks"):
        scene.get_pointcloud(mask_dynamic=True)
    # a scene without frames has no colours
    scene.imgs = None
    assert set(scene.get_pointcloud()) == {"xyz"}


def test_hierarchical_driver_collects_every_clip(monkeypatch, tmp_path):
    """The synthetic clip of tests/test_gpu_hier.py through hierarchical_alignment with the collector on: one cloud per clip, in
    clip order, and the PLY of all of them holds the sum of the per-clip counts."""
    import align3r_amd.dust3r.inference as inf_mod
    from align3r_amd.tool import hierarchical as hz
    from align3r_amd.tool.pointcloud import read_ply, write_ply_parts
    from test_gpu_hier import _scene
    N, H, W = 8, 32, 48
    cams, world, f = _scene(N, H, W)
    rng = np.random.default_rng(0)
    frames = [torch.from_numpy(rng.uniform(-1, 1, (3, H, W)).astype(np.float32)) for _ in range(N)]

    def fake_inference(pairs, model, device, batch_size=1, verbose=False):
        gi = [int(a["instance"]) for a, b in pairs]
        gj = [int(b["instance"]) for a, b in pairs]
        p1 = np.stack([0.7 * ((world[i] - cams[i][1]) @ cams[i][0]) for i in gi]).astype(np.float32)
        p2 = np.stack([0.7 * ((world[j] - cams[i][1]) @ cams[i][0]) for i, j in zip(gi, gj)]).astype(np.float32)
        c = (2 + 8 * rng.random((len(pairs), H, W))).astype(np.float32)
        return dict(view1=dict(idx=[a["idx"] for a, b in pairs], img=[frames[i] for i in gi]),
                    view2=dict(idx=[b["idx"] for a, b in pairs], img=[frames[j] for j in gj]),
                    pred1=dict(pts3d=torch.from_numpy(p1), conf=torch.from_numpy(c)),
                    pred2=dict(pts3d_in_other_view=torch.from_numpy(p2), conf=torch.from_numpy(c.copy())))

    monkeypatch.setattr(inf_mod, "inference", fake_inference)
    imgs = [dict(idx=i, instance=str(i), true_shape=np.int32([[H, W]])) for i in range(N)]
    torch.manual_seed(0)
    clouds = []
    res = hz.hierarchical_alignment(imgs, None, "cuda", clip_size=3, niter=10, schedule="linear", lr=0.01, min_conf_thr=1.5,
                                    pointcloud_collector=clouds)
    assert res["keyframes_id"] == [0, 3, 6] and len(clouds) == 3
    # every confidence is clamped to 10 > 1.5 and every depth is finite: each clip exports all of its pixels
    assert [len(c["xyz"]) for c in clouds] == [3 * H * W, 3 * H * W, 2 * H * W]
    want = np.clip(np.rint(255 * (frames[3].permute(1, 2, 0).numpy() * 0.5 + 0.5).clip(0, 1)), 0, 255).astype(np.uint8)
    assert np.array_equal(clouds[1]["rgb"][:H * W], want.reshape(-1, 3))            # clip 1 starts with frame 3
    path = tmp_path / "scene.ply"
    assert write_ply_parts(path, [(c["xyz"], c["rgb"]) for c in clouds]) == N * H * W
    xyz, rgb = read_ply(path)
    assert len(xyz) == sum(len(c["xyz"]) for c in clouds) == N * H * W
    assert xyz.tobytes() == np.concatenate([c["xyz"] for c in clouds]).tobytes() and np.isfinite(xyz).all()
    assert np.array_equal(rgb, np.concatenate([c["rgb"] for c in clouds]))
