"""GPU: the renderer (csrc/render.hip) -- ops.render_points against render_ref(), the numpy restatement of tests/render_cases.py.

Every comparison is exact: depth bits, winner indices and colours.  The definition is integer arithmetic on keys after a float64
projection whose every operation is rounded on its own, on the device as in numpy (tests/test_render_cpu.py checks the restatement
itself and that the surface cases are no empty pictures).  The scene tests build small synthetic scenes as tests/test_gpu_scene.py
does and compare scene.render / scene.render_views with the restatement on the arrays of get_pointcloud().
"""
import numpy as np
import pytest
import torch

import render_cases as rc
from test_gpu_scene import make_mixed_scene, make_scene

pytestmark = pytest.mark.gpu


def _dev(a):
    return torch.from_numpy(np.array(a)).cuda()               # a copy: the shared cases are read-only


def _render(ref, H, W, radius, rgb=True, index=True, cams=None):
    from align3r_amd import ops
    return ops.render_points(_dev(ref["xyz"]), _dev(ref["rgb"]) if rgb else None, cams=ref["cams"] if cams is None else cams,
                             shape=(H, W), radius=radius, near=rc.NEAR, background=rc.BACKGROUND, want_index=index)


def _same(got, depth, index, out_rgb):
    assert got["depth"].dtype == torch.float32 and got["depth"].cpu().numpy().tobytes() == depth.tobytes()
    if index is not None:
        assert got["index"].dtype == torch.int32 and np.array_equal(got["index"].cpu().numpy(), index)
    if out_rgb is not None:
        assert got["rgb"].dtype == torch.uint8 and np.array_equal(got["rgb"].cpu().numpy(), out_rgb)


@pytest.mark.parametrize("case", rc.CASES, ids=rc.case_id)
def test_render_points_equals_the_restatement(case):
    kind, M, (H, W), Cn, radius = case
    ref = rc.ref_case(case)
    got = _render(ref, H, W, radius)
    assert set(got) == {"depth", "rgb", "index"} and got["depth"].shape == (Cn, H, W) and got["rgb"].shape == (Cn, H, W, 3)
    _same(got, ref["depth"], ref["index"], ref["out_rgb"])


REPEAT = [c for c in rc.CASES if c[1] == 70001 or (c[0] == "pile" and c[1] == 8193)]


@pytest.mark.parametrize("case", REPEAT, ids=rc.case_id)
def test_the_same_call_twice_gives_the_same_bytes_and_outputs_are_independent(case):
    kind, M, (H, W), Cn, radius = case
    ref = rc.ref_case(case)
    a, b = _render(ref, H, W, radius), _render(ref, H, W, radius)
    for k in ("depth", "rgb", "index"):
        assert torch.equal(a[k], b[k]), k
    # leaving out the colours and / or the index changes nothing else
    no_rgb = _render(ref, H, W, radius, rgb=False)
    assert set(no_rgb) == {"depth", "index"}
    _same(no_rgb, ref["depth"], ref["index"], None)
    no_idx = _render(ref, H, W, radius, index=False)
    assert set(no_idx) == {"depth", "rgb"}
    _same(no_idx, ref["depth"], None, ref["out_rgb"])
    bare = _render(ref, H, W, radius, rgb=False, index=False)
    assert set(bare) == {"depth"}
    _same(bare, ref["depth"], None, None)


@pytest.mark.parametrize("case", [c for c in rc.CASES if c[3] == 3 and c[1] in (65, 8193, 70001) and c[4] in (0, 3)], ids=rc.case_id)
def test_a_camera_batch_equals_the_cameras_one_by_one(case):
    kind, M, (H, W), Cn, radius = case
    ref = rc.ref_case(case)
    for c in range(Cn):
        one = _render(ref, H, W, radius, cams=ref["cams"][c:c + 1])
        _same(one, ref["depth"][c:c + 1], ref["index"][c:c + 1], ref["out_rgb"][c:c + 1])


@pytest.mark.parametrize("case", [c for c in rc.CASES if c[1] in (1000, 70001) and c[4] in (0, 1, 3)], ids=rc.case_id)
def test_every_form_of_the_splat_gives_the_same_pictures(case):
    """a3r_render_set_form: the camera loop or a camera grid axis; the keys read nine pixels at a time, one at a time or not at
    all."""
    from align3r_amd import ops
    kind, M, (H, W), Cn, radius = case
    ref = rc.ref_case(case)
    old = ops.render_set_form(-1)
    try:
        for form in range(6):
            ops.render_set_form(form)
            assert ops.render_set_form(-1) == form
            _same(_render(ref, H, W, radius), ref["depth"], ref["index"], ref["out_rgb"])
    finally:
        ops.render_set_form(old)


def test_an_empty_cloud_gives_empty_pictures():
    from align3r_amd import ops
    cams = rc.near_origin_cams(2, 5, 7, 1)
    xyz = torch.empty((0, 3), dtype=torch.float32, device="cuda")
    got = ops.render_points(xyz, torch.empty((0, 3), dtype=torch.uint8, device="cuda"), cams=cams, shape=(5, 7), radius=2, near=rc.NEAR,
                            background=(1, 2, 3), want_index=True)
    assert (got["depth"] == 0).all() and (got["index"] == -1).all() and got["depth"].shape == (2, 5, 7)
    assert (got["rgb"] == torch.tensor([1, 2, 3], dtype=torch.uint8, device="cuda")).all()
    got = ops.render_points(xyz, cams=cams, shape=(5, 7))
    assert set(got) == {"depth"} and (got["depth"] == 0).all()


def test_the_python_entry_refuses_bad_arguments():
    from align3r_amd import ops
    xyz = _dev(np.zeros((4, 3), np.float32))
    cams = rc.near_origin_cams(1, 4, 4, 1)
    with pytest.raises(RuntimeError, match="radius"):
        ops.render_points(xyz, cams=cams, shape=(4, 4), radius=9)
    with pytest.raises(RuntimeError, match="near_z"):
        ops.render_points(xyz, cams=cams, shape=(4, 4), near=0.0)
    with pytest.raises(RuntimeError, match="image size"):
        ops.render_points(xyz, cams=cams, shape=(0, 4))
    bad = cams.copy()
    bad[0, 12] = np.nan
    with pytest.raises(RuntimeError, match="camera 0"):
        ops.render_points(xyz, cams=bad, shape=(4, 4))
    with pytest.raises(RuntimeError, match="rgb"):
        ops.render_points(xyz, torch.zeros((4, 3), dtype=torch.uint8), cams=cams, shape=(4, 4))           # colours on the host
    K = np.eye(3)[None].copy()
    K[0, 0, 1] = 0.5
    with pytest.raises(ValueError, match="skew"):
        ops.render_points(xyz, w2c=np.eye(4)[None], K=K, shape=(4, 4))
    with pytest.raises(ValueError, match="background"):
        ops.render_points(xyz, cams=cams, shape=(4, 4), background=(0, 0, 256))
    # w2c / K as the signature takes them: the same picture as through the table
    K = np.array([[[8.0, 0, 2], [0, 8, 2], [0, 0, 1]]])
    ray = xyz + torch.tensor([0.0, 0.0, 1.0], device="cuda")          # four points on the optical axis: one pixel, index 0 wins
    a = ops.render_points(ray, w2c=np.eye(4)[None], K=K, shape=(4, 4), want_index=True)
    b = ops.render_points(ray, cams=ops.render_cameras(torch.eye(4, dtype=torch.float64)[None, :3], torch.from_numpy(K)), shape=(4, 4), want_index=True)
    assert torch.equal(a["depth"], b["depth"]) and torch.equal(a["index"], b["index"])
    assert int((a["index"] >= 0).sum()) == 1 and int(a["index"][0, 2, 2]) == 0 and float(a["depth"][0, 2, 2]) == 1.0


# ------------------------------------------------------------------------------------------------- scenes
def _look_cams(scene, n, seed):
    """n cameras near the scene's own ones: the poses of images 0 .. n-1 nudged, float64 [n,4,4], and their intrinsics [n,3,3] with
    the focals shortened unequally (fx != fy) and the principal point off the pixel grid."""
    g = np.random.default_rng(seed)
    poses = scene.get_im_poses().detach().cpu().numpy().astype(np.float64)[:n].copy()
    poses[:, :3, 3] += 0.02 * g.standard_normal((n, 3))
    K = scene.get_intrinsics().detach().cpu().numpy().astype(np.float64)[:n].copy()
    K[:, 0, 0] *= 0.9
    K[:, 1, 1] *= 0.8
    K[:, :2, 2] += (4.3, 1.8)                                       # towards the centre of the larger picture
    return poses, K


@pytest.mark.parametrize("kind, radius", [("plain", 0), ("plain", 2), ("flow", 1)])
def test_scene_render_equals_the_restatement_on_get_pointcloud(kind, radius):
    from align3r_amd.tool.render import world_to_camera
    scene, _ = make_scene(kind, 4, 36, 44)
    dynamic = kind == "flow"
    pc = scene.get_pointcloud(mask_dynamic=dynamic)
    M = pc["xyz"].shape[0]
    assert 0 < M < scene.n_imgs * scene.max_area
    poses, K = _look_cams(scene, 3, 4)
    H, W = 40, 52                                                   # not the images' own shape
    bg = (9, 8, 7)
    got = scene.render(poses, K, (H, W), mask_dynamic=dynamic, radius=radius, background=bg, with_index=True)
    cams = rc.make_cams(world_to_camera(poses), K[:, 0, 0], K[:, 1, 1], K[:, 0, 2], K[:, 1, 2])
    depth, index, out_rgb = rc.render_ref(pc["xyz"].cpu().numpy(), pc["rgb"].cpu().numpy(), cams, H, W, radius, 1e-6, bg)
    assert (index >= 0).sum() > H * W // 8 and (index < 0).any()    # a picture, not a blank
    _same(got, depth, index, out_rgb)
    assert set(scene.render(poses, K, (H, W))) == {"depth", "rgb"}
    # another threshold is another cloud
    pc5 = scene.get_pointcloud(min_conf_thr=5.0, mask_dynamic=dynamic)
    assert 0 < pc5["xyz"].shape[0] < M
    got5 = scene.render(poses[:1], K[:1], (H, W), min_conf_thr=5.0, mask_dynamic=dynamic, radius=radius, background=bg, with_index=True)
    d5, i5, c5 = rc.render_ref(pc5["xyz"].cpu().numpy(), pc5["rgb"].cpu().numpy(), cams[:1], H, W, radius, 1e-6, bg)
    _same(got5, d5, i5, c5)


def test_render_views_shows_every_kept_pixel_of_an_image_at_its_own_place(tmp_path):
    """scene.render_views of image i, restricted to image i's own kept points at radius 0: `index` holds at each kept pixel that
    pixel's rank among the image's kept pixels, -1 elsewhere, and the depth is get_depthmaps()[i] within 1e-4 relative.

    The bound: the engine forms a world point in fp32 from its fp32 pose, the renderer takes that point back into the camera in
    float64 -- about ten fp32 roundings of 6e-8, each relative to |world| <= z (1 + |t| / z); this scene has |t| <= z, so the
    difference stays near 1e-6 z and the bound has a tenfold margin and more."""
    scene, _ = make_mixed_scene()
    P, N = scene.max_area, scene.n_imgs
    thr = float(torch.cat([c.flatten() for c in scene.im_conf]).median())          # about half of every image is kept
    pc = scene.get_pointcloud(min_conf_thr=thr, with_index=True)
    depthmaps = scene.get_depthmaps()
    t = scene.get_im_poses()[:, :3, 3].norm(dim=1)
    assert all(float(t[i]) <= float(depthmaps[i].min()) for i in range(N))          # the premise of the bound
    worst = 0.0
    for i in range(N):
        h, w = scene.imshapes[i]
        own = pc["index"][(pc["index"] >= i * P) & (pc["index"] < (i + 1) * P)].cpu().numpy() - i * P       # ascending: row-major
        assert 0 < len(own) < h * w
        want = np.full(h * w, -1, np.int64)
        want[own] = np.arange(len(own))
        view, = scene.render_views(i, min_conf_thr=thr, radius=0, with_index=True, points_of=[i])
        assert view["index"].shape == (h, w) and view["rgb"].shape == (h, w, 3)
        assert np.array_equal(view["index"].cpu().numpy().reshape(-1), want)
        own_t = torch.from_numpy(own).cuda()
        d, ref = view["depth"].reshape(-1)[own_t].double(), depthmaps[i].reshape(-1)[own_t].double()
        err = float(((d - ref).abs() / ref).max())
        print(f"render_views image {i}: kept {len(own)} of {h * w}, max relative depth difference {err:.3e}")
        worst = max(worst, err)
        assert err <= 1e-4, (i, err)
        assert (view["depth"].reshape(-1)[torch.from_numpy(want < 0).cuda()] == 0).all()
    # every view of the whole scene in one go: two shapes, two calls underneath, each image at its own shape; the kept pixels of
    # an image are covered in its own view (by their own point or by a nearer one)
    views = scene.render_views(min_conf_thr=thr, radius=1, with_index=True)
    assert [tuple(v["depth"].shape) for v in views] == [tuple(s) for s in scene.imshapes]
    one_by_one = [scene.render_views([i], min_conf_thr=thr, radius=1, with_index=True)[0] for i in (3, 0)]
    for v, i in zip(one_by_one, (3, 0)):
        assert all(torch.equal(v[k], views[i][k]) for k in ("depth", "rgb", "index"))
    both = scene.render_views([3, 0], min_conf_thr=thr, radius=1, with_index=True)
    assert all(torch.equal(both[s][k], views[i][k]) for s, i in enumerate((3, 0)) for k in ("depth", "rgb", "index"))
    for i, v in enumerate(views):
        own = pc["index"][(pc["index"] >= i * P) & (pc["index"] < (i + 1) * P)].long() - i * P
        assert (v["index"].reshape(-1)[own] >= 0).all()
    with pytest.raises(IndexError):
        scene.render_views([N])
    # files: render_XXXX.png holds the view's colours
    import PIL.Image
    saved = scene.save_renders(str(tmp_path / "pics"), idx=[1, 2], min_conf_thr=thr, radius=1)
    for v, i in zip(saved, (1, 2)):
        assert np.array_equal(np.asarray(PIL.Image.open(tmp_path / "pics" / f"render_{i:04d}.png")), views[i]["rgb"].cpu().numpy())
        assert torch.equal(v["rgb"], views[i]["rgb"])


@pytest.mark.parametrize("mode", ["--hierarchical", "--flow-hierarchical"])
def test_run_clip_refuses_render_with_the_hierarchical_modes(mode, capsys):
    from align3r_amd.tool.run_clip import parse
    base = ["--images", "frames", "--weights", "w.pth", "--out", "out", "--render", "r"]
    with pytest.raises(SystemExit):
        parse(base + [mode])
    assert "--render cannot be combined" in capsys.readouterr().err
    assert parse(base + ["--flow"]).render == "r"
