"""GPU: TSDF fusion (csrc/tsdf.hip) against the numpy restatement of tests/tsdf_cases.py -- in bytes, no tolerance: sequential
float64 sums in frame order, no fused products, integer compaction -- at the level of ops.tsdf_* and through the scene methods."""
import ctypes as C

import numpy as np
import pytest
import torch

import tsdf_cases as tc
from test_gpu_scene import make_mixed_scene, make_scene

pytestmark = pytest.mark.gpu


def _dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _integrate(c, **kw):
    from align3r_amd import ops
    return ops.tsdf_integrate(_dev(c["depth"]), _dev(c["weight"]), _dev(c["rgb"]), c["cams"], c["origin"], c["dims"], c["voxel"], c["trunc"],
                              near=c["near"], max_depth=c["max_depth"], **kw)


def _same_grid(got, c):
    tsdf, wsum, rgb = got
    nx, ny, nz = c["dims"]
    assert tsdf.shape == (nz, ny, nx) and tsdf.dtype == torch.float32 and wsum.shape == (nz, ny, nx)
    assert wsum.cpu().numpy().tobytes() == c["wsum"].tobytes()
    assert tsdf.cpu().numpy().tobytes() == c["tsdf"].tobytes()
    if c["rgb"] is None:
        assert rgb is None
    else:
        assert rgb.shape == (nz, ny, nx, 3) and np.array_equal(rgb.cpu().numpy(), c["out_rgb"])


def _same_mesh(got, c):
    xyz, rgb, faces = got
    assert xyz.dtype == torch.float32 and faces.dtype == torch.int32
    assert xyz.shape == c["xyz"].shape and faces.shape == c["faces"].shape
    assert xyz.cpu().numpy().tobytes() == c["xyz"].tobytes()
    assert np.array_equal(faces.cpu().numpy(), c["faces"])
    if c["mesh_rgb"] is None:
        assert rgb is None
    else:
        assert np.array_equal(rgb.cpu().numpy(), c["mesh_rgb"])


@pytest.mark.parametrize("name", tc.CASES)
def test_integrate_and_mesh_equal_the_restatement(name):
    from align3r_amd import ops
    c = tc.ref(name)
    got = _integrate(c)
    _same_grid(got, c)
    # the surface of the device's own grid, and of the restatement's grid
    _same_mesh(ops.tsdf_mesh(got[0], got[1], got[2], c["origin"], c["voxel"], c["min_weight"]), c)
    _same_mesh(ops.tsdf_mesh(_dev(c["tsdf"]), _dev(c["wsum"]), _dev(c["out_rgb"]), c["origin"], c["voxel"], c["min_weight"]), c)
    if c["rgb"] is not None:                # leaving the colours out changes nothing else
        plain = ops.tsdf_mesh(got[0], got[1], None, c["origin"], c["voxel"], c["min_weight"])
        assert plain[1] is None and plain[0].cpu().numpy().tobytes() == c["xyz"].tobytes() and np.array_equal(plain[2].cpu().numpy(), c["faces"])


@pytest.mark.parametrize("name", ["gates-13x9x7", "frames-260", "sphere-noisy", "ragged-70x65x40"])
def test_the_same_call_twice_and_every_form_give_the_same_bytes(name):
    from align3r_amd import ops
    c = tc.ref(name)
    stats = torch.zeros(2, dtype=torch.int64, device="cuda")
    old = ops.tsdf_set_form(0)
    try:
        first = _integrate(c, skip_stats=stats)
        _same_grid(first, c)
        _same_grid(_integrate(c), c)
        tested, skipped = (int(v) for v in stats.cpu())
        nx, ny, nz = c["dims"]
        bricks = -(-nx // 32) * -(-ny // 8) * nz
        assert tested == bricks * len(c["cams"]) and 0 <= skipped <= tested
        if name in ("gates-13x9x7", "ragged-70x65x40"):
            assert skipped > 0                          # the test does skip here, and the bytes above did not notice
        assert ops.tsdf_set_form(1) == 0
        _same_grid(_integrate(c), c)
        assert ops.tsdf_set_form(7) == 1 and ops.tsdf_set_form(-1) == 1         # values outside [0, 1] only query
    finally:
        ops.tsdf_set_form(old)
    m1 = ops.tsdf_mesh(first[0], first[1], first[2], c["origin"], c["voxel"], c["min_weight"])
    m2 = ops.tsdf_mesh(first[0], first[1], first[2], c["origin"], c["voxel"], c["min_weight"])
    assert all(torch.equal(a, b) for a, b in zip(m1, m2))
    _same_mesh(m1, c)


def test_a_batch_of_frames_is_summed_in_frame_order():
    """The restatement adds frame after frame; the kernel must do the same, whatever its brick test leaves out.  The frames one by
    one, summed on the host in float64 in the same order, give the same W."""
    c = tc.ref("sphere-noisy")
    _same_grid(_integrate(c), c)
    N = len(c["cams"])
    W = np.zeros(c["wsum"].shape)
    for n in range(N):
        one = dict(c, depth=c["depth"][n:n + 1], weight=c["weight"][n:n + 1], rgb=c["rgb"][n:n + 1], cams=c["cams"][n:n + 1])
        _, wsum, _ = _integrate(one)
        W = W + wsum.cpu().numpy().astype(np.float64)       # each frame's weights are fp32 values: the per-frame sum is exact
    assert W.astype(np.float32).tobytes() == c["wsum"].tobytes()
    assert (c["wsum"] > 4).any()                            # voxels seen by several frames


def test_no_frames_and_no_surface():
    from align3r_amd import ops
    z = lambda *s, dt=torch.float32: torch.zeros(s, dtype=dt, device="cuda")
    tsdf, wsum, rgb = ops.tsdf_integrate(z(0, 24), z(0, 24), z(0, 24, 3, dt=torch.uint8), np.zeros((0, 17)), (0, 0, 0), (5, 4, 3), 0.1, 0.3)
    assert (tsdf == 1).all() and (wsum == 0).all() and (rgb == 0).all() and tsdf.shape == (3, 4, 5)
    xyz, colours, faces = ops.tsdf_mesh(tsdf, wsum, rgb, (0, 0, 0), 0.1, 1.0)
    assert xyz.shape == (0, 3) and colours.shape == (0, 3) and faces.shape == (0, 3)


def _lib_einval():
    return -1                      # A3R_EINVAL of include/a3r.h


def test_capacity_and_sentinels_through_the_c_entry():
    from align3r_amd import _lib
    from align3r_amd._lib import ptr, stream_ptr
    lib = _lib.load()
    c = tc.ref("ragged-70x65x40")
    nx, ny, nz = c["dims"]
    V, F = len(c["xyz"]), len(c["faces"])
    tsdf, wsum, rgb = _dev(c["tsdf"]), _dev(c["wsum"]), _dev(c["out_rgb"])
    origin = np.asarray(c["origin"], np.float64)
    ws_bytes = int(lib.a3r_tsdf_mesh_workspace_bytes(nx, ny, nz))
    assert ws_bytes >= 4 * nx * ny * nz
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device="cuda")
    nv, nf = C.c_longlong(0), C.c_longlong(0)
    _lib.check(lib.a3r_tsdf_mesh_count(ptr(tsdf), ptr(wsum), nx, ny, nz, c["min_weight"], ptr(ws), ws_bytes, C.byref(nv), C.byref(nf),
                                       stream_ptr()))
    assert (nv.value, nf.value) == (V, F)

    def export(cap_v, cap_f):
        bufs = (torch.full((cap_v, 3), -7.0, device="cuda"), torch.full((cap_v, 3), 201, dtype=torch.uint8, device="cuda"),
                torch.full((cap_f, 3), -5, dtype=torch.int32, device="cuda"))
        nv.value = nf.value = -1
        rc = lib.a3r_tsdf_mesh_export(ptr(tsdf), ptr(wsum), ptr(rgb), nx, ny, nz, origin.ctypes.data, c["voxel"], c["min_weight"], ptr(ws),
                                      ws_bytes, cap_v, cap_f, ptr(bufs[0]), ptr(bufs[1]), ptr(bufs[2]), C.byref(nv), C.byref(nf), stream_ptr())
        torch.cuda.synchronize()
        return rc, [b.cpu().numpy() for b in bufs]
    rc, (xyz, col, faces) = export(V + 64, F + 64)
    assert rc == 0 and (nv.value, nf.value) == (V, F)
    assert xyz[:V].tobytes() == c["xyz"].tobytes() and np.array_equal(col[:V], c["mesh_rgb"]) and np.array_equal(faces[:F], c["faces"])
    assert (xyz[V:] == -7.0).all() and (col[V:] == 201).all() and (faces[F:] == -5).all()
    for cap_v, cap_f in ((V - 1, F), (V, F - 1)):
        rc, (xyz, col, faces) = export(cap_v, cap_f)
        assert rc == _lib_einval() and (nv.value, nf.value) == (V, F)
        msg = lib.a3r_last_error().decode()
        assert str(V) in msg and str(F) in msg and "capacit" in msg
        assert (xyz == -7.0).all() and (col == 201).all() and (faces == -5).all()
    assert lib.a3r_tsdf_mesh_count(ptr(tsdf), ptr(wsum), nx, ny, nz, c["min_weight"], ptr(ws), 1024, C.byref(nv), C.byref(nf),
                                   stream_ptr()) == _lib_einval()
    assert "workspace too small" in lib.a3r_last_error().decode()
    # the entry itself refuses what ops refuses, naming the field
    cams = np.ascontiguousarray(tc.build("plane")["cams"])
    p = tc.build("plane")
    d, w = _dev(p["depth"]), _dev(p["weight"])
    cams_dev = torch.from_numpy(cams.reshape(-1).copy()).cuda()
    out = torch.empty(8 * 8 * 8, device="cuda")
    o3 = np.zeros(3)

    def integrate(N=1, P=768, dims=(8, 8, 8), voxel=0.1, trunc=0.3, near=1e-6):
        return lib.a3r_tsdf_integrate(ptr(d), ptr(w), None, ptr(cams_dev), cams.ctypes.data, N, P, o3.ctypes.data, voxel, *dims, trunc, near,
                                      float("inf"), ptr(out), ptr(out), None, None, stream_ptr())
    for kw, word in ((dict(dims=(2048, 1024, 1024)), "dims"), (dict(voxel=0.0), "voxel"), (dict(trunc=0.0), "trunc"), (dict(near=-1.0), "near"),
                     (dict(N=3, P=1 << 30), "N * P"), (dict(P=767), "h * w")):
        assert integrate(**kw) == _lib_einval()
        assert word in lib.a3r_last_error().decode(), (kw, lib.a3r_last_error())


# ------------------------------------------------------------------------------------------------- scenes
def _scene_inputs(scene, min_conf_thr=None, mask_dynamic=False, weight="conf"):
    """The arrays get_tsdf hands down, rebuilt from the scene's own getters: depth and weight [N,P], rgb [N,P,3], cams."""
    from align3r_amd import ops
    from align3r_amd.tool.render import world_to_camera
    host = lambda t: t.detach().cpu().numpy()
    P, N = scene.max_area, scene.n_imgs
    depth = host(scene.get_depthmaps(raw=True)).astype(np.float32)
    pc = scene.get_pointcloud(min_conf_thr=min_conf_thr, mask_dynamic=mask_dynamic, with_index=True)
    keep = np.zeros(N * P, bool)
    keep[host(pc["index"])] = True
    conf = np.zeros((N, P), np.float32)
    for n, cm in enumerate(scene._mask_confidences()):
        conf[n, :cm.numel()] = host(cm).reshape(-1)
    wt = np.where(keep.reshape(N, P), conf if weight == "conf" else np.float32(1), np.float32(0)).astype(np.float32)
    rgb = np.zeros((N, P, 3), np.uint8)
    for n, im in enumerate(scene.imgs):
        u8 = np.clip(np.rint(255.0 * np.asarray(im)), 0, 255).astype(np.uint8).reshape(-1, 3)
        rgb[n, :len(u8)] = u8
    K = np.zeros((N, 3, 3))
    K[:, 0, 0] = K[:, 1, 1] = host(scene.get_focals()).astype(np.float64).reshape(-1)
    K[:, :2, 2] = host(scene.get_principal_points()).astype(np.float64)
    K[:, 2, 2] = 1
    cams = ops.tsdf_cameras(world_to_camera(host(scene.get_im_poses()).astype(np.float64)), K, [tuple(s) for s in scene.imshapes])
    return depth, wt, rgb, cams, host(pc["xyz"])


def _voxel_for(scene, cells=24):
    xyz = scene.get_pointcloud()["xyz"]
    return float((xyz.max(0).values - xyz.min(0).values).max()) / cells


@pytest.mark.parametrize("kind", ["plain", "flow", "mixed"])
def test_scene_tsdf_and_fused_mesh_equal_the_restatement(kind, tmp_path):
    from align3r_amd.tool.pointcloud import read_ply_mesh
    scene = make_mixed_scene()[0] if kind == "mixed" else make_scene(kind, 4, 36, 44)[0]
    dynamic = kind == "flow"
    v = _voxel_for(scene)
    depth, wt, rgb, cams, pts = _scene_inputs(scene, mask_dynamic=dynamic)
    assert (wt > 0).any() and (wt == 0).any()
    tsdf, wsum, colours, origin, voxel, dims = scene.get_tsdf(v, mask_dynamic=dynamic)
    # the box: the kept points padded by trunc, on the host in float64
    trunc = 3 * v
    lo = np.floor((pts.astype(np.float64).min(0) - trunc) / v)
    hi = np.floor((pts.astype(np.float64).max(0) + trunc) / v) + 1
    assert voxel == v and tuple(dims) == tuple(int(n) for n in hi - lo) and np.array_equal(np.asarray(origin), lo * v)
    want = tc.tsdf_ref(depth, wt, rgb, cams, origin, dims, v, trunc)
    assert tsdf.cpu().numpy().tobytes() == want[0].tobytes() and wsum.cpu().numpy().tobytes() == want[1].tobytes()
    assert np.array_equal(colours.cpu().numpy(), want[2])
    assert (want[1] > 0).any()
    # the mesh; min_weight defaults to the smallest positive weight the scene assigns
    min_weight = float(wt[wt > 0].min())
    mesh = scene.get_fused_mesh(v, mask_dynamic=dynamic)
    mx, mc, mf = tc.mesh_ref(want[0], want[1], want[2], origin, v, min_weight)
    assert len(mx) > 0 and len(mf) > 0
    assert mesh["xyz"].cpu().numpy().tobytes() == mx.tobytes() and np.array_equal(mesh["faces"].cpu().numpy(), mf)
    assert np.array_equal(mesh["rgb"].cpu().numpy(), mc)
    # other arguments reach the weights
    d5, w5, r5, _, pts5 = _scene_inputs(scene, min_conf_thr=5.0, mask_dynamic=dynamic, weight="uniform")
    assert 0 < (w5 > 0).sum() < (wt > 0).sum() and set(np.unique(w5)) == {0.0, 1.0}
    got5 = scene.get_tsdf(v, trunc=2.5 * v, min_conf_thr=5.0, mask_dynamic=dynamic, weight="uniform", bounds=(origin, dims), max_depth=1e3)
    want5 = tc.tsdf_ref(d5, w5, r5, cams, origin, dims, v, 2.5 * v, max_depth=1e3)
    assert got5[0].cpu().numpy().tobytes() == want5[0].tobytes() and got5[1].cpu().numpy().tobytes() == want5[1].tobytes()
    assert got5[1].cpu().numpy().tobytes() != want[1].tobytes()
    if dynamic:                                 # the masks reach the weights
        d_all, w_all, _, _, _ = _scene_inputs(scene, mask_dynamic=False)
        assert (w_all > 0).sum() > (wt > 0).sum()
        got_all = scene.get_tsdf(v, bounds=(origin, dims))
        want_all = tc.tsdf_ref(d_all, w_all, rgb, cams, origin, dims, v, trunc)
        assert got_all[1].cpu().numpy().tobytes() == want_all[1].tobytes() != want[1].tobytes()
    # limits and files
    with pytest.raises(ValueError, match=r"bounds=.*max_depth=.*voxel"):
        scene.get_tsdf(v, mask_dynamic=dynamic, max_voxels=int(np.prod(dims)) - 1)
    with pytest.raises(ValueError, match="weight"):
        scene.get_tsdf(v, weight="best")
    saved = scene.save_fused_mesh(str(tmp_path / "fused.ply"), v, mask_dynamic=dynamic)
    b_xyz, b_faces, b_rgb, b_face_rgb = read_ply_mesh(str(tmp_path / "fused.ply"))
    assert b_xyz.tobytes() == mx.tobytes() and np.array_equal(b_faces, mf) and np.array_equal(b_rgb, mc) and b_face_rgb is None
    assert torch.equal(saved["xyz"], mesh["xyz"])


def test_the_other_optimizers_inherit_the_methods():
    from align3r_amd.dust3r.cloud_opt.modular_optimizer import ModularPointCloudOptimizer
    from align3r_amd.dust3r.cloud_opt.optimizer import PointCloudOptimizer
    from align3r_amd.dust3r.cloud_opt_flow.optimizer import PointCloudOptimizer as FlowOptimizer
    for cls in (ModularPointCloudOptimizer, FlowOptimizer):
        for name in ("get_tsdf", "get_fused_mesh", "save_fused_mesh"):
            assert getattr(cls, name) is getattr(PointCloudOptimizer, name)


def test_run_clip_fused_mesh_switch(capsys):
    from align3r_amd.tool.run_clip import parse
    base = ["--images", "frames", "--weights", "w.pth", "--out", "out"]
    a = parse(base + ["--fused-mesh", "m.ply", "--fused-voxel", "0.05", "--fused-trunc", "0.2", "--fused-max-depth", "9"])
    assert (a.fused_mesh, a.fused_voxel, a.fused_trunc, a.fused_max_depth) == ("m.ply", 0.05, 0.2, 9.0)
    for extra, word in ((["--fused-mesh", "m.ply"], "--fused-voxel"), (["--fused-voxel", "0.1"], "--fused-mesh"),
                        (["--fused-mesh", "m.ply", "--fused-voxel", "0"], "--fused-voxel"),
                        (["--fused-mesh", "m.ply", "--fused-voxel", "0.1", "--hierarchical"], "--fused-mesh cannot be combined"),
                        (["--fused-mesh", "m.ply", "--fused-voxel", "0.1", "--flow-hierarchical"], "--fused-mesh cannot be combined")):
        with pytest.raises(SystemExit):
            parse(base + extra)
        assert word in capsys.readouterr().err


def test_run_clip_writes_a_fused_mesh(tmp_path):
    """The driver's own step on a scene: the file it writes holds get_fused_mesh's arrays, and the result names the counts."""
    from align3r_amd.tool.pointcloud import read_ply_mesh
    from align3r_amd.tool.run_clip import parse, write_fused_mesh
    scene, _ = make_scene("flow", 4, 36, 44)
    v = _voxel_for(scene)
    path = str(tmp_path / "fused.ply")
    a = parse(["--images", "frames", "--weights", "w.pth", "--out", str(tmp_path), "--flow", "--fused-mesh", path, "--fused-voxel", repr(v)])
    n_vertices, n_faces = write_fused_mesh(scene, a)
    want = scene.get_fused_mesh(v, mask_dynamic=True)                       # --flow: the dynamic pixels are masked out
    b_xyz, b_faces, _, _ = read_ply_mesh(path)
    assert (n_vertices, n_faces) == (len(b_xyz), len(b_faces)) == (want["xyz"].shape[0], want["faces"].shape[0])
    assert n_vertices > 0 and n_faces > 0
    assert b_xyz.tobytes() == want["xyz"].cpu().numpy().tobytes() and np.array_equal(b_faces, want["faces"].cpu().numpy())
    other = scene.get_fused_mesh(v, mask_dynamic=False)
    assert other["xyz"].shape != want["xyz"].shape or not torch.equal(other["xyz"], want["xyz"])
