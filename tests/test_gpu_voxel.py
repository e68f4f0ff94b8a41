"""GPU: voxel-grid downsampling (csrc/voxel.hip) -- ops.voxel_downsample against voxel_ref(), the numpy restatement of
tests/voxel_cases.py, and scene.get_pointcloud(voxel_size=...) against the restatement on the arrays of get_pointcloud().

Every comparison is exact: winner rows, counts, the bytes of the coordinates and the colours.  The definition is integer arithmetic
on keys, values and sums after float64 quotients whose every operation is rounded on its own, on the device as in numpy
(tests/test_voxel_cpu.py checks the restatement itself and that the cases are what they claim).
"""
import ctypes as C

import numpy as np
import pytest
import torch

import voxel_cases as vc
from test_gpu_scene import make_mixed_scene, make_scene

pytestmark = pytest.mark.gpu


def _dev(a):
    return torch.from_numpy(np.array(a)).cuda()               # a copy: the shared cases are read-only


def _run(xyz, voxel, priority=None, rgb=None, **kw):
    from align3r_amd import ops
    return ops.voxel_downsample(_dev(xyz), voxel, priority=None if priority is None else _dev(priority),
                                rgb=None if rgb is None else _dev(rgb), **kw)


def _same(got, ref, rgb=True):
    V = len(ref["index"])
    assert got["dropped"] == ref["dropped"] and isinstance(got["dropped"], int)
    assert got["index"].dtype == torch.int32 and got["index"].shape == (V,) and np.array_equal(got["index"].cpu().numpy(), ref["index"])
    assert got["count"].dtype == torch.int32 and got["count"].shape == (V,) and np.array_equal(got["count"].cpu().numpy(), ref["count"])
    assert got["xyz"].dtype == torch.float32 and got["xyz"].shape == (V, 3) and got["xyz"].cpu().numpy().tobytes() == ref["xyz"].tobytes()
    if rgb:
        assert got["rgb"].dtype == torch.uint8 and got["rgb"].shape == (V, 3) and np.array_equal(got["rgb"].cpu().numpy(), ref["rgb"])
    else:
        assert "rgb" not in got


@pytest.mark.parametrize("reduce", ["best", "mean"])
@pytest.mark.parametrize("case", vc.CASES, ids=vc.case_id)
def test_voxel_downsample_equals_the_restatement(case, reduce):
    ref = vc.ref_case(case)
    got = _run(ref["xyz"], ref["voxel"], ref["priority"], ref["rgb"], reduce=reduce)
    assert set(got) == {"xyz", "rgb", "index", "count", "dropped"}
    _same(got, ref[reduce])


REPEAT = [c for c in vc.CASES if c[1] >= 70001 or (c[0] in ("pile", "edges_rep", "nan_prio") and c[1] in (31, 8193, 8198))]


@pytest.mark.parametrize("reduce", ["best", "mean"])
@pytest.mark.parametrize("case", REPEAT, ids=vc.case_id)
def test_the_same_call_twice_gives_the_same_bytes_and_outputs_are_independent(case, reduce):
    ref = vc.ref_case(case)
    a = _run(ref["xyz"], ref["voxel"], ref["priority"], ref["rgb"], reduce=reduce)
    b = _run(ref["xyz"], ref["voxel"], ref["priority"], ref["rgb"], reduce=reduce)
    for k in ("xyz", "rgb", "index", "count"):
        assert torch.equal(a[k], b[k]) and a[k].cpu().numpy().tobytes() == b[k].cpu().numpy().tobytes(), k
    # leaving out the colours changes nothing else
    _same(_run(ref["xyz"], ref["voxel"], ref["priority"], None, reduce=reduce), ref[reduce], rgb=False)
    # leaving out the priorities changes the winners and nothing else: counts and, in mean mode, positions and colours stay
    bare = _run(ref["xyz"], ref["voxel"], None, ref["rgb"], reduce=reduce)
    _same(bare, vc.voxel_ref(ref["xyz"], ref["voxel"], None, ref["rgb"], reduce))
    if reduce == "mean":
        assert sorted(map(bytes, a["xyz"].cpu().numpy())) == sorted(map(bytes, bare["xyz"].cpu().numpy()))


@pytest.mark.parametrize("kind, M, slots", [("surface", 8193, 16384), ("spread", 8191, 8192)])
def test_a_tight_table_gives_the_same_result(kind, M, slots):
    """slots = the smallest power of two above M; the spread case fills all slots but one, so probe chains cross the whole table."""
    xyz, voxel, priority, rgb = vc.cloud(kind, M, 1)
    for reduce in ("best", "mean"):
        ref = vc.voxel_ref(xyz, voxel, priority, rgb, reduce)
        tight = _run(xyz, voxel, priority, rgb, reduce=reduce, slots=slots)
        _same(tight, ref)
        _same(_run(xyz, voxel, priority, rgb, reduce=reduce), ref)
        _same(_run(xyz, voxel, priority, rgb, reduce=reduce, slots=4 * slots), ref)
    if kind == "spread":
        assert len(ref["index"]) == M == slots - 1


def test_the_result_does_not_depend_on_the_order_of_the_rows():
    xyz, voxel, _, rgb = vc.cloud("surface", 8193, 1)
    g = np.random.default_rng(11)
    priority = g.permutation(len(xyz)).astype(np.float32)          # distinct
    perm = g.permutation(len(xyz))
    for reduce in ("best", "mean"):
        a = _run(xyz, voxel, priority, rgb, reduce=reduce)
        b = _run(xyz[perm], voxel, priority[perm], rgb[perm], reduce=reduce)
        host = lambda d, k: d[k].cpu().numpy()
        pairs_a = sorted(zip(host(a, "index").tolist(), host(a, "count").tolist()))
        pairs_b = sorted(zip(perm[host(b, "index")].tolist(), host(b, "count").tolist()))
        assert pairs_a == pairs_b and len(pairs_a) > 1000
        # the rows themselves, matched by original winner row
        oa, ob = np.argsort(host(a, "index")), np.argsort(perm[host(b, "index")])
        assert host(a, "xyz")[oa].tobytes() == host(b, "xyz")[ob].tobytes() and np.array_equal(host(a, "rgb")[oa], host(b, "rgb")[ob])


@pytest.mark.parametrize("reduce", ["best", "mean"])
def test_min_count_and_empty_results(reduce):
    case = ("surface", 8193, 4)
    ref = vc.ref_case(case)
    top = int(ref["best"]["count"].max())
    seen = []
    for min_count in (1, 2, 3, top + 1):
        want = vc.voxel_ref(ref["xyz"], ref["voxel"], ref["priority"], ref["rgb"], reduce, min_count)
        _same(_run(ref["xyz"], ref["voxel"], ref["priority"], ref["rgb"], reduce=reduce, min_count=min_count), want)
        seen.append(len(want["index"]))
    assert seen[0] > seen[1] > seen[2] > seen[3] == 0
    # no points at all
    got = _run(np.zeros((0, 3), np.float32), 0.5, np.zeros(0, np.float32), np.zeros((0, 3), np.uint8), reduce=reduce)
    assert got["xyz"].shape == (0, 3) and got["rgb"].shape == (0, 3) and got["index"].shape == (0,) and got["count"].shape == (0,)
    assert got["dropped"] == 0
    # every point dropped
    got = _run(np.full((5, 3), np.nan, np.float32), 0.5, reduce=reduce)
    assert got["xyz"].shape == (0, 3) and got["dropped"] == 5


def test_capacity_and_sentinels_through_the_c_entry():
    from align3r_amd import _lib
    from align3r_amd._lib import ptr, stream_ptr
    lib = _lib.load()
    case = ("surface", 8193, 1)
    ref = vc.ref_case(case)
    xyz, priority, rgb = _dev(ref["xyz"]), _dev(ref["priority"]), _dev(ref["rgb"])
    M, voxel = len(ref["xyz"]), float(ref["voxel"])
    for reduce, mode in (("best", _lib.VOXEL_BEST), ("mean", _lib.VOXEL_MEAN)):
        want = ref[reduce]
        ws_bytes = int(lib.a3r_voxel_workspace_bytes(M, 0, mode))
        assert ws_bytes >= 4 * M + (20 + 48 * mode) * 16384
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device="cuda")
        V, dropped = C.c_longlong(-1), C.c_longlong(-1)
        rc = lib.a3r_voxel_count(ptr(xyz), ptr(priority), M, voxel, mode, 1, 0, ptr(ws), ws_bytes, C.byref(V), C.byref(dropped), stream_ptr())
        assert rc == 0 and V.value == len(want["index"]) and dropped.value == 0
        V = int(V.value)

        def buffers(cap):
            return (torch.full((cap, 3), -7.0, dtype=torch.float32, device="cuda"), torch.full((cap, 3), 201, dtype=torch.uint8, device="cuda"),
                    torch.full((cap,), -5, dtype=torch.int32, device="cuda"), torch.full((cap,), -9, dtype=torch.int32, device="cuda"))

        def export(cap, bufs):
            n, d = C.c_longlong(-1), C.c_longlong(-1)
            rc = lib.a3r_voxel_export(ptr(xyz), ptr(priority), ptr(rgb), M, voxel, mode, 1, 0, ptr(ws), ws_bytes, cap, *(ptr(b) for b in bufs),
                                      C.byref(n), C.byref(d), stream_ptr())
            torch.cuda.synchronize()
            return rc, int(n.value)
        bufs = buffers(V + 64)
        rc, n = export(V + 64, bufs)
        assert rc == 0 and n == V
        o_xyz, o_rgb, o_idx, o_cnt = (b.cpu().numpy() for b in bufs)
        assert o_xyz[:V].tobytes() == want["xyz"].tobytes() and np.array_equal(o_rgb[:V], want["rgb"])
        assert np.array_equal(o_idx[:V], want["index"]) and np.array_equal(o_cnt[:V], want["count"])
        assert (o_xyz[V:] == -7.0).all() and (o_rgb[V:] == 201).all() and (o_idx[V:] == -5).all() and (o_cnt[V:] == -9).all()
        bufs = buffers(V - 1)
        rc, n = export(V - 1, bufs)
        assert rc == _lib_einval() and n == V
        msg = lib.a3r_last_error().decode()
        assert str(V) in msg and "capacity" in msg
        o_xyz, o_rgb, o_idx, o_cnt = (b.cpu().numpy() for b in bufs)
        assert (o_xyz == -7.0).all() and (o_rgb == 201).all() and (o_idx == -5).all() and (o_cnt == -9).all()
    # the entry refuses a table that could fill up, and a small workspace, before any launch
    n, d = C.c_longlong(0), C.c_longlong(0)
    for slots, word in ((8192, "must exceed"), (12000, "power of two")):
        assert lib.a3r_voxel_count(ptr(xyz), None, M, voxel, 0, 1, slots, ptr(ws), ws_bytes, C.byref(n), C.byref(d), stream_ptr()) == _lib_einval()
        assert word in lib.a3r_last_error().decode()
    assert lib.a3r_voxel_count(ptr(xyz), None, M, voxel, 0, 1, 0, ptr(ws), 1024, C.byref(n), C.byref(d), stream_ptr()) == _lib_einval()
    assert "workspace too small" in lib.a3r_last_error().decode()


def _lib_einval():
    return -1                      # A3R_EINVAL of include/a3r.h


# ------------------------------------------------------------------------------------------------- scenes
def _scene_ref(scene, voxel, reduce="best", min_count=1, mask_dynamic=False, min_conf_thr=None):
    """The restatement on the arrays of get_pointcloud(with_index=True), the priorities = the confidences at the index."""
    pc = scene.get_pointcloud(min_conf_thr=min_conf_thr, mask_dynamic=mask_dynamic, with_index=True)
    P = scene.max_area
    conf = np.zeros((scene.n_imgs, P), np.float32)
    for n, (c, (h, w)) in enumerate(zip(scene._mask_confidences(), scene.imshapes)):
        conf[n, :h * w] = c.detach().float().cpu().numpy().reshape(-1)
    index = pc["index"].cpu().numpy()
    ref = vc.voxel_ref(pc["xyz"].cpu().numpy(), voxel, conf.reshape(-1)[index], pc["rgb"].cpu().numpy(), reduce, min_count)
    ref["index"] = index[ref["index"]]
    return ref, len(index)


def _scene_voxel(scene):
    """An edge that puts several points into most cells of the small scenes: a sixteenth of the cloud's extent."""
    xyz = scene.get_pointcloud()["xyz"]
    return float((xyz.max(0).values - xyz.min(0).values).max()) / 16


@pytest.mark.parametrize("kind", ["plain", "mono", "flow", "mixed"])
def test_scene_get_pointcloud_voxel_equals_the_restatement(kind, tmp_path):
    from align3r_amd.tool.pointcloud import read_ply
    scene, _ = make_mixed_scene() if kind == "mixed" else make_scene(kind, 4, 36, 44)
    voxel = _scene_voxel(scene)
    settings = [dict(), dict(reduce="mean"), dict(min_count=2)]
    if kind == "flow":
        settings += [dict(mask_dynamic=True), dict(mask_dynamic=True, reduce="mean")]
    for kw in settings:
        ref, M = _scene_ref(scene, voxel, **kw)
        V = len(ref["index"])
        assert 0 < V < M / 2
        got = scene.get_pointcloud(voxel_size=voxel, with_index=True, **kw)
        assert set(got) == {"xyz", "rgb", "count", "index"}
        assert got["xyz"].cpu().numpy().tobytes() == ref["xyz"].tobytes() and np.array_equal(got["rgb"].cpu().numpy(), ref["rgb"])
        assert np.array_equal(got["count"].cpu().numpy(), ref["count"]) and np.array_equal(got["index"].cpu().numpy(), ref["index"])
        assert got["index"].dtype == torch.int32 and got["count"].dtype == torch.int32
        assert set(scene.get_pointcloud(voxel_size=voxel, **kw)) == {"xyz", "rgb", "count"}
    # voxel_size=None is today's path: the same keys and bytes as a call without the new arguments
    for kw in (dict(), dict(with_index=True), dict(min_conf_thr=5.0, with_index=True)):
        old, new = scene.get_pointcloud(**kw), scene.get_pointcloud(voxel_size=None, reduce="mean", min_count=3, **kw)
        assert list(old) == list(new) and all(torch.equal(old[k], new[k]) and old[k].dtype == new[k].dtype for k in old)
    # the file
    ref, _ = _scene_ref(scene, voxel)
    pc = scene.save_pointcloud(tmp_path / "voxel.ply", voxel_size=voxel)
    pts, cols = read_ply(tmp_path / "voxel.ply")
    assert len(pts) == len(ref["index"]) == pc["xyz"].shape[0]
    assert pts.tobytes() == ref["xyz"].tobytes() and np.array_equal(cols, ref["rgb"])


def test_scene_reports_dropped_points_once():
    scene, _ = make_scene("plain", 4, 36, 44)
    M = scene.get_pointcloud()["xyz"].shape[0]
    with pytest.warns(UserWarning, match="in no voxel") as rec:
        got = scene.get_pointcloud(voxel_size=1e-9)                  # every coordinate is beyond 2^20 cells of a nanometre
    dropped = int(str(rec[0].message).split(": ")[1].split(" of ")[0])
    assert len(rec) == 1 and 0 < dropped <= M and int(got["count"].sum()) + dropped == M


@pytest.mark.parametrize("mode", ["single", "hierarchical"])
def test_run_clip_writes_a_voxel_cloud(mode, monkeypatch, tmp_path):
    """run_clip --pointcloud-voxel on the synthetic clip of tests/test_gpu_scene_mesh.py's run_clip test (the pair forward, the loader
    and the checkpoint replaced; the driver, the aligner and the voxel kernels real): the PLY holds n_points rows, fewer than the
    unreduced cloud."""
    import align3r_amd.dust3r.inference as inf_mod
    import align3r_amd.dust3r.model as model_mod
    import align3r_amd.dust3r.utils.image_pose as pose_mod
    from align3r_amd.tool import run_clip
    from align3r_amd.tool.pointcloud import read_ply
    from test_gpu_hier import _scene
    N, H, W = (8, 32, 48) if mode == "hierarchical" else (4, 32, 48)
    cams, world, f = _scene(N, H, W)
    rng = np.random.default_rng(0)
    frames = [torch.from_numpy(rng.uniform(-1, 1, (3, H, W)).astype(np.float32)) for _ in range(N)]

    def fake_inference(pairs, model, device, batch_size=1, verbose=False):
        gi = [int(a["instance"]) for a, b in pairs]
        gj = [int(b["instance"]) for a, b in pairs]
        p1 = np.stack([0.7 * ((world[i] - cams[i][1]) @ cams[i][0]) for i in gi]).astype(np.float32)
        p2 = np.stack([0.7 * ((world[j] - cams[i][1]) @ cams[i][0]) for i, j in zip(gi, gj)]).astype(np.float32)
        c = (1 + 4 * rng.random((len(pairs), H, W))).astype(np.float32)
        return dict(view1=dict(idx=[a["idx"] for a, b in pairs], img=[frames[i] for i in gi]),
                    view2=dict(idx=[b["idx"] for a, b in pairs], img=[frames[j] for j in gj]),
                    pred1=dict(pts3d=torch.from_numpy(p1), conf=torch.from_numpy(c)),
                    pred2=dict(pts3d_in_other_view=torch.from_numpy(p2), conf=torch.from_numpy(c.copy())))

    class FakeModel:
        def to(self, device):
            return self

    monkeypatch.setattr(inf_mod, "inference", fake_inference)
    monkeypatch.setattr(model_mod.AsymmetricCroCo3DStereo, "from_pretrained", staticmethod(lambda path: FakeModel()))
    monkeypatch.setattr(pose_mod, "load_images",
                        lambda folder, size, **kw: ([dict(idx=i, instance=str(i), true_shape=np.int32([[H, W]])) for i in range(N)], None))

    def run(extra, name):
        torch.manual_seed(0)
        rng.bit_generator.state = np.random.default_rng(0).bit_generator.state
        path = tmp_path / name
        argv = ["--images", "frames", "--weights", "w.pth", "--out", str(tmp_path / "out"), "--niter", "10", "--min-conf-thr", "2.5", "--quiet",
                "--pointcloud", str(path)] + extra
        if mode == "hierarchical":
            argv += ["--hierarchical", "--clip-size", "3"]
        return run_clip.main(argv), read_ply(path)
    full, (pts_full, cols_full) = run([], "full.ply")
    assert full["n_points"] == full["n_points_full"] == len(pts_full) > 0
    extent = float((pts_full.max(0) - pts_full.min(0)).max())
    res, (pts, cols) = run(["--pointcloud-voxel", repr(extent / 24), "--pointcloud-reduce", "mean"], "voxel.ply")
    assert res["n_points"] == len(pts) == len(cols) and res["n_points_full"] == len(pts_full)
    assert 0 < res["n_points"] < res["n_points_full"]
    if mode == "hierarchical":
        # the clips' clouds were reduced together, without priorities: the restatement on the unreduced file
        want = vc.voxel_ref(pts_full, extent / 24, None, cols_full, "mean")
        assert pts.tobytes() == want["xyz"].tobytes() and np.array_equal(cols, want["rgb"])
