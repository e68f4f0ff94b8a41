"""GPU: the scene as a triangle mesh (csrc/scene.hip: a3r_align_scene_mesh_count / _export, AlignEngine.count_mesh / export_mesh,
scene.get_mesh / save_mesh, run_clip --mesh).

The mesh is an integer-valued function of the kept mask and the image shapes, so nothing here is approximate: the expected faces
come from align3r_amd.tool.pointcloud.mesh_faces_host (pinned to the reference's pts3d_to_trimesh / cat_meshes by
tests/test_mesh_cpu.py) on the kept mask the test composes itself from conf, thr, dyn and isfinite(engine.points()); the vertices
must be bitwise those of export_points.  Every comparison is array_equal / torch.equal.

Shapes: 37x41 (P = 1517: not a multiple of 4 -- the scalar loads --, two chunks, rows straddling the 1024-pixel chunk edge), 40x52
(16-byte loads for both rows, three chunks), a mono-parameterised 37x41, a mixed scene of 24x32 and 32x24 (each image's own w) and
one of 32x48 and 24x40 (padding pixels, a row below that needs scalar loads beside one that does not).  Engines are built as in
tests/test_gpu_scene.py.
"""
import ctypes as C
import functools
import json
import os

import numpy as np
import pytest
import torch

import align_cases as ac
from conftest import GOLDEN
from test_gpu_scene import _problem, _views, make_mixed_scene, make_scene

pytestmark = pytest.mark.gpu

THR = 1.0
CHUNK = 1024                  # pixels per workgroup of the scene kernels


# ------------------------------------------------------------------------------------------------- engines
def mixed_scene(shapes, seed=9):
    """A plain scene over images of the given shapes (per-edge prediction lists), as make_mixed_scene of test_gpu_scene builds its own."""
    N, edges = len(shapes), ac.window_graph(len(shapes), 2)
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
    im = (0.05 * rng.standard_normal((N, 7))).astype(np.float32)
    im[:, 3] += 1
    scene.engine.set_params(depth=(0.1 * rng.standard_normal((N, scene.max_area))).astype(np.float32), im_poses=im)
    return scene


@functools.lru_cache(maxsize=None)
def holder(name):
    """The scene (kept alive with its engine) of a named shape; built once per run."""
    if name == "plain_37x41":
        return make_scene("plain", 3, 37, 41)[0]
    if name == "plain_40x52":
        return make_scene("plain", 6, 40, 52)[0]
    if name == "mono_37x41":
        return make_scene("mono", 3, 37, 41)[0]
    if name == "mixed_24x32_32x24":
        return mixed_scene([(24, 32), (32, 24), (24, 32), (32, 24)])
    if name == "mixed_32x48_24x40":
        return make_mixed_scene()[0]
    raise KeyError(name)


SHAPES = ["plain_37x41", "plain_40x52", "mono_37x41", "mixed_24x32_32x24", "mixed_32x48_24x40"]


def engine(name):
    return holder(name).engine


# ------------------------------------------------------------------------------------------------- expectation
def kept_maps(eng, conf, thr, dyn):
    """The kept rule composed in numpy: inside the image, conf > thr, not dynamic, finite world point.  One bool [h,w] per image."""
    pts = eng.points().cpu().numpy()
    keep = (np.asarray(conf, np.float32).reshape(eng.N, eng.P) > np.float32(thr)) & np.isfinite(pts).all(-1)
    if dyn is not None:
        keep &= ~np.asarray(dyn, bool).reshape(eng.N, eng.P)
    return [keep[n, :h * w].reshape(h, w) for n, (h, w) in enumerate(eng.imshapes)]


def check_mesh(eng, conf, thr=THR, dyn=None, rgb=None, sides=(False, True)):
    """export_mesh against mesh_faces_host + export_points, count_mesh against both.  Returns (V, F single-sided)."""
    from align3r_amd.tool.pointcloud import mesh_faces_host
    valid = kept_maps(eng, conf, thr, dyn)
    V = int(sum(v.sum() for v in valid))
    pc = eng.export_points(conf, thr, dyn=dyn, rgb=rgb)
    assert pc["xyz"].shape[0] == V
    single = None
    for ds in sides:
        faces, colour = mesh_faces_host(valid, double_sided=ds)
        got = eng.export_mesh(conf, thr, dyn=dyn, rgb=rgb, double_sided=ds)
        assert set(got) == ({"xyz", "faces"} | ({"rgb", "face_rgb"} if rgb is not None else set()))
        assert got["xyz"].dtype == torch.float32 and got["faces"].dtype == torch.int32
        assert got["xyz"].shape == (V, 3) and torch.equal(got["xyz"].view(torch.int32), pc["xyz"].view(torch.int32))
        assert got["faces"].shape == (len(faces), 3) and np.array_equal(got["faces"].cpu().numpy(), faces)
        if rgb is not None:
            assert got["rgb"].dtype == got["face_rgb"].dtype == torch.uint8 and torch.equal(got["rgb"], pc["rgb"])
            assert np.array_equal(got["face_rgb"].cpu().numpy(), pc["rgb"].cpu().numpy()[colour].reshape(-1, 3))
        assert eng.count_mesh(conf, thr, dyn=dyn, double_sided=ds) == (V, len(faces))
        if not ds:
            single = got["faces"].cpu().numpy()
    return V, (len(single) if single is not None else None)


def rand_rgb(eng, seed=1):
    return np.random.default_rng(seed).integers(0, 256, (eng.N, eng.P, 3), dtype=np.uint8)


def quads(eng):
    return sum((h - 1) * (w - 1) for h, w in eng.imshapes)


# ------------------------------------------------------------------------------------------------- mask patterns
@pytest.mark.parametrize("name", SHAPES)
def test_random_masks(name):
    """About 70 % kept (real-valued confidences, some exactly at the threshold: dropped), with and without a 30 % dynamic mask."""
    eng = engine(name)
    rng = np.random.default_rng(11)
    keep = rng.random((eng.N, eng.P)) < 0.7
    conf = np.where(keep, THR + 0.01 + rng.random((eng.N, eng.P)), THR * rng.random((eng.N, eng.P))).astype(np.float32)
    conf[rng.random((eng.N, eng.P)) < 0.02] = THR                 # strict compare
    rgb = rand_rgb(eng)
    V, F = check_mesh(eng, conf, rgb=rgb)
    real = sum(h * w for h, w in eng.imshapes)
    assert 0.6 * real < V < 0.8 * real and 0 < F < 2 * quads(eng)
    dyn = rng.random((eng.N, eng.P)) < 0.3
    dyn[-1] = True                                                # one image fully dynamic
    V2, F2 = check_mesh(eng, conf, dyn=dyn, rgb=rgb)
    assert 0 < V2 < V and 0 < F2 < F
    check_mesh(eng, conf, dyn=dyn)                                # no colours at all


@pytest.mark.parametrize("name", SHAPES)
def test_all_none_one_checkerboard(name):
    eng = engine(name)
    N, P = eng.N, eng.P
    rgb = rand_rgb(eng, 2)
    real = sum(h * w for h, w in eng.imshapes)
    # all kept (the padding entries of conf hold a kept value too: they are never kept): every quad gives two triangles -- a
    # wrap from a row end to the next row or a missing last row / column would change the count
    full = np.full((N, P), 2.0, np.float32)
    assert check_mesh(eng, full, rgb=rgb) == (real, 2 * quads(eng))
    assert eng.count_mesh(full, THR, double_sided=True) == (real, 4 * quads(eng))
    # none kept: an empty mesh is a success
    assert check_mesh(eng, np.zeros((N, P), np.float32), rgb=rgb) == (0, 0)
    got = eng.export_mesh(np.zeros((N, P), np.float32), THR, rgb=rgb)
    assert got["xyz"].shape == (0, 3) and got["faces"].shape == (0, 3) and got["face_rgb"].shape == (0, 3)
    # one kept pixel
    one = np.zeros((N, P), np.float32)
    one[N - 1, eng.imshapes[N - 1][1] + 1] = 2.0
    assert check_mesh(eng, one, rgb=rgb) == (1, 0)
    # checkerboard: every triangle has two neighbours of different parity among its corners
    board = np.zeros((N, P), np.float32)
    for n, (h, w) in enumerate(eng.imshapes):
        y, x = np.divmod(np.arange(h * w), w)
        board[n, :h * w] = 2.0 * ((x + y) % 2 == 0)
    assert check_mesh(eng, board, rgb=rgb) == (sum((h * w + 1) // 2 for h, w in eng.imshapes), 0)


@pytest.mark.parametrize("name", ["plain_37x41", "plain_40x52", "mono_37x41", "mixed_32x48_24x40"])      # more than one chunk
def test_regions_ending_at_a_chunk_boundary(name):
    """Kept pixels [0, 1024) and, apart, [1024, end): the faces across the boundary vanish, those on either side stay."""
    eng = engine(name)
    assert eng.P > CHUNK
    p = np.arange(eng.P)[None, :].repeat(eng.N, 0)
    below, above = check_mesh(eng, 2.0 * (p < CHUNK).astype(np.float32)), check_mesh(eng, 2.0 * (p >= CHUNK).astype(np.float32))
    whole = check_mesh(eng, np.full((eng.N, eng.P), 2.0, np.float32), sides=(False,))
    assert below[0] + above[0] == whole[0] and 0 < below[1] and 0 < above[1] and below[1] + above[1] < whole[1]
    # and a region whose last kept pixel is the last of a chunk while the next chunk starts kept again one row further
    w = eng.imshapes[0][1]
    check_mesh(eng, 2.0 * ((p < CHUNK) | (p >= CHUNK + w)).astype(np.float32), rgb=rand_rgb(eng, 3))


@pytest.mark.parametrize("name", ["plain_37x41", "plain_40x52", "mono_37x41", "mixed_32x48_24x40"])
def test_non_finite_depths_take_their_triangles_with_them(name):
    """A NaN and a +inf among the depth parameters (beside a chunk edge, a row end, the first and the last pixel): those pixels are
    no vertices and every triangle touching them is gone."""
    from align3r_amd.tool.pointcloud import mesh_faces_host
    eng = engine(name)
    N, P = eng.N, eng.P
    saved = eng.params["depth"].clone()
    h1, w1 = eng.imshapes[1]
    hot = [(0, 0, np.nan), (0, 5, np.inf), (0, CHUNK - 1, np.nan), (0, CHUNK, np.inf), (1, w1 - 1, np.inf), (1, 2 * w1, np.nan),
           (1, h1 * w1 - 1, np.nan), (2, CHUNK + 3, np.inf)]
    try:
        depth = saved.clone()
        for n, p, v in hot:
            depth[n, p] = v
        eng.set_params(depth=depth, reset_optimizer=False)
        conf = np.full((N, P), 2.0, np.float32)
        valid = kept_maps(eng, conf, THR, None)
        flat = [v.ravel() for v in valid]
        assert all(not flat[n][p] for n, p, _ in hot) and sum(int(v.sum()) for v in valid) == sum(v.size for v in valid) - len(hot)
        V, F = check_mesh(eng, conf, rgb=rand_rgb(eng, 4))
        full, _ = mesh_faces_host([np.ones_like(v) for v in valid])
        assert V == sum(v.size for v in valid) - len(hot) and F < len(full)
        got = eng.export_mesh(conf, THR)
        assert torch.isfinite(got["xyz"]).all()
    finally:
        eng.set_params(depth=saved, reset_optimizer=False)
    assert check_mesh(eng, np.full((N, P), 2.0, np.float32), sides=(False,)) == (sum(h * w for h, w in eng.imshapes), 2 * quads(eng))


@pytest.mark.parametrize("name", ["plain_37x41", "mixed_32x48_24x40"])
def test_double_sided_holds_the_single_sided_blocks(name):
    """[A, A', B, B'] per image: A and B are the single-sided faces, the primed blocks the same triangles wound backwards with the
    same colours; two calls give equal bits."""
    eng = engine(name)
    rng = np.random.default_rng(5)
    conf = (2.0 * (rng.random((eng.N, eng.P)) < 0.7)).astype(np.float32)
    rgb = rand_rgb(eng, 5)
    one, two = eng.export_mesh(conf, THR, rgb=rgb), eng.export_mesh(conf, THR, rgb=rgb, double_sided=True)
    again = eng.export_mesh(conf, THR, rgb=rgb, double_sided=True)
    assert set(two) == set(again) and all(torch.equal(two[k], again[k]) for k in two)
    assert torch.equal(one["xyz"], two["xyz"]) and torch.equal(one["rgb"], two["rgb"])
    f1, c1, f2, c2 = (t.cpu().numpy() for t in (one["faces"], one["face_rgb"], two["faces"], two["face_rgb"]))
    assert len(f2) == 2 * len(f1) > 0
    # the block sizes of every image, counted from the kept mask
    at1 = at2 = 0
    for v in kept_maps(eng, conf, THR, None):
        diag = v[:-1, 1:] & v[1:, :-1]
        for k in (int((diag & v[:-1, :-1]).sum()), int((diag & v[1:, 1:]).sum())):
            blk, blk_c = f1[at1:at1 + k], c1[at1:at1 + k]
            assert np.array_equal(f2[at2:at2 + k], blk) and np.array_equal(c2[at2:at2 + k], blk_c)
            assert np.array_equal(f2[at2 + k:at2 + 2 * k], blk[:, ::-1]) and np.array_equal(c2[at2 + k:at2 + 2 * k], blk_c)
            at1, at2 = at1 + k, at2 + 2 * k
    assert at1 == len(f1) and at2 == len(f2)


# ------------------------------------------------------------------------------------------------- goldens through the device
META = json.load(open(os.path.join(GOLDEN, "mesh.json")))["cases"]


@pytest.mark.parametrize("name", list(META))
def test_golden_cases_through_the_device(name):
    """The reference's own faces and colours (tests/golden/mesh.npz), with every dense index replaced by the pixel's rank."""
    g = np.load(os.path.join(GOLDEN, "mesh.npz"))
    c, shapes = META[name]["case"], [tuple(s) for s in META[name]["shapes"]]
    valid = [g[f"valid_{c}_{n}"] for n in range(len(shapes))]
    imgs = [g[f"img_{c}_{n}"] for n in range(len(shapes))]
    ref_faces, ref_colors = g[f"faces_{c}"], g[f"colors_{c}"]
    if len(shapes) == 1:                                          # an aligner needs two images: a second one, fully dropped
        shapes, valid, imgs = shapes * 2, valid + [np.zeros_like(valid[0])], imgs * 2
    scene = mixed_scene(shapes, seed=3)
    eng = scene.engine
    N, P = eng.N, eng.P
    conf, rgb = np.zeros((N, P), np.float32), np.zeros((N, P, 3), np.uint8)
    for n, (h, w) in enumerate(shapes):
        conf[n, :h * w] = 2.0 * valid[n].ravel()
        rgb[n, :h * w] = imgs[n].reshape(-1, 3)
    keep = np.concatenate([v.ravel() for v in valid])
    rank = np.where(keep, np.cumsum(keep) - 1, -1)
    got = eng.export_mesh(conf, THR, rgb=rgb, double_sided=True)
    assert got["xyz"].shape[0] == keep.sum()
    assert np.array_equal(got["faces"].cpu().numpy(), rank[ref_faces]) and np.array_equal(got["face_rgb"].cpu().numpy(), ref_colors)
    assert eng.count_mesh(conf, THR, double_sided=True) == (int(keep.sum()), len(ref_faces))
    check_mesh(eng, conf, rgb=rgb)


# ------------------------------------------------------------------------------------------------- sharded engine
def test_sharded_engine_gives_the_fused_mesh():
    from align3r_amd.aligner import AlignEngine, ShardedAlignEngine
    N, H, W = 4, 36, 44
    prob = _problem(N, H, W, 11)
    fused = AlignEngine(*prob["args"], device="cuda:0")
    shard = ShardedAlignEngine(*prob["args"], device="cuda:0", local_shards=3)
    fused.set_params(**prob["init"])
    shard.set_params(**prob["init"])
    rng = np.random.default_rng(2)
    conf = (1 + 9 * rng.random((N, H * W))).astype(np.float32)
    rgb = rng.integers(0, 256, (N, H * W, 3), dtype=np.uint8)
    dyn = prob["flow"]["dyn"].reshape(N, -1)
    for ds in (False, True):
        a, b = fused.export_mesh(conf, 5.0, dyn=dyn, rgb=rgb, double_sided=ds), shard.export_mesh(conf, 5.0, dyn=dyn, rgb=rgb, double_sided=ds)
        assert set(a) == set(b) == {"xyz", "rgb", "faces", "face_rgb"} and a["faces"].shape[0] > 0
        assert all(torch.equal(a[k], b[k]) for k in a)
        assert shard.count_mesh(conf, 5.0, dyn=dyn, double_sided=ds) == (a["xyz"].shape[0], a["faces"].shape[0])
    check_mesh(shard, conf, thr=5.0, dyn=dyn, rgb=rgb)


# ------------------------------------------------------------------------------------------------- the C entry points
@pytest.mark.parametrize("name", ["plain_37x41", "plain_40x52"])
def test_refusals_and_sentinels_through_the_c_entry(name):
    """Capacities above the counts: the tails keep their canaries.  One vertex or one face short, a short workspace, face colours
    without rgb: an error, not one output element written, the needed counts returned where they are known, and the handle works
    on afterwards."""
    from align3r_amd._lib import check, ptr, stream_ptr
    eng = engine(name)
    lib, dev, N, P = eng.lib, eng.device, eng.N, eng.P
    rng = np.random.default_rng(8)
    conf = torch.from_numpy((2.0 * (rng.random((N, P)) < 0.7)).astype(np.float32)).to(dev)
    rgb = torch.from_numpy(rand_rgb(eng, 8)).to(dev)
    want = eng.export_mesh(conf, THR, rgb=rgb, double_sided=True)
    V, F = want["xyz"].shape[0], want["faces"].shape[0]
    assert V > 64 and F > 64
    ws = torch.empty(int(lib.a3r_align_scene_mesh_workspace_bytes(N, P)), dtype=torch.uint8, device=dev)
    assert ws.data_ptr() % 16 == 0

    def buffers(vcap, fcap):
        return (torch.full((vcap, 3), -12345.5, device=dev), torch.full((vcap, 3), 0xAB, dtype=torch.uint8, device=dev),
                torch.full((fcap, 3), -7, dtype=torch.int32, device=dev), torch.full((fcap, 3), 0xCD, dtype=torch.uint8, device=dev))

    def untouched(b):
        torch.cuda.synchronize()
        return bool((b[0] == -12345.5).all() and (b[1] == 0xAB).all() and (b[2] == -7).all() and (b[3] == 0xCD).all())

    def export(b, vcap, fcap, wsb=None, src=rgb, face_rgb=True, vertex_rgb=True):
        nv, nf = C.c_longlong(-1), C.c_longlong(-1)
        rc = lib.a3r_align_scene_mesh_export(eng.handle, ptr(conf), THR, None, ptr(src), ptr(ws), ws.numel() if wsb is None else wsb, 1, vcap,
                                             fcap, ptr(b[0]), ptr(b[1]) if vertex_rgb else None, ptr(b[2]), ptr(b[3]) if face_rgb else None,
                                             C.byref(nv), C.byref(nf), stream_ptr())
        torch.cuda.synchronize()
        return rc, nv.value, nf.value, lib.a3r_last_error().decode()

    b = buffers(V + 64, F + 64)
    assert export(b, V + 64, F + 64)[:3] == (0, V, F)
    assert torch.equal(b[0][:V], want["xyz"]) and torch.equal(b[1][:V], want["rgb"])
    assert torch.equal(b[2][:F], want["faces"]) and torch.equal(b[3][:F], want["face_rgb"])
    assert (b[0][V:] == -12345.5).all() and (b[1][V:] == 0xAB).all() and (b[2][F:] == -7).all() and (b[3][F:] == 0xCD).all()
    # the optional outputs left out
    b2 = buffers(V, F)
    assert export(b2, V, F, src=None, face_rgb=False, vertex_rgb=False)[:3] == (0, V, F)
    assert torch.equal(b2[0], want["xyz"]) and torch.equal(b2[2], want["faces"]) and (b2[1] == 0xAB).all() and (b2[3] == 0xCD).all()
    # one vertex short, one face short
    for vcap, fcap, word in ((V - 1, F, "vertex capacity"), (V, F - 1, "face capacity")):
        b = buffers(vcap, fcap)
        rc, nv, nf, msg = export(b, vcap, fcap)
        assert rc != 0 and (nv, nf) == (V, F) and word in msg and untouched(b), msg
    # a short workspace (one byte and one part short), face colours without the source
    b = buffers(V, F)
    for wsb in (ws.numel() - 1, ws.numel() - N * P * 4, 4):
        rc, nv, nf, msg = export(b, V, F, wsb=wsb)
        assert rc != 0 and (nv, nf) == (0, 0) and "workspace too small" in msg and untouched(b), msg
    rc, nv, nf, msg = export(b, V, F, src=None, vertex_rgb=False)
    assert rc != 0 and "out_face_rgb needs the rgb" in msg and untouched(b), msg
    nv, nf = C.c_longlong(-1), C.c_longlong(-1)
    assert lib.a3r_align_scene_mesh_count(eng.handle, ptr(conf), THR, None, ptr(ws), 4, 1, C.byref(nv), C.byref(nf), stream_ptr()) != 0
    assert "workspace too small" in lib.a3r_last_error().decode()
    assert lib.a3r_align_scene_mesh_count(eng.handle, ptr(conf), THR, None, ptr(ws[4:]), ws.numel(), 1, C.byref(nv), C.byref(nf),
                                          stream_ptr()) != 0
    assert "16-byte aligned" in lib.a3r_last_error().decode()
    assert lib.a3r_align_scene_mesh_count(eng.handle, None, THR, None, ptr(ws), ws.numel(), 1, C.byref(nv), C.byref(nf), stream_ptr()) != 0
    assert "null confidence" in lib.a3r_last_error().decode()
    # the handle is as usable as before
    check(lib.a3r_align_scene_mesh_count(eng.handle, ptr(conf), THR, None, ptr(ws), ws.numel(), 1, C.byref(nv), C.byref(nf), stream_ptr()))
    assert (nv.value, nf.value) == (V, F)
    again = eng.export_mesh(conf, THR, rgb=rgb, double_sided=True)
    assert all(torch.equal(want[k], again[k]) for k in want)


# ------------------------------------------------------------------------------------------------- scene API, files, driver
@pytest.mark.parametrize("kind", ["plain", "flow"])
def test_get_mesh_and_save_mesh(kind, tmp_path):
    """global_aligner -> scene.get_mesh() / save_mesh() -> read_ply_mesh, plain and flow class: the vertices are get_pointcloud's, the
    faces those of get_masks() (and the dynamic masks), the file holds what get_mesh returns."""
    from align3r_amd.tool.pointcloud import mesh_faces_host, read_ply_mesh
    scene, _ = make_scene(kind, 4, 37, 41)
    kw = dict(mask_dynamic=True) if kind == "flow" else {}
    mesh, pc = scene.get_mesh(**kw), scene.get_pointcloud(**kw)
    assert set(mesh) == {"xyz", "rgb", "faces", "face_rgb"}
    assert torch.equal(mesh["xyz"], pc["xyz"]) and torch.equal(mesh["rgb"], pc["rgb"])
    valid = [m.cpu().numpy() for m in scene.get_masks()]
    if kind == "flow":
        valid = [v & ~np.asarray(torch.as_tensor(d).cpu(), bool) for v, d in zip(valid, scene.dynamic_masks)]
    assert torch.isfinite(scene.engine.points()).all()
    faces, colour = mesh_faces_host(valid)
    V = sum(int(v.sum()) for v in valid)
    assert 0 < V < 4 * 37 * 41 and len(faces) > 0 and mesh["xyz"].shape[0] == V
    assert np.array_equal(mesh["faces"].cpu().numpy(), faces)
    assert np.array_equal(mesh["face_rgb"].cpu().numpy(), pc["rgb"].cpu().numpy()[colour])
    two = scene.get_mesh(min_conf_thr=5.0, double_sided=True, **kw)
    assert two["faces"].shape[0] == 2 * scene.get_mesh(min_conf_thr=5.0, **kw)["faces"].shape[0]
    saved = scene.save_mesh(tmp_path / "scene.ply", **kw)
    xyz, f, rgb, frgb = read_ply_mesh(tmp_path / "scene.ply")
    assert xyz.tobytes() == saved["xyz"].cpu().numpy().tobytes() == mesh["xyz"].cpu().numpy().tobytes()
    assert np.array_equal(f, faces) and np.array_equal(rgb, pc["rgb"].cpu().numpy()) and np.array_equal(frgb, mesh["face_rgb"].cpu().numpy())
    if kind == "plain":
        with pytest.raises(RuntimeError, match="get_mesh.*no dynamic masks"):
            scene.get_mesh(mask_dynamic=True)
        scene.imgs = None                                         # a scene without frames has no colours
        assert set(scene.get_mesh()) == {"xyz", "faces"}
        scene.save_mesh(tmp_path / "plain.ply")
        got = read_ply_mesh(tmp_path / "plain.ply")
        assert got[2] is None and got[3] is None and np.array_equal(got[1], faces)


@pytest.mark.parametrize("mode", ["single", "hierarchical"])
def test_run_clip_writes_a_mesh(mode, monkeypatch, tmp_path):
    """run_clip --mesh on the synthetic clip of tests/test_gpu_hier.py (the pair forward, the loader and the checkpoint replaced; the
    driver, the aligner and the mesh kernels real): the file's faces all index existing vertices, and with --hierarchical it holds
    every clip's mesh with the vertex offsets added."""
    import align3r_amd.dust3r.inference as inf_mod
    import align3r_amd.dust3r.model as model_mod
    import align3r_amd.dust3r.utils.image_pose as pose_mod
    from align3r_amd.tool import run_clip
    from align3r_amd.tool.pointcloud import read_ply, read_ply_mesh
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
    torch.manual_seed(0)
    path, cloud = tmp_path / "scene_mesh.ply", tmp_path / "scene.ply"
    argv = ["--images", "frames", "--weights", "w.pth", "--out", str(tmp_path / "out"), "--niter", "10", "--min-conf-thr", "2.5", "--quiet",
            "--mesh", str(path), "--pointcloud", str(cloud)]
    if mode == "hierarchical":
        argv += ["--hierarchical", "--clip-size", "3", "--mesh-double-sided"]
    res = run_clip.main(argv)
    xyz, faces, rgb, face_rgb = read_ply_mesh(path)
    V, F = len(xyz), len(faces)
    assert (res["mesh"], res["n_vertices"], res["n_faces"]) == (str(path), V, F) and 0 < V <= N * H * W and F > 0
    if mode == "single":
        assert V < N * H * W                                         # the threshold bites (the hierarchical driver clamps confidences)
    assert faces.min() >= 0 and faces.max() < V and rgb.shape == (V, 3) and face_rgb.shape == (F, 3)
    # the vertices are the point cloud written beside it; every face is a pixel triangle of ONE frame: its corners lie within one
    # frame's vertex range, i.e. less than a frame's pixels apart
    pts, cols = read_ply(cloud)
    assert xyz.tobytes() == pts.tobytes() and np.array_equal(rgb, cols)
    assert (faces.max(1) - faces.min(1) <= W + 1).all()
    if mode == "hierarchical":
        assert F % 2 == 0 and faces.max() >= V - H * W               # the last clip's faces carry the offsets of the clips before
    base = ["--images", "x", "--weights", "y", "--out", "z"]
    assert run_clip.parse(base).mesh is None and run_clip.parse(base + ["--mesh", "m.ply"]).mesh_double_sided is False
    with pytest.raises(SystemExit):
        run_clip.parse(base + ["--mesh-double-sided"])
