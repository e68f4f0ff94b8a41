"""CPU (no GPU): the checker and the host side of the renderer (csrc/render.hip) -- render_ref() of tests/render_cases.py against a
naive per-point loop and under a permutation of the points, the conditions that keep the GPU comparison from passing on empty
pictures, world_to_camera, the PNG writer, and the refusals of a3r_render_points, which need no device."""
import ctypes as C

import numpy as np
import pytest

import render_cases as rc


def _small_cases():
    return [c for c in rc.CASES if c[1] <= 65]


@pytest.mark.parametrize("case", _small_cases(), ids=rc.case_id)
def test_render_ref_equals_a_naive_loop(case):
    kind, M, (H, W), Cn, radius = case
    ref = rc.ref_case(case)
    depth, index, col = rc.render_naive(ref["xyz"], ref["rgb"], ref["cams"], H, W, radius, rc.NEAR)
    assert depth.tobytes() == ref["depth"].tobytes()
    assert np.array_equal(index, ref["index"]) and np.array_equal(col, ref["out_rgb"])


@pytest.mark.parametrize("case", [c for c in rc.CASES if c[1] in (65, 1000) and c[4] in (0, 3)], ids=rc.case_id)
def test_render_ref_is_invariant_under_a_permutation_of_the_points(case):
    """The same points in another order, each carrying its index along: bitwise the same pictures.  Without the carried indices the
    depths are still the same, and a winner differs from the original one only on an exact depth tie."""
    kind, M, (H, W), Cn, radius = case
    ref = rc.ref_case(case)
    perm = np.random.default_rng(8).permutation(M)
    depth, index, col = rc.render_ref(ref["xyz"][perm], ref["rgb"], ref["cams"], H, W, radius, rc.NEAR, ids=perm)
    assert depth.tobytes() == ref["depth"].tobytes()
    assert np.array_equal(index, ref["index"]) and np.array_equal(col, ref["out_rgb"])
    depth, index, _ = rc.render_ref(ref["xyz"][perm], None, ref["cams"], H, W, radius, rc.NEAR)
    assert depth.tobytes() == ref["depth"].tobytes()
    hit = index >= 0
    assert np.array_equal(hit, ref["index"] >= 0)
    back, want = perm[index[hit]], ref["index"][hit]
    assert (back >= want).all()                                                # the original picture holds the lowest index of a tie
    cam_of = np.broadcast_to(np.arange(Cn)[:, None, None], hit.shape)[hit]
    for c in range(Cn):
        zf = rc.project(ref["xyz"], ref["cams"][c], rc.NEAR)[3]
        assert np.array_equal(zf[back[cam_of == c]], zf[want[cam_of == c]])    # another winner has the same depth bits


@pytest.mark.parametrize("case", [c for c in rc.CASES if c[0] == "surface" and c[1] >= 1000], ids=rc.case_id)
def test_surface_cases_are_not_empty_pictures(case):
    """What keeps the GPU comparison from passing on empty pictures, per camera: at least half the points are drawn, at least one
    pixel stays empty, at least one pixel receives two or more points."""
    kind, M, (H, W), Cn, radius = case
    ref = rc.ref_case(case)
    for c in range(Cn):
        ok, row, col, _ = rc.project(ref["xyz"], ref["cams"][c], rc.NEAR)
        centre_inside = ok & (row >= 0) & (row < H) & (col >= 0) & (col < W)     # the footprint holds its centre at every radius
        assert centre_inside.sum() >= M / 2, (c, int(centre_inside.sum()))
        assert (ref["index"][c] < 0).any()
        assert np.bincount(row[centre_inside] * W + col[centre_inside], minlength=H * W).max() >= 2
        assert np.array_equal(ref["depth"][c] > 0, ref["index"][c] >= 0)


def test_hand_worked_pixels():
    """Half to even, the near plane, ties and clipping on numbers worked out by hand: the restatement itself."""
    cams = rc.make_cams(np.concatenate([np.eye(3), np.zeros((3, 1))], 1)[None], 8.0, 8.0, 2.0, 2.0)
    pts = np.array([[-2.5 / 8, 0, 1],        # u = -0.5 -> column 0 (rint(-0.5) = -0; floor(u + 0.5) = 0 as well)
                    [-1.5 / 8, 1 / 8, 1],    # u = 0.5 -> column 0 (floor(u + 0.5) = 1), v = 3
                    [0.5 / 8, 1 / 8, 2],     # u = 2.25 at z = 2: column 2, v = 2.5 -> row 2
                    [1.5 / 8, -2 / 8, 1],    # u = 3.5 -> column 4: outside a 4-wide picture
                    [0, 0, 0.25],            # on the near plane: drawn
                    [0, 0, 0.2499999],       # below it: not drawn
                    [0, 0, 0.25]], np.float32)   # a tie with point 4: the lower index wins
    depth, index, _ = rc.render_ref(pts, None, cams, 4, 4, 0, 0.25)
    want = np.full((4, 4), -1)
    want[2, 0], want[3, 0], want[2, 2] = 0, 1, 4
    assert np.array_equal(index[0], want)
    assert depth[0, 2, 2] == np.float32(0.25) and depth[0, 3, 0] == 1 and depth[0, 0, 0] == 0
    # radius 1: point 3 (column 4, row 0) reaches column 3 of rows 0 and 1
    depth, index, _ = rc.render_ref(pts[3:4], None, cams, 4, 4, 1, 0.25)
    assert (index[0] >= 0).sum() == 2 and index[0, 0, 3] == 0 and index[0, 1, 3] == 0


def test_world_to_camera():
    from align3r_amd.tool.render import world_to_camera
    g = np.random.default_rng(0)
    q, _ = np.linalg.qr(g.standard_normal((5, 3, 3)))
    c2w = np.zeros((5, 4, 4))
    c2w[:, :3, :3], c2w[:, :3, 3], c2w[:, 3, 3] = q, g.standard_normal((5, 3)), 1
    w2c = world_to_camera(c2w)
    assert w2c.shape == (5, 3, 4) and w2c.dtype == np.float64
    assert np.array_equal(w2c[:, :, :3], np.swapaxes(q, 1, 2))                 # R^T exactly
    assert np.array_equal(w2c[:, :, 3], -(np.swapaxes(q, 1, 2) @ c2w[:, :3, 3, None])[..., 0])
    full = np.concatenate([w2c, np.broadcast_to([0, 0, 0, 1.0], (5, 1, 4))], 1)
    assert np.abs(full @ c2w - np.eye(4)).max() < 1e-14
    assert np.array_equal(world_to_camera(c2w[:, :3]), w2c) and np.array_equal(world_to_camera(c2w[0]), w2c[0])
    import torch
    assert np.array_equal(world_to_camera(torch.from_numpy(c2w.astype(np.float32))), world_to_camera(c2w.astype(np.float32)))
    with pytest.raises(ValueError):
        world_to_camera(np.zeros((3, 3)))


def test_write_png_round_trip(tmp_path):
    import PIL.Image
    from align3r_amd.tool.render import write_png
    pic = np.random.default_rng(1).integers(0, 256, (5, 7, 3), dtype=np.uint8)
    path = write_png(str(tmp_path / "a.png"), pic)
    assert np.array_equal(np.asarray(PIL.Image.open(path)), pic)
    import torch
    write_png(str(tmp_path / "b.png"), torch.from_numpy(pic[..., 0].copy()))
    assert np.array_equal(np.asarray(PIL.Image.open(tmp_path / "b.png")), pic[..., 0])
    with pytest.raises(ValueError):
        write_png(str(tmp_path / "c.png"), pic.astype(np.float32))


def test_render_cameras_table_and_skew():
    from align3r_amd import ops
    w2c = np.arange(2 * 16, dtype=np.float64).reshape(2, 4, 4)
    K = np.zeros((2, 3, 3))
    K[:, 0, 0], K[:, 1, 1], K[:, 0, 2], K[:, 1, 2], K[:, 2, 2] = 100, 101, 50, 40, 1
    cams = ops.render_cameras(w2c, K)
    assert cams.shape == (2, 16) and np.array_equal(cams[1, :12], np.arange(16, 28)) and cams[0, 12:].tolist() == [100, 101, 50, 40]
    assert np.array_equal(cams, rc.make_cams(w2c, 100, 101, 50, 40))
    assert np.array_equal(ops.render_cameras(w2c[:, :3], K), cams)
    K[1, 0, 1] = 1e-3
    with pytest.raises(ValueError, match="skew"):
        ops.render_cameras(w2c, K)
    with pytest.raises(ValueError, match="float64"):
        ops.render_cameras(w2c.astype(np.float32), K)


def test_refusals_need_no_device():
    """Every A3R_EINVAL of a3r_render_points is raised before anything is launched: the pointers below are host memory."""
    from align3r_amd import _lib
    lib = _lib.load()
    for name in ("a3r_render_workspace_bytes", "a3r_render_points", "a3r_render_set_form"):
        assert name in _lib.SIGNATURES and hasattr(lib, name), name
    assert C.sizeof(_lib.RenderCam) == 128
    assert lib.a3r_render_workspace_bytes(3, 48, 64) == 3 * 48 * 64 * 8
    assert lib.a3r_render_workspace_bytes(1, 1, 1) == 256 and lib.a3r_render_workspace_bytes(1, 1, 1) % 16 == 0
    assert lib.a3r_render_workspace_bytes(0, 4, 4) == 0 and lib.a3r_render_workspace_bytes(1, -4, 4) == 0
    assert lib.a3r_render_workspace_bytes(2, 1 << 15, 1 << 15) == 0 and lib.a3r_render_workspace_bytes(1, 1 << 16, 1 << 16) == 0

    xyz = np.zeros((4, 3), np.float32)
    rgb = np.zeros((4, 3), np.uint8)
    cams = rc.make_cams(np.concatenate([np.eye(3), np.zeros((3, 1))], 1)[None], 8.0, 8.0, 2.0, 2.0)
    bg = np.zeros(3, np.uint8)
    ws = np.zeros(4096 + 16, np.uint8)
    ws_ptr = (ws.ctypes.data + 15) & ~15
    depth, out_rgb, index = np.zeros(16, np.float32), np.zeros(48, np.uint8), np.zeros(16, np.int32)
    p = lambda a: a.ctypes.data
    good = dict(xyz=p(xyz), rgb=p(rgb), M=4, cams_dev=p(cams), cams_host=p(cams), n_cams=1, H=4, W=4, radius=1, near=0.5, bg=p(bg), ws=ws_ptr,
                ws_bytes=4096, depth=p(depth), out_rgb=p(out_rgb), index=p(index))

    def refused(word, **change):
        a = dict(good, **change)
        rcode = lib.a3r_render_points(a["xyz"], a["rgb"], a["M"], a["cams_dev"], a["cams_host"], a["n_cams"], a["H"], a["W"], a["radius"],
                                      a["near"], a["bg"], a["ws"], a["ws_bytes"], a["depth"], a["out_rgb"], a["index"], None)
        msg = lib.a3r_last_error().decode()
        assert rcode == -1 and word in msg, (change, rcode, msg)

    refused("null xyz", xyz=None)
    refused("cams", cams_dev=None)
    refused("cams", cams_host=None)
    refused("null depth", depth=None)
    refused("background", bg=None)
    refused("M = -1", M=-1)
    refused("2^31", M=1 << 31)
    refused("n_cams", n_cams=0)
    refused("n_cams", n_cams=-2)
    refused("image size", H=0)
    refused("image size", W=-1)
    refused("below 2^31", n_cams=1, H=1 << 16, W=1 << 15)
    refused("below 2^31", n_cams=1, H=(1 << 31) - 1, W=(1 << 31) - 1)
    refused("radius", radius=-1)
    refused("radius", radius=9)
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        refused("near_z", near=bad)
    refused("out_rgb needs rgb", rgb=None)
    refused("workspace too small", ws_bytes=64)
    refused("workspace too small", ws=None)
    refused("16-byte aligned", ws=ws_ptr + 8)
    for k in (0, 11, 12, 15):
        for bad in (np.nan, np.inf):
            c = cams.copy()
            c[0, k] = bad
            refused("camera 0", cams_host=p(c))
    with pytest.raises(RuntimeError, match="radius"):
        _lib.check(lib.a3r_render_points(p(xyz), None, 4, p(cams), p(cams), 1, 4, 4, 9, 0.5, None, ws_ptr, 4096, p(depth), None, None, None))
    # the form switch: values outside [0, 7] only query
    old = lib.a3r_render_set_form(-1)
    assert lib.a3r_render_set_form(3) == old and lib.a3r_render_set_form(8) == 3 and lib.a3r_render_set_form(old) == 3
    assert lib.a3r_render_set_form(-1) == old


@pytest.mark.parametrize("mode", ["--hierarchical", "--flow-hierarchical"])
def test_run_clip_refuses_render_with_the_hierarchical_modes(mode, capsys):
    from align3r_amd.tool.run_clip import parse
    base = ["--images", "frames", "--weights", "w.pth", "--out", "out", "--render", "r"]
    with pytest.raises(SystemExit):
        parse(base + [mode])
    assert "--render cannot be combined" in capsys.readouterr().err
    a = parse(base)
    assert a.render == "r" and a.render_radius == 1 and parse(base[:6]).render is None
    assert parse(base + ["--flow", "--render-radius", "3"]).render_radius == 3
    for extra in (["--render-radius", "9"], ["--render-radius", "-1"]):
        with pytest.raises(SystemExit):
            parse(base + extra)
    with pytest.raises(SystemExit):
        parse(base[:6] + ["--render-radius", "2"])
    assert "--render-radius belongs to --render" in capsys.readouterr().err
