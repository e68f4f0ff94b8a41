"""CPU (no GPU): the numpy restatement of the TSDF definition (tests/tsdf_cases.py) checked on its own -- against a scalar loop, for
the gates its cases are built to produce, and for the properties of the surface it extracts -- and the argument checks of
ops.tsdf_*, which raise before the library is touched."""
import math

import numpy as np
import pytest
import torch

import tsdf_cases as tc


def _scalar_ref(c):
    """One voxel at a time, one frame at a time, Python floats: the definition read aloud."""
    nx, ny, nz = c["dims"]
    ox, oy, oz = (float(o) for o in c["origin"])
    vs, trunc, near, max_depth = float(c["voxel"]), float(c["trunc"]), float(c["near"]), float(c["max_depth"])
    shapes = tc.cam_shapes(c["cams"])
    tsdf, wsum = np.zeros((nz, ny, nx), np.float32), np.zeros((nz, ny, nx), np.float32)
    out_rgb = np.zeros((nz, ny, nx, 3), np.uint8)
    for k in range(nz):
        for j in range(ny):
            for i in range(nx):
                X, Y, Z = ox + (i + 0.5) * vs, oy + (j + 0.5) * vs, oz + (k + 0.5) * vs
                W = S = Wc = 0.0
                C = [0.0, 0.0, 0.0]
                for n in range(len(c["cams"])):
                    R = [float(e) for e in c["cams"][n, :16]]
                    h, w = int(shapes[n, 0]), int(shapes[n, 1])
                    xc = (R[0] * X + R[1] * Y) + R[2] * Z + R[3]
                    yc = (R[4] * X + R[5] * Y) + R[6] * Z + R[7]
                    zc = (R[8] * X + R[9] * Y) + R[10] * Z + R[11]
                    if not zc >= near:
                        continue
                    u, v = R[12] * (xc / zc) + R[14], R[13] * (yc / zc) + R[15]
                    if not (abs(u) < 2.0 ** 30 and abs(v) < 2.0 ** 30):
                        continue
                    col, row = round(u), round(v)                   # Python rounds half to even
                    if not (0 <= col < w and 0 <= row < h):
                        continue
                    d, wd = float(c["depth"][n, row * w + col]), float(c["weight"][n, row * w + col])
                    if not (math.isfinite(d) and math.isfinite(wd) and wd > 0 and d > 0 and d <= max_depth):
                        continue
                    sdf = d - zc
                    if sdf < -trunc:
                        continue
                    W += wd
                    S += wd * min(1.0, sdf / trunc)
                    if sdf <= trunc and c["rgb"] is not None:
                        Wc += wd
                        for ch in range(3):
                            C[ch] += wd * float(c["rgb"][n, row * w + col, ch])
                tsdf[k, j, i] = np.float32(S / W) if W != 0 else 1.0
                wsum[k, j, i] = np.float32(W)
                if Wc != 0:
                    out_rgb[k, j, i] = [min(round(C[ch] / Wc), 255) for ch in range(3)]
    return tsdf, wsum, out_rgb


@pytest.mark.parametrize("name", ["gates-13x9x7", "gates-1x8x8", "gates-13x9x7-norgb"])
def test_the_vectorised_restatement_equals_the_scalar_loop(name):
    c = tc.ref(name)
    tsdf, wsum, out_rgb = _scalar_ref(c)
    assert tsdf.tobytes() == c["tsdf"].tobytes() and wsum.tobytes() == c["wsum"].tobytes()
    if c["rgb"] is not None:
        assert np.array_equal(out_rgb, c["out_rgb"])
    else:
        assert c["out_rgb"] is None and c["mesh_rgb"] is None


def test_the_gate_cases_produce_every_gate():
    """Each way a (voxel, frame) pair can end, counted by the restatement; the numbers follow from the construction of the cases."""
    want = dict(behind=1170, uv_range=108, outside=435, weight=168, depth=98, max_depth=35, hidden=123, no_colour=101, used=320,
                tie=285, minus_half=18, at_front=35, at_back=54, clamped=101)
    got = tc.ref("gates-13x9x7")["reasons"]
    assert got == want
    # a pair ends exactly one way
    nx, ny, nz = tc.build("gates-13x9x7")["dims"]
    assert sum(got[k] for k in ("behind", "uv_range", "outside", "weight", "depth", "max_depth", "hidden", "used")) == 3 * nx * ny * nz
    assert got["behind"] >= nx * ny * nz + nx * ny                # the camera that looks away, and the layer Z = 0 of camera 0
    for name in tc.GATE_CASES:
        r = tc.ref(name)["reasons"]
        assert r["behind"] and r["outside"] and r["depth"] and r["max_depth"] and r["hidden"] and r["no_colour"] and r["used"], name
        assert r["tie"] and r["at_front"], name
    assert tc.ref("gates-33x17x5")["reasons"]["minus_half"] and tc.ref("gates-33x17x5")["reasons"]["uv_range"]
    assert tc.ref("gates-1x8x8")["reasons"]["at_back"]
    # the looking-away camera contributes nothing: two cameras give the result of one
    a, b = tc.ref("gates-13x9x7-1cam"), tc.ref("gates-13x9x7-2cam")
    assert a["tsdf"].tobytes() == b["tsdf"].tobytes() and a["wsum"].tobytes() == b["wsum"].tobytes()
    # non-finite inputs never reach an output
    for name in tc.GATE_CASES:
        r = tc.ref(name)
        assert np.isfinite(r["tsdf"]).all() and np.isfinite(r["wsum"]).all() and (r["wsum"] >= 0).all() and (np.abs(r["tsdf"]) <= 1).all()
    # mixed shapes share one padded array
    c = tc.build("gates-13x9x7")
    assert c["depth"].shape == (3, 768) and tc.cam_shapes(c["cams"]).tolist() == [[24, 32], [16, 20], [16, 20]]
    assert tc.ref("gates-1x8x8")["xyz"].shape == (0, 3) and tc.ref("gates-1x8x8")["faces"].shape == (0, 3)
    assert tc.ref("frames-260")["depth"].shape[0] == 260


def _pixel_depth_change(c):
    """The largest depth difference between two neighbouring pixels (8-neighbourhood) that both carry a surface and of which at
    least one is used: a voxel is compared with the depth of the nearest pixel, whose ray misses the voxel by up to half a pixel in
    each direction."""
    worst = 0.0
    for n, (h, w) in enumerate(tc.cam_shapes(c["cams"]).tolist()):
        d = c["depth"][n, :h * w].reshape(h, w).astype(np.float64)
        used = c["weight"][n, :h * w].reshape(h, w) > 0
        for dy, dx in ((0, 1), (1, 0), (1, 1), (1, -1)):
            a = (slice(0, h - dy), slice(max(0, -dx), w - max(0, dx)))
            b = (slice(dy, h), slice(max(0, dx), w - max(0, -dx)))
            pair = (d[a] > 0) & (d[b] > 0) & (used[a] | used[b])
            if pair.any():
                worst = max(worst, float(np.abs(d[a] - d[b])[pair].max()))
    return worst


@pytest.mark.parametrize("name", tc.SURFACE_CASES + ["sphere-noisy", "ragged-70x65x40", "gates-13x9x7"])
def test_every_face_names_three_distinct_vertices(name):
    c = tc.ref(name)
    V, f = len(c["xyz"]), c["faces"]
    assert V > 0 and len(f) > 0 and len(f) % 2 == 0
    assert f.min() >= 0 and f.max() < V
    assert (f[:, 0] != f[:, 1]).all() and (f[:, 1] != f[:, 2]).all() and (f[:, 0] != f[:, 2]).all()
    assert c["mesh_rgb"].shape == (V, 3) and np.isfinite(c["xyz"]).all()


def test_the_plane_is_found_where_it_is():
    c = tc.ref("plane")
    bound = math.sqrt(3) * c["voxel"] + _pixel_depth_change(c)
    dist = np.abs(c["xyz"][:, 2].astype(np.float64) - tc.PLANE_Z)
    print(f"plane: {len(c['xyz'])} vertices, {len(c['faces'])} faces, largest distance {dist.max():.3e}, bound {bound:.3e}")
    assert len(c["xyz"]) > 50 and len(c["faces"]) > 50
    assert dist.max() <= bound


def test_the_sphere_is_closed_and_lies_on_the_sphere():
    c = tc.ref("sphere")
    V, f = len(c["xyz"]), c["faces"].astype(np.int64)
    assert V > 1000 and len(f) > 2000
    e = np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])
    e.sort(1)
    _, shared = np.unique(e[:, 0] * V + e[:, 1], return_counts=True)
    assert (shared == 2).all()                                     # every edge lies between exactly two triangles
    assert V - len(shared) + len(f) == 2                           # one closed surface without handles
    # outward orientation: the signed volume is the ball's, within the discretisation
    p = c["xyz"].astype(np.float64) - tc.SPHERE_CENTRE
    volume = np.einsum("ij,ij->i", p[f[:, 0]], np.cross(p[f[:, 1]], p[f[:, 2]])).sum() / 6
    assert abs(abs(volume) - 4 / 3 * math.pi * tc.SPHERE_RADIUS ** 3) < 0.05 * 4 / 3 * math.pi * tc.SPHERE_RADIUS ** 3
    delta = _pixel_depth_change(c)
    bound = math.sqrt(3) * c["voxel"] + delta
    dist = np.abs(np.linalg.norm(p, axis=1) - tc.SPHERE_RADIUS)
    print(f"sphere: {V} vertices, {len(f)} faces, largest distance {dist.max():.3e}, depth change per pixel {delta:.3e}, bound {bound:.3e}")
    assert dist.max() <= bound


def test_cameras_table_and_argument_checks_raise_without_a_device():
    from align3r_amd import ops
    c = tc.build("gates-13x9x7")
    N = len(c["cams"])
    w2c = np.concatenate([c["cams"][:, :12].reshape(N, 3, 4), np.tile([[[0.0, 0, 0, 1]]], (N, 1, 1))], 1)
    K = np.zeros((N, 3, 3))
    K[:, 0, 0], K[:, 1, 1], K[:, 0, 2], K[:, 1, 2], K[:, 2, 2] = c["cams"][:, 12], c["cams"][:, 13], c["cams"][:, 14], c["cams"][:, 15], 1
    shapes = tc.cam_shapes(c["cams"])
    cams = ops.tsdf_cameras(w2c, K, shapes)
    assert cams.tobytes() == c["cams"].tobytes()
    assert ops.tsdf_cameras(torch.from_numpy(w2c[:, :3]), torch.from_numpy(K), shapes.tolist()).tobytes() == c["cams"].tobytes()
    skew, endless = K.copy(), w2c.copy()
    skew[1, 0, 1] = 0.1
    endless[2, 1, 3] = np.inf
    for bad, word in (((w2c.astype(np.float32), K, shapes), "float64"), ((w2c[:, :2], K, shapes), r"\[N,3,4\]"), ((w2c, K[:2], shapes), "K is"),
                      ((w2c, skew, shapes), "skew"), ((w2c, K, shapes[:2]), "shapes"), ((w2c, K, -shapes), "shapes"),
                      ((endless, K, shapes), "finite")):
        with pytest.raises(ValueError, match=word):
            ops.tsdf_cameras(*bad)

    depth, weight, rgb = torch.from_numpy(c["depth"]), torch.from_numpy(c["weight"]), torch.from_numpy(c["rgb"])
    good = dict(depth=depth, weight=weight, rgb=rgb, cams=cams, origin=c["origin"], dims=c["dims"], voxel=c["voxel"], trunc=c["trunc"])

    def refused(word, **change):
        with pytest.raises(ValueError, match=word):
            ops.tsdf_integrate(**{**good, **change})
    refused("voxel", voxel=0.0)
    refused("voxel", voxel=float("nan"))
    refused("trunc", trunc=-1.0)
    refused("near", near=0.0)
    refused("max_depth", max_depth=0.0)
    refused("origin", origin=(0.0, 1.0))
    refused("origin", origin=(0.0, 1.0, float("inf")))
    refused("dims", dims=(4, 0, 4))
    refused("dims", dims=(4, 4))
    refused("2\\^31", dims=(2048, 1024, 1024))
    refused("depth must be torch.float32", depth=depth.double())
    refused("depth must be a torch tensor", depth=c["depth"])
    refused("weight has shape", weight=weight[:, :-1])
    refused("rgb must be torch.uint8", rgb=rgb.float())
    refused("rgb has shape", rgb=rgb[..., :2])
    refused("weight must be contiguous", weight=weight.t().contiguous().t())
    refused("cams", cams=cams[:2])
    refused("cams", cams=cams.astype(np.float32))
    small = cams.copy()
    small[:, 16:].view(np.int32)[0] = (32, 32)
    refused("camera 0: h \\* w = 32 \\* 32", cams=small)
    nonfinite = cams.copy()
    nonfinite[1, 3] = np.nan
    refused("non-finite", cams=nonfinite)
    refused("on the device", )                     # everything is well-formed and on the CPU: the last check

    grid = torch.zeros((4, 5, 6))
    colours = torch.zeros((4, 5, 6, 3), dtype=torch.uint8)
    for word, args in (("min_weight", (grid, grid, colours, (0, 0, 0), 0.1, 0.0)), ("voxel", (grid, grid, colours, (0, 0, 0), -0.1, 1.0)),
                       ("wsum has shape", (grid, grid[:3], colours, (0, 0, 0), 0.1, 1.0)), ("rgb has shape", (grid, grid, colours[:3], (0, 0, 0), 0.1, 1.0)),
                       ("tsdf must be torch.float32", (grid.double(), grid, None, (0, 0, 0), 0.1, 1.0)), ("origin", (grid, grid, None, (0, 0), 0.1, 1.0)),
                       ("on the device", (grid, grid, None, (0, 0, 0), 0.1, 1.0))):
        with pytest.raises(ValueError, match=word):
            ops.tsdf_mesh(*args)
