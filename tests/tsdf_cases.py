"""Shared cases of the TSDF tests (csrc/tsdf.hip): tsdf_ref() and mesh_ref(), the numpy restatements of the definition in
include/a3r.h, and the case table.

The definition, float64 with every operation rounded on its own (numpy's element-wise products and sums are not fused):
    voxel (i, j, k): X = ox + (i + 0.5) * voxel (Y, Z likewise), arrays [nz, ny, nx]
    per frame n ascending: xc = (R00 X + R01 Y) + R02 Z + t0 (yc, zc likewise), u = fx (xc / zc) + cx, v = fy (yc / zc) + cy
      skipped unless zc >= near, |u|, |v| < 2^30, col = rint(u) in [0, w), row = rint(v) in [0, h)          (p = row * w + col)
      skipped unless d = depth[n, p] and wd = weight[n, p] are finite, wd > 0, d > 0, d <= max_depth
      sdf = d - zc; skipped if sdf < -trunc;  W += wd, S += wd * min(1, sdf / trunc)
      where sdf <= trunc and colours are given: Wc += wd, C += wd * rgb[n, p]
    tsdf = float32(S / W), 1 where W == 0; wsum = float32(W); out_rgb = min(rint(C / Wc), 255), 0 where Wc == 0
    surface nets: see mesh_ref

Cases (build(name) -> the inputs; ref(name) -> the inputs plus the restatement's outputs, computed once per process):
  gates-*   voxel 0.25 with voxel centres at multiples of 0.25, trunc 0.25, max_depth 4, three cameras of mixed shape in one padded
            array (P = 768): camera 0 (24 x 32, identity, fx = fy = 8, cx = 15.5) sees the plane z = 1 with bands of zero, negative, NaN
            and infinite weights and of zero, NaN, infinite, negative and too large depths -- its u is a half-pixel tie wherever
            8 X / Z is an integer, -0.5 and w - 0.5 included, the layer Z = 0.75 has sdf == trunc, Z = 1.25 has sdf == -trunc, Z = 1.5 is
            hidden, Z = 0 is behind the camera; camera 1 (16 x 20) looks away: every voxel is behind it; camera 2 (16 x 20) stands
            2e-9 in front of the layer Z = 0.5 (near = 1e-9), whose voxels project beyond 2^30, and sees a random depth map.
            Ragged dims (13, 9, 7), (33, 17, 5) and (1, 8, 8) -- the last has no cells; -norgb: rgb = None; -1cam, -2cam: fewer cameras.
  frames-260  260 frames of 4 x 6 pixels around a (13, 9, 7) grid: more frames than a workgroup has threads.
  plane     one camera in front of the plane z = 1.03 (fronto-parallel), voxel 0.05, trunc 0.15.
  sphere    a sphere of radius 20 voxels inside a 48^3 grid seen by six cameras of 96 x 96 pixels on the axes at 20 radii; a pixel
            has weight 1 where the ray meets the surface at cos >= 0.35 to the normal, else 0.  Why these numbers: a surface point
            whose normal is 54.7 degrees off every axis is met at up to 57.3 degrees; a voxel sqrt(3) voxels above it is seen on a
            pixel whose own surface point lies 8 degrees further out, still above the threshold, so every corner of a surface cell is
            observed; and a ray above the threshold runs 0.7 radii = 14 voxels through the ball, more than trunc = 5 voxels, so no
            voxel behind the ball counts as inside.
  sphere-noisy  a (44, 46, 45) grid, 0.2 % depth noise, random weights and a seventh camera: many frames per voxel, the order of
            the sums matters.
  ragged-70x65x40  a 70 x 65 x 40 grid whose lowest slices cut the sphere, three cameras: several workgroups in every direction, more than one
            scan chunk, bricks outside every camera's view.
"""
import functools

import numpy as np

EDGES = [(0, 1), (0, 2), (0, 4), (1, 3), (1, 5), (2, 3), (2, 6), (3, 7), (4, 5), (4, 6), (5, 7), (6, 7)]
LIM = float(1 << 30)

GATE_CASES = ["gates-13x9x7", "gates-33x17x5", "gates-1x8x8", "gates-13x9x7-norgb", "gates-13x9x7-1cam", "gates-13x9x7-2cam"]
SURFACE_CASES = ["plane", "sphere"]
CASES = GATE_CASES + ["frames-260"] + SURFACE_CASES + ["sphere-noisy", "ragged-70x65x40"]


# ------------------------------------------------------------------------------------------------- the restatement
def make_cams(w2c, K, shapes):
    """[N,17] float64: w2c[:, :3, :4] row-major, fx, fy, cx, cy and (h, w) as two int32 in the last column (a3r_tsdf_cam)."""
    w2c, K = np.asarray(w2c, np.float64), np.asarray(K, np.float64)
    N = len(w2c)
    cams = np.zeros((N, 17))
    cams[:, :12] = w2c[:, :3, :].reshape(N, 12)
    cams[:, 12], cams[:, 13], cams[:, 14], cams[:, 15] = K[:, 0, 0], K[:, 1, 1], K[:, 0, 2], K[:, 1, 2]
    cams[:, 16:].view(np.int32)[:] = np.asarray(shapes, np.int32)
    return cams


def cam_shapes(cams):
    return np.ascontiguousarray(cams)[:, 16:].view(np.int32).copy()


def voxel_centres(origin, dims, voxel):
    """X, Y, Z float64 [nz, ny, nx]."""
    nx, ny, nz = dims
    voxel = np.float64(voxel)
    x = np.float64(origin[0]) + (np.arange(nx, dtype=np.float64) + 0.5) * voxel
    y = np.float64(origin[1]) + (np.arange(ny, dtype=np.float64) + 0.5) * voxel
    z = np.float64(origin[2]) + (np.arange(nz, dtype=np.float64) + 0.5) * voxel
    Z, Y, X = np.meshgrid(z, y, x, indexing="ij")
    return X, Y, Z


def tsdf_ref(depth, weight, rgb, cams, origin, dims, voxel, trunc, near=1e-6, max_depth=np.inf, reasons=None):
    """The integration: a loop over the frames, vectorised over the voxels.  Returns tsdf, wsum [nz,ny,nx] float32 and out_rgb
    [nz,ny,nx,3] uint8 (None without rgb).  reasons: a dict that receives the number of (voxel, frame) pairs by outcome."""
    depth, weight = np.asarray(depth, np.float32), np.asarray(weight, np.float32)
    N, P = depth.shape
    X, Y, Z = voxel_centres(origin, dims, voxel)
    trunc, near, max_depth = np.float64(trunc), np.float64(near), np.float64(max_depth)
    W, S, Wc = np.zeros(X.shape), np.zeros(X.shape), np.zeros(X.shape)
    C = np.zeros(X.shape + (3,))
    count = dict(behind=0, uv_range=0, outside=0, weight=0, depth=0, max_depth=0, hidden=0, no_colour=0, used=0, tie=0, minus_half=0,
                 at_front=0, at_back=0, clamped=0)
    shapes = cam_shapes(cams)
    with np.errstate(all="ignore"):
        for n in range(N):
            R = cams[n]
            fx, fy, cx, cy = R[12], R[13], R[14], R[15]
            h, w = int(shapes[n, 0]), int(shapes[n, 1])
            xc = (R[0] * X + R[1] * Y) + R[2] * Z + R[3]
            yc = (R[4] * X + R[5] * Y) + R[6] * Z + R[7]
            zc = (R[8] * X + R[9] * Y) + R[10] * Z + R[11]
            u = fx * (xc / zc) + cx
            v = fy * (yc / zc) + cy
            front = zc >= near
            ranged = front & (np.abs(u) < LIM) & (np.abs(v) < LIM)
            col, row = np.rint(u), np.rint(v)
            inside = ranged & (col >= 0) & (col < w) & (row >= 0) & (row < h)
            p = np.where(inside, row * w + col, 0).astype(np.int64)
            d, wd = depth[n][p].astype(np.float64), weight[n][p].astype(np.float64)
            w_ok = inside & np.isfinite(wd) & (wd > 0)
            d_ok = w_ok & np.isfinite(d) & (d > 0)
            near_enough = d_ok & (d <= max_depth)
            sdf = d - zc
            use = near_enough & ~(sdf < -trunc)
            t = np.minimum(1.0, sdf / trunc)
            W = np.where(use, W + wd, W)
            S = np.where(use, S + wd * t, S)
            paint = use & (sdf <= trunc)
            if rgb is not None:
                Wc = np.where(paint, Wc + wd, Wc)
                C = np.where(paint[..., None], C + wd[..., None] * rgb[n][p].astype(np.float64), C)
            for key, a, b in (("behind", ~front, None), ("uv_range", front, ~ranged), ("outside", ranged, ~inside),
                              ("weight", inside, ~w_ok), ("depth", w_ok, ~d_ok), ("max_depth", d_ok, ~near_enough),
                              ("hidden", near_enough, ~use), ("no_colour", use, ~paint), ("used", use, None),
                              ("tie", inside, np.abs(u - np.floor(u)) == 0.5), ("minus_half", inside, u == -0.5),
                              ("at_front", use, sdf == trunc), ("at_back", use, sdf == -trunc), ("clamped", use, sdf > trunc)):
                count[key] += int((a if b is None else a & b).sum())
        tsdf = np.where(W == 0, 1.0, S / W).astype(np.float32)
        wsum = W.astype(np.float32)
        out_rgb = None
        if rgb is not None:
            out_rgb = np.where(Wc[..., None] == 0, 0.0, np.minimum(np.rint(C / Wc[..., None]), 255.0)).astype(np.uint8)
    if reasons is not None:
        reasons.update(count)
    return tsdf, wsum, out_rgb


def mesh_ref(tsdf, wsum, rgb, origin, voxel, min_weight):
    """The surface: xyz [V,3] float32, rgb [V,3] uint8 (None without rgb), faces [F,3] int32."""
    tsdf, wsum = np.asarray(tsdf, np.float32), np.asarray(wsum, np.float32)
    nz, ny, nx = tsdf.shape
    empty = (np.zeros((0, 3), np.float32), None if rgb is None else np.zeros((0, 3), np.uint8), np.zeros((0, 3), np.int32))
    if min(nx, ny, nz) < 2:
        return empty
    observed = wsum.astype(np.float64) >= np.float64(min_weight)
    inside = tsdf < 0
    corner = lambda a, c: a[(c >> 2):nz - 1 + (c >> 2), ((c >> 1) & 1):ny - 1 + ((c >> 1) & 1), (c & 1):nx - 1 + (c & 1)]
    all_obs = functools.reduce(np.logical_and, [corner(observed, c) for c in range(8)])
    any_in = functools.reduce(np.logical_or, [corner(inside, c) for c in range(8)])
    any_out = functools.reduce(np.logical_or, [~corner(inside, c) for c in range(8)])
    active = all_obs & any_in & any_out                                     # [nz-1, ny-1, nx-1]
    kk, jj, ii = np.nonzero(active)                                         # the order of (k, j, i): the cells' linear order
    V = len(kk)
    if V == 0:
        return empty
    f = [corner(tsdf, c)[active].astype(np.float64) for c in range(8)]
    total, cnt = np.zeros((V, 3)), np.zeros(V)
    with np.errstate(all="ignore"):
        for a, b in EDGES:
            cross = (f[a] < 0) != (f[b] < 0)
            s = f[a] / (f[a] - f[b])
            for ax in range(3):
                da, db = float((a >> ax) & 1), float((b >> ax) & 1)
                total[:, ax] = np.where(cross, total[:, ax] + (da + s * (db - da)), total[:, ax])
            cnt += cross
        m = total / cnt[:, None]
    voxel = np.float64(voxel)
    xyz = np.stack([np.float64(origin[0]) + ((ii.astype(np.float64) + 0.5) + m[:, 0]) * voxel,
                    np.float64(origin[1]) + ((jj.astype(np.float64) + 0.5) + m[:, 1]) * voxel,
                    np.float64(origin[2]) + ((kk.astype(np.float64) + 0.5) + m[:, 2]) * voxel], 1).astype(np.float32)
    out_rgb = None
    if rgb is not None:
        total_c = sum(corner(rgb.astype(np.int64), c)[active] for c in range(8))        # [V, 3]
        out_rgb = ((2 * total_c + 8) // 16).astype(np.uint8)
    # vertex ids on the voxel grid's linear index (-1: no vertex)
    nvox = nx * ny * nz
    vid = np.full(nvox, -1, np.int64)
    vid[(kk * ny + jj) * nx + ii] = np.arange(V)
    ins, n, step = inside.reshape(-1), (nx, ny, nz), (1, nx, nx * ny)
    lin = np.arange(nvox)
    g = (lin % nx, (lin // nx) % ny, lin // (nx * ny))
    keys, tris = [], []
    for a in range(3):
        b, c = (a + 1) % 3, (a + 2) % 3
        ok = (g[a] + 1 < n[a]) & (g[b] >= 1) & (g[b] <= n[b] - 2) & (g[c] >= 1) & (g[c] <= n[c] - 2)
        l = lin[ok]
        l = l[ins[l] != ins[l + step[a]]]
        q = np.stack([vid[l - step[b] - step[c]], vid[l - step[c]], vid[l], vid[l - step[b]]], 1)
        keep = (q >= 0).all(1)
        l, q = l[keep], q[keep]
        flip = ~ins[l]
        t1 = np.where(flip[:, None], q[:, [0, 2, 1]], q[:, [0, 1, 2]])
        t2 = np.where(flip[:, None], q[:, [0, 3, 2]], q[:, [0, 2, 3]])
        keys.append(l * 3 + a)
        tris.append(np.stack([t1, t2], 1))                                  # [n, 2, 3]
    keys, tris = np.concatenate(keys), np.concatenate(tris)
    faces = tris[np.argsort(keys, kind="stable")].reshape(-1, 3).astype(np.int32)
    return xyz, out_rgb, faces


# ------------------------------------------------------------------------------------------------- scenes
def look_at(eye, target, up=(0.0, 1.0, 0.0)):
    """World-to-camera [3,4] of a camera at `eye` whose +z axis points at `target`."""
    eye, target = np.asarray(eye, np.float64), np.asarray(target, np.float64)
    z = target - eye
    z /= np.linalg.norm(z)
    up = np.asarray(up, np.float64)
    if abs(np.dot(up, z)) > 0.9:
        up = np.array([1.0, 0.0, 0.0])
    x = np.cross(up, z)
    x /= np.linalg.norm(x)
    y = np.cross(z, x)
    R = np.stack([x, y, z])
    return np.concatenate([R, (-R @ eye)[:, None]], 1)


def pixel_rays(w2c, K, h, w):
    """(camera centre [3], world directions [h*w,3] with unit camera-z component)."""
    R, t = w2c[:, :3], w2c[:, 3]
    col, row = np.meshgrid(np.arange(w, dtype=np.float64), np.arange(h, dtype=np.float64))
    d_cam = np.stack([(col - K[0, 2]) / K[0, 0], (row - K[1, 2]) / K[1, 1], np.ones_like(col)], -1).reshape(-1, 3)
    return -R.T @ t, d_cam @ R


def sphere_depth(w2c, K, h, w, centre, radius):
    """Depth (camera z) of the sphere's near surface per pixel, 0 where the ray misses; cos of the angle between ray and normal."""
    o, d = pixel_rays(w2c, K, h, w)
    oc = o - centre
    a, b, c = (d * d).sum(1), 2 * d @ oc, oc @ oc - radius * radius
    disc = b * b - 4 * a * c
    hit = disc > 0
    z = np.where(hit, (-b - np.sqrt(np.where(hit, disc, 0.0))) / (2 * a), 0.0)
    hit &= z > 0
    normal = (o + z[:, None] * d - centre) / radius
    cos = -(normal * d).sum(1) / np.sqrt(a)
    return np.where(hit, z, 0.0), np.where(hit, cos, 0.0)


def _pad(maps, P, dtype, tail=()):
    out = np.zeros((len(maps), P) + tail, dtype)
    for n, m in enumerate(maps):
        m = np.asarray(m).reshape((-1,) + tail)
        out[n, :len(m)] = m
    return out


def _gates(dims, n_cams=3, colour=True, seed=0):
    nx, ny, nz = dims
    g = np.random.default_rng(seed)
    voxel, trunc = 0.25, 0.25
    origin = (-0.125 - 0.25 * (nx // 2), -0.125 - 0.25 * (ny // 2), -0.125)      # centres at multiples of 0.25, Z from 0
    shapes = [(24, 32), (16, 20), (16, 20)][:n_cams]
    P = 768
    eye = np.concatenate([np.eye(3), np.zeros((3, 1))], 1)
    away = np.concatenate([np.diag([-1.0, 1.0, -1.0]), np.zeros((3, 1))], 1)
    close = eye.copy()
    close[2, 3] = -(0.5 - 2e-9)
    w2c = np.stack([eye, away, close])[:n_cams]
    K = np.zeros((3, 3, 3))
    K[:, 2, 2] = 1
    K[0, 0, 0], K[0, 1, 1], K[0, 0, 2], K[0, 1, 2] = 8.0, 8.0, 15.5, 11.25
    K[1, 0, 0], K[1, 1, 1], K[1, 0, 2], K[1, 1, 2] = 9.0, 9.5, 10.0, 8.0
    K[2, 0, 0], K[2, 1, 1], K[2, 0, 2], K[2, 1, 2] = 6.5, 7.25, 9.75, 7.6
    d0, w0 = np.ones((24, 32), np.float32), np.ones((24, 32), np.float32)
    w0[:, 0:3], w0[:, 3:6], w0[:, 6:9], w0[:, 9:12] = 0.0, -1.0, np.nan, np.inf
    d0[0:3], d0[3:6], d0[6:8], d0[8:10], d0[20:22] = 0.0, np.nan, np.inf, 5.0, -1.0
    depths = [d0, g.uniform(0.5, 2.0, (16, 20)).astype(np.float32), g.uniform(0.2, 1.5, (16, 20)).astype(np.float32)][:n_cams]
    weights = [w0, g.uniform(0.5, 2.0, (16, 20)).astype(np.float32), g.uniform(0.5, 2.0, (16, 20)).astype(np.float32)][:n_cams]
    rgb = [g.integers(0, 256, s + (3,), dtype=np.uint8) for s in shapes]
    return dict(depth=_pad(depths, P, np.float32), weight=_pad(weights, P, np.float32), rgb=_pad(rgb, P, np.uint8, (3,)) if colour else None,
                cams=make_cams(w2c, K[:n_cams], shapes), origin=origin, dims=dims, voxel=voxel, trunc=trunc, near=1e-9, max_depth=4.0,
                min_weight=0.5)


def _frames(n_frames, dims, seed=1):
    nx, ny, nz = dims
    g = np.random.default_rng(seed)
    voxel = 0.1
    centre = np.array([0.05, -0.02, 0.4])
    origin = tuple(centre - 0.5 * voxel * np.array(dims))
    h, w = 4, 6
    w2c, K = [], []
    for n in range(n_frames):
        ang = 2 * np.pi * n / n_frames
        eye = centre + np.array([1.5 * np.cos(ang), 0.4 * np.sin(3 * ang), 1.5 * np.sin(ang)])
        w2c.append(look_at(eye, centre + 0.1 * g.standard_normal(3)))
        K.append(np.array([[3.0 + g.random(), 0, 2.5 + 0.3 * g.random()], [0, 3.0 + g.random(), 1.5 + 0.3 * g.random()], [0, 0, 1]]))
    depth = g.uniform(1.2, 1.8, (n_frames, h * w)).astype(np.float32)
    weight = g.uniform(0.1, 3.0, (n_frames, h * w)).astype(np.float32)
    weight[g.random((n_frames, h * w)) < 0.2] = 0
    rgb = g.integers(0, 256, (n_frames, h * w, 3), dtype=np.uint8)
    return dict(depth=depth, weight=weight, rgb=rgb, cams=make_cams(np.stack(w2c), np.stack(K), [(h, w)] * n_frames), origin=origin,
                dims=dims, voxel=voxel, trunc=0.3, near=1e-6, max_depth=np.inf, min_weight=0.1)


PLANE_Z = 1.03


def _plane():
    voxel, h, w = 0.05, 24, 32
    K = np.array([[40.0, 0, 15.5], [0, 40.0, 11.5], [0, 0, 1]])
    w2c = np.concatenate([np.eye(3), np.zeros((3, 1))], 1)
    g = np.random.default_rng(2)
    depth = np.full((1, h * w), PLANE_Z, np.float32)
    return dict(depth=depth, weight=np.ones((1, h * w), np.float32), rgb=g.integers(0, 256, (1, h * w, 3), dtype=np.uint8),
                cams=make_cams(w2c[None], K[None], [(h, w)]), origin=(-0.3, -0.25, 0.7), dims=(12, 10, 13), voxel=voxel, trunc=0.15,
                near=1e-6, max_depth=np.inf, min_weight=1.0)


SPHERE_CENTRE = np.array([0.011, -0.007, 0.004])
SPHERE_RADIUS = 1.0                 # 20 voxels
SPHERE_DIST = 20.0                  # the cameras' distance from the centre: rays within 3 degrees of parallel
SPHERE_COS = 0.35


def _sphere(dims=(48, 48, 48), offset=(0.0, 0.0, 0.0), eyes=None, focal=800.0, noise=0.0, seed=3):
    voxel, h, w = 0.05, 96, 96
    centre, radius = SPHERE_CENTRE, SPHERE_RADIUS
    g = np.random.default_rng(seed)
    origin = tuple(centre - 0.5 * voxel * np.array(dims) + np.asarray(offset) + 0.013)     # the sphere's centre is no voxel's centre
    if eyes is None:
        eyes = [s * SPHERE_DIST * np.eye(3)[a] for a in range(3) for s in (1, -1)]
    K = np.array([[focal, 0, 47.5], [0, focal, 47.5], [0, 0, 1]])
    w2c, depth, weight = [], [], []
    for e in eyes:
        m = look_at(centre + e, centre)
        z, cos = sphere_depth(m, K, h, w, centre, radius)
        wt = (cos >= SPHERE_COS).astype(np.float32)
        if noise:
            z = z * (1 + noise * g.standard_normal(z.shape))
            wt = wt * g.uniform(0.5, 4.0, wt.shape).astype(np.float32)
        w2c.append(m); depth.append(z.astype(np.float32)); weight.append(wt)
    N = len(eyes)
    rgb = g.integers(0, 256, (N, h * w, 3), dtype=np.uint8)
    return dict(depth=np.stack(depth), weight=np.stack(weight), rgb=rgb, cams=make_cams(np.stack(w2c), np.stack([K] * N), [(h, w)] * N),
                origin=origin, dims=dims, voxel=voxel, trunc=5 * voxel, near=1e-6, max_depth=np.inf,
                min_weight=0.5 if noise else 1.0)


@functools.lru_cache(maxsize=None)
def build(name):
    if name.startswith("gates-"):
        parts = name.split("-")
        dims = tuple(int(n) for n in parts[1].split("x"))
        opt = parts[2] if len(parts) > 2 else ""
        return _gates(dims, n_cams={"1cam": 1, "2cam": 2}.get(opt, 3), colour=opt != "norgb")
    if name == "frames-260":
        return _frames(260, (13, 9, 7))
    if name == "plane":
        return _plane()
    if name == "sphere":
        return _sphere()
    if name == "sphere-noisy":
        six = [s * SPHERE_DIST * np.eye(3)[a] for a in range(3) for s in (1, -1)]
        return _sphere(dims=(44, 46, 45), eyes=six + [SPHERE_DIST * np.array([0.6, 0.5, -0.62])], noise=0.002, seed=4)
    if name == "ragged-70x65x40":
        r = 6 * SPHERE_RADIUS
        return _sphere(dims=(70, 65, 40), offset=(0.5, -0.4, 0.8), eyes=[r * np.array([0.0, 0.0, 1.0]), r * np.array([0.8, 0.1, 0.59]),
                                                                            r * np.array([-0.3, 0.9, 0.3])], focal=150.0, noise=0.002, seed=5)
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def ref(name):
    """build(name) plus reasons, tsdf, wsum, out_rgb and the mesh xyz, mesh_rgb, faces of the restatement."""
    c = dict(build(name))
    c["reasons"] = {}
    c["tsdf"], c["wsum"], c["out_rgb"] = tsdf_ref(c["depth"], c["weight"], c["rgb"], c["cams"], c["origin"], c["dims"], c["voxel"],
                                                  c["trunc"], c["near"], c["max_depth"], reasons=c["reasons"])
    c["xyz"], c["mesh_rgb"], c["faces"] = mesh_ref(c["tsdf"], c["wsum"], c["out_rgb"], c["origin"], c["voxel"], c["min_weight"])
    return c
