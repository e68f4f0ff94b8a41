"""Shared cases of the rendering tests (csrc/render.hip): render_ref(), the numpy restatement of the definition in include/a3r.h, the
clouds and cameras by kind, and the sizes.

The definition, per camera (w2c [3,4] float64 row-major, fx, fy, cx, cy float64) and point m = (x, y, z) float32, on float64 copies,
every operation rounded on its own:
    xc = (R00*x + R01*y) + R02*z + t0  (yc, zc likewise);  u = fx * (xc / zc) + cx;  v = fy * (yc / zc) + cy;  zf = float32(zc)
    drawn iff zc >= near, zf finite, u and v finite, |u|, |v| < 2^30
    col = int(rint(u)), row = int(rint(v)) (half to even); footprint = pixels (row + dy, col + dx), |dx|, |dy| <= radius, inside the image
    key = (bits(zf) << 32) | m;  a pixel's result = the minimum key (np.minimum.at on uint64)
    depth = zf of the winner or 0;  index = its m or -1;  rgb = rgb_in[m] or background

Kinds (every kind gives (xyz [M,3] float32, cams [C,16] float64) for (M, H, W, C, radius)):
  surface  the height field of match_cases.cloud('surface'), seen by cameras a little off the origin whose field of view is wider
           than the cloud: most points are drawn, the border stays empty, and with M above the pixel count pixels collect many points
  pile     every point on one ray of camera 0 (x = y = 0), depths drawn from four values: thousands of exact depth ties on one pixel,
           the lowest index must win under full contention
  halfpix  fx, fy, cx, cy powers of two (or halves) and dyadic coordinates at z = 1, identity pose: u and v land exactly on k + 0.5,
           including u = -0.5 (rounds to -0: column 0) and u = W - 0.5 (rounds to W or W - 1 by parity) -- pins half-to-even
           against floor(x + 0.5)
  edge     points within radius + 1 pixels of all four borders, inside and outside: the footprints clip
  hostile  NaN and +-inf coordinates, zc negative, zc == near exactly, zc one ulp below near, coordinates of 1e30 (u beyond 2^30)
           and of 1e-30, zc above FLT_MAX (the cameras' [R|t] is [2 I | t], so zc = 2 z exactly) -- mixed into a surface cloud so
           that the picture is not empty
"""
import functools

import numpy as np

import match_cases as mc

KINDS = ("surface", "pile", "halfpix", "edge", "hostile")
SIZES = [1, 63, 65, 1000, 8193, 70001]
IMAGES = [(1, 1), (3, 5), (48, 64), (96, 128)]
CAMS = [1, 3]
RADII = [0, 1, 3, 8]
NEAR = 0.25                   # a power of two: the hostile kind places zc exactly on it
BACKGROUND = (7, 200, 31)

# (kind, M, (H, W), C, radius): every kind at every size and every radius; image sizes and camera counts cycle with them so that
# each image size and each camera count meets each kind
CASES = []
for _k, _kind in enumerate(KINDS):
    for _s, _M in enumerate(SIZES):
        for _r, _radius in enumerate(RADII):
            _img = IMAGES[(_k + _s + _r) % len(IMAGES)]
            if (_M >= 8193 and _radius == 8) or (_kind == "surface" and _M >= 1000):
                # big footprints of big clouds stay on the big pictures (the restatement's time); the big surface cases keep an
                # empty border (tests/test_render_cpu.py asserts it)
                _img = IMAGES[2 + ((_s + _r) % 2)]
            CASES.append((_kind, _M, _img, CAMS[(_s + _r) % 2], _radius))


def case_id(case):
    kind, M, (H, W), C, radius = case
    return f"{kind}-M{M}-{H}x{W}-C{C}-r{radius}"


def make_cams(w2c, fx, fy, cx, cy):
    """[C,16] float64: 12 entries of [R|t] row-major, then fx, fy, cx, cy (a3r_render_cam)."""
    w2c = np.asarray(w2c, np.float64)
    C = len(w2c)
    cams = np.empty((C, 16), np.float64)
    cams[:, :12] = w2c[:, :3, :4].reshape(C, 12)
    for k, a in enumerate((fx, fy, cx, cy)):
        cams[:, 12 + k] = np.broadcast_to(np.asarray(a, np.float64), (C,))
    return cams


def project(xyz, cam, near):
    """One camera [16] on all points: (ok [M] bool = the point may draw, row [M], col [M] int64 (0 where not ok), zf [M] float32)."""
    xyz = np.asarray(xyz, np.float32).reshape(-1, 3)
    x, y, z = (xyz[:, k].astype(np.float64) for k in range(3))
    R, (fx, fy, cx, cy) = cam[:12], cam[12:]
    with np.errstate(all="ignore"):
        xc = (R[0] * x + R[1] * y) + R[2] * z + R[3]
        yc = (R[4] * x + R[5] * y) + R[6] * z + R[7]
        zc = (R[8] * x + R[9] * y) + R[10] * z + R[11]
        u = fx * (xc / zc) + cx
        v = fy * (yc / zc) + cy
        zf = zc.astype(np.float32)
        ok = (zc >= near) & np.isfinite(zf) & np.isfinite(u) & np.isfinite(v) & (np.abs(u) < 2.0 ** 30) & (np.abs(v) < 2.0 ** 30)
        col = np.rint(np.where(ok, u, 0)).astype(np.int64)
        row = np.rint(np.where(ok, v, 0)).astype(np.int64)
    return ok, row, col, zf


def render_ref(xyz, rgb, cams, H, W, radius, near, background=BACKGROUND, ids=None):
    """The restatement: (depth [C,H,W] float32, index [C,H,W] int32, rgb [C,H,W,3] uint8 or None when rgb is None).  ids: the index
    each point carries into its key and into `index` (default: its row; rgb is looked up by the carried index)."""
    xyz = np.asarray(xyz, np.float32).reshape(-1, 3)
    cams = np.asarray(cams, np.float64).reshape(-1, 16)
    M, C = len(xyz), len(cams)
    m = np.arange(M, dtype=np.uint64) if ids is None else np.asarray(ids).astype(np.uint64)
    empty = np.uint64(0xFFFFFFFFFFFFFFFF)
    keys = np.full((C, H * W), empty, np.uint64)
    with np.errstate(all="ignore"):
        for c in range(C):
            ok, row, col, zf = project(xyz, cams[c], near)
            row, col = row[ok], col[ok]
            key = (zf[ok].view(np.uint32).astype(np.uint64) << np.uint64(32)) | m[ok]
            for dy in range(-radius, radius + 1):
                for dx in range(-radius, radius + 1):
                    r, q = row + dy, col + dx
                    inside = (r >= 0) & (r < H) & (q >= 0) & (q < W)
                    np.minimum.at(keys[c], r[inside] * W + q[inside], key[inside])
    hit = keys != empty
    depth = np.where(hit, (keys >> np.uint64(32)).astype(np.uint32).view(np.float32), np.float32(0)).astype(np.float32)
    index = np.where(hit, (keys & np.uint64(0xFFFFFFFF)).astype(np.int64), -1).astype(np.int32)
    out_rgb = None
    if rgb is not None:
        rgb = np.asarray(rgb, np.uint8).reshape(-1, 3)
        out_rgb = np.empty((C, H * W, 3), np.uint8)
        out_rgb[:] = np.asarray(background, np.uint8)
        out_rgb[hit] = rgb[index[hit]]
        out_rgb = out_rgb.reshape(C, H, W, 3)
    return depth.reshape(C, H, W), index.reshape(C, H, W), out_rgb


def render_naive(xyz, rgb, cams, H, W, radius, near, background=BACKGROUND):
    """The definition once more as a per-point Python loop with a plain comparison per pixel (the checker of render_ref on the
    smallest sizes)."""
    xyz = np.asarray(xyz, np.float32).reshape(-1, 3)
    cams = np.asarray(cams, np.float64).reshape(-1, 16)
    C = len(cams)
    depth, index = np.zeros((C, H, W), np.float32), np.full((C, H, W), -1, np.int32)
    col_out = np.empty((C, H, W, 3), np.uint8)
    col_out[:] = np.asarray(background, np.uint8)
    with np.errstate(all="ignore"):
        for c in range(C):
            R = cams[c]
            for m, p in enumerate(xyz):
                x, y, z = (np.float64(a) for a in p)
                xc = (R[0] * x + R[1] * y) + R[2] * z + R[3]
                yc = (R[4] * x + R[5] * y) + R[6] * z + R[7]
                zc = (R[8] * x + R[9] * y) + R[10] * z + R[11]
                u, v, zf = R[12] * (xc / zc) + R[14], R[13] * (yc / zc) + R[15], np.float32(zc)
                if not (zc >= near and np.isfinite(zf) and np.isfinite(u) and np.isfinite(v) and abs(u) < 2.0 ** 30 and abs(v) < 2.0 ** 30):
                    continue
                q0, r0 = int(np.rint(u)), int(np.rint(v))
                for r in range(max(r0 - radius, 0), min(r0 + radius, H - 1) + 1):
                    for q in range(max(q0 - radius, 0), min(q0 + radius, W - 1) + 1):
                        if index[c, r, q] < 0 or zf < depth[c, r, q]:        # ascending m: an equal depth keeps the earlier point
                            depth[c, r, q], index[c, r, q] = zf, m
                            if rgb is not None:
                                col_out[c, r, q] = rgb[m]
    return depth, index, (col_out if rgb is not None else None)


def _rot(ax, ay):
    cx_, sx, cy_, sy = np.cos(ax), np.sin(ax), np.cos(ay), np.sin(ay)
    return np.array([[1, 0, 0], [0, cx_, -sx], [0, sx, cx_]]) @ np.array([[cy_, 0, sy], [0, 1, 0], [-sy, 0, cy_]])


def near_origin_cams(C, H, W, seed, fov_scale=0.25):
    """Cameras a little off the origin looking down +z.  The surface cloud spans |x / z|, |y / z| <= 1; a focal of fov_scale * size
    puts it into the middle half of the picture: a border of a quarter of the size (12 pixels of 48) stays empty, at radius 8 too."""
    g = np.random.default_rng(seed)
    w2c = np.zeros((C, 3, 4))
    for c in range(C):
        w2c[c, :, :3] = _rot(*(0.03 * g.standard_normal(2)))
        w2c[c, :, 3] = 0.05 * g.standard_normal(3)
    return make_cams(w2c, fov_scale * W, fov_scale * H, W / 2 - 0.25, H / 2 + 0.125)


def colours(M, seed=3):
    return np.random.default_rng(seed).integers(0, 256, (M, 3), dtype=np.uint8)


def scene(kind, M, H, W, C, radius):
    """(xyz [M,3] float32, cams [C,16] float64) of a case."""
    g = np.random.default_rng(1000 + M + 7 * H + radius)
    if kind == "surface":
        return mc.cloud("surface", M, 21), near_origin_cams(C, H, W, 5)
    if kind == "pile":
        depths = np.array([1.0, 1.5, 1.5000001, 3.0], np.float32)             # two of them neighbours in fp32
        xyz = np.zeros((M, 3), np.float32)
        xyz[:, 2] = depths[g.integers(0, 4, M)]
        w2c = np.zeros((C, 3, 4))
        w2c[:, :, :3] = np.eye(3)
        w2c[1:, 0, 3] = 0.125 * np.arange(1, C)                               # the other cameras see the ray from the side
        return xyz, make_cams(w2c, float(W), float(H), W // 2, H // 2)
    if kind == "halfpix":
        # identity pose, z = 1 or 2, f = 8: u = 8 * (x / z) + cx with x a multiple of 1/16 at z = 1 (1/8 at z = 2): u is k / 2 exactly
        k = g.integers(-3, 2 * W + 4, M)                                       # u = k / 2 - 0.5 ... includes -0.5 and W - 0.5
        l = g.integers(-3, 2 * H + 4, M)
        k[:4], l[:4] = [0, 2 * W, 0, 2 * W][:min(4, M)], [0, 0, 2 * H, 2 * H][:min(4, M)]   # the four corners at -0.5 / size - 0.5
        z = g.choice([1.0, 2.0], M)
        xyz = np.stack([(k / 2 - 0.5 - W / 2) / 8 * z, (l / 2 - 0.5 - H / 2) / 8 * z, z], 1).astype(np.float32)
        assert np.array_equal(xyz[:, 0].astype(np.float64) / z * 8 + W / 2, k / 2 - 0.5)      # exact in fp32 and in the projection
        w2c = np.zeros((C, 3, 4))
        w2c[:, :, :3] = np.eye(3)
        w2c[1:, 0, 3] = 0.0625 * np.arange(1, C)                               # shifts u by half a pixel per camera at z = 1
        return xyz, make_cams(w2c, 8.0, 8.0, W / 2, H / 2)
    if kind == "edge":
        # pixel targets within radius + 1 of a border, on either side of it
        side = g.integers(0, 4, M)
        off = g.uniform(-(radius + 1), radius + 1, M)
        along_w, along_h = g.uniform(-1, W, M), g.uniform(-1, H, M)
        u = np.where(side == 0, off, np.where(side == 1, W - 1 + off, along_w))
        v = np.where(side == 2, off, np.where(side == 3, H - 1 + off, along_h))
        z = g.uniform(1, 3, M)
        f = 0.8 * max(H, W)
        xyz = np.stack([(u - W / 2) / f * z, (v - H / 2) / f * z, z], 1).astype(np.float32)
        w2c = np.zeros((C, 3, 4))
        w2c[:, :, :3] = np.eye(3)
        w2c[1:, 1, 3] = 0.01 * np.arange(1, C)
        return xyz, make_cams(w2c, f, f, W / 2, H / 2)
    if kind == "hostile":
        xyz = mc.cloud("surface", M, 22).copy()
        cams = near_origin_cams(C, H, W, 6)
        # [R|t] = [2 I | (0.01 c, 0, 0)]: zc = 2 z exactly, so z = 3.4e38 gives a zc above FLT_MAX (finite in float64, zf = +inf),
        # z = NEAR / 2 a zc on the near plane and the fp32 value below NEAR / 2 a zc one (fp32) ulp below it
        cams[:, :12] = 0
        cams[:, [0, 5, 10]] = 2
        cams[:, 3] = 0.01 * np.arange(C)
        on = np.float32(NEAR) / 2
        below = np.nextafter(on, np.float32(0))
        bad = np.array([[np.nan, 0, 2], [0, np.nan, 2], [0, 0, np.nan], [np.inf, 0, 2], [0, -np.inf, 2], [0, 0, np.inf], [0, 0, -np.inf],
                        [0.1, 0.1, -2], [0, 0, 0], [0, 0, -0.0], [0.01, 0.01, on], [0.01, -0.01, below], [1e30, 0, 1], [0, -1e30, 1],
                        [1e30, 1e30, 1e30], [1e-30, 1e-30, 1e-30], [1e-30, 1e-30, 1], [0, 0, 3.4e38], [3e38, 3e38, 3.4e38],
                        [1e20, 0, 1e-3 + NEAR]], np.float32)
        where = g.permutation(M)[:len(bad)]
        xyz[where] = bad[:len(where)]
        return xyz, cams
    raise KeyError(kind)


@functools.lru_cache(maxsize=None)
def ref_case(case):
    """The restatement of a whole case, computed once per session: dict(xyz, rgb, cams, depth, index, out_rgb).  Callers leave the
    arrays unchanged."""
    kind, M, (H, W), C, radius = case
    xyz, cams = scene(kind, M, H, W, C, radius)
    rgb = colours(M)
    depth, index, out_rgb = render_ref(xyz, rgb, cams, H, W, radius, NEAR)
    out = dict(xyz=xyz, rgb=rgb, cams=cams, depth=depth, index=index, out_rgb=out_rgb)
    for a in out.values():
        a.setflags(write=False)
    return out
