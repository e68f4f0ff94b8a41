"""Scenes, float64 oracles and agreement rules for the solvers of the MST initialisation (tests/test_init_cases_cpu.py,
tests/test_gpu_init.py): the batched PnP, the Umeyama solve and umeyama_moments_kernel of csrc/init.hip and
the per-pixel passes of csrc/init_maps.hip.  numpy only.

PnP.  `pnp_oracle` restates the algorithm in the header of csrc/init.hip in float64 on the fp32-rounded inputs the kernel reads:
  sample   step = ceil(HW / 16384), n = ceil(HW / step), pixel p * step for p < n, used when its mask byte is set; ray of pixel
           (px, py) = ((px - ppx) / f, (py - ppy) / f, 1) with f, ppx, ppy rounded to fp32 (the descriptor holds floats);
  start    the 17 raw moments of (x = ray, y = world point, weight 1) and the similarity (s, Rwc, T) with s Rwc x + T ~ y in closed
           form (np.linalg.svd, R = U diag(1, 1, det(U V^T)) V^T); world -> camera R = Rwc^T, t = -R T (the scale is dropped);
  steps    `iterations` damped Gauss-Newton steps on the reprojection error e (pixels) over the points in front of the camera
           (z > 0; the others get weight 0), Cauchy weights 1 / (1 + |e|^2 / tau^2), tau = max(40 * 2^-it, 5); left perturbation
           c' = c + omega x c + v; (J^T W J + 1e-9 trace I) delta = -J^T W e, solved with np.linalg.solve; a step whose matrix is not
           positive definite is skipped; R <- exp([omega]x) R, t <- exp([omega]x) t + v (Rodrigues);
  finish   valid = n_used >= 6, at least half of the used points in front, det R > 0, finite t; inliers = points in front with
           |e|^2 < 25; truncated error = sum over the points in front of min(|e|^2, 25); c2w = [R^T, -R^T t].
The oracle is written independently of the kernel (vectorised numpy, LAPACK SVD and solve) and accumulates its sums in extended
precision (ACC = np.longdouble, a 64-bit mantissa on x86), so that the order of summation moves it by 1e-15 also after 0 and 1
iterations, where the row-band scene amplifies the noise of a float64 sum to 4e-12.  Agreement rule:
equal valid flags, equal inlier counts, truncated error within 4 fp32 ulp (relative; a float64 sum rounded once), every c2w entry v
within 2^-22 * max(1, |v|) (2 fp32 ulp: the kernel is float64 inside, the oracle moves by 1e-15 under a change of the summation
order, so what remains is the final cast).  Two cap conditions keep that rule honest and are asserted on the CPU for every problem
of the batch (tests/test_init_cases_cpu.py): no point in front of the camera has | |e| - 5 px | < 1e-4 px at the oracle's final pose
(then the inlier count has to be equal), and the oracle's c2w moves by less than 1e-12 under four random point orders.

Umeyama.  `umeyama_oracle`: the 17 float64 raw moments of the fp32 inputs
  [0] sum w  [1..3] sum w x  [4..6] sum w y  [7] sum w |x|^2  [8..16] sum w y_r x_c
and the closed form s = (S0 + S1 + d S2) / var_x, R = U diag(1, 1, d) V^T, T = ym - s R xm, d = det(U V^T).  Scenes (a) to (g) of
umeyama_scenes().  Agreement rule: s, R, T within 2^-22 * max(1, |v|); the nearly collinear and the far-centroid scene, whose optimum
is ill-conditioned in the raw moments, within max(that, 16 x the oracle's own spread over four point orders).  Cap: that spread is
below 1e-10 relative for every scene compared at 2 ulp.  The two others measure 2.3e-10 (collinear) and 1.9e-7 (centroid (300, -200,
500): var_x and cov are differences of sums 4e5 times their size, in the kernel as here); no choice of points brings the stated
far-centroid scene under 1e-10 in float64 raw moments, so their cap is 16 x spread < 1e-5, three orders below what one fp32
accumulator does (0.14 measured), and the spread enters their bound as stated.  P = 1 (var_x = 0: s = 0 / 0 in kernel and oracle alike) is left out; P = 3 is a well-shaped
triangle, whose similarity is determined, and is compared like the others.

Weiszfeld focal.  `weiszfeld_f64` restates post_process.py:36-60 in float64; `weiszfeld_f32` restates the kernel: fp32 per-pixel
arithmetic, float64 sums, an fp32 focal between the iterations.  Rule, per map: |got - float64| <= max(8 ulp, 8 x |fp32 restatement -
float64|), ulp = 2^-23 f (the factor covers the kernel's fused qx ux + qy uy, which numpy does not fuse).
"""
import functools

import numpy as np

PNP_MAX_POINTS = 16384
ULP2 = 2.0 ** -22                   # 2 fp32 ulp at 1
INLIER_PX = 5.0
BOUNDARY_GAP = 1e-4                 # px: no point in front this close to the inlier threshold
PNP_SPREAD_CAP = 1e-12
UME_SPREAD_CAP = 1e-10
PNP_ITERATIONS = (0, 1, 10)
ACC = np.longdouble                 # the PnP oracle's sums: extended precision where the platform has it (x86: 64-bit mantissa)


def f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


def rot(ax, ay=0.0, az=0.0):
    cx, sx, cy, sy, cz, sz = np.cos(ax), np.sin(ax), np.cos(ay), np.sin(ay), np.cos(az), np.sin(az)
    Rx = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
    Ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    Rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])
    return Rz @ Ry @ Rx


def random_rot(rng):
    q, r = np.linalg.qr(rng.standard_normal((3, 3)))
    q = q * np.sign(np.diag(r))
    return q * np.linalg.det(q)


def ortho_err(R):
    """max |R R^T - I| and |det R - 1| of [..., 3, 3] matrices."""
    R = np.asarray(R, dtype=np.float64)
    return float(np.abs(R @ np.swapaxes(R, -1, -2) - np.eye(3)).max()), float(np.abs(np.linalg.det(R) - 1).max())


# ------------------------------------------------------------------------------------------------ closed-form similarity
def moments17(x, y, w, dt=np.float64):
    """The 17 raw moments of float64 x, y [P,3], w [P], accumulated in dt."""
    x, y, w = x.astype(dt), y.astype(dt), w.astype(dt)
    wy = w[:, None] * y
    return np.concatenate([[w.sum()], (w[:, None] * x).sum(0), wy.sum(0), [(w * (x * x).sum(1)).sum()],
                           (wy[:, :, None] * x[:, None, :]).sum(0).reshape(9)])


def similarity_from_moments(m, guard=False):
    """(s, R, T) with s R x + T ~ y from the 17 moments.  guard: the PnP start's w0 > 0 and var_x > 0 fall-backs to 1."""
    w0 = m[0]
    if guard and not w0 > 0:
        w0 = 1.0
    xm, ym = m[1:4] / w0, m[4:7] / w0
    var_x = m[7] / w0 - xm @ xm
    if guard and not var_x > 0:
        var_x = 1.0
    cov = (m[8:17].reshape(3, 3) / w0 - np.outer(ym, xm)).astype(np.float64)
    U, S, Vt = np.linalg.svd(cov)
    d = np.array([1.0, 1.0, 1.0 if np.linalg.det(U @ Vt) >= 0 else -1.0])
    R = (U * d) @ Vt
    s = (S * d).sum() / var_x
    return float(s), R, (ym - s * R @ xm).astype(np.float64)


def umeyama_oracle(x, y, w, order=None):
    """x, y [P,3], w [P] float32 -> (s, R [3,3], T [3]) float64.  order: a permutation of the points (summation order)."""
    assert x.dtype == y.dtype == w.dtype == np.float32
    x, y, w = x.astype(np.float64), y.astype(np.float64), w.astype(np.float64)
    if order is not None:
        x, y, w = x[order], y[order], w[order]
    return similarity_from_moments(moments17(x, y, w))


def pack_sRT(s, R, T):
    return np.concatenate([[s], np.asarray(R).reshape(9), np.asarray(T).reshape(3)])


def umeyama_spread(x, y, w, seed=0):
    """Largest |deviation| / max(1, |value|) of the packed (s, R, T) over four random point orders."""
    base = pack_sRT(*umeyama_oracle(x, y, w))
    rng = np.random.default_rng(seed)
    dev = 0.0
    for _ in range(4):
        v = pack_sRT(*umeyama_oracle(x, y, w, rng.permutation(len(w))))
        dev = max(dev, float((np.abs(v - base) / np.maximum(1, np.abs(base))).max()))
    return dev


def _similar(rng, x, s=None, noise=0.0):
    R, T = random_rot(rng), rng.standard_normal(3)
    s = 0.5 + 2 * rng.random() if s is None else s
    return s * x @ R.T + T + noise * rng.standard_normal(x.shape)


GENERIC_P = (3, 255, 1023, 1024, 1025, 3000)       # P = 1: see the module docstring
SPECIAL_P = 1500                                   # scenes (b) to (f): two chunks of the moments kernel, the second one partial
LOOSE = ("d_collinear", "e_far")                   # bound = max(2 ulp, 16 x the oracle's order spread)


@functools.lru_cache(maxsize=None)
def umeyama_scenes():
    """name -> dict(X [E,P,3], Y [N,P,3], W [E,P] float32, y_index [E]).  Problem e registers X[e] onto Y[y_index[e]]."""
    out = {}
    rng = np.random.default_rng(11)
    for P in GENERIC_P:                                                          # (a) two problems per size
        X = rng.standard_normal((2, P, 3))
        if P == 3:
            X[:] = [[0.0, 0.0, 0.0], [1.0, 0.1, 0.2], [0.2, 1.1, -0.3]]
            X[1] += 0.5
        Y = np.stack([_similar(rng, X[e], noise=0.0 if P == 3 else 0.01) for e in range(2)])
        out[f"a_generic_P{P}"] = dict(X=X, Y=Y, W=0.5 + rng.random((2, P)), y_index=[0, 1])
    P = SPECIAL_P
    x = rng.standard_normal((P, 3))                                              # (b) the unconstrained optimum is a reflection
    out["b_mirror"] = dict(X=x[None], Y=(_similar(rng, x * [1.0, 1.0, -1.0], noise=0.05))[None], W=0.5 + rng.random((1, P)), y_index=[0])
    x = rng.standard_normal((P, 3)); x[:, 2] = 0.0                               # (c) coplanar, z = 0 exactly, rigid image
    out["c_coplanar"] = dict(X=x[None], Y=_similar(rng, x, s=1.0)[None], W=0.5 + rng.random((1, P)), y_index=[0])
    u = np.array([0.6, -0.48, 0.64])                                             # (d) 1e-3 off a line
    x = rng.standard_normal((P, 1)) * u + 1e-3 * rng.standard_normal((P, 3))
    out["d_collinear"] = dict(X=x[None], Y=_similar(rng, x)[None], W=0.5 + rng.random((1, P)), y_index=[0])
    x = rng.standard_normal((P, 3)) + [300.0, -200.0, 500.0]                     # (e) far from the origin, unit spread
    out["e_far"] = dict(X=x[None], Y=_similar(rng, x, noise=0.01)[None], W=0.5 + rng.random((1, P)), y_index=[0])
    x = rng.standard_normal((P, 3))                                              # (f) half of the weights exactly 0, garbage there
    y = _similar(rng, x, noise=0.01)
    w = 0.5 + rng.random(P)
    dead = rng.permutation(P)[:P // 2]
    w[dead] = 0.0
    x[dead] = 1e6 * rng.standard_normal((len(dead), 3))
    y[dead] = -3e7 * rng.standard_normal((len(dead), 3))
    out["f_zero_weights"] = dict(X=x[None], Y=y[None], W=w[None], y_index=[0], dead=dead)
    E, N, P = 130, 7, 64                                                         # (g) more problems than one block of the solve
    Y = rng.standard_normal((N, P, 3)) * [1.0, 2.0, 0.5]
    yi = [(3 * e + e // 7) % N for e in range(E)]
    X = np.stack([_similar(rng, Y[yi[e]], noise=0.02) for e in range(E)])
    out["g_batch130"] = dict(X=X, Y=Y, W=0.5 + rng.random((E, P)), y_index=yi)
    for sc in out.values():
        for k in "XYW":
            sc[k] = f32(sc[k])
    return out


@functools.lru_cache(maxsize=None)
def umeyama_expected():
    """name -> (want [E,13] float64, spread [E]) of every scene."""
    out = {}
    for name, sc in umeyama_scenes().items():
        E = len(sc["y_index"])
        want = np.stack([pack_sRT(*umeyama_oracle(sc["X"][e], sc["Y"][sc["y_index"][e]], sc["W"][e])) for e in range(E)])
        spread = np.array([umeyama_spread(sc["X"][e], sc["Y"][sc["y_index"][e]], sc["W"][e], seed=e) for e in range(E)])
        out[name] = (want, spread)
    return out


def umeyama_bound(name, want, spread):
    """[E,13] bound of scene `name` (module docstring)."""
    b = ULP2 * np.maximum(1, np.abs(want))
    if name in LOOSE:
        b = np.maximum(b, 16 * spread[:, None] * np.maximum(1, np.abs(want)))
    return b


# ------------------------------------------------------------------------------------------------ PnP
def pnp_sample(H, W, mask):
    step = -(-(H * W) // PNP_MAX_POINTS)
    n = -(-(H * W) // step)
    pix = np.arange(n, dtype=np.int64) * step
    return step, n, pix[np.asarray(mask).reshape(-1)[pix] != 0]


def pnp_focal_candidates(H, W):
    return [float(f) for f in np.geomspace(max(W, H) / 2, max(W, H) * 3, 21)]


def _residuals(R, t, X, rx, ry, f):
    c = X @ R.T + t
    z = c[:, 2]
    zz = np.where(np.abs(z) > 1e-9, z, 1e-9)
    xz, yz = c[:, 0] / zz, c[:, 1] / zz
    ex, ey = (xz - rx) * f, (yz - ry) * f
    return z, zz, xz, yz, ex, ey


def pnp_oracle(pts, mask, focal, pp=None, iterations=10, order=None):
    """pts [H,W,3] float32, mask [H,W] -> dict(valid, inliers, err, c2w [4,4] float64, used, front, gap, step, focal).
    gap = the smallest | |e| - 5 px | over the points in front of the camera at the final pose.  order: a numpy Generator that
    shuffles the points (summation order)."""
    assert pts.dtype == np.float32
    H, W, _ = pts.shape
    step, _, pix = pnp_sample(H, W, mask)
    if order is not None:
        pix = order.permutation(pix)
    f = float(np.float32(focal))
    cx, cy = (W / 2, H / 2) if pp is None else pp
    cx, cy = float(np.float32(cx)), float(np.float32(cy))
    X = pts.reshape(-1, 3)[pix].astype(np.float64)
    py, px = pix // W, pix % W
    rx, ry = (px - cx) / f, (py - cy) / f
    used = len(pix)
    # start
    rays = np.stack([rx, ry, np.ones(used)], 1)
    _, Rwc, T = similarity_from_moments(moments17(rays, X, np.ones(used), ACC), guard=True)
    R, t = Rwc.T, -Rwc.T @ T
    # steps
    for it in range(iterations):
        tau = max(40.0 * 2.0 ** -it, 5.0)
        z, zz, xz, yz, ex, ey = _residuals(R, t, X, rx, ry, f)
        w = np.where(z > 0, 1.0 / (1.0 + (ex * ex + ey * ey) / (tau * tau)), 0.0)
        iz, o = f / zz, np.zeros(used)
        Jx = np.stack([-xz * yz * f, (1 + xz * xz) * f, -yz * f, iz, o, -xz * iz], 1)
        Jy = np.stack([-(1 + yz * yz) * f, xz * yz * f, xz * f, o, iz, -yz * iz], 1)
        Jx, Jy, wl = Jx.astype(ACC), Jy.astype(ACC), w.astype(ACC)
        A = (((Jx * wl[:, None])[:, :, None] * Jx[:, None, :]).sum(0) + ((Jy * wl[:, None])[:, :, None] * Jy[:, None, :]).sum(0)).astype(np.float64)
        g = -(((wl * ex)[:, None] * Jx).sum(0) + ((wl * ey)[:, None] * Jy).sum(0)).astype(np.float64)
        tr = np.trace(A)
        if not (tr > 0 and np.isfinite(tr)):
            continue
        A = A + 1e-9 * tr * np.eye(6)
        if not np.isfinite(A).all() or np.linalg.eigvalsh(A).min() <= 0:
            continue
        dl = np.linalg.solve(A, g)
        om = dl[:3]
        th = np.linalg.norm(om)
        K = np.array([[0, -om[2], om[1]], [om[2], 0, -om[0]], [-om[1], om[0], 0]])
        ca, cb = (np.sin(th) / th, (1 - np.cos(th)) / (th * th)) if th > 1e-12 else (1.0, 0.5)
        dR = np.eye(3) + ca * K + cb * K @ K
        R, t = dR @ R, dR @ t + dl[3:]
    # finish
    z, _, _, _, ex, ey = _residuals(R, t, X, rx, ry, f)
    e2 = ex * ex + ey * ey
    front = z > 0
    valid = bool(used >= 6 and front.sum() >= 0.5 * used and np.linalg.det(R) > 0 and np.isfinite(t.sum()))
    c2w = np.eye(4)
    c2w[:3, :3], c2w[:3, 3] = R.T, -R.T @ t
    gap = float(np.abs(np.sqrt(e2[front]) - INLIER_PX).min()) if front.any() else np.inf
    return dict(valid=valid, inliers=int((front & (e2 < 25.0)).sum()), err=float(np.minimum(e2[front], 25.0).astype(ACC).sum()), c2w=c2w, used=used,
                front=int(front.sum()), gap=gap, step=step, focal=f)


def _surface(H, W, f, pp, c2w, depth=None):
    """World points seen by the pinhole (f, pp, c2w) looking at a wavy surface (the scene of test_pnp_on_device)."""
    ys, xs = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    d = 3 + 0.6 * np.sin(xs / W * 5) * np.cos(ys / H * 4) if depth is None else depth(xs, ys)
    cx, cy = (W / 2, H / 2) if pp is None else pp
    cam = np.stack([(xs - cx) / f * d, (ys - cy) / f * d, d], -1)
    return cam @ c2w[:3, :3].T + c2w[:3, 3]


def true_pose():
    c2w = np.eye(4)
    c2w[:3, :3] = rot(0.0, 0.3) @ rot(-0.2)
    c2w[:3, 3] = [0.4, -0.2, 1.0]
    return c2w


def _outliers(rng, world, frac):
    noisy = world.copy()
    bad = rng.random(world.shape[:2]) < frac
    noisy[bad] += rng.standard_normal((int(bad.sum()), 3))
    return noisy


# the focal search (focal = None: 21 candidates each, 84 problems): name -> (H, W, true focal, pp, checkerboard mask).  Small maps: with
# n points whose errors spread over a few pixels, the smallest distance to the 5 px threshold is about 1 / n px, and the cap asks
# for 1e-4 px on every one of the 84 x 3 problems; the subsample (step > 1) is covered by the scenes with a given focal.
SEARCH = {
    "search_37x41_checker": (37, 41, 44.0, None, True),
    "search_33x70": (33, 70, 120.0, (33.5, 17.25), False),
    "search_24x36": (24, 36, 30.0, None, False),
    "search_5x7": (5, 7, 9.0, None, False),
}


@functools.lru_cache(maxsize=None)
def pnp_scenes():
    """name -> dict(pts [H,W,3] float32, mask [H,W] bool, focal | None, pp | None, truth c2w, kind).  kind: 'clean' (the truth is
    recovered to the rounding of the inputs), 'outliers20' / 'outliers40' (3e-2 / 8e-2 of test_pnp_on_device), 'invalid', 'search'."""
    rng = np.random.default_rng(5)
    c2w = true_pose()
    out = {}

    def add(name, H, W, f, kind, pp=None, mask=None, world=None, focal="given"):
        world = _surface(H, W, f, pp, c2w) if world is None else world
        out[name] = dict(pts=f32(world), mask=np.ones((H, W), bool) if mask is None else mask, focal=f if focal == "given" else None, pp=pp,
                         truth=c2w, kind=kind, true_focal=f)

    add("129x128_step2", 129, 128, 150.0, "clean")
    add("129x128_step2_pp", 129, 128, 150.0, "clean", pp=(70.25, 60.5))
    add("150x230_step3_out20", 150, 230, 260.0, "outliers20", world=_outliers(rng, _surface(150, 230, 260.0, None, c2w), 0.2))
    ys, xs = np.mgrid[:37, :41]
    add("37x41_checker", 37, 41, 50.0, "clean", mask=(xs + ys) % 2 == 0)
    add("96x128_out40", 96, 128, 150.0, "outliers40", world=_outliers(rng, _surface(96, 128, 150.0, None, c2w), 0.4))
    band = np.zeros((33, 70), bool)
    band[10:13] = True
    add("33x70_rows10-12", 33, 70, 80.0, "clean", mask=band)
    add("5x7", 5, 7, 9.0, "clean")
    few = np.zeros((37, 41), bool)                                   # five pixels in general position: a pose, but not a valid one
    few[[3, 9, 20, 30, 35], [5, 33, 18, 4, 38]] = True
    add("37x41_five_pixels", 37, 41, 50.0, "invalid", mask=few)
    # a camera that looks away from most of its points: the 55 % of the pixels nearest the centre see points BEHIND it (their
    # projection is consistent: x / z = ray), the rim in front.  The start follows the rim (larger ray variance), the steps fit it.
    H, W, f = 37, 41, 50.0
    ys, xs = np.mgrid[:H, :W]
    r2 = ((xs - W / 2) / W) ** 2 + ((ys - H / 2) / H) ** 2
    behind = r2 <= np.sort(r2.ravel())[int(0.55 * H * W)]
    add("37x41_looking_away", H, W, f, "invalid",
        world=_surface(H, W, f, None, c2w, depth=lambda x, y: np.where(behind, -1.0, 1.0) * (3 + 0.6 * np.sin(x / W * 5) * np.cos(y / H * 4))))
    out["37x41_looking_away"]["behind"] = behind
    # the focal search (focal = None: 21 candidates each, 84 problems)
    for name, (H, W, f, pp, checker) in SEARCH.items():
        ys, xs = np.mgrid[:H, :W]
        add(name, H, W, f, "search", focal=None, pp=pp, mask=(xs + ys) % 2 == 0 if checker else None)
    return out


def pnp_problems():
    """The one batch: [(scene name, focal)] -- the given-focal scenes in order, then 21 candidates per search scene.  This is the order
    linear_pnp_many builds from pnp_items()."""
    out = []
    for name, sc in pnp_scenes().items():
        H, W, _ = sc["pts"].shape
        out += [(name, f) for f in ([sc["focal"]] if sc["focal"] is not None else pnp_focal_candidates(H, W))]
    return out


@functools.lru_cache(maxsize=None)
def pnp_expected(iterations):
    """The oracle's result for every problem of the batch at this iteration count."""
    sc = pnp_scenes()
    return [pnp_oracle(sc[name]["pts"], sc[name]["mask"], f, sc[name]["pp"], iterations) for name, f in pnp_problems()]


def pnp_search_pick(results):
    """linear_pnp_many's choice among the candidates of one item: valid, at least one inlier, most inliers, then the smallest truncated
    error.  results: the oracle dicts of the 21 candidates.  Returns (index | None, margin): margin = how far the runner-up is behind --
    inliers if they differ, else the relative difference of the truncated errors."""
    ok = [k for k, r in enumerate(results) if r["valid"] and r["inliers"] > 0]
    if not ok:
        return None, np.inf
    ok.sort(key=lambda k: (results[k]["inliers"], -results[k]["err"]), reverse=True)
    if len(ok) == 1:
        return ok[0], np.inf
    a, b = results[ok[0]], results[ok[1]]
    margin = float(a["inliers"] - b["inliers"]) if a["inliers"] != b["inliers"] else (b["err"] - a["err"]) / max(b["err"], 1e-300)
    return ok[0], margin


# ------------------------------------------------------------------------------------------------ Weiszfeld focal
WEISZFELD_SHAPES = ((5, 7), (37, 41), (33, 64), (96, 128))


@functools.lru_cache(maxsize=None)
def weiszfeld_maps(H, W):
    """[3,H,W,3] float32 point maps of pinholes with focals 0.45, 1.0 and 2.3 x max(H, W) seeing a smooth surface, each with a z = 0
    pixel, an all-zero pixel (0 / 0), a NaN pixel and a z = +inf pixel; and the three focals."""
    rng = np.random.default_rng(H * 1000 + W)
    ys, xs = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    focals = [0.45 * max(H, W), 1.0 * max(H, W), 2.3 * max(H, W)]
    maps = []
    for b, f in enumerate(focals):
        d = 2 + 0.5 * np.sin(xs / W * 4 + b) * np.cos(ys / H * 3)
        m = np.stack(((xs - W / 2) / f * d, (ys - H / 2) / f * d, d), -1) + 0.01 * rng.standard_normal((H, W, 3))
        m[0, 0, 2] = 0.0
        m[1, 2] = 0.0
        m[H - 1, W - 2] = np.nan
        m[H // 2, W - 1, 2] = np.inf
        maps.append(m)
    return f32(np.stack(maps)), focals


def _weiszfeld(maps, dt, iterations):
    B, H, W, _ = maps.shape
    ys, xs = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    ux, uy = (xs.reshape(-1) - dt(W / 2)).astype(dt), (ys.reshape(-1) - dt(H / 2)).astype(dt)
    out = []
    for p in maps.reshape(B, -1, 3).astype(dt):
        with np.errstate(all="ignore"):
            qx, qy = p[:, 0] / p[:, 2], p[:, 1] / p[:, 2]
        qx, qy = np.where(np.isfinite(qx), qx, dt(0)), np.where(np.isfinite(qy), qy, dt(0))
        dot, sq = qx * ux + qy * uy, qx * qx + qy * qy
        f = dt(dot.astype(np.float64).sum() / sq.astype(np.float64).sum())
        for _ in range(iterations):
            dx, dy = ux - f * qx, uy - f * qy
            w = dt(1) / np.maximum(np.sqrt(dx * dx + dy * dy), dt(1e-8))
            f = dt((w * dot).astype(np.float64).sum() / (w * sq).astype(np.float64).sum())
        out.append(max(float(f), 0.0))
    return np.array(out)


def weiszfeld_f64(maps, iterations=10):
    """post_process.py:36-60 ('weiszfeld', principal point at the centre, min_focal = 0) in float64 on the fp32 maps."""
    return _weiszfeld(maps, np.float64, iterations)


def weiszfeld_f32(maps, iterations=10):
    """The kernel's arithmetic: fp32 per pixel, float64 sums, an fp32 focal."""
    return _weiszfeld(maps, np.float32, iterations)


# ------------------------------------------------------------------------------------------------ depth_init
FLT_MAX = float(np.finfo(np.float32).max)


@functools.lru_cache(maxsize=None)
def depth_scene(N=3, P=1517, scale=0.37):
    """dict(pts [N,P,3], w2c [N,3,4] float32, scale, z, want, zbound [N,P] float64): random rotations, camera depths in [1, 6], for a fifth
    of the pixels in [-4, -0.5] and for a twelfth in [2e-3, 0.5], where log z is steep.  Pixel 0 of every image is NaN, pixel 1 has z = +inf, and pixel 2 of image 1 (whose t_z is 0)
    is the origin: z = 0 exactly.  z = float64 depth of the fp32 inputs, with the fp32 product q * scale the kernel forms first;
    want = log z with _set_depthmap's clean-up (z <= 0 or NaN -> 0, +inf -> FLT_MAX); zbound = 8 * 2^-24 * (|m0 a| + |m1 b| + |m2 c| +
    |m3|) bounds the fp32 evaluation of z (three products and three sums, each a rounding of a partial sum no larger than that)."""
    rng = np.random.default_rng(22)
    w2c = np.zeros((N, 3, 4))
    pts = np.zeros((N, P, 3))
    for n in range(N):
        R, t = random_rot(rng), rng.standard_normal(3)
        if n == 1:
            t[2] = 0.0
        kind = rng.random(P)
        z = np.where(kind < 0.2, -0.5 - 3.5 * rng.random(P), np.where(kind < 0.28, 2e-3 * 250.0 ** rng.random(P), 1 + 5 * rng.random(P)))
        cam = np.stack([rng.standard_normal(P) * z, rng.standard_normal(P) * z, z], 1)
        pts[n] = (cam - t) @ R / scale
        w2c[n, :, :3], w2c[n, :, 3] = R, t
    pts, w2c = f32(pts), f32(w2c)
    pts[:, 0] = np.nan
    pts[:, 1] = 0.0
    pts[:, 1, 2] = np.where(w2c[:, 2, 2] >= 0, np.inf, -np.inf)
    pts[1, 2] = 0.0
    sp = (pts * np.float32(scale)).astype(np.float64)
    m = w2c[:, 2].astype(np.float64)
    with np.errstate(all="ignore"):
        terms = m[:, None, :3] * sp
        z = terms.sum(-1) + m[:, None, 3]
        zbound = 8 * 2.0 ** -24 * (np.abs(terms).sum(-1) + np.abs(m[:, None, 3]))
        want = np.where(z > 0, np.minimum(np.log(z), FLT_MAX), 0.0)
    want[np.isnan(z)] = 0.0
    return dict(pts=pts, w2c=w2c, scale=scale, z=z, want=want, zbound=zbound)
