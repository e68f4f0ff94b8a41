"""Shared cases of the tracking tests (csrc/track.hip): track_ref(), the vectorised numpy restatement of the definition in
include/a3r.h, track_naive(), one Python loop per track that checks the restatement itself, the inputs by kind, and the sizes.

The definition.  Inputs: xyz [N,H,W,3] float32, keep [N,H,W] uint8, flow_a / flow_b [E,2,H,W] float32 (channel 0 = x, 1 = y),
steps [C,S,4] int32 rows (frame_from, frame_to, edge, reversed), seeds [M,2] float32 (x, y) or None = every pixel (x = m % W,
y = m // W), fb_thr.  The forward field of a step is flow_b[edge] if reversed else flow_a[edge], the backward field the other one.
float64 on float64 copies, every operation rounded on its own:
    bilinear(F, x, y): x0 = floor(x), x1 = min(x0 + 1, W - 1), ax = x - x0 (y likewise);
                       top = F[y0,x0] + ax * (F[y0,x1] - F[y0,x0]), bot on row y1, val = top + ay * (bot - top)
    start at the seed, alive iff x, y finite and inside [0, W-1] x [0, H-1]; record at t = 0 in steps[c,0].frame_from (S = 0: frame 0)
    per step:  f = bilinear(fwd, x, y); xn = x + f.x, yn = y + f.y; ends unless xn, yn finite and inside
               b = bilinear(bwd, xn, yn); dx = f.x + b.x, dy = f.y + b.y; ends unless dx * dx + dy * dy < fb_thr * fb_thr
               (x, y) = (xn, yn); record at t = s + 1 in frame_to
    record(t, n): col = rint(x), row = rint(y) (half to even), pix = row * W + col, xy = float32(x, y); state 2 and xyz = xyz[n,pix]
                  if keep[n,pix] and xyz[n,pix] is finite, else state 1 and zeros; an ended track: state 0, pix -1, zeros

The graph of every case is a path of S + 1 frames: edge k joins frames k and k + 1 and is stored as (k, k + 1) for even k and as
(k + 1, k) for odd k, so a chain that walks the path meets both `reversed` values as soon as it has two steps.  A kind gives the
field `up[k]` that leads from frame k to k + 1 and `down[k]` that leads back; flow_a[k] is up[k] for even k and down[k] for odd k.
Chains: 0 walks 0 .. S, 1 walks S .. 0, 2 goes 0, 1, 0, 1, ...

Kinds:
  translate  up = (+2, +1) everywhere, down = (-2, -1): integer steps, the exact inverse; positions are seed + s * (2, 1) and a
             track ends exactly in the step that leaves the image
  halfpix    up = (0.25, -0.5), down the negative, seeds on multiples of 0.25: exact arithmetic, positions on k + 0.5 in both
             parities -- pins half-to-even against floor(x + 0.5)
  border     integer seeds, step 0 places them (border_targets): interior pixels land exactly on column W - 1, column 0, row H - 1
             or row 0 (alive); the pixels of the last column / row stay (even row / column) or move by the spacing of float64 at
             W - 1 / H - 1 (odd: the next float64 above the border, ended); those of the first column / row stay or move by -2^-126
             (the smallest step a float32 flow makes below 0 without a subnormal; ended).  Later steps have zero flow.  fb_thr = inf,
             the backward field is noise: it is still sampled at the border, where x1 / y1 clamp
  threshold  up = (1, 0); down = (2, 4) where x + y is even and (2, 3.984375) where it is odd: at an integer target the
             disagreement is (3, 4) -- 25 < 25 is false, ended -- or (3, 3.984375) -- alive; fb_thr = 5
  smooth     up = low-frequency sinusoids of 3 px amplitude plus 1.5 px in x, down = minus that plus a sinusoidal disagreement of
             4 px amplitude; fb_thr = 3: tracks end by both causes, a share survives (tests/test_tracks_cpu.py asserts it)
  hostile    noise flow with NaN and +-inf at scattered pixels, seeds that are NaN, infinite, outside the image and on its corners,
             keep = 0 at a third of the pixels, NaN and inf xyz at kept pixels; fb_thr = inf
"""
import functools
import math

import numpy as np

KINDS = ("translate", "halfpix", "border", "threshold", "smooth", "hostile")
ALL = 0                       # M = ALL: seeds=None, every pixel

# (kind, (H, W), M, S, C): images (1,1), (3,5), (48,64), (96,128); M in {1, 63, 65, 1000, every pixel}; S in {0, 1, 2, 7}; C in {1, 3}
CASES = [
    ("translate", (1, 1), 1, 0, 1), ("translate", (1, 1), ALL, 1, 1), ("translate", (3, 5), ALL, 2, 1), ("translate", (3, 5), 63, 1, 3),
    ("translate", (48, 64), 1000, 7, 3), ("translate", (96, 128), ALL, 2, 1),
    ("halfpix", (3, 5), 65, 2, 1), ("halfpix", (3, 5), 1, 7, 3), ("halfpix", (48, 64), ALL, 7, 1), ("halfpix", (96, 128), 1000, 1, 1),
    ("border", (3, 5), ALL, 1, 1), ("border", (48, 64), 63, 1, 1), ("border", (48, 64), ALL, 2, 3), ("border", (96, 128), ALL, 1, 1),
    ("threshold", (3, 5), ALL, 1, 1), ("threshold", (48, 64), 65, 2, 1), ("threshold", (48, 64), ALL, 7, 3),
    ("smooth", (3, 5), 63, 7, 1), ("smooth", (48, 64), 1000, 1, 1), ("smooth", (48, 64), ALL, 7, 1), ("smooth", (96, 128), 65, 2, 3),
    ("smooth", (96, 128), ALL, 7, 1),
    ("hostile", (1, 1), 63, 1, 1), ("hostile", (3, 5), 65, 2, 3), ("hostile", (48, 64), ALL, 0, 1), ("hostile", (48, 64), 1000, 7, 1),
    ("hostile", (96, 128), ALL, 1, 3),
]


def case_id(case):
    kind, (H, W), M, S, C = case
    return f"{kind}-{H}x{W}-M{M or 'all'}-S{S}-C{C}"


def n_tracks(case):
    kind, (H, W), M, S, C = case
    return M or H * W


# ------------------------------------------------------------------------------------------------- the restatement
def _inside(x, y, H, W):
    with np.errstate(invalid="ignore"):
        return (x >= 0) & (x <= W - 1) & (y >= 0) & (y <= H - 1)          # false for NaN; an infinity is outside


def _bilinear(F, x, y):
    """F [2,H,W] float64 at positions inside the image -> (val_x, val_y)"""
    H, W = F.shape[1:]
    xf, yf = np.floor(x), np.floor(y)
    x0, y0 = xf.astype(np.int64), yf.astype(np.int64)
    x1, y1 = np.minimum(x0 + 1, W - 1), np.minimum(y0 + 1, H - 1)
    ax, ay = x - xf, y - yf
    out = []
    with np.errstate(invalid="ignore", over="ignore"):
        for k in range(2):
            G = F[k]
            top = G[y0, x0] + ax * (G[y0, x1] - G[y0, x0])
            bot = G[y1, x0] + ax * (G[y1, x1] - G[y1, x0])
            out.append(top + ay * (bot - top))
    return out


def seed_positions(seeds, H, W):
    if seeds is None:
        m = np.arange(H * W)
        return (m % W).astype(np.float64), (m // W).astype(np.float64)
    seeds = np.asarray(seeds, np.float32)
    return seeds[:, 0].astype(np.float64), seeds[:, 1].astype(np.float64)


def track_ref(xyz, keep, flow_a, flow_b, steps, seeds=None, fb_thr=3.0):
    """dict(xy [C,S+1,M,2] float32, xyz [C,S+1,M,3] float32, pix [C,S+1,M] int32, state [C,S+1,M] uint8) and, for the tests of the
    cases themselves, cause [C,S,M] uint8: 1 = the track ended in this step by leaving the image, 2 = by the forward-backward test."""
    xyz, keep = np.asarray(xyz, np.float32), np.asarray(keep)
    N, H, W, _ = xyz.shape
    steps = np.asarray(steps, np.int32)
    steps = steps[None] if steps.ndim == 2 else steps
    C, S = steps.shape[:2]
    fa, fb = np.asarray(flow_a, np.float32).astype(np.float64), np.asarray(flow_b, np.float32).astype(np.float64)
    sx, sy = seed_positions(seeds, H, W)
    M = len(sx)
    thr2 = np.float64(fb_thr) * np.float64(fb_thr)
    out = dict(xy=np.zeros((C, S + 1, M, 2), np.float32), xyz=np.zeros((C, S + 1, M, 3), np.float32),
               pix=np.full((C, S + 1, M), -1, np.int32), state=np.zeros((C, S + 1, M), np.uint8), cause=np.zeros((C, S, M), np.uint8))
    flat_xyz, flat_keep = xyz.reshape(N, H * W, 3), keep.reshape(N, H * W)

    def record(c, t, n, alive, x, y):
        xs, ys = np.where(alive, x, 0.0), np.where(alive, y, 0.0)
        pix = np.rint(ys).astype(np.int64) * W + np.rint(xs).astype(np.int64)
        p = flat_xyz[n, pix]
        seen = alive & (flat_keep[n, pix] != 0) & np.isfinite(p).all(1)
        out["xy"][c, t] = np.stack([xs, ys], 1).astype(np.float32)
        out["xyz"][c, t] = np.where(seen[:, None], p, np.float32(0))
        out["pix"][c, t] = np.where(alive, pix, -1)
        out["state"][c, t] = np.where(seen, 2, np.where(alive, 1, 0))

    for c in range(C):
        x, y = sx.copy(), sy.copy()
        alive = _inside(x, y, H, W)
        record(c, 0, steps[c, 0, 0] if S else 0, alive, x, y)
        for s in range(S):
            _, to, e, rev = (int(v) for v in steps[c, s])
            fwd, bwd = (fb[e], fa[e]) if rev else (fa[e], fb[e])
            xs, ys = np.where(alive, x, 0.0), np.where(alive, y, 0.0)
            fx, fy = _bilinear(fwd, xs, ys)
            with np.errstate(invalid="ignore", over="ignore"):
                xn, yn = xs + fx, ys + fy
                ok1 = alive & _inside(xn, yn, H, W)
                bx, by = _bilinear(bwd, np.where(ok1, xn, 0.0), np.where(ok1, yn, 0.0))
                dx, dy = fx + bx, fy + by
                ok2 = ok1 & (dx * dx + dy * dy < thr2)
            out["cause"][c, s] = np.where(alive & ~ok1, 1, np.where(ok1 & ~ok2, 2, 0))
            x, y, alive = np.where(ok2, xn, x), np.where(ok2, yn, y), ok2
            record(c, s + 1, to, alive, x, y)
    return out


def track_naive(xyz, keep, flow_a, flow_b, steps, seeds=None, fb_thr=3.0):
    """The same definition, one track at a time on Python floats (IEEE doubles, one rounding per operation; round() is half to
    even): the four outputs of track_ref."""
    xyz, keep = np.asarray(xyz, np.float32), np.asarray(keep)
    N, H, W, _ = xyz.shape
    steps = np.asarray(steps, np.int32)
    steps = steps[None] if steps.ndim == 2 else steps
    C, S = steps.shape[:2]
    sx, sy = seed_positions(seeds, H, W)
    M = len(sx)
    thr2 = float(fb_thr) * float(fb_thr)
    out = dict(xy=np.zeros((C, S + 1, M, 2), np.float32), xyz=np.zeros((C, S + 1, M, 3), np.float32),
               pix=np.full((C, S + 1, M), -1, np.int32), state=np.zeros((C, S + 1, M), np.uint8))

    def inside(x, y):
        return 0.0 <= x <= W - 1 and 0.0 <= y <= H - 1

    def bilinear(F, x, y):
        x0, y0 = math.floor(x), math.floor(y)
        x1, y1 = min(x0 + 1, W - 1), min(y0 + 1, H - 1)
        ax, ay = x - x0, y - y0
        val = []
        for k in range(2):
            f00, f01, f10, f11 = float(F[k, y0, x0]), float(F[k, y0, x1]), float(F[k, y1, x0]), float(F[k, y1, x1])
            top = f00 + ax * (f01 - f00)
            bot = f10 + ax * (f11 - f10)
            val.append(top + ay * (bot - top))
        return val

    def record(c, t, m, n, alive, x, y):
        if not alive:
            return
        pix = round(y) * W + round(x)
        out["xy"][c, t, m] = (x, y)
        out["pix"][c, t, m] = pix
        p = xyz[n].reshape(-1, 3)[pix]
        if keep[n].reshape(-1)[pix] and all(math.isfinite(float(v)) for v in p):
            out["xyz"][c, t, m], out["state"][c, t, m] = p, 2
        else:
            out["state"][c, t, m] = 1

    for c in range(C):
        for m in range(M):
            x, y = float(sx[m]), float(sy[m])
            alive = inside(x, y)
            record(c, 0, m, int(steps[c, 0, 0]) if S else 0, alive, x, y)
            for s in range(S):
                _, to, e, rev = (int(v) for v in steps[c, s])
                if not alive:
                    break
                fwd, bwd = (flow_b[e], flow_a[e]) if rev else (flow_a[e], flow_b[e])
                fx, fy = bilinear(fwd, x, y)
                xn, yn = x + fx, y + fy
                alive = inside(xn, yn)
                if alive:
                    bx, by = bilinear(bwd, xn, yn)
                    dx, dy = fx + bx, fy + by
                    alive = dx * dx + dy * dy < thr2
                    x, y = xn, yn
                record(c, s + 1, m, to, alive, x, y)
    return out


# ------------------------------------------------------------------------------------------------- the cases
def path_graph(S):
    """edges of the path of S + 1 frames: (k, k + 1) for even k, (k + 1, k) for odd k"""
    return [(k, k + 1) if k % 2 == 0 else (k + 1, k) for k in range(S)]


def path_chains(S, C):
    """steps [C,S,4] on path_graph(S): chain 0 walks 0 .. S, chain 1 walks S .. 0, chain 2 goes 0, 1, 0, 1, ..."""
    walks = [list(range(S + 1)), list(range(S, -1, -1)), [t % 2 for t in range(S + 1)]][:C]
    steps = np.zeros((C, S, 4), np.int32)
    for c, walk in enumerate(walks):
        for s, (a, b) in enumerate(zip(walk[:-1], walk[1:])):
            k = min(a, b)
            stored_forward = k % 2 == 0                     # the edge is stored as (k, k + 1)
            steps[c, s] = (a, b, k, int((b > a) != stored_forward))
    return steps


def border_targets(H, W):
    """(fx, fy [H,W] float32, alive [H,W] bool): the flow of the border kind's step 0 and which pixels survive it (H, W >= 3)."""
    fx, fy = np.zeros((H, W), np.float32), np.zeros((H, W), np.float32)
    alive = np.ones((H, W), bool)
    ys, xs = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    inner = (xs > 0) & (xs < W - 1) & (ys > 0) & (ys < H - 1)
    q = (xs + ys) % 4
    fx[inner & (q == 0)] = (W - 1 - xs)[inner & (q == 0)]
    fx[inner & (q == 1)] = -xs[inner & (q == 1)]
    fy[inner & (q == 2)] = (H - 1 - ys)[inner & (q == 2)]
    fy[inner & (q == 3)] = -ys[inner & (q == 3)]
    tiny = np.float32(2.0 ** -126)
    odd_row, odd_col = ys % 2 == 1, xs % 2 == 1
    for sel, field, step in (((xs == W - 1) & odd_row, fx, np.float32(np.spacing(np.float64(W - 1)))), ((xs == 0) & odd_row, fx, -tiny),
                             ((ys == H - 1) & odd_col & ~inner & (xs > 0) & (xs < W - 1), fy, np.float32(np.spacing(np.float64(H - 1)))),
                             ((ys == 0) & odd_col & (xs > 0) & (xs < W - 1), fy, -tiny)):
        field[sel] = step
        alive[sel] = False
    return fx, fy, alive


def _fields(kind, H, W, S, g):
    """(up, down [S,2,H,W] float32, fb_thr)"""
    ys, xs = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    up, down = np.zeros((S, 2, H, W), np.float32), np.zeros((S, 2, H, W), np.float32)
    if kind == "translate":
        up[:, 0], up[:, 1] = 2, 1
        return up, -up, 3.0
    if kind == "halfpix":
        up[:, 0], up[:, 1] = 0.25, -0.5
        return up, -up, 3.0
    if kind == "border":
        if S:
            up[0, 0], up[0, 1], _ = border_targets(H, W)
            down[0] = g.standard_normal((2, H, W))
        return up, down, math.inf
    if kind == "threshold":
        up[:, 0] = 1
        down[:, 0] = 2
        down[:, 1] = np.where((xs + ys) % 2 == 0, 4.0, 3.984375)
        return up, down, 5.0
    if kind == "smooth":
        u, v = xs / W, ys / H
        for k in range(S):
            up[k, 0] = 1.5 + 3 * np.sin(2 * np.pi * (u + 0.5 * v) + k)
            up[k, 1] = 3 * np.cos(2 * np.pi * (v + 0.25 * u) + 0.7 * k)
            # a product of two sinusoids that drifts slowly from edge to edge: below the threshold on about three quarters of the
            # image, and a track that agreed in one step mostly agrees in the next
            wave = 4 * np.sin(2 * np.pi * (1.5 * u + 0.5 * v) + 0.2 * k) * np.sin(2 * np.pi * (v + 0.25 * u) + 0.5 + 0.2 * k)
            down[k, 0] = -up[k, 0] + wave
            down[k, 1] = -up[k, 1] + 0.5 * wave
        return up, down, 3.0
    assert kind == "hostile"
    up, down = (2 * g.standard_normal((S, 2, H, W))).astype(np.float32), (2 * g.standard_normal((S, 2, H, W))).astype(np.float32)
    for f in (up, down):
        r = g.random(f.shape)
        f[r < 0.02] = np.nan
        f[(r >= 0.02) & (r < 0.03)] = np.inf
        f[(r >= 0.03) & (r < 0.04)] = -np.inf
    return up, down, math.inf


def _seeds(kind, H, W, M, g):
    """[M,2] float32 (x, y)"""
    if kind in ("translate", "border", "threshold"):                        # integer pixels
        return np.stack([g.integers(0, W, M), g.integers(0, H, M)], 1).astype(np.float32)
    if kind == "halfpix":                                                  # multiples of 0.25 inside the image
        return np.stack([g.integers(0, 4 * (W - 1) + 1, M), g.integers(0, 4 * (H - 1) + 1, M)], 1).astype(np.float32) / 4
    s = np.stack([g.uniform(0, W - 1, M), g.uniform(0, H - 1, M)], 1).astype(np.float32)
    if kind == "hostile":
        bad = [(np.nan, 0), (0, np.nan), (np.inf, 0), (0, -np.inf), (-1, 0), (0, -0.5), (W, 0), (0, H), (W - 1, H - 1), (0, 0),
               (W - 1, 0), (0, H - 1), (np.float32(W - 1) + np.spacing(np.float32(max(W - 1, 1))), 0)]
        for k in range(0, M, 5):
            s[k] = bad[(k // 5) % len(bad)]
    return s


def make_case(case):
    """dict(xyz, keep, flow_a, flow_b, steps, seeds (None = every pixel), fb_thr, N, edges) of a case"""
    kind, (H, W), M, S, C = case
    g = np.random.default_rng(1000 * KINDS.index(kind) + 7 * H + M + 31 * S + C)
    N = S + 1
    up, down, fb_thr = _fields(kind, H, W, S, g)
    even = (np.arange(S) % 2 == 0)[:, None, None, None]
    flow_a, flow_b = np.where(even, up, down), np.where(even, down, up)
    xyz = g.standard_normal((N, H, W, 3)).astype(np.float32)
    keep = (g.random((N, H, W)) < (0.67 if kind == "hostile" else 0.8)).astype(np.uint8)
    if kind == "hostile":
        r = g.random((N, H, W))
        xyz[r < 0.05, 0] = np.nan
        xyz[(r >= 0.05) & (r < 0.08), 2] = np.inf
        xyz[(r >= 0.08) & (r < 0.1), 1] = -np.inf
    return dict(xyz=xyz, keep=keep, flow_a=np.ascontiguousarray(flow_a, np.float32), flow_b=np.ascontiguousarray(flow_b, np.float32),
                steps=path_chains(S, C), seeds=None if M == ALL else _seeds(kind, H, W, M, g), fb_thr=fb_thr, N=N, edges=path_graph(S))


@functools.lru_cache(maxsize=None)
def ref_case(case):
    """make_case(case) plus ref = track_ref of it, computed once per process and read-only"""
    d = make_case(case)
    d["ref"] = track_ref(d["xyz"], d["keep"], d["flow_a"], d["flow_b"], d["steps"], d["seeds"], d["fb_thr"])
    for v in list(d.values()) + list(d["ref"].values()):
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return d
