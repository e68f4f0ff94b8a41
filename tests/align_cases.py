"""Problem builder for the aligner path tests (tests/test_align_cases_cpu.py, tests/test_gpu_align_paths.py).  numpy only.

The aligner picks its kernel forms from the pixel count P = H * W (P % 4, P against the 1024-pixel chunk) and from the number of
incident edge sides of an image (batches of EB = 8, a 2-deep prefetch).  This module builds problems that reach those forms and
for which a comparison of an fp32 kernel with the float64 oracle is well posed:

  flow_problem        a flow-variant problem in the conventions of tests/test_gpu_align.py (_scene, the config-4 test), with dynamic
                      masks that are really set and, where pxl_thre bites, a guard band around the threshold;
  flow_pixel_losses   float64 restatement of the per-pixel, per-component smooth-L1 value of oracle/align_ref.c's
                      a3r_oracle_flow_loss_grad -- it exists to find the pixels near the threshold;
  degree_class_graph  an edge list whose images have 1, 2, 7, 8, 9, 16 and 17 incident edge sides;
  prior_problem       raw log-depths with a clamped share for the depth prior.

Guard band.  `l < pxl_thre` is a discontinuity; the kernels evaluate l in fp32, the oracle in float64, and one pixel component
counted on one side only moves the flow loss by about pxl_thre / count -- 2e-5 at these sizes against a 1e-6 tolerance.  So every
source pixel for which some incident edge side has a component with |l - pxl_thre| < GUARD * pxl_thre is marked dynamic (masked
out) in its source image.  A pixel's l depends on its own depth and the two cameras only, so masking it changes no other pixel
and one pass is enough.  GUARD = 1e-3 is three orders above the fp32 rounding of l (a few 1e-6 relative at these coordinates).
"""
import numpy as np

GUARD = 1e-3
# Smallest admissible depth of a flow-term point in its target camera (flow_min_qz).  fp32 rounding of qz is about 1e-7 for
# coordinates of order 1 and reaches the flow gradients as 1e-7 / qz^2: 1.6e-6 at 0.25, below the 1e-5 gradient tolerance.
MIN_QZ = 0.25

# H, W: P % 4 = 1, 2, 3 (one short of a chunk), one pixel in the second chunk, fewer pixels than a wave
RAGGED = [(37, 41), (34, 33), (31, 33), (25, 41), (3, 2)]
# P % 4 == 0, P > 1024, P % 1024 != 0: the vectorised forms with a ragged last chunk
VEC_RAGGED = [(36, 44), (40, 52)]

DEGREE_CLASSES = (1, 2, 7, 8, 9, 16, 17)


def complete_graph(N):
    return [(i, j) for i in range(N) for j in range(N) if i != j]


def window_graph(N, width=5):
    """|i - j| <= width, both directions."""
    return [(i, j) for i in range(N) for j in range(N) if i != j and abs(i - j) <= width]


def degrees(edges, N):
    """Incident edge sides per image: an edge (i, j) is one side of i and one side of j."""
    d = np.zeros(N, np.int64)
    for i, j in edges:
        d[i] += 1
        d[j] += 1
    return d


def degree_class_graph():
    """(edges, N): 15 images, 57 directed edges, no edge twice.  Images 0..6 have 17, 16, 9, 8, 7, 2 and 1 incident edge sides:
    against the flow pass's batches of EB = 8 that is two full + odd tail, two full, full + 1, full, one short of full, and the
    2-deep prefetch with an even and an odd count below one batch.  Images 7..14 are the partners (8, 8, 8, 6, 6, 6, 6, 6)."""
    A, B, C, D, E_, two, one = range(7)
    F = list(range(7, 15))
    both = lambda a, b: [(a, b), (b, a)]
    edges = []
    for f in F:
        edges += both(A, f) + both(B, f)
    edges.append((A, one))
    for f in F[:4]:
        edges += both(C, f)
    edges.append((two, C))
    for f in F[4:]:
        edges += both(D, f)
    for f in F[:3]:
        edges += both(E_, f)
    edges.append((E_, two))
    assert len(set(edges)) == len(edges)
    return edges, 15


# ------------------------------------------------------------------------------------------------- ego-flow restatement
def _signed_expm1(x):
    return (np.sign(x) * np.expm1(np.abs(x))).astype(np.float32)


def _pose_rt(im_poses):
    """[N,3,4] = [R | T] in fp32, the arithmetic of the oracle's quat_to_R / signed_expm1f."""
    q = np.asarray(im_poses, np.float32)
    n = np.sqrt(q[:, 0] * q[:, 0] + q[:, 1] * q[:, 1] + q[:, 2] * q[:, 2] + q[:, 3] * q[:, 3])
    x, y, z, w = q[:, 0] / n, q[:, 1] / n, q[:, 2] / n, q[:, 3] / n
    two = np.float32(2)
    tx, ty, tz = two * x, two * y, two * z
    twx, twy, twz = tx * w, ty * w, tz * w
    txx, txy, txz = tx * x, ty * x, tz * x
    tyy, tyz, tzz = ty * y, tz * y, tz * z
    o = np.float32(1)
    R = np.stack([o - (tyy + tzz), txy - twz, txz + twy,
                  txy + twz, o - (txx + tzz), tyz - twx,
                  txz - twy, tyz + twx, o - (txx + tyy)], axis=1).reshape(-1, 3, 3)
    return np.concatenate([R, _signed_expm1(q[:, 4:7])[:, :, None]], axis=2).astype(np.float32)


def flow_pixel_losses(problem, poses=None, dyn=None, with_qz=False):
    """(l, valid): l [E, 2, 2, P] float64, the smooth-L1 value of (edge, direction, component x/y, source pixel) as
    a3r_oracle_flow_loss_grad evaluates it at the problem's initial parameters; valid [E, 2, P], True where the source pixel is not
    dynamic.  Direction 0: source ei -> target ej against flow_ij; direction 1: source ej -> target ei against flow_ji.
    `poses`: [N,3,4] camera-to-world [R | T] (default: computed here in fp32 like the oracle); `dyn`: masks instead of the problem's.
    with_qz: also qz [E, 2, P], the depth of the source pixel's point in the target camera, by which the projection divides."""
    H, W = problem["H"], problem["W"]
    P, N = H * W, problem["N"]
    init, fl = problem["init"], problem["flow"]
    dyn = fl["dyn"] if dyn is None else dyn
    RT = (_pose_rt(init["im_poses"]) if poses is None else np.asarray(poses, np.float32)).astype(np.float64)
    focals = np.asarray(init["im_focals"], np.float32).reshape(-1)
    focals = np.repeat(focals[:1], N) if problem["kw"].get("shared_focal") else focals
    f = np.exp(focals / np.float32(problem["focal_break"])).astype(np.float32).astype(np.float64)
    pp0 = np.asarray([(W / 2, H / 2)] * N, np.float32)
    im_pp = init.get("im_pp")
    pp = (pp0 + 10 * np.asarray(im_pp if im_pp is not None else np.zeros((N, 2)), np.float32)).astype(np.float32).astype(np.float64)
    p = np.arange(P)
    x, y = (p % W).astype(np.float64), (p // W).astype(np.float64)
    depth = np.asarray(init["depth"], np.float32).reshape(N, P).astype(np.float64)
    E = len(problem["edges"])
    l = np.zeros((E, 2, 2, P))
    valid = np.zeros((E, 2, P), bool)
    qzs = np.zeros((E, 2, P))
    for e, (i, j) in enumerate(problem["edges"]):
        for d, (s, t, gt) in enumerate(((i, j, fl["flow_ij"][e]), (j, i, fl["flow_ji"][e]))):
            dp = np.exp(depth[s]) + 1e-6
            Xs = np.stack([dp * ((x - pp[s, 0]) / f[s]), dp * ((y - pp[s, 1]) / f[s]), dp])            # [3, P]
            v = RT[s, :, :3] @ Xs + RT[s, :, 3:4] - RT[t, :, 3:4]
            Y = RT[t, :, :3].T @ v
            qx, qy, qz = f[t] * Y[0] + pp[t, 0] * Y[2], f[t] * Y[1] + pp[t, 1] * Y[2], Y[2] + 1e-6 * dp
            for k, est in enumerate((qx / qz - x, qy / qz - y)):
                dlt = est - np.asarray(gt, np.float32).reshape(2, P)[k].astype(np.float64)
                ad = np.abs(dlt)
                l[e, d, k] = np.where(ad < 1.0, 0.5 * dlt * dlt, ad - 0.5)
            valid[e, d] = ~np.asarray(dyn, bool).reshape(N, P)[s]
            qzs[e, d] = qz
    return (l, valid, qzs) if with_qz else (l, valid)


def flow_min_qz(problem):
    """Smallest target-camera depth qz over the pixels the flow term sees.  The projection divides by qz, so the fp32 rounding of qz
    (about 1e-7 of the point's coordinates, which are of order 1 here) enters the flow values with 1 / qz and their gradients with
    1 / qz^2: a problem with points near a target camera's plane compares rounding noise, not kernels."""
    _, valid, qz = flow_pixel_losses(problem, with_qz=True)
    return float(qz[valid].min())


def flow_sums(l, valid, pxl_thre):
    """The oracle's sums[0..3] = (S_0, C_0, S_1, C_1) from the restated values."""
    inc = (l < float(np.float32(pxl_thre))) & valid[:, :, None, :]          # the oracle takes the threshold as a C float
    return np.asarray([np.where(inc[:, 0], l[:, 0], 0.0).sum(), inc[:, 0].sum(), np.where(inc[:, 1], l[:, 1], 0.0).sum(), inc[:, 1].sum()],
                      np.float64)


def guard_band_mask(problem, dyn, band=GUARD):
    """[N,P] bool: source pixels with a component of some incident edge side within band * pxl_thre of pxl_thre."""
    N, P = problem["N"], problem["H"] * problem["W"]
    thre = float(np.float32(problem["flow"]["pxl_thre"]))
    l, _ = flow_pixel_losses(problem, dyn=dyn)
    near = (np.abs(l - thre) < band * thre).any(axis=2)                   # [E, 2, P]
    out = np.zeros((N, P), bool)
    for e, (i, j) in enumerate(problem["edges"]):
        out[i] |= near[e, 0]
        out[j] |= near[e, 1]
    return out


def flow_problem(N, H, W, edges, seed, *, dyn_frac, pxl_thre, thre, shared_focal, train_pp, full_dynamic=True, guard=True,
                 temporal_smoothing_weight=0.01, start_epoch=0.0):
    """A flow-variant problem: near-identity quaternions, depths around 0 (unit depth), flow fields N(0, 2 px), dynamic masks drawn
    at dyn_frac with the LAST image fully dynamic (full_dynamic), principal-point offsets of about half a pixel with train_pp.
    Where pxl_thre bites (< 1e8) and guard is set, the guard band of the module docstring is added to the dynamic masks.

    Returns a dict: N, H, W, edges, args (positional arguments of AlignEngine / AlignOracle), kw (their keyword arguments, `flow`
    included), flow (the same dict as kw["flow"]), init (set_params arguments), dyn_drawn [N,P] (masks before the guard band),
    guard_mask [N,P] (pixels the guard band added), focal_break."""
    rng = np.random.default_rng(seed)
    E, P = len(edges), H * W
    assert set(range(N)) == {i for e in edges for i in e}, "every image must appear in an edge"
    p1 = rng.standard_normal((E, P, 3), dtype=np.float32)
    p2 = rng.standard_normal((E, P, 3), dtype=np.float32)
    w1 = np.log1p(9 * rng.random((E, P), dtype=np.float32))
    w2 = np.log1p(9 * rng.random((E, P), dtype=np.float32))
    dyn = rng.random((N, P)) < dyn_frac
    if full_dynamic:
        dyn[N - 1] = True
    flow = dict(flow_ij=2 * rng.standard_normal((E, 2, P), dtype=np.float32), flow_ji=2 * rng.standard_normal((E, 2, P), dtype=np.float32),
                dyn=dyn.copy(), weight=0.01, thre=float(thre), start_epoch=float(start_epoch), num_total_iter=50, pxl_thre=float(pxl_thre))
    unit = lambda n, k: (0.05 * rng.standard_normal((n, k))).astype(np.float32)
    pw, im = unit(E, 8), unit(N, 7)
    pw[:, 3] += 1.0
    im[:, 3] += 1.0                                              # quaternions near identity
    init = dict(pw_poses=pw, depth=(0.1 * rng.standard_normal((N, P))).astype(np.float32), im_poses=im,
                im_focals=np.full(N, 20 * np.log(max(H, W)), np.float32))
    if train_pp:
        init["im_pp"] = unit(N, 2)
    kw = dict(shared_focal=bool(shared_focal), temporal_smoothing_weight=float(temporal_smoothing_weight), translation_weight=1.0,
              train_pp=bool(train_pp), flow=flow)
    prob = dict(N=N, H=H, W=W, edges=list(edges), kw=kw, flow=flow, init=init, dyn_drawn=dyn, focal_break=20.0,
                args=([i for i, j in edges], [j for i, j in edges], p1, p2, w1, w2, [(H, W)] * N))
    prob["guard_mask"] = np.zeros((N, P), bool)
    if guard and pxl_thre < 1e8:
        prob["guard_mask"] = guard_band_mask(prob, dyn) & ~dyn
        flow["dyn"] = dyn | prob["guard_mask"]
    return prob


def without_flow(problem):
    """Keyword arguments of the same problem built without the ego-flow term."""
    kw = dict(problem["kw"])
    kw["flow"] = None
    return kw


# ------------------------------------------------------------------------------------------------- depth prior
PRIOR_CLAMP_RAW = -16.0      # exp(-16) = 1.1e-7 < 1e-6: clamped, the prior passes no gradient
PRIOR_FLOOR_RAW = -10.0      # exp(-10) = 4.5e-5 > 1e-6: every other pixel is at least this, nothing is near the clamp


def prior_problem(N, H, W, seed, *, dyn_frac=0.3, clamp_frac=0.1, flow=False):
    """A flow-variant problem (window graph, ego-flow term only with flow=True, then never dropped and with pxl_thre out of reach)
    whose current and initial log-depth maps each have clamp_frac of their pixels at PRIOR_CLAMP_RAW, drawn independently, and all
    others in [-0.3, 1.3] (current) and [-1.5, 1.5] (initial).  The unclamped depths stay of order 1 because the ego-flow term projects
    them into the other cameras, whose centres are about 0.1 away: shallower points come within rounding of a target camera's plane
    (see flow_min_qz; with depths down to exp(-3.5) some lay behind it), and the comparison measured that, not the kernels.
    Adds prior=dict(weight, dyn [N,P], init [N,P]) and clamped [N,P] (current map below the clamp)."""
    edges = window_graph(N)
    prob = flow_problem(N, H, W, edges, seed, dyn_frac=dyn_frac, pxl_thre=1e9, thre=1e9, shared_focal=False, train_pp=False,
                        full_dynamic=False)
    if not flow:
        prob["kw"]["flow"] = None
    rng = np.random.default_rng(seed + 1000)
    P = H * W
    cur = (0.3 + 0.3 * rng.standard_normal((N, P))).clip(-0.3, 1.3).astype(np.float32)
    ini = (cur + 0.3 * rng.standard_normal((N, P))).clip(-1.5, 1.5).astype(np.float32)
    c_cur, c_ini = rng.random((N, P)) < clamp_frac, rng.random((N, P)) < clamp_frac
    cur[c_cur] = PRIOR_CLAMP_RAW
    ini[c_ini] = PRIOR_CLAMP_RAW
    assert cur[~c_cur].min() >= PRIOR_FLOOR_RAW and ini[~c_ini].min() >= PRIOR_FLOOR_RAW
    prob["init"]["depth"] = cur
    # a pixel at exp(-16) sits in its camera's centre, where the ego-flow is ill-conditioned: the flow term does not see it
    prob["flow"]["dyn"] = prob["flow"]["dyn"] | c_cur
    prob["prior"] = dict(weight=0.05, dyn=rng.random((N, P)) < dyn_frac, init=ini)
    prob["clamped"] = c_cur
    assert not flow or flow_min_qz(prob) >= MIN_QZ
    return prob
