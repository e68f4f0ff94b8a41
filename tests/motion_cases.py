"""Scenes, oracle and agreement rule for the motion-mask tests (tests/test_motion_cpu.py, tests/test_gpu_motion.py).  numpy only.

Scenes.  N ground-truth pinholes on a shallow arc look at a wavy surface; the optical flow of every edge is the true ego flow plus
a rectangle that "moves" 6 px and a region whose extra motion ramps linearly from 0 to 6 px, so that pixels sit on both sides of the
threshold close to it.  The pair geometry is INJECTED (true intrinsics and relative poses, no PnP), in both of PairViewer's forms:
pairs alternate between "camera i is the world frame" (depth_i = z of pred_i[e], depth_j = z of inv(rel) applied to pred_j[e]) and
"camera j is" (depth_i = z of inv(rel) applied to pred_j[e + M], depth_j = z of pred_i[e + M]).  The edges come in the symmetric
order the reference requires: M forward edges, then their reverses.

Oracle.  `oracle` restates cloud_opt_flow/optimizer.py:207-235 in float64 on the fp32-rounded inputs of the mask kernels: the table
of directed entries (ops.MOTION_ENTRY: depth row and (r, t), H = K_tgt R_rel K_src^-1, K_tgt t_rel), the stacked pointmaps, the
flow fields, the per-image entry lists and the threshold.  It returns the mean normalised error per image and FLAGS every pixel
whose decision a rounding error of an fp32 evaluation could change.

eps.  The fp32 evaluation of err = |tgt_xy - (x, y) - flow| does about ten roundings (the dot product for the depth, the reciprocal,
three multiply-adds, the division, two subtractions, the norm), each of relative size 2^-24 on intermediate values no larger than
S_e = max(W, H, the largest finite |coordinate| of tgt and |flow| of the entry); the materialised depth map of the torch function
(an fp32 geotrf) and the host-built fp32 H add a few more of the same size.  Bound: delta_e = 32 * 2^-24 * S_e on every err of
entry e.  With R_e = max - min, nerr = (err - min) / R_e moves by at most (delta + delta) / R_e + nerr * 2 delta / R_e <= 4 delta_e /
R_e; the mean over an image's entries by at most the largest of these, plus deg * 2^-24 for the summation:
    eps_n = max over the entries e of image n of 4 * delta_e / R_e  +  (deg_n + 2) * 2^-24.
A pixel of image n is flagged when |mean - thre| <= eps_n.  Every pixel of image n is flagged when one of its entries has
0 < R_e <= 4 delta_e (a range the rounding noise can reach; R_e == 0 exactly, which only an exactly representable constant map gives,
is NaN in every evaluation and is compared as NaN).

Agreement rule (`check_agreement`): the mask equals the oracle's on unflagged pixels; either value on flagged ones; the mean stays
within eps_n of the oracle's wherever that is finite; NaN exactly where the oracle has NaN (and the mask is False there).
"""
import numpy as np

MAX_FLAGGED = 0.05            # the cap: a scene with more flagged pixels tests nothing
THRE = 0.35
ROUNDINGS = 32

ENTRY = np.dtype([('depth_row', '<i4'), ('flow_row', '<i4'), ('image', '<i4'), ('pad', '<i4'), ('depth_rt', '<f4', (4,)),
                  ('Hm', '<f4', (9,)), ('Kt', '<f4', (3,))])          # = align3r_amd.ops.MOTION_ENTRY (asserted in the tests)

# name: (N, graph, H, W, keyword arguments of make_scene)
SCENES = {
    "2x(5x7)": (2, "complete", 5, 7, dict(rect=(1, 3, 1, 4), ramp=(3, 5, 0, 7))),                  # fewer pixels than a wave, P % 4 != 0, M = 1
    "3x(37x41)": (3, "complete", 37, 41, dict()),                                                    # scalar tail, degree 2 everywhere
    "5x(36x44)": (5, "swin-2-noncyclic", 36, 44, dict()),                                            # vector loads, degrees 2 to 4
    "4x(40x52)": (4, "complete", 40, 52, dict(rect=(30, 38, 8, 30), ramp=(22, 27, 4, 48), offset=0.5, calm=(0, 4, 0, 52))),
}


def forward_edges(N, graph):
    if graph == "complete":
        return [(i, j) for i in range(N) for j in range(i + 1, N)]
    if graph == "swin-2-noncyclic":
        return [(i, j) for i in range(N) for j in (i + 1, i + 2) if j < N]
    raise KeyError(graph)


def vote_lists(edges, N):
    """cloud_opt_flow/optimizer.py:228-232: e ascending, err_i[e] (entry e) to image edges[e][0], err_j[e] (entry M + e) to edges[e][1]."""
    M = len(edges) // 2
    lists = [[] for _ in range(N)]
    for e in range(M):
        lists[edges[e][0]].append(e)
        lists[edges[e][1]].append(M + e)
    return lists


def make_scene(N, graph, H, W, rect=None, ramp=None, offset=0.0, calm=None, seed=0):
    """dict(edges, pred_i, pred_j [E,H,W,3], conf [E,H,W], flow_ij, flow_ji [E,2,H,W], K [N,3,3], c2w [N,4,4], geom, lists, moving, ...),
    everything float32.  rect / ramp = (y0, y1, x0, x1); offset: a constant extra flow everywhere except inside `calm` (puts the
    minimum of every error map inside `calm` and leaves the maximum in the rectangle)."""
    rng = np.random.default_rng(seed)
    rect = rect or (H // 4, H // 4 + H // 3, W // 5, W // 5 + W // 3)
    ramp = ramp or (H - H // 4, H - H // 4 + max(H // 8, 1), 2, W - 2)
    mid = (N - 1) / 2
    f = np.float32(1.25 * max(H, W))
    K = np.zeros((N, 3, 3), np.float32)
    K[:, 0, 0] = K[:, 1, 1] = f
    K[:, 0, 2], K[:, 1, 2], K[:, 2, 2] = W / 2, H / 2, 1
    c2w = np.zeros((N, 4, 4))
    depth = []
    xs, ys = np.meshgrid(np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64))
    for n in range(N):
        a = 0.05 * (n - mid)
        c2w[n] = np.eye(4)
        c2w[n, :3, :3] = [[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]]
        c2w[n, :3, 3] = [0.15 * (n - mid), 0.01 * n, 0.0]
        depth.append(3 + 0.5 * np.sin(xs * 16.0 / W / 3.0 + n) + 0.2 * np.cos(ys * 8.0 / H + 0.5 * n))
    c2w = c2w.astype(np.float32).astype(np.float64)
    Kd = K.astype(np.float64)
    world = []
    for n in range(N):
        cam = np.stack([(xs - Kd[n, 0, 2]) / Kd[n, 0, 0], (ys - Kd[n, 1, 2]) / Kd[n, 1, 1], np.ones_like(xs)], -1) * depth[n][..., None]
        world.append(cam @ c2w[n, :3, :3].T + c2w[n, :3, 3])
    to_cam = lambda X, n: (X - c2w[n, :3, 3]) @ c2w[n, :3, :3]

    def true_flow(i, j):
        c = to_cam(world[i], j)
        return np.stack([Kd[j, 0, 0] * c[..., 0] / c[..., 2] + Kd[j, 0, 2] - xs, Kd[j, 1, 1] * c[..., 1] / c[..., 2] + Kd[j, 1, 2] - ys])

    extra = np.full((H, W), float(offset))
    if calm:
        extra[calm[0]:calm[1], calm[2]:calm[3]] = 0.0
    moving = np.zeros((H, W), bool)
    moving[rect[0]:rect[1], rect[2]:rect[3]] = True
    extra[moving] = 6.0
    y0, y1, x0, x1 = ramp
    extra[y0:y1, x0:x1] = np.maximum(extra[y0:y1, x0:x1], 6.0 * (np.arange(x0, x1) - x0) / max(x1 - 1 - x0, 1))
    fwd = forward_edges(N, graph)
    edges = fwd + [(j, i) for i, j in fwd]
    E, M = len(edges), len(fwd)
    pred_i = np.stack([to_cam(world[i], i) for i, j in edges]).astype(np.float32)
    pred_j = np.stack([to_cam(world[j], i) for i, j in edges]).astype(np.float32)
    flow_ij = np.stack([true_flow(i, j) for i, j in edges])
    flow_ji = np.stack([true_flow(j, i) for i, j in edges])
    flow_ij[:, 0] += extra
    flow_ji[:, 0] += extra
    conf = (1 + 5 * rng.random((E, H, W))).astype(np.float32)
    # injected pair geometry, alternating between PairViewer's two forms
    rel = lambda a, b: (np.linalg.inv(c2w[b]) @ c2w[a]).astype(np.float32)          # pose of camera a in the frame of camera b
    eye = np.eye(4, dtype=np.float32)
    z = np.asarray([0, 0, 1, 0], np.float32)
    pose_i, pose_j, row_i, row_j, rt_i, rt_j = [], [], [], [], [], []
    for e, (i, j) in enumerate(fwd):
        if e % 2 == 0:          # the pair's point cloud is expressed in camera i
            r = rel(j, i)
            pose_i.append(eye); pose_j.append(r)
            row_i.append(e); rt_i.append(z)
            row_j.append(E + e); rt_j.append(np.linalg.inv(r.astype(np.float64))[2].astype(np.float32))
        else:                   # in camera j
            r = rel(i, j)
            pose_i.append(r); pose_j.append(eye)
            row_i.append(E + e + M); rt_i.append(np.linalg.inv(r.astype(np.float64))[2].astype(np.float32))
            row_j.append(e + M); rt_j.append(z)
    geom = dict(K_i=np.stack([K[i] for i, j in fwd]), K_j=np.stack([K[j] for i, j in fwd]), pose_i=np.stack(pose_i), pose_j=np.stack(pose_j),
                depth_i=(np.asarray(row_i, np.int64), np.stack(rt_i)), depth_j=(np.asarray(row_j, np.int64), np.stack(rt_j)))
    return dict(N=N, H=H, W=W, edges=edges, pred_i=pred_i, pred_j=pred_j, conf=conf, flow_ij=flow_ij.astype(np.float32),
                flow_ji=flow_ji.astype(np.float32), K=K, c2w=c2w.astype(np.float32), geom=geom, lists=vote_lists(edges, N), moving=moving)


def entries_from_geometry(geom, edges, E):
    """The table of directed entries in float64 arithmetic, rounded to fp32 (the tests use the package's own fp32 host construction,
    cloud_opt_flow.optimizer.motion_entries; this one serves the oracle-only checks and must agree with it to fp32 rounding)."""
    M = len(edges) // 2
    d = lambda a: np.asarray(a, np.float64)
    rec = np.zeros(2 * M, ENTRY)
    sides = ((d(geom['pose_i']), d(geom['pose_j']), d(geom['K_j']), d(geom['K_i']), geom['depth_i'], 0, 0),
             (d(geom['pose_j']), d(geom['pose_i']), d(geom['K_i']), d(geom['K_j']), geom['depth_j'], E, 1))
    for half, (src, tgt, K, K_src, (row, rt), flow0, side) in enumerate(sides):
        for e in range(M):
            Rt = tgt[e, :3, :3].T
            rel_R, rel_t = Rt @ src[e, :3, :3], Rt @ (src[e, :3, 3] - tgt[e, :3, 3])
            k = half * M + e
            rec['Hm'][k] = (K[e] @ rel_R @ np.linalg.inv(K_src[e])).reshape(9)
            rec['Kt'][k] = K[e] @ rel_t
            rec['depth_row'][k], rec['depth_rt'][k] = row[e], rt[e]
            rec['flow_row'][k], rec['image'][k] = flow0 + e, edges[e][side]
    return rec


def depth_maps(sc):
    """The materialised fp32 depth maps D_i, D_j [M,H,W] a PairViewer would hand out for the injected geometry (geotrf in fp32)."""
    pts = np.concatenate([sc['pred_i'], sc['pred_j']])
    out = []
    for row, rt in (sc['geom']['depth_i'], sc['geom']['depth_j']):
        rt = np.asarray(rt, np.float32)
        out.append(np.stack([(pts[r] @ t[:3] + t[3]).astype(np.float32) for r, t in zip(row, rt)]))
    return out


def oracle(entries, pred_i, pred_j, flow_ij, flow_ji, lists, H, W, thre=THRE):
    """(mean [N,H,W] float64, mask [N,H,W] bool, flagged [N,H,W] bool, info).  entries: ENTRY records; pred_* [E,H*W,3] or [E,H,W,3];
    flow_* [E,2,H,W]; lists: per image its entries in averaging order."""
    N, P = len(lists), H * W
    pts = np.concatenate([np.asarray(pred_i, np.float32).reshape(-1, P, 3), np.asarray(pred_j, np.float32).reshape(-1, P, 3)]).astype(np.float64)
    flow = np.concatenate([np.asarray(flow_ij, np.float32).reshape(-1, 2, P), np.asarray(flow_ji, np.float32).reshape(-1, 2, P)]).astype(np.float64)
    thre32 = float(np.float32(thre))
    p = np.arange(P)
    x, y = (p % W).astype(np.float64), (p // W).astype(np.float64)
    one = np.ones(P)
    eps32 = float(np.float32(1e-6))
    ulp = 2.0 ** -24
    nerr, tol, rng_info = [], [], []
    with np.errstate(all="ignore"):
        for k, r in enumerate(entries):
            rt, Hm, Kt = r['depth_rt'].astype(np.float64), r['Hm'].astype(np.float64).reshape(3, 3), r['Kt'].astype(np.float64)
            D = pts[r['depth_row']] @ rt[:3] + rt[3]
            disp = 1.0 / (D + eps32)
            tgt = Hm @ np.stack([x, y, one]) + disp[None, :] * Kt[:, None]
            tq = tgt / (tgt[2:3] + eps32)
            fl = flow[r['flow_row']]
            err = np.sqrt((tq[0] - x - fl[0]) ** 2 + (tq[1] - y - fl[1]) ** 2)
            mn, mx = np.min(err), np.max(err)                      # NaN propagates, as amin / amax
            R = mx - mn
            nerr.append((err - mn) / R)
            mags = np.concatenate([np.abs(tgt).ravel(), np.abs(tq).ravel(), np.abs(fl).ravel()])
            S = max(float(W), float(H), float(mags[np.isfinite(mags)].max(initial=0.0)))
            delta = ROUNDINGS * ulp * S
            tol.append((4 * delta / R if np.isfinite(R) and R > 0 else np.nan, bool(np.isfinite(R) and 0 < R <= 4 * delta)))
            rng_info.append((float(mn), float(mx), int(np.argmin(err)) if np.isfinite(R) else -1, int(np.argmax(err)) if np.isfinite(R) else -1))
        mean = np.zeros((N, P))
        flagged = np.zeros((N, P), bool)
        eps = np.zeros(N)
        for n, l in enumerate(lists):
            acc = np.zeros(P)
            for k in l:
                acc = acc + nerr[k]
            mean[n] = acc / len(l)
            e_n = max((tol[k][0] for k in l if np.isfinite(tol[k][0])), default=0.0) + (len(l) + 2) * ulp
            eps[n] = e_n
            flagged[n] = np.abs(mean[n] - thre32) <= e_n
            if any(tol[k][1] for k in l):
                flagged[n] = True
        mask = mean > thre32
    info = dict(eps=eps, flagged=float(flagged.mean()), masked=[float(m.mean()) for m in mask], ranges=rng_info,
                nan_images=[n for n in range(N) if np.isnan(mean[n]).any()])
    return mean.reshape(N, H, W), mask.reshape(N, H, W), flagged.reshape(N, H, W), info


def check_agreement(got_mask, got_mean, mean, mask, flagged, info):
    """Asserts the agreement rule; got_mean may be None.  Returns the number of flagged pixels on which got_mask differs."""
    got_mask = np.asarray(got_mask).astype(bool).reshape(mask.shape)
    wrong = (got_mask != mask) & ~flagged
    assert not wrong.any(), (int(wrong.sum()), np.argwhere(wrong)[:5].tolist())
    nan = np.isnan(mean)
    assert not got_mask[nan].any(), "a pixel whose mean is NaN is masked"
    if got_mean is not None:
        got_mean = np.asarray(got_mean, np.float64).reshape(mean.shape)
        assert np.array_equal(np.isnan(got_mean), nan), "NaN does not sit where the oracle has it"
        fin = np.isfinite(mean)
        dev = np.where(fin, np.abs(got_mean - mean), 0.0)
        assert (dev <= info["eps"][:, None, None]).all(), (float(dev.max()), info["eps"].tolist())
    return int(((got_mask != mask) & flagged).sum())


def assert_cap(info, mask, nan_case=False):
    """The conditions under which a scene is a test at all."""
    assert info["flagged"] <= MAX_FLAGGED, info["flagged"]
    if not nan_case:
        for n, m in enumerate(mask):
            assert m.any() and not m.all(), (n, "an image needs a masked and an unmasked pixel")
