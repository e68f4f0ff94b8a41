"""MST initialisation of the global aligner, after dust3r/cloud_opt/init_im_poses.py:69-252.

The reference builds this step on third-party solvers that are not available here -- roma.rigid_points_registration (SVD
Procrustes, :415-418) and cv2.solvePnPRansac with SQPNP (:442-482, stochastic).  This module restates the published algorithms
(weighted Umeyama; PnP with known intrinsics as a closed-form start + robust Gauss-Newton on the reprojection error instead of
RANSAC; both solved on the device by the kernels of csrc/init.hip -- no LAPACK, no host round trip per problem).
PINNED against the reference's own code run on the CPU (tests/golden/mst.npz from make_goldens_mst.py, tests/test_gpu_mst_parity.py):
the edge scores (commons.py:20-25), the spanning tree (scipy.sparse.csgraph) and the walk over it as the verbose lines print it,
the Weiszfeld focals (post_process.py:36-60) with the stale-`i_j` quirk, the chain of registrations, and what init_from_pts3d
(:83-126) writes into the optimiser -- with closed-form stand-ins for two roma functions in the fixture.  The PnP SOLVE has no
parity with cv2 (its RANSAC is stochastic and absent; the fixture replaces it by a recorder): it is pinned to a float64 restatement
of its own algorithm and to ground truth (tests/init_cases.py, tests/test_gpu_init.py) and validated by what it is for: the
alignment loss after initialisation and the recovered geometry on synthetic scenes (tests/test_gpu_api.py).
It is a one-off O(E*P) host-orchestrated step, not the inner loop.
Everything the tree decides -- the spanning tree, the root, the walk with its re-queues, which step gives which image its pose,
which edge gives which image its focal (the quirk included), who goes to PnP, the verbose lines -- depends on the E edge scores
only and is decided ONCE, by plan_spanning_tree (pure host code, tests/test_mst_plan_cpu.py).  Two executors run that plan:
minimum_spanning_tree (torch arithmetic; host inputs, ragged shapes, per-image presets) and _mst_device (launches of liba3r, the
path production takes).  The quaternion formula both tails write is commons.rotmats_to_unitquats.
"""
from __future__ import annotations

from typing import NamedTuple

import numpy as np
import scipy.sparse as sp
import torch

from .commons import rotmat_to_unitquat, rotmats_to_unitquats, signed_log1p


PNP_MAX_POINTS = 16384

# ------------------------------------------------------------------------------------------------ small solvers
def _solve_from_moments(m):
    """[B,17] raw moments (float64, CPU) -> lists of (s, R float32 [3,3], T float32 [3]) : weighted Umeyama in closed form."""
    m = m.double()
    w0 = m[:, 0:1]
    xm, ym = m[:, 1:4] / w0, m[:, 4:7] / w0
    var_x = m[:, 7] / w0[:, 0] - xm.square().sum(-1)
    cov = m[:, 8:17].reshape(-1, 3, 3) / w0[:, :, None] - ym[:, :, None] * xm[:, None, :]
    U, S, Vt = (torch.from_numpy(a) for a in np.linalg.svd(cov.numpy()))      # host path: a handful of camera centres
    d = torch.ones_like(S)
    d[:, 2] = torch.sign(torch.det(U @ Vt))
    R = (U * d[:, None, :]) @ Vt
    s = (S * d).sum(-1) / var_x
    T = ym - s[:, None] * torch.einsum('bij,bj->bi', R, xm)
    return [(float(s[k]), R[k].float(), T[k].float()) for k in range(len(m))]


def umeyama_solve(x, y, w, x_off, y_off, w_off, P):
    """B weighted similarity registrations on the device, no synchronisation: a3r_umeyama_moments (17 float64 moments per problem,
    fixed summation order) + a3r_umeyama_solve (closed form, 3x3 SVD by one-sided Jacobi).  x, y, w flat float32 device tensors, *_off int64
    element offsets [B] (device).  Returns a float32 device tensor [B,13] = (s, R row-major, T)."""
    from ... import _lib
    from ..._lib import check, ptr, stream_ptr
    lib = _lib.load()
    B = int(x_off.numel())
    nch = int(lib.a3r_umeyama_chunks(P))
    partial = torch.empty((B, nch, 17), dtype=torch.float64, device=x.device)
    out = torch.empty((B, 13), dtype=torch.float32, device=x.device)
    with torch.cuda.device(x.device):
        check(lib.a3r_umeyama_moments(ptr(x), ptr(y), ptr(w), ptr(x_off), ptr(y_off), ptr(w_off), B, P, ptr(partial), stream_ptr()),
              "a3r_umeyama_moments")
        check(lib.a3r_umeyama_solve(ptr(partial), nch, B, ptr(out), stream_ptr()), "a3r_umeyama_solve")
    return out


def _unpack_sRT(sol):
    """[13] -> (s 0-d, R [3,3], T [3]) views of one solution."""
    return sol[0], sol[1:10].reshape(3, 3), sol[10:13]


def rigid_points_registration(x, y, w):
    """Weighted Umeyama: (s, R, T) minimising sum w |s R x + T - y|^2 for x, y [P,3], w [P].  Device float32 tensors: solved on
    the device, the result stays there (s is a 0-d tensor).  CPU tensors (the tiny camera-centre problems of
    align_multiple_poses): float64 closed form on the host, s a python float."""
    if not x.is_cuda:
        x, y, w = x.reshape(-1, 3).double(), y.reshape(-1, 3).double(), w.reshape(-1).double()
        m = torch.cat([w.sum()[None], (w[:, None] * x).sum(0), (w[:, None] * y).sum(0), (w * x.square().sum(-1)).sum()[None],
                       torch.einsum('p,pi,pj->ij', w, y, x).reshape(9)])[None]
        return _solve_from_moments(m)[0]
    x, y, w = x.reshape(-1, 3).float().contiguous(), y.reshape(-1, 3).float().contiguous(), w.reshape(-1).float().contiguous()
    zero = torch.zeros(1, dtype=torch.int64, device=x.device)
    return _unpack_sRT(umeyama_solve(x, y, w, zero, zero, zero, x.shape[0])[0])


def rigid_points_registration_batched(X, Y, W, y_index):
    """E registrations in two launches: X [E,P,3] against Y[y_index[e]] ([N,P,3]) with weights W [E,P] (contiguous float32, device).
    Returns the device tensor [E,13] = (s, R row-major, T) per edge."""
    E, P, _ = X.shape
    dev = X.device
    ar = torch.arange(E, device=dev, dtype=torch.int64)
    yi = torch.as_tensor(y_index, device=dev, dtype=torch.int64)
    return umeyama_solve(X, Y, W, ar * (P * 3), yi * (P * 3), ar * P, P)


def inv_rigid(T):
    """Inverse of [..., 4, 4] rigid transforms [R t; 0 1] in closed form: [R^T, -R^T t; 0 1] (no LAPACK call, no synchronisation)."""
    Rt = T[..., :3, :3].transpose(-1, -2)
    out = torch.zeros_like(T)
    out[..., :3, :3] = Rt
    out[..., :3, 3] = -(Rt @ T[..., :3, 3:4])[..., 0]
    out[..., 3, 3] = 1
    return out


def sRT_to_4x4(scale, R, T, device):
    """4x4 similarity from (s, R, T); s may be a python number or a 0-d tensor on `device` (no synchronisation either way)."""
    trf = torch.eye(4, device=device)
    trf[:3, :3] = torch.as_tensor(R, device=device, dtype=torch.float32) * scale
    trf[:3, 3] = torch.as_tensor(T, device=device, dtype=torch.float32).ravel()
    return trf


def geotrf(trf, pts):
    return pts @ trf[:3, :3].T + trf[:3, 3]


def estimate_focals(pts3d):
    """Weiszfeld focals of B pointmaps [B,H,W,3] with the principal point at the centre (post_process.py:36-60), batched on the
    device: one synchronisation for all of them.  Returns a list of B floats.  A list of maps of different shapes is processed
    shape group by shape group."""
    if isinstance(pts3d, (list, tuple)):
        out = [None] * len(pts3d)
        groups = {}
        for k, p in enumerate(pts3d):
            groups.setdefault(tuple(p.shape), []).append(k)
        for ks in groups.values():
            for k, f in zip(ks, estimate_focals(torch.stack([pts3d[k] for k in ks]))):
                out[k] = f
        return out
    B, H, W, _ = pts3d.shape
    if B > 256:                                   # bound the temporaries (a complete 64-frame graph has 4032 pointmaps)
        return [f for k in range(0, B, 256) for f in estimate_focals(pts3d[k:k + 256])]
    dev = pts3d.device
    ys, xs = torch.meshgrid(torch.arange(H, device=dev), torch.arange(W, device=dev), indexing='ij')
    # float64 throughout: a focal is one number per map, and an fp32 Weiszfeld iteration leaves it an ulp or two off the value the
    # reference's arithmetic converges to (measured against its float64 run, tests/test_gpu_mst_parity.py); this path is the fallback
    pixels = torch.stack((xs - W / 2, ys - H / 2), -1).reshape(1, -1, 2).double()
    p = pts3d.reshape(B, -1, 3).double()
    xy_over_z = (p[..., :2] / p[..., 2:3]).nan_to_num(posinf=0, neginf=0)
    dot_xy_px = (xy_over_z * pixels).sum(-1)
    dot_xy_xy = xy_over_z.square().sum(-1)
    focal = dot_xy_px.mean(-1) / dot_xy_xy.mean(-1)
    for _ in range(10):
        dis = (pixels - focal[:, None, None] * xy_over_z).norm(dim=-1)
        wgt = dis.clip(min=1e-8).reciprocal()
        focal = (wgt * dot_xy_px).mean(-1) / (wgt * dot_xy_xy).mean(-1)
    return focal.clip(min=0).cpu().tolist()          # post_process.py:60-61 with the defaults min_focal=0, max_focal=inf


def estimate_focal(pts3d_i):
    """One pointmap [H,W,3] -> focal."""
    return estimate_focals(pts3d_i[None])[0]


def pnp_batched(problems, iterations=10):
    """Camera-to-world poses of B images from their world-space point maps, ONE batch on the device (a3r_pnp_solve, csrc/init.hip) and
    one synchronisation.  problems: list of (pts3d [H,W,3] float32 device, mask [H,W] bool device, focal float, pp (x, y) or None).
    Each problem uses a regular subsample of at most PNP_MAX_POINTS pixels (plenty for a 6-dof fit; the reference's RANSAC draws
    minimal sets).  Returns (info [B,4] numpy: valid, inliers (< 5 px, in front), truncated squared error, focal;  c2w [B,4,4] device)."""
    from ... import _lib
    from ..._lib import check, ptr, stream_ptr
    lib = _lib.load()
    B = len(problems)
    home = problems[0][0].device
    dev = home if home.type == "cuda" else torch.device("cuda")      # the solver runs on the GPU; host tensors are moved there
    rec = np.zeros(B, dtype=np.dtype([('pts', '<u8'), ('msk', '<u8'), ('H', '<i4'), ('W', '<i4'), ('step', '<i4'), ('n', '<i4'),
                                      ('focal', '<f4'), ('ppx', '<f4'), ('ppy', '<f4'), ('pad', '<f4')]))
    assert rec.dtype.itemsize == int(lib.a3r_pnp_desc_bytes())
    keep = []                                                     # the kernels read these buffers: keep them alive until the sync
    for b, (pts, msk, focal, pp) in enumerate(problems):
        H, W, _ = pts.shape
        pts = pts.to(device=dev, dtype=torch.float32).contiguous()
        m8 = msk.to(device=dev, dtype=torch.uint8).contiguous()
        keep += [pts, m8]
        step = -(-(H * W) // PNP_MAX_POINTS)
        c = (W / 2, H / 2) if pp is None else pp
        rec[b] = (pts.data_ptr(), m8.data_ptr(), H, W, step, -(-(H * W) // step), focal, c[0], c[1], 0.0)
    n_max = int(rec['n'].max())
    desc = torch.from_numpy(rec.view(np.uint8).copy()).to(dev)
    work = torch.empty(int(lib.a3r_pnp_work_bytes(B, n_max)), dtype=torch.uint8, device=dev)
    c2w = torch.empty((B, 4, 4), dtype=torch.float32, device=dev)
    info = torch.empty((B, 4), dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        check(lib.a3r_pnp_solve(ptr(desc), B, n_max, iterations, ptr(work), ptr(c2w), ptr(info), stream_ptr()), "a3r_pnp_solve")
    info = info.cpu().numpy()                                     # the one synchronisation
    del keep
    return info, c2w.to(home)


def pnp_focal_candidates(H, W):
    """fast_pnp's focal search (:459-470): 21 focals in geomspace(S / 2, 3 S), S = max(W, H)."""
    return [float(f) for f in np.geomspace(max(W, H) / 2, max(W, H) * 3, 21)]


def linear_pnp_many(items, iterations=10):
    """items: list of (pts3d [H,W,3], focal or None, mask [H,W], pp or None).  focal=None (an image that is never the first view of
    an edge, e.g. the last frame of a non-symmetrised graph): like fast_pnp, try 21 focals and keep the one with the most inliers
    (reprojection error < 5 px, in front of the camera; ties -- every point an inlier for several focals on a smooth scene -- go to
    the smallest truncated squared error).  One device batch for everything.  Returns a list of None | (focal, c2w)."""
    problems, owner = [], []
    for k, (pts, focal, msk, pp) in enumerate(items):
        for f in ([float(focal)] if focal is not None else pnp_focal_candidates(*pts.shape[:2])):
            problems.append((pts, msk, f, pp))
            owner.append(k)
    if not problems:
        return []
    info, c2w = pnp_batched(problems, iterations)
    out = [None] * len(items)
    best = {}
    for b, k in enumerate(owner):
        valid, inl, err, f = info[b]
        if not valid:
            continue
        if items[k][1] is not None:
            if inl > 0:                      # fast_pnp returns None when no pose scores an inlier (`if not best[0]: return None`, :480)
                out[k] = (float(f), c2w[b])
        elif inl > 0 and (k not in best or (inl, -err) > best[k][0]):
            best[k] = ((inl, -err), b)
    for k, (_, b) in best.items():
        out[k] = (float(info[b][3]), c2w[b])
    return out


def linear_pnp(pts3d, focal, msk, pp=None, iterations=10):
    """Camera-to-world pose of an image whose pixels see the world points pts3d [H,W,3] (stands in for fast_pnp :442-482):
    closed-form start + robust Gauss-Newton on the reprojection error, on the device (linear_pnp_many; `iterations` plays the
    role of fast_pnp's niter_PnP).  Returns None | (focal, c2w [4,4])."""
    return linear_pnp_many([(pts3d, focal, msk.to(pts3d.device), pp)], iterations)[0]


# ------------------------------------------------------------------------------------------------ the tree
def compute_edge_scores(edges, conf_i, conf_j):
    """mean(conf_i) * mean(conf_j) per edge (commons.py:20-25); conf_*: per-edge maps (list, or a tensor with a leading E axis)."""
    si = torch.stack([c.float().mean() for c in conf_i]).cpu()
    sj = torch.stack([c.float().mean() for c in conf_j]).cpu()
    return {tuple(e): float(si[k] * sj[k]) for k, e in enumerate(edges)}


class TreePlan(NamedTuple):
    """What init='mst' decides from the edge scores alone (plan_spanning_tree); both executors below run it."""
    root: tuple          # (i, j, k0): the two images placed first and their edge
    root_maps: tuple     # ((side, edge, image),) * 2: the stacked map (side 0 = pred_i, 1 = pred_j) that fills each root image
    keyed: bool          # init_priors: the key pose moves both root maps; image 0 takes the key pose and the key focal
    steps: list          # (edge k, known side 0 = i | 1 = j, known image, new image), in order
    pose_src: dict       # image -> 'eye' | 'key' | index of the step whose (R, T) is its pose
    focal_src: dict      # image -> 'key' | the edge whose first-view Weiszfeld focal it takes
    missing: list        # the images without a pose, ascending: handed to PnP
    lines: list          # (score, i, j, i_is_new, j_is_new) per visited edge: the verbose lines (print_tree_lines)
    requeued: int        # how often the walk put an edge back ("let's try again later")


def plan_spanning_tree(n_imgs, edges, scores, rooted_at_image0=False):
    """The spanning tree over -scores (scipy.sparse.csgraph), its root and the walk over it (:129-252), on the host and from the
    scores alone: no tensor, no device, no printing.  scores: {(i, j): float} for every edge.  rooted_at_image0 (init_priors,
    cloud_opt_flow/init_im_poses.py:173-215): the root is the first tree edge, best first, that touches image 0."""
    edges = [tuple(e) for e in edges]
    eidx = {e: k for k, e in enumerate(edges)}
    graph = sp.dok_array((n_imgs, n_imgs))
    for (i, j), v in scores.items():
        graph[i, j] = -v
    msp = sp.csgraph.minimum_spanning_tree(graph).tocoo()
    todo = sorted(zip(-msp.data, msp.row.tolist(), msp.col.tolist()))
    if rooted_at_image0:
        for _ in range(len(todo)):                # the edges passed over go back to the far end
            score, i, j = todo.pop()
            if i == 0 or j == 0:
                break
            todo.insert(0, (score, i, j))
        assert i == 0 or j == 0, 'every image has an edge, so the spanning forest has one at image 0'
    else:
        score, i, j = todo.pop()
    k0 = eidx[(i, j)]
    root = (i, j, k0)
    if rooted_at_image0 and i != 0:               # j == 0: the reverse edge's maps live in image 0's frame
        kk = eidx[(j, i)]
        root_maps = ((1, kk, i), (0, kk, j))
    else:
        root_maps = ((0, k0, i), (1, k0, j))
    pose_src = {0: 'key'} if rooted_at_image0 else {i: 'eye'}
    focal_src = {0: 'key'} if rooted_at_image0 else {i: k0}
    lines = [(score, i, j, True, True)]
    done, steps, requeued, last_k = {i, j}, [], 0, k0
    while todo:
        score, i, j = todo.pop()
        focal_src.setdefault(i, last_k)           # the reference uses the PREVIOUS edge's map here (:199), re-queued edges included
        if (i in done) == (j in done):
            assert i not in done
            todo.insert(0, (score, i, j))
            requeued += 1
            continue
        k = last_k = eidx[(i, j)]
        steps.append((k, 0, i, j) if i in done else (k, 1, j, i))
        lines.append((score, i, j, i not in done, j not in done))
        done |= {i, j}
        pose_src.setdefault(i, len(steps) - 1)    # always the edge's first image, whichever side is new
    for (i, j), _ in sorted(scores.items(), key=lambda kv: -kv[1]):
        focal_src.setdefault(i, eidx[(i, j)])
    missing = [i for i in range(n_imgs) if i not in pose_src]
    return TreePlan(root, root_maps, bool(rooted_at_image0), steps, pose_src, focal_src, missing, lines, requeued)


def print_tree_lines(plan):
    """The reference's verbose lines: a star marks the image an edge places."""
    for score, i, j, i_new, j_new in plan.lines:
        print(f" init edge ({i}{'*' * i_new},{j}{'*' * j_new}) {score=}")


def _plan_focals(plan, n_imgs, edge_focal, init_priors):
    """Per image: the focal the plan assigns it (None: no edge has it as its first view)."""
    im_focals = [None] * n_imgs
    for img, src in plan.focal_src.items():
        im_focals[img] = float(init_priors[2][0]) if src == 'key' else edge_focal[src]
    return im_focals


def minimum_spanning_tree(imshapes, edges, pred_i, pred_j, conf_i, conf_j, im_conf, min_conf_thr, device, init_priors=None,
                          has_im_poses=True, verbose=True):
    """plan_spanning_tree executed in torch.  pred_* [E,H,W,3], conf_* [E,H,W] device tensors, or per-edge lists when the images
    have different shapes.  Returns (pts3d list, msp_edges, im_focals list, im_poses [N,4,4])."""
    n_imgs = len(imshapes)
    plan = plan_spanning_tree(n_imgs, edges, compute_edge_scores(edges, conf_i, conf_j), init_priors is not None)
    if verbose:
        print_tree_lines(plan)
    edge_focal = estimate_focals(pred_i) if has_im_poses else None      # every edge's Weiszfeld focal of its first view, one batch
    preds, confs = (pred_i, pred_j), (conf_i, conf_j)
    pts3d = [None] * n_imgs
    if plan.keyed:
        keypose = torch.as_tensor(np.array(init_priors[0]).astype(np.float32), device=device)
    for side, k, img in plan.root_maps:
        pts3d[img] = geotrf(keypose, preds[side][k]) if plan.keyed else preds[side][k].clone()
    sols = []
    for k, side, known, new in plan.steps:
        s, R, T = rigid_points_registration(preds[side][k], pts3d[known], confs[side][k])
        pts3d[new] = geotrf(sRT_to_4x4(s, R, T, device), preds[1 - side][k])
        sols.append((R, T))
    msp_edges = [plan.root[:2]] + [tuple(edges[k]) for k, _, _, _ in plan.steps]
    if not has_im_poses:
        return pts3d, msp_edges, None, None
    im_focals = _plan_focals(plan, n_imgs, edge_focal, init_priors)
    im_poses = [None] * n_imgs
    for img, src in plan.pose_src.items():
        im_poses[img] = keypose if src == 'key' else torch.eye(4, device=device) if src == 'eye' else sRT_to_4x4(1, *sols[src], device)
    items = [(pts3d[i], im_focals[i], (im_conf[i] > min_conf_thr).to(device), None) for i in plan.missing]
    for i, res in zip(plan.missing, linear_pnp_many(items)):             # every missing pose in ONE device batch
        if res:
            im_focals[i], im_poses[i] = res
        else:
            im_poses[i] = torch.eye(4, device=device)
    return pts3d, msp_edges, im_focals, torch.stack(im_poses)


def edge_views(scene, dev, preds=None):
    """Per-edge [h,w,3] / [h,w] views of the engine's stacked (zero-filled to max_area) predictions and raw confidences: one
    tensor per edge, shaped like the image it belongs to (side i: image i of the edge, side j: image j)."""
    E = len(scene.edges)
    ci, cj = scene._raw_conf_i.to(dev).reshape(E, -1), scene._raw_conf_j.to(dev).reshape(E, -1)
    pred_i, pred_j = preds if preds is not None else scene._device_predictions(dev)
    if scene._uniform:
        H, W = scene.imshape
        return pred_i.reshape(E, H, W, 3), pred_j.reshape(E, H, W, 3), ci.reshape(E, H, W), cj.reshape(E, H, W)
    sh = scene.imshapes
    pi = [pred_i[e, :sh[i][0] * sh[i][1]].view(*sh[i], 3) for e, (i, j) in enumerate(scene.edges)]
    pj = [pred_j[e, :sh[j][0] * sh[j][1]].view(*sh[j], 3) for e, (i, j) in enumerate(scene.edges)]
    return (pi, pj, [ci[e, :sh[i][0] * sh[i][1]].view(*sh[i]) for e, (i, j) in enumerate(scene.edges)],
            [cj[e, :sh[j][0] * sh[j][1]].view(*sh[j]) for e, (i, j) in enumerate(scene.edges)])


# ------------------------------------------------------------------------------------------------ device fast path
def _signed_log1p_np(x):
    return (np.sign(x) * np.log1p(np.abs(x))).astype(np.float32)


def _mst_device(scene, niter_PnP=10, init_priors=None):
    """init_minimum_spanning_tree + init_from_pts3d for a problem whose images share one shape and whose predictions are on the GPU:
    the same plan (plan_spanning_tree) as minimum_spanning_tree runs, with every per-pixel pass a launch of liba3r (csrc/init_maps.hip, the Umeyama / PnP
    solvers of init.hip) and the algebra on poses / quaternions in numpy on the host from three small read-backs -- no torch
    arithmetic on the device, hence no dependence on which torch kernels (or rocBLAS) a process has loaded so far: the first call
    costs what every later call costs.
    init_priors = [key pose, key depth, [key focal]] (the clip stage of tool/hierarchical.py; cloud_opt_flow/init_im_poses.py:173-215):
    the tree is rooted at the first edge that touches image 0, image 0 gets the key pose and the key focal, and the two root maps
    are moved by the key pose with a3r_sim3_apply reading an uploaded (1, R, T) record -- a launch, like every other map here."""
    import ctypes as C
    from ... import _lib
    from ..._lib import check, ptr, stream_ptr
    from . import _native
    lib = _lib.load()
    eng = scene._need_engine()
    dev = eng.device
    edges = [tuple(e) for e in scene.edges]
    E, N, P = len(edges), scene.n_imgs, scene.max_area
    H, W = scene.imshape
    pred_i, pred_j = scene._device_predictions(dev)                         # [E, P, 3]
    conf_i, conf_j = scene._raw_conf_i, scene._raw_conf_j                    # [E, P]
    # ---- edge scores (commons.py:20-25) and every edge's Weiszfeld focal of its first view: two launches, one read-back each
    mean = scene._edge_conf_mean
    if mean is None:
        _, _, mean = _native.conf_prepare(conf_i, conf_j, 'id', want_weights=False)
    focal_dev = _native.weiszfeld_focal(pred_i.view(E, H, W, 3))
    mean = mean.cpu().numpy()
    edge_focal = focal_dev.cpu().numpy().tolist()
    scores = {e: float(np.float32(mean[2 * k]) * np.float32(mean[2 * k + 1])) for k, e in enumerate(edges)}
    # ---- the walk over the tree is decided on the host (it depends on the scores only), then enqueued: per tree edge one
    # registration of the known side onto the world points so far and one similarity applied to the other side
    plan = plan_spanning_tree(N, edges, scores, init_priors is not None)
    if scene.verbose:
        print_tree_lines(plan)
    steps, preds, confs = plan.steps, (pred_i, pred_j), (conf_i, conf_j)
    pts = torch.empty((N, P, 3), dtype=torch.float32, device=dev)
    at = lambda t, byte: C.c_void_p(t.data_ptr() + byte)
    keypose = None
    if plan.keyed:
        keypose = np.array(init_priors[0]).astype(np.float32)
        rec = np.concatenate(([1.0], keypose[:3, :3].reshape(9), keypose[:3, 3])).astype(np.float32)
        rec_dev = torch.from_numpy(rec).to(dev)
    for side, k, img in plan.root_maps:
        if plan.keyed:
            with torch.cuda.device(dev):
                check(lib.a3r_sim3_apply(at(preds[side], 12 * P * k), ptr(rec_dev), 0, 1.0, at(pts, 12 * P * img), P, stream_ptr()), "a3r_sim3_apply")
        else:
            pts[img].copy_(preds[side][k])
    T = len(steps)
    nch = int(lib.a3r_umeyama_chunks(P))
    st = stream_ptr()
    if T:
        off = np.asarray([[k * P * 3, known * P * 3, k * P] for k, _, known, _ in steps], dtype=np.int64)
        off_dev = torch.from_numpy(np.ascontiguousarray(off.T)).to(dev)          # [3, T]: x, y, w element offsets
        partial = torch.empty((nch, 17), dtype=torch.float64, device=dev)
        tree_sols = torch.empty((T, 13), dtype=torch.float32, device=dev)
        with torch.cuda.device(dev):
            for t, (k, side, known, new) in enumerate(steps):
                check(lib.a3r_umeyama_moments(ptr(preds[side]), ptr(pts), ptr(confs[side]), at(off_dev, 8 * t), at(off_dev, 8 * (T + t)), at(off_dev, 8 * (2 * T + t)),
                                              1, P, ptr(partial), st), "a3r_umeyama_moments")
                check(lib.a3r_umeyama_solve(ptr(partial), nch, 1, at(tree_sols, 52 * t), st), "a3r_umeyama_solve")
                check(lib.a3r_sim3_apply(at(preds[1 - side], 12 * P * k), at(tree_sols, 52 * t), 1, 1.0, at(pts, 12 * P * new), P, st), "a3r_sim3_apply")
    # ---- all E pairwise registrations pred_i[e] -> pts[i] (init_from_pts3d :100-109), enqueued before the first read-back
    offs = np.asarray([[e * P * 3 for e in range(E)], [i * P * 3 for i, _ in edges], [e * P for e in range(E)]], dtype=np.int64)
    offs_dev = torch.from_numpy(offs).to(dev)
    sols = umeyama_solve(pred_i, pts, conf_i, offs_dev[0], offs_dev[1], offs_dev[2], P)
    tree = tree_sols.cpu().numpy() if T else np.zeros((0, 13), np.float32)
    im_poses = np.tile(np.eye(4, dtype=np.float32), (N, 1, 1))
    for img, src in plan.pose_src.items():
        if src == 'key':
            im_poses[img] = keypose
        elif src != 'eye':
            im_poses[img, :3, :3] = tree[src, 1:10].reshape(3, 3)
            im_poses[img, :3, 3] = tree[src, 10:13]
    im_focals = _plan_focals(plan, N, edge_focal, init_priors)
    if plan.missing:                                                         # every missing pose in ONE device batch
        masks = _native.mask_gt(scene._im_conf_stack, scene.min_conf_thr)
        res = linear_pnp_many([(pts[i].view(H, W, 3), im_focals[i], masks[i].view(H, W), None) for i in plan.missing])
        for i, r in zip(plan.missing, res):
            if r:
                im_focals[i] = r[0]
                im_poses[i] = r[1].cpu().numpy()
    sols = sols.cpu().numpy()
    # ---- pairwise poses, global scale, image poses, depth maps, focals: what init_from_pts3d writes into the optimiser (:100-126)
    pw = np.empty((E, 8), np.float32)
    pw[:, 0:4] = rotmats_to_unitquats(sols[:, 1:10].reshape(E, 3, 3))
    pw[:, 4:7] = _signed_log1p_np(sols[:, 10:13] / sols[:, 0:1])
    pw[:, 7] = np.log(sols[:, 0])
    s_factor = float(np.exp(np.float32(np.log(scene.base_scale)) - pw[:, 7].mean(dtype=np.float32))) if scene.norm_pw_scale else 1.0
    im_poses[:, :3, 3] *= np.float32(s_factor)
    if not scene.if_use_mono:
        Rt = np.transpose(im_poses[:, :3, :3], (0, 2, 1))
        w2c = np.concatenate((Rt, -(Rt @ im_poses[:, :3, 3:4])), axis=2).astype(np.float32)          # [N, 3, 4]
        _native.depth_init(pts, torch.from_numpy(np.ascontiguousarray(w2c)).to(dev), s_factor, eng.params['depth'])
    new = dict(pw_poses=torch.from_numpy(pw))
    if eng.flags['train_poses']:
        poses = np.empty((N, 7), np.float32)
        poses[:, 0:4] = rotmats_to_unitquats(im_poses[:, :3, :3])
        poses[:, 4:7] = _signed_log1p_np(im_poses[:, :3, 3])
        new['im_poses'] = torch.from_numpy(poses)
    if eng.flags['train_focals']:
        focals = eng.params['im_focals'].cpu().numpy().copy()
        _write_focal_rows(scene, focals, im_focals, np.zeros(N, bool))
        new['im_focals'] = torch.from_numpy(focals)
    eng.set_params(**new)
    _state_written(scene)


def _shared_focal(im_focals):
    """The one focal of a shared_focal problem: the mean of the per-image estimates (cloud_opt_flow/init_im_poses.py:147-148)."""
    if any(f is None for f in im_focals):      # an image that is no edge's first view and whose PnP failed: the reference's sum() raises too
        raise ValueError('shared_focal: an image got no focal estimate')
    return sum(im_focals) / len(im_focals)


def _write_focal_rows(scene, focals, im_focals, known_focal):
    """The engine's focal rows (tensor or array, written in place): focal_break * log f for every image that has an estimate and
    is not preset; a shared_focal problem has one row, the mean estimate."""
    eng = scene._need_engine()
    if eng.shared_focal:
        if eng.flags['train_focals']:
            focals[0] = scene.focal_break * float(np.log(_shared_focal(im_focals)))
        return
    for i, f in enumerate(im_focals):
        if f is not None and not known_focal[i]:
            focals[i] = scene.focal_break * float(np.log(f))


def _pad_rows(t, P):
    """[n, ...] -> [P, ...], zero-filled (what optimizer._ravel_hw does to a map that is already flat)."""
    return torch.cat((t, t.new_zeros((P - len(t),) + tuple(t.shape[1:])))) if len(t) < P else t


def _quat_rows(R, like):
    """[B,3,3] device rotations -> [B,4] unit quaternions next to `like`: one read-back, commons.rotmats_to_unitquats, one upload."""
    return torch.from_numpy(rotmats_to_unitquats(R.detach().cpu().numpy())).to(device=like.device, dtype=like.dtype)


def _state_written(scene):
    """The end of init_from_pts3d: the flow variant captures the depth maps for its prior BEFORE the loss is evaluated
    (cloud_opt_flow/init_im_poses.py:149-154), then the verbose line."""
    scene._mst_state_written()
    if scene.verbose:
        print(' init loss =', float(scene()))


def _frozen_masks(scene):
    """Per image: is the pose / the focal preset?  (get_known_poses / get_known_focal_mask of the reference.)  The stacked class
    presets all images at once (its train_* flags); ModularPointCloudOptimizer keeps per-image masks in scene._frozen."""
    eng, N = scene._need_engine(), scene.n_imgs
    fz = scene._frozen
    pose = np.ones(N, bool) if not eng.flags['train_poses'] else (fz['pose'].copy() if fz else np.zeros(N, bool))
    focal = np.ones(N, bool) if not eng.flags['train_focals'] else (fz['focal'].copy() if fz else np.zeros(N, bool))
    return pose, focal


def init_minimum_spanning_tree(scene, init_priors=None, niter_PnP=10):
    """init_minimum_spanning_tree + init_from_pts3d (:69-126) on a mirror PointCloudOptimizer that is already on a device."""
    eng = scene._need_engine()
    dev = eng.device
    known_pose, known_focal = _frozen_masks(scene)
    fz = scene._frozen
    per_image = fz is not None and (fz['pose'].any() or fz['focal'].any())       # the device path knows handle-wide switches only
    if scene._fast and eng.flags['train_poses'] and scene.n_imgs > 1 and not per_image:
        return _mst_device(scene, niter_PnP, init_priors)
    E, N, P = len(scene.edges), scene.n_imgs, scene.max_area
    stacked = scene._device_predictions(dev)               # held to the end of this function: the registrations below read side i again
    pred_i, pred_j, conf_i, conf_j = edge_views(scene, dev, stacked)
    pts3d, _, im_focals, im_poses = minimum_spanning_tree(scene.imshapes, scene.edges, pred_i, pred_j, conf_i, conf_j, scene.im_conf,
                                                          scene.min_conf_thr, dev, init_priors=init_priors, verbose=scene.verbose)
    # ---- init_from_pts3d (:83-126); the known-poses branch (nkp > 1) re-aligns everything on the preset poses
    nkp = int(known_pose.sum())
    if nkp == 1:
        raise NotImplementedError('Would be simpler to just align everything afterwards on the single known pose')
    if nkp > 1:
        # one global similarity carries the tree's cameras and pointmaps onto the known poses (:88-99); the preset poses themselves
        # are left alone below, as _set_pose without force does
        kp = torch.from_numpy(known_pose).to(im_poses.device)
        s, R, T = align_multiple_poses(im_poses[kp], scene.get_im_poses().to(im_poses.device)[kp])
        trf = sRT_to_4x4(s, R, T, dev)
        im_poses = trf @ im_poses
        im_poses[:, :3, :3] /= s
        pts3d = [geotrf(trf, p.reshape(-1, 3)).reshape(p.shape) for p in pts3d]
    pw = eng.params['pw_poses'].clone()
    # all E pairwise registrations pred_i[e] -> pts3d[i] in ONE launch of the moments kernel + one batched 3x3 SVD
    # (stacked buffers zero-filled to max_area; the padded tail carries zero confidence = zero weight)
    sols = rigid_points_registration_batched(stacked[0].reshape(E, P, 3),
                                             torch.stack([_pad_rows(p.reshape(-1, 3).float(), P) for p in pts3d]).contiguous(),
                                             scene._raw_conf_i.to(dev).reshape(E, P).float().contiguous(), [i for i, _ in scene.edges])
    pw[:, 0:4] = _quat_rows(sols[:, 1:10].reshape(E, 3, 3), pw)
    pw[:, 4:7] = signed_log1p(sols[:, 10:13] / sols[:, 0:1])
    pw[:, 7] = sols[:, 0].log()
    s_factor = torch.exp(np.log(scene.base_scale) - pw[:, 7].mean()) if scene.norm_pw_scale else 1.0      # stays on the device
    im_poses = im_poses.clone()
    im_poses[:, :3, 3] *= s_factor
    pts3d = [p * s_factor for p in pts3d]
    poses = eng.params['im_poses'].clone()
    depth = eng.params['depth'].clone()
    focals = eng.params['im_focals'].clone()
    if not scene.if_use_mono:
        w2c = inv_rigid(im_poses)
        for i in range(N):
            d = geotrf(w2c[i], pts3d[i].reshape(-1, 3))[:, 2]
            depth[i] = _pad_rows(d, P).log().nan_to_num(neginf=0)  # _set_depthmap: _ravel_hw zero-fill, log(0) -> 0
    free = torch.from_numpy(~known_pose).to(poses.device)
    if free.any():
        poses[free, 0:4] = _quat_rows(im_poses[:, :3, :3], poses)[free]
        poses[free, 4:7] = signed_log1p(im_poses[:, :3, 3])[free].to(poses.dtype)
    _write_focal_rows(scene, focals, im_focals, known_focal)
    eng.set_params(pw_poses=pw, depth=depth, im_poses=poses, im_focals=focals)
    _state_written(scene)


# ------------------------------------------------------------------------------------------------ known poses
def align_multiple_poses(src_poses, target_poses):
    """(s, R, T) registering camera centres + a point on each optical axis of src onto target (init_im_poses.py:503-511)."""
    def center_and_z(poses):
        c = poses[:, :3, 3].double().cpu()
        n = len(c)
        d = [float((c[i] - c[j]).norm()) for i in range(n) for j in range(i + 1, n)]
        eps = float(np.median(d)) / 100 if d else 0.0                 # get_med_dist_between_poses / 100
        return torch.cat((c, c + eps * poses[:, :3, 2].double().cpu()))
    x, y = center_and_z(src_poses), center_and_z(target_poses)
    return rigid_points_registration(x, y, torch.ones(len(x), dtype=torch.float64))


def init_from_known_poses(scene, niter_PnP=10, min_conf_thr=3):
    """init='known_poses' (init_im_poses.py:27-66): every image pose and focal is preset; each pairwise pose is the similarity that
    carries the pair's two predicted cameras (identity and the PnP pose of view 2) onto the known ones, each depth map the
    best-confidence pairwise prediction at that scale.  PnP is the linear stand-in above (cv2 absent): parity unpinned."""
    eng = scene._need_engine()
    dev = eng.device
    if eng.flags['train_poses']:
        raise AssertionError('not all poses are known')
    if eng.flags['train_focals']:
        raise AssertionError('not all focals are known')          # the reference asserts nkf == n_imgs
    E, P = len(scene.edges), scene.max_area
    pred_i, pred_j, conf_i, _ = edge_views(scene, dev)
    known_poses = scene.get_im_poses()
    im_focals = scene.get_focals().reshape(-1)
    im_pp = scene.get_principal_points()
    pw = eng.params['pw_poses'].clone()
    best = {}
    cmin = [float(c.min()) for c in conf_i]
    focals_h, pp_h = im_focals.cpu().tolist(), im_pp.cpu().tolist()
    pnp = linear_pnp_many([(pred_j[e], focals_h[i], conf_i[e] > min(min_conf_thr, cmin[e] - 0.1), (pp_h[i][0], pp_h[i][1]))
                           for e, (i, j) in enumerate(scene.edges)])
    for e, (i, j) in enumerate(scene.edges):
        P1 = torch.eye(4, device=dev)
        if pnp[e] is None:
            raise RuntimeError(f'PnP failed on edge ({i},{j})')
        P2 = pnp[e][1]
        s, R, T = align_multiple_poses(torch.stack((P1, P2)), known_poses[[i, j]])
        pw[e, 0:4] = rotmat_to_unitquat(R).to(dev)
        pw[e, 4:7] = signed_log1p(T.to(dev) / s)
        pw[e, 7] = float(np.log(s))
        score = float(conf_i[e].mean())
        if score > best.get(i, (0,))[0]:
            best[i] = (score, e, s)
    depth = eng.params['depth'].clone()
    if not scene.if_use_mono:
        for n in range(scene.n_imgs):
            _, e, s = best[n]
            depth[n] = _pad_rows(pred_i[e][:, :, 2].reshape(-1) * s, P).log().nan_to_num(neginf=0)
    eng.set_params(pw_poses=pw, depth=depth)
