"""Goldens of the ModularPointCloudOptimizer (dust3r/cloud_opt/modular_optimizer.py) -> tests/golden/alignmod.npz / .json.

    python tests/golden/make_goldens_modular.py [--out tests/golden]

Drives the reference's class on the CPU with the stand-ins that make_goldens.py installs (this file imports its helpers and
does not edit it).  _set_pose needs roma.rotmat_to_unitquat, which that stand-in lacks: a closed-form one (largest-component
branch selection, float64, XYZW) is added here and named in the metadata.  The reference's global_aligner() cannot build the
modular class (it forgets two constructor arguments), so the class is constructed directly.

Layout per case `tag` (as alignx.*): inputs per edge (shared between cases of the same shapes, named in the JSON), the
seed-17 initial state, the start state after the presets (and the adaptor perturbation), derived matrices and world points, loss0 with its per-edge sums, autograd gradients (rows of frozen
parameters are zero; the masks are in the JSON), the parameters after 1 / 5 / 50 iterations of the reference's own loop and
the loss curve.  Per-image parameters are stacked: depth [N, max_area] zero-filled like _ravel_hw.
"""
from __future__ import annotations

import argparse
import json
import os
import sys

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import numpy as np
import torch

import make_goldens as mg

SHAPE = (12, 16)
MIXED = [(12, 16), (12, 16), (10, 12), (14, 10)]
# tag, shapes, dist, kwargs of the class, presets; a preset is (kind, mask as the caller writes it)
CASES = [
    dict(tag="none", shapes=[SHAPE] * 4, dist="l1", kw={}, presets=[]),
    dict(tag="pose1", shapes=[SHAPE] * 4, dist="l1", kw={}, presets=[("pose", 1)]),
    dict(tag="pose2", shapes=[SHAPE] * 5, dist="l1", kw={}, presets=[("pose", [True, False, False, True, False])]),
    dict(tag="intr", shapes=[SHAPE] * 4, dist="l1", kw=dict(optimize_pp=True), presets=[("intrinsics", "int64:1,2")]),
    dict(tag="mixed", shapes=MIXED, dist="l2", kw={}, presets=[("pose", 2), ("focal", [0])]),
    dict(tag="adapt", shapes=[SHAPE] * 4, dist="l1", kw=dict(allow_pw_adaptors=True),
         presets=[("pose", "bool:1,0,1,0"), ("focal", None), ("pp", [3])]),
]


def rotmat_to_unitquat(R):
    """Rotation matrix -> XYZW unit quaternion, closed form with the largest-component branch selection (float64)."""
    R = torch.as_tensor(R, dtype=torch.float64)
    m00, m01, m02, m10, m11, m12, m20, m21, m22 = R.reshape(9).tolist()
    tr = m00 + m11 + m22
    if tr > 0:
        s = np.sqrt(tr + 1.0) * 2
        q = ((m21 - m12) / s, (m02 - m20) / s, (m10 - m01) / s, 0.25 * s)
    elif m00 > m11 and m00 > m22:
        s = np.sqrt(1.0 + m00 - m11 - m22) * 2
        q = (0.25 * s, (m01 + m10) / s, (m02 + m20) / s, (m21 - m12) / s)
    elif m11 > m22:
        s = np.sqrt(1.0 + m11 - m00 - m22) * 2
        q = ((m01 + m10) / s, 0.25 * s, (m12 + m21) / s, (m02 - m20) / s)
    else:
        s = np.sqrt(1.0 + m22 - m00 - m11) * 2
        q = ((m02 + m20) / s, (m12 + m21) / s, 0.25 * s, (m10 - m01) / s)
    return torch.tensor(q, dtype=torch.float32)


def decode_mask(m):
    """The mask object a caller would pass: 'int64:1,2' -> integer array, 'bool:1,0,1,0' -> boolean array, else as written."""
    if isinstance(m, str):
        kind, vals = m.split(":")
        vals = [int(v) for v in vals.split(",")]
        return np.asarray(vals, dtype=np.int64) if kind == "int64" else np.asarray(vals, dtype=bool)
    return m


def known_values(N, shapes, seed):
    """Deterministic known cameras for every image (a preset takes the ones its mask selects)."""
    rng = np.random.default_rng(seed)
    poses = np.zeros((N, 4, 4), np.float32)
    for n in range(N):
        q = rng.standard_normal(4)
        x, y, z, w = q / np.linalg.norm(q)
        poses[n, :3, :3] = [[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                            [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                            [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]]
        poses[n, :3, 3] = rng.standard_normal(3)
        poses[n, 3, 3] = 1
    focals = np.asarray([1.1 * max(h, w) + 0.5 * n for n, (h, w) in enumerate(shapes)], np.float32)
    pps = np.asarray([(w / 2 + 1.5 - n, h / 2 - 2.0 + 0.5 * n) for n, (h, w) in enumerate(shapes)], np.float32)
    return poses, focals, pps


def stack_params(net, P):
    rav = lambda t: torch.cat((t.reshape(-1), t.new_zeros(P - t.numel())))
    d = dict(pw_poses=net.pw_poses, pw_adaptors=net.pw_adaptors,
             depth=torch.stack([rav(p) for p in net.im_depthmaps]), im_poses=torch.stack(list(net.im_poses)),
             im_focals=torch.stack([p.reshape(()) for p in net.im_focals]), im_pp=torch.stack(list(net.im_pp)))
    return {k: v.detach().numpy().copy() for k, v in d.items()}


def stack_grads(net, P):
    z = lambda p: torch.zeros_like(p) if p.grad is None else p.grad
    rav = lambda t: torch.cat((t.reshape(-1), t.new_zeros(P - t.numel())))
    d = dict(pw_poses=z(net.pw_poses), pw_adaptors=z(net.pw_adaptors),
             depth=torch.stack([rav(z(p)) for p in net.im_depthmaps]), im_poses=torch.stack([z(p) for p in net.im_poses]),
             im_focals=torch.stack([z(p).reshape(()) for p in net.im_focals]), im_pp=torch.stack([z(p) for p in net.im_pp]))
    return {k: v.detach().numpy().copy() for k, v in d.items()}


def generate(out):
    mg.import_reference(aligner=True)
    sys.modules["roma"].rotmat_to_unitquat = rotmat_to_unitquat
    from dust3r.cloud_opt.modular_optimizer import ModularPointCloudOptimizer
    from dust3r.cloud_opt.base_opt import global_alignment_iter
    from dust3r.utils.geometry import geotrf
    meta = dict(note="roma stand-in of make_goldens.py plus rotmat_to_unitquat: closed form, largest-component branch, float64, XYZW",
                seed=17, cases=[])
    g = {}
    lr, sched, niter = 0.05, "cosine", 50
    for case in CASES:
        tag, shapes = case["tag"], [tuple(s) for s in case["shapes"]]
        N = len(shapes)
        P = max(h * w for h, w in shapes)
        edges = [(i, j) for i in range(N) for j in range(N) if i != j]
        E = len(edges)
        rng = np.random.default_rng(23)
        p1 = [rng.standard_normal(shapes[i] + (3,)).astype(np.float32) for i, j in edges]
        p2 = [rng.standard_normal(shapes[j] + (3,)).astype(np.float32) for i, j in edges]
        c1 = [(1 + 9 * rng.random(shapes[i])).astype(np.float32) for i, j in edges]
        c2 = [(1 + 9 * rng.random(shapes[j])).astype(np.float32) for i, j in edges]
        tt = lambda lst: [torch.from_numpy(a) for a in lst]
        torch.manual_seed(17)
        net = ModularPointCloudOptimizer(dict(idx=[i for i, j in edges]), dict(idx=[j for i, j in edges]),
                                         dict(pts3d=tt(p1), conf=tt(c1)), dict(pts3d_in_other_view=tt(p2), conf=tt(c2)),
                                         False, [], dist=case["dist"], verbose=False, min_conf_thr=3, **case["kw"])
        # cases with the same shapes share one set of inputs (same generator seed): stored once under the name in the JSON
        inputs = "in_" + "_".join(f"{h}x{w}" for h, w in shapes)
        for e in range(E):
            g[f"{inputs}_p1_{e}"], g[f"{inputs}_p2_{e}"], g[f"{inputs}_c1_{e}"], g[f"{inputs}_c2_{e}"] = p1[e], p2[e], c1[e], c2[e]
        for k, v in stack_params(net, P).items():
            g[f"{tag}_init_{k}"] = v
        # ---- presets
        poses, focals, pps = known_values(N, shapes, seed=29)
        g[f"{tag}_known_poses"], g[f"{tag}_known_focals"], g[f"{tag}_known_pp"] = poses, focals, pps
        presets_meta = []
        for kind, m in case["presets"]:
            msk = decode_mask(m)
            idx = [int(i) for i in net._get_msk_indices(msk)]
            if kind == "pose":
                net.preset_pose([torch.from_numpy(poses[i]) for i in idx], msk)
            elif kind == "focal":
                net.preset_focal([float(focals[i]) for i in idx], msk)
            elif kind == "pp":
                net.preset_principal_point([pps[i] for i in idx], msk)
            else:
                Ks = []
                for i in idx:
                    K = torch.eye(3)
                    K[0, 0] = K[1, 1] = float(focals[i])
                    K[0, 2], K[1, 2] = float(pps[i][0]), float(pps[i][1])
                    Ks.append(K)
                net.preset_intrinsics(Ks, msk)
            presets_meta.append(dict(kind=kind, mask=m, indices=idx))
        with torch.no_grad():
            if case["kw"].get("allow_pw_adaptors"):      # a non-trivial starting point for the adaptors (they initialise at 0)
                net.pw_adaptors.copy_(0.5 * torch.randn_like(net.pw_adaptors))
        for k, v in stack_params(net, P).items():
            if k != "depth":                             # no preset touches the depth maps: start_depth == init_depth
                g[f"{tag}_start_{k}"] = v
        frozen = dict(pose=[not p.requires_grad for p in net.im_poses], focal=[not p.requires_grad for p in net.im_focals],
                      pp=[not p.requires_grad for p in net.im_pp])
        rav = lambda t: torch.cat((t.reshape(-1, 3), t.new_zeros(P - t.shape[0] * t.shape[1], 3)))
        with torch.no_grad():
            g[f"{tag}_pw_poses_4x4"] = net.get_pw_poses().numpy()
            g[f"{tag}_adaptors"] = net.get_adaptors().numpy()
            g[f"{tag}_im_poses_4x4"] = net.get_im_poses().numpy()
            g[f"{tag}_focals"] = net.get_focals().numpy()
            g[f"{tag}_pp"] = net.get_principal_points().numpy()
            g[f"{tag}_pts3d0"] = torch.stack([rav(p) for p in net.get_pts3d()]).numpy()
            # per edge and side: the SUM of the weighted distances over the image's pixels (the loss takes their mean, then / E)
            pw, ad, pts = net.get_pw_poses(), net.get_adaptors(), net.get_pts3d()
            sums = np.zeros((E, 2), np.float64)
            for e, (i, j) in enumerate(edges):
                ij = f"{i}_{j}"
                sums[e, 0] = float(net.dist(pts[i], geotrf(pw[e], ad[e] * net.pred_i[ij]), weight=net.conf_trf(net.conf_i[ij])).double().sum())
                sums[e, 1] = float(net.dist(pts[j], geotrf(pw[e], ad[e] * net.pred_j[ij]), weight=net.conf_trf(net.conf_j[ij])).double().sum())
            g[f"{tag}_edge_sums"] = sums
        loss0 = net()
        loss0.backward()
        g[f"{tag}_loss0"] = np.float64(loss0.item())
        for k, v in stack_grads(net, P).items():
            g[f"{tag}_grad_{k}"] = v
        trainable = [n for n, p in net.named_parameters() if p.requires_grad]
        for p in net.parameters():
            p.grad = None
        opt = torch.optim.Adam([p for p in net.parameters() if p.requires_grad], lr=lr, betas=(0.9, 0.9))
        losses = []
        for it in range(niter):
            loss, _ = global_alignment_iter(net, it, niter, lr, 1e-6, opt, sched)
            losses.append(loss)
            if it + 1 in (1, 5, 50):
                for k, v in stack_params(net, P).items():
                    g[f"{tag}_k{it + 1}_{k}"] = v
        g[f"{tag}_losses"] = np.asarray(losses, np.float64)
        meta["cases"].append(dict(tag=tag, inputs=inputs, shapes=[list(s) for s in shapes], dist=case["dist"], kw=case["kw"], presets=presets_meta,
                                  frozen=frozen, norm_pw_scale=bool(net.norm_pw_scale), schedule=sched, lr=lr, lr_min=1e-6,
                                  niter=niter, edges=[list(e) for e in edges], trainable=trainable))
        print("alignmod", tag, "loss0", float(loss0), "->", losses[-1], "norm_pw_scale", net.norm_pw_scale, "frozen", frozen)
    np.savez_compressed(os.path.join(out, "alignmod.npz"), **g)
    with open(os.path.join(out, "alignmod.json"), "w") as f:
        json.dump(meta, f)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=HERE)
    generate(ap.parse_args().out)
