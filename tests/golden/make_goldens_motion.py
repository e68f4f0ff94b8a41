"""Golden of the self-computed motion masks (dust3r/cloud_opt_flow/optimizer.py:156-235) -> tests/golden/motion.npz.

    python tests/golden/make_goldens_motion.py [--out tests/golden]

Runs the reference's own get_motion_mask_from_pairs on a bare object that carries only what the method reads (edges, flow fields,
DepthBasedWarping, threshold), with the stand-ins make_goldens.py installs for the reference's missing third-party imports and ONE
more: PairViewer of the module under test is replaced by a class that hands out prescribed intrinsics, poses and depth maps, pair
after pair (the pair geometry -- Weiszfeld focal + cv2's RANSAC-PnP -- is therefore NOT pinned here).  Everything after it -- the
ego flow of DepthBasedWarping, the error norm, the per-pair min-max normalisation, the per-image mean and the threshold -- is the
reference's code.  The scene is tests/motion_cases.py's recipe at 3 x (12 x 16), complete graph, with both depth forms.

motion.npz: edges, pred_i, pred_j, flow_ij, flow_ji (the inputs), K_i, K_j, pose_i, pose_j, D_i, D_j (what the stand-in returned),
depth_row_*, depth_rt_* (the same depth maps as a row of the stacked pointmaps and a 4-float (r, t)), thre, masks [N,H,W] (the
reference's result).
"""
from __future__ import annotations

import argparse
import contextlib
import io
import os
import sys
import types

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import numpy as np
import torch

SCENE = (3, "complete", 12, 16, dict(rect=(2, 7, 3, 9), ramp=(9, 11, 1, 15)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=HERE)
    a = ap.parse_args()
    import make_goldens as mg
    import motion_cases as mc
    mg.import_reference(aligner=True)
    import dust3r.cloud_opt_flow.optimizer as ro
    from dust3r.utils.goem_opt import DepthBasedWarping

    N, graph, H, W, kw = SCENE
    sc = mc.make_scene(N, graph, H, W, **kw)
    edges, g = sc["edges"], sc["geom"]
    M = len(edges) // 2
    D_i, D_j = mc.depth_maps(sc)
    t = torch.from_numpy
    served = []

    class PrescribedPairViewer:
        def __init__(self, view1, view2, pred1, pred2, verbose=False):
            self.k = len(served)
            served.append(self.k)

        def get_intrinsics(self):
            return torch.stack([t(g["K_i"][self.k]), t(g["K_j"][self.k])])

        def get_im_poses(self):
            return torch.stack([t(g["pose_i"][self.k]), t(g["pose_j"][self.k])])

        def get_depthmaps(self):
            return [t(D_i[self.k]), t(D_j[self.k])]

    ro.PairViewer = PrescribedPairViewer
    ro.tqdm = lambda x, *args, **kwargs: x
    obj = types.SimpleNamespace(is_symmetrized=True, edges=edges, n_imgs=N, _ei=[i for i, j in edges], _ej=[j for i, j in edges],
                                flow_ij=t(sc["flow_ij"]), flow_ji=t(sc["flow_ji"]), depth_wrapper=DepthBasedWarping(),
                                motion_mask_thre=mc.THRE)
    E = len(edges)
    view = dict(idx=list(range(E)))
    pred1 = dict(pts3d=t(sc["pred_i"]), conf=t(sc["conf"]))
    pred2 = dict(pts3d_in_other_view=t(sc["pred_j"]), conf=t(sc["conf"]))
    with contextlib.redirect_stdout(io.StringIO()), contextlib.redirect_stderr(io.StringIO()):
        ro.PointCloudOptimizer.get_motion_mask_from_pairs(obj, view, dict(idx=list(range(E))), pred1, pred2)
    assert served == list(range(M))
    masks = torch.stack(obj.dynamic_masks).numpy()
    assert masks.dtype == bool and masks.shape == (N, H, W)
    np.savez_compressed(os.path.join(a.out, "motion.npz"), edges=np.asarray(edges, np.int32), pred_i=sc["pred_i"], pred_j=sc["pred_j"],
                        flow_ij=sc["flow_ij"], flow_ji=sc["flow_ji"], K_i=g["K_i"], K_j=g["K_j"], pose_i=g["pose_i"], pose_j=g["pose_j"],
                        D_i=D_i, D_j=D_j, depth_row_i=g["depth_i"][0], depth_rt_i=g["depth_i"][1], depth_row_j=g["depth_j"][0],
                        depth_rt_j=g["depth_j"][1], thre=np.float64(mc.THRE), masks=masks)
    print("motion.npz: masked share per image", masks.reshape(N, -1).mean(1).tolist())


if __name__ == "__main__":
    main()
