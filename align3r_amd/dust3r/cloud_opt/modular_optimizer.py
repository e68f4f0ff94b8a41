"""ModularPointCloudOptimizer behind the reference's API (dust3r/cloud_opt/modular_optimizer.py): the global alignment with
SOME cameras known.  preset_pose / preset_focal / preset_principal_point / preset_intrinsics accept a subset of the images
and freeze exactly those parameters; everything else is optimised by the same fused kernels as PointCloudOptimizer, with
per-image train masks on the engine (AlignEngine.set_train_masks -> a3r_align_set_train_masks).

Differences from the stacked class that this module carries:
  * the loss averages each edge side over its OWN image's pixels and divides by the number of edges (base_opt.py:356-367)
    instead of dividing one grand sum by the total area (optimizer.py:223-241).  For images of one shape the two are the same
    number and nothing is done; for mixed shapes the factor total_area / (E * area of that edge side) is folded into the loss
    weights on the host (edge_mean_factors), which enter the l1 and the l2 loss linearly;
  * norm_pw_scale stays on while at most one pose is known (modular_optimizer.py:46-48);
  * the reference's class has no mono-depth parameterisation (plain log-depth maps always, :30,127-128): `if_use_mono` and
    `mono_depths` are accepted for the common call signature and IGNORED.
fx_and_fy=True and the edge-sharded engine are refused (NotImplementedError).
"""
from __future__ import annotations

import numpy as np
import torch

from .optimizer import PointCloudOptimizer


def msk_indices(msk, n_imgs):
    """Image indices selected by a preset mask (modular_optimizer.py:73-86): None = all, an int, a list / tuple or an array /
    tensor of booleans (one per image) or of integer indices."""
    if msk is None:
        return list(range(n_imgs))
    if isinstance(msk, (bool, np.bool_)):
        raise ValueError(f'bad {msk=}')
    if isinstance(msk, (int, np.integer)):
        return [int(msk)]
    if torch.is_tensor(msk):
        msk = msk.detach().cpu().numpy()
    msk = np.asarray(msk)
    if msk.dtype == np.bool_:
        assert len(msk) == n_imgs
        return np.where(msk)[0].tolist()
    if np.issubdtype(msk.dtype, np.integer):
        return [int(i) for i in msk.reshape(-1)]
    raise ValueError(f'bad {msk=}')


def edge_mean_factors(edges, imshapes):
    """Per edge, for side i and side j: total_area_side / (E * area of the edge's image on that side).  Multiplying the stacked
    loss weights by it turns  sum / total_area  into the reference's mean over edges of per-image means."""
    areas = [h * w for h, w in imshapes]
    E = len(edges)
    tot_i, tot_j = sum(areas[i] for i, j in edges), sum(areas[j] for i, j in edges)
    f_i = np.asarray([tot_i / (E * areas[i]) for i, j in edges], dtype=np.float64)
    f_j = np.asarray([tot_j / (E * areas[j]) for i, j in edges], dtype=np.float64)
    return f_i, f_j


class ModularPointCloudOptimizer(PointCloudOptimizer):
    def __init__(self, view1, view2, pred1, pred2, if_use_mono=False, mono_depths=None, optimize_pp=False, fx_and_fy=False,
                 focal_brake=20, **kw):
        if fx_and_fy:
            raise NotImplementedError('fx_and_fy=True: the per-image parameter rows of the aligner kernels are 16 floats wide end '
                                      'to end and all 16 are taken (one focal per image)')
        if kw.get('edge_shards') is not None or kw.get('edge_shard_group') is not None:
            raise NotImplementedError('ModularPointCloudOptimizer: the edge-sharded engine has no per-image train masks')
        kw.pop('edge_shards', None)
        kw.pop('edge_shard_group', None)
        # parameters are drawn in the reference's order (pairwise poses, depth maps image by image, image poses): that of the
        # stacked class without mono
        super().__init__(view1, view2, pred1, pred2, False, None, optimize_pp=optimize_pp, focal_break=focal_brake, **kw)
        self.focal_brake = focal_brake
        N = self.n_imgs
        self._frozen = dict(pose=np.zeros(N, bool), focal=np.zeros(N, bool), pp=np.zeros(N, bool))

    # ------------------------------------------------------------------ engine
    def _stacked_weights(self):
        w_i, w_j = super()._stacked_weights()
        if not self._uniform:
            f_i, f_j = edge_mean_factors(self.edges, self.imshapes)
            w_i = w_i * torch.as_tensor(f_i, dtype=torch.float32, device=w_i.device)[:, None]
            w_j = w_j * torch.as_tensor(f_j, dtype=torch.float32, device=w_j.device)[:, None]
        return [w_i, w_j]

    def _train_masks(self):
        """What goes to the engine: None for a group without a frozen image (the handle-wide switch decides alone)."""
        return {k: (~v if v.any() else None) for k, v in self._frozen.items()}

    def _build_engine(self, device):
        eng = super()._build_engine(device)
        eng.set_train_masks(**self._train_masks())
        return eng

    def _msk_indices(self, msk):
        return msk_indices(msk, self.n_imgs)

    # ------------------------------------------------------------------ presets (modular_optimizer.py:38-68)
    def _set_known(self, group, idxs, msk):
        """Exactly the touched images become known: their rows are frozen through the engine's per-image train masks."""
        for idx in idxs:
            self._frozen[group][idx] = True
        if group == 'pose':
            # normalize scale if there's less than 1 known pose (:46-48)
            self.norm_pw_scale = bool(self._frozen['pose'].sum() <= 1)
            self.engine.flags.update(norm_pw_scale=self.norm_pw_scale)
        self.engine.set_train_masks(**self._train_masks())

    def _announce_preset(self, group, idx, value):
        if self.verbose:
            print(f" (setting {dict(pose='pose', focal='focal', pp='principal point')[group]} #{idx} = {value})")

    def preset_intrinsics(self, known_intrinsics, msk=None):
        if isinstance(known_intrinsics, torch.Tensor) and known_intrinsics.ndim == 2:
            known_intrinsics = [known_intrinsics]
        known_intrinsics = [torch.as_tensor(K) for K in known_intrinsics]
        for K in known_intrinsics:
            assert K.shape == (3, 3)
        self.preset_focal([K.diagonal()[:2].mean() for K in known_intrinsics], msk)
        self.preset_principal_point([K[:2, 2] for K in known_intrinsics], msk)

    def get_known_focal_mask(self):
        return torch.from_numpy(self._frozen['focal'].copy())

    def get_known_pose_mask(self):
        return torch.from_numpy(self._frozen['pose'].copy())
