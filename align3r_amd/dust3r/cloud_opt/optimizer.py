"""PointCloudOptimizer behind the reference's API, computed by liba3r's fused aligner kernels.

Mirrors dust3r/cloud_opt/optimizer.py:16-277 + base_opt.py:45-464 for the stacked fast path: same
constructor keywords, parameter names / parameterisation (pw_poses [E,8], im_depthmaps | scalemaps+shifts,
im_poses [N,7], im_focals = focal_break*log f, im_pp), same random initial state for the same torch seed
(parameters are drawn in the reference's order), same getters and the same optimisation loop
(Adam betas (0.9, 0.9), cosine/linear schedule).  Gradients are analytic (the reference uses autograd).
init='mst' (also on preset poses) is pinned against the reference's own control flow -- tree, scores, focals, registrations and the
written state (tests/golden/mst.npz, roma stand-ins in the fixture); its PnP solve and init='known_poses', whose only non-trivial
step is that PnP, are a stand-in for cv2's RANSAC: unpinned, validated by purpose (init_im_poses.py of this package).
allow_pw_adaptors=True (gradient + Adam on pw_adaptors in the kernels) and images of different shapes in one problem (per-edge
lists, every map zero-filled to max_area like _ravel_hw) are supported and pinned against reference goldens (tests/golden/alignx.npz).
"""
from __future__ import annotations

import os

import numpy as np
import torch

from ...aligner import AlignEngine
from ...obs16 import check_obs_dtype
from . import _native
from .init_im_poses import inv_rigid
from .commons import get_conf_trf, get_imshapes, rotmat_to_unitquat, signed_expm1, signed_log1p, unitquat_to_rotmat


class PointCloudOptimizer:
    POSE_DIM = 7
    _frozen = None                  # per-image preset masks: ModularPointCloudOptimizer only (init_im_poses._frozen_masks)

    def __init__(self, view1, view2, pred1, pred2, if_use_mono, mono_depths, dist='l1', conf='log', min_conf_thr=3,
                 base_scale=0.5, allow_pw_adaptors=False, pw_break=20, rand_pose=torch.randn, iterationsCount=None,
                 verbose=True, optimize_pp=False, focal_break=20, edge_shards=None, edge_shard_group=None, obs_dtype='fp32'):
        # obs_dtype='fp16': the engine stores the pair observations packed (aligner.AlignEngine, obs16.py); the initialisations keep
        # reading the fp32 predictions, which then stay in host memory and are staged on the device while an initialisation runs
        self.obs_dtype = check_obs_dtype(obs_dtype)
        # edge_shards=K / edge_shard_group=<process group>: the edge-sharded engine (aligner.ShardedAlignEngine) instead of the fused
        # one; the initialisations (init='mst' / 'known_poses') still work on the gathered observations
        if edge_shards is not None and edge_shard_group is not None:
            raise ValueError('pass edge_shards or edge_shard_group, not both')
        self.edge_shards, self.edge_shard_group = edge_shards, edge_shard_group
        idx1 = view1['idx'] if isinstance(view1['idx'], list) else torch.as_tensor(view1['idx']).tolist()
        idx2 = view2['idx'] if isinstance(view2['idx'], list) else torch.as_tensor(view2['idx']).tolist()
        self.edges = [(int(i), int(j)) for i, j in zip(idx1, idx2)]
        self.is_symmetrized = set(self.edges) == {(j, i) for i, j in self.edges}
        if dist not in ('l1', 'l2'):
            raise KeyError(dist)
        self.dist = dist
        self.verbose = verbose
        self.if_use_mono = bool(if_use_mono)
        self.allow_pw_adaptors = bool(allow_pw_adaptors)            # base_opt.py:117-118: pw_adaptors.requires_grad_(allow_pw_adaptors)
        indices = sorted({i for e in self.edges for i in e})       # base_opt.py:164-167
        assert indices == list(range(len(indices))), 'bad pair indices: missing values '
        self.n_imgs = len(indices)
        E, N = len(self.edges), self.n_imgs
        # the predictions come as one tensor [E,H,W,3] (inference() on same-size pairs) or as per-edge lists (multiple shapes:
        # inference() collates with lists=True, dust3r/inference.py:72)
        as_f = lambda t: torch.as_tensor(t).float()
        p_i, p_j = pred1['pts3d'], pred2['pts3d_in_other_view']
        c_i, c_j = pred1['conf'], pred2['conf']
        self.imshapes = get_imshapes(self.edges, p_i, p_j)
        areas = [h * w for h, w in self.imshapes]
        self.imshape = self.imshapes[0]                              # optimizer.py:41
        self.max_area = P = max(areas)
        self._uniform = all(s == self.imshapes[0] for s in self.imshapes)
        if self._uniform and torch.is_tensor(p_i) and torch.is_tensor(p_j):
            self._pred_i, self._pred_j = as_f(p_i).reshape(E, P, 3), as_f(p_j).reshape(E, P, 3)      # views: no copy
            self._conf_i, self._conf_j = as_f(c_i).reshape(E, P), as_f(c_j).reshape(E, P)
        else:
            # _ravel_hw (optimizer.py:271-277): every map is flattened and zero-filled up to max_area
            self._pred_i = torch.stack([_ravel_hw(as_f(p_i[e]), P) for e in range(E)])
            self._pred_j = torch.stack([_ravel_hw(as_f(p_j[e]), P) for e in range(E)])
            self._conf_i = torch.stack([_ravel_hw(as_f(c_i[e]), P) for e in range(E)])
            self._conf_j = torch.stack([_ravel_hw(as_f(c_j[e]), P) for e in range(E)])
        self.min_conf_thr = min_conf_thr
        self.conf_trf = get_conf_trf(conf)
        self._conf_mode = conf
        # Predictions that are already on the GPU (inference(keep_on_device=True), the multi-GPU gather) stay there: the per-image
        # confidence, the loss weights and the per-edge mean confidence are three launches of csrc/init_maps.hip instead of a trip
        # of both confidence stacks through host memory and a Python loop of CPU maximums (round 2: 0.5 s of a 1.5 s clip).
        self._fast = bool(self._uniform and P % 4 == 0 and _native.on_device(self._conf_i, self._conf_j))
        self._edge_conf_mean = None
        if self._fast:
            self._raw_conf_i, self._raw_conf_j = self._conf_i, self._conf_j
            self._im_conf_stack = _native.im_conf_max(self._conf_i, self._conf_j, self.edges, N)
            im_conf = [self._im_conf_stack[n].view(*self.imshapes[n]) for n in range(N)]
        else:
            self._raw_conf_i, self._raw_conf_j = self._conf_i.cpu(), self._conf_j.cpu()     # kept for the MST initialisation
            # per-image confidence = max over the edges it appears in (base_opt.py:169-175)
            im_conf = [torch.zeros(hw) for hw in self.imshapes]
            for e, (i, j) in enumerate(self.edges):
                (hi, wi), (hj, wj) = self.imshapes[i], self.imshapes[j]
                im_conf[i] = torch.maximum(im_conf[i], self._raw_conf_i[e, :hi * wi].view(hi, wi))
                im_conf[j] = torch.maximum(im_conf[j], self._raw_conf_j[e, :hj * wj].view(hj, wj))
        self.im_conf = im_conf
        self.base_scale, self.pw_break, self.focal_break = base_scale, pw_break, focal_break
        self.norm_pw_scale = True
        self.rand_pose = rand_pose
        self.has_im_poses = True
        # ---- parameters, drawn in the reference's order (base_opt.py:116-117; optimizer.py:29-38)
        init = dict(pw_poses=rand_pose((E, 1 + self.POSE_DIM)), pw_adaptors=torch.zeros(E, 2))
        if not self.if_use_mono:
            if self._uniform:
                # the reference draws torch.randn(H, W) / 10 - 3 per image (optimizer.py:33): same draws, same arithmetic, written
                # straight into the rows of one buffer
                depth = torch.empty(N, P)
                for n, (H, W) in enumerate(self.imshapes):
                    torch.randn(H, W, out=depth[n].view(H, W))
                init['depth'] = depth.div_(10).sub_(3)
            else:
                init['depth'] = torch.stack([_ravel_hw(torch.randn(H, W) / 10 - 3, P) for H, W in self.imshapes])
            self.mono_depths = None
        else:
            init['depth'] = torch.zeros(N, P)
            init['shifts'] = torch.zeros(N)
            self.mono_depths = torch.stack([_ravel_hw(as_f(m).reshape(hw), P) for m, hw in zip(mono_depths, self.imshapes)])
        init['im_poses'] = torch.stack([rand_pose(self.POSE_DIM) for _ in range(N)])
        init['im_focals'] = torch.tensor([float(focal_break * np.log(max(H, W))) for H, W in self.imshapes])
        self._init = init
        self._flags = dict(train_poses=True, train_focals=True, train_pp=bool(optimize_pp), train_adaptors=self.allow_pw_adaptors)
        self.total_area_i = sum(areas[i] for i, j in self.edges)         # optimizer.py:70-71
        self.total_area_j = sum(areas[j] for i, j in self.edges)
        self.engine = None
        self.device = torch.device('cpu')
        self._grid = None
        self.imgs = None
        if 'img' in view1 and 'img' in view2:
            imgs = [None] * N
            for v in range(E):
                imgs[self.edges[v][0]] = view1['img'][v]
                imgs[self.edges[v][1]] = view2['img'][v]
            self.imgs = [(torch.as_tensor(im).float().cpu().permute(1, 2, 0).numpy() * 0.5 + 0.5).clip(0, 1) for im in imgs]

    # ------------------------------------------------------------------ placement
    def to(self, device):
        device = torch.device(device)
        if device.type != 'cuda':
            raise RuntimeError('PointCloudOptimizer: this build has no CPU compute path; pass a HIP device ("cuda")')
        if device.index is None:
            device = torch.device('cuda', torch.cuda.current_device())
        self.device = device
        state = self._current_state()          # a repeated .to() keeps the parameter values (nn.Module.to semantics)
        self.engine = self._build_engine(device)
        self.engine.set_params(**(state or self._init))
        # keep handles on the engine's device tensors instead of the (possibly host) originals: no second copy stays alive, and
        # .to() can be called again like nn.Module.to (the confidences are re-derived from the raw host copies)
        if self.obs_dtype == 'fp32':
            self._pred_i, self._pred_j = self.engine.pred_i, self.engine.pred_j
        else:
            # the engine holds packed records only, and nothing here keeps an fp32 stack on the device: the predictions stay in host
            # memory (moved there if they came on the device, so that the caller can free its copy) and the initialisations stage
            # them through _device_predictions for as long as they run
            self._pred_i, self._pred_j = self._pred_i.cpu(), self._pred_j.cpu()
        self._conf_i, self._conf_j = self._raw_conf_i, self._raw_conf_j
        self._grid = None
        return self

    def _device_predictions(self, device):
        """The stacked fp32 predictions [E,P,3] of both sides on `device`, for the initialisations.  obs_dtype='fp32': the engine's own
        tensors.  obs_dtype='fp16': a temporary upload of the host copies kept here -- 24 E P bytes that live only while the caller
        holds them (the peak during an initialisation is the packed records plus this; afterwards the records alone)."""
        if self.obs_dtype == 'fp32':
            return self._pred_i, self._pred_j
        return tuple(t.to(device, torch.float32).contiguous() for t in (self._pred_i, self._pred_j))

    def _stacked_weights(self):
        E, P = len(self.edges), self.max_area
        if self._fast and self._conf_mode in _native.CONF_MODES and _native.on_device(self._conf_i, self._conf_j):
            w_i, w_j, self._edge_conf_mean = _native.conf_prepare(self._conf_i, self._conf_j, self._conf_mode)
            return [w_i, w_j]
        out = []
        for conf, side in ((self._conf_i, 0), (self._conf_j, 1)):
            w = self.conf_trf(conf)
            if not self._uniform:
                area = torch.tensor([self.imshapes[e[side]][0] * self.imshapes[e[side]][1] for e in self.edges], device=w.device)
                pad = torch.arange(P, device=w.device)[None, :] >= area[:, None]
                w = w.masked_fill(pad, 0.0)
            out.append(w.reshape(E, P))
        return out

    def _engine_kwargs(self, device):
        """What every engine of this class and its variants is built from: the graph, the stacked observations and the settings."""
        w_i, w_j = self._stacked_weights()
        return dict(ei=[i for i, j in self.edges], ej=[j for i, j in self.edges], pred_i=self._pred_i, pred_j=self._pred_j,
                    w_i=w_i, w_j=w_j, imshapes=self.imshapes, mono=self.mono_depths, base_scale=self.base_scale,
                    pw_break=self.pw_break, focal_break=self.focal_break, norm_pw_scale=self.norm_pw_scale, dist=self.dist,
                    device=device, obs_dtype=self.obs_dtype, **self._flags)

    def _build_engine(self, device):
        if self.edge_shards is not None or self.edge_shard_group is not None:
            from ...aligner import ShardedAlignEngine
            return ShardedAlignEngine(local_shards=self.edge_shards, group=self.edge_shard_group, **self._engine_kwargs(device))
        return AlignEngine(**self._engine_kwargs(device))

    def _current_state(self):
        """Parameter values of the live engine (host copies), or None before the first .to()."""
        if self.engine is None:
            return None
        keys = ['pw_poses', 'pw_adaptors', 'depth', 'im_poses', 'im_focals', 'im_pp'] + (['shifts'] if self.if_use_mono else [])
        return {k: self.engine.params[k].detach().cpu().clone() for k in keys}

    def _need_engine(self):
        if self.engine is None:
            raise RuntimeError('call .to(device) first (global_aligner does)')
        return self.engine

    @property
    def n_edges(self):
        return len(self.edges)

    @property
    def str_edges(self):
        return [f'{i}_{j}' for i, j in self.edges]

    @property
    def imsizes(self):
        return [(w, h) for h, w in self.imshapes]

    # ------------------------------------------------------------------ parameter views (reference names)
    @property
    def pw_poses(self):
        return self._need_engine().params['pw_poses']

    @property
    def pw_adaptors(self):
        return self._need_engine().params['pw_adaptors']

    @property
    def im_poses(self):
        return self._need_engine().params['im_poses']

    @property
    def im_focals(self):
        return self._need_engine().params['im_focals'][:, None]

    @property
    def im_pp(self):
        return self._need_engine().params['im_pp']

    @property
    def im_depthmaps(self):
        assert not self.if_use_mono
        return self._need_engine().params['depth']

    @property
    def scalemaps(self):
        assert self.if_use_mono
        return self._need_engine().params['depth']

    @property
    def shifts(self):
        assert self.if_use_mono
        return self._need_engine().params['shifts'][:, None]

    # ------------------------------------------------------------------ getters (optimizer.py:137-206, base_opt.py:184-229)
    def _get_poses(self, poses):
        Q = poses[:, :4]
        Q = Q / Q.norm(dim=-1, keepdim=True)
        T = signed_expm1(poses[:, 4:7])
        RT = torch.zeros(poses.shape[0], 4, 4, device=poses.device)
        RT[:, :3, :3] = unitquat_to_rotmat(Q)
        RT[:, :3, 3] = T
        RT[:, 3, 3] = 1
        return RT

    def get_adaptors(self):
        adapt = self.pw_adaptors                                     # base_opt.py:177-182
        adapt = torch.cat((adapt[:, 0:1], adapt), dim=-1)            # (scale_xy, scale_xy, scale_z)
        if self.norm_pw_scale:
            adapt = adapt - adapt.mean(dim=1, keepdim=True)
        return (adapt / self.pw_break).exp()

    def get_pw_norm_scale_factor(self):
        if self.norm_pw_scale:
            return (np.log(self.base_scale) - self.pw_poses[:, -1].mean()).exp()
        return 1

    def get_pw_scale(self):
        return self.pw_poses[:, -1].exp() * self.get_pw_norm_scale_factor()

    def get_pw_poses(self):
        RT = self._get_poses(self.pw_poses)
        RT[:, :3] *= self.get_pw_scale().view(-1, 1, 1)
        return RT

    def get_im_poses(self):
        return self._get_poses(self.im_poses)

    def get_focals(self):
        return (self.im_focals / self.focal_break).exp()

    def get_principal_points(self):
        return self._need_engine().pp0 + 10 * self.im_pp

    def get_intrinsics(self):
        K = torch.zeros((self.n_imgs, 3, 3), device=self.device)
        f = self.get_focals().flatten()
        K[:, 0, 0] = K[:, 1, 1] = f
        K[:, :2, 2] = self.get_principal_points()
        K[:, 2, 2] = 1
        return K

    def get_known_focal_mask(self):
        return torch.tensor([not self._flags['train_focals']] * self.n_imgs)

    def get_depthmaps(self, raw=False):
        p = self._need_engine().params
        if not self.if_use_mono:
            res = p['depth'].exp()
        else:
            res = self.engine.mono * p['depth'].exp() + p['shifts'][:, None]
        if not raw:
            res = [dm[:h * w].view(h, w) for dm, (h, w) in zip(res, self.imshapes)]
        return res

    def _pixel_grid(self):
        """_grid of optimizer.py:55-56: xy pixel grid of every image, zero-filled up to max_area [N,P,2]."""
        if self._grid is None or self._grid.device != self.device:
            grids = []
            for H, W in self.imshapes:
                ys, xs = torch.meshgrid(torch.arange(H, device=self.device), torch.arange(W, device=self.device), indexing='ij')
                grids.append(_ravel_hw(torch.stack((xs, ys), -1).float(), self.max_area))
            self._grid = torch.stack(grids)
        return self._grid

    def depth_to_pts3d(self):
        depth = self.get_depthmaps(raw=True)                                   # [N,P]
        grid = self._pixel_grid()
        pp = self.get_principal_points()[:, None]
        f = self.get_focals()[:, None]
        rel = torch.cat((depth[..., None] * (grid - pp) / f, depth[..., None]), -1)
        RT = self.get_im_poses()
        return torch.einsum('bij,bpj->bpi', RT[:, :3, :3], rel) + RT[:, None, :3, 3]

    def get_pts3d(self, raw=False):
        res = self.depth_to_pts3d()
        if not raw:
            res = [dm[:h * w].view(h, w, 3) for dm, (h, w) in zip(res, self.imshapes)]
        return res

    def get_conf(self, mode=None):
        trf = self.conf_trf if mode is None else get_conf_trf(mode)
        return [trf(c) for c in self.im_conf]

    # ------------------------------------------------------------------ output files (base_opt.py:279-343)
    def get_tum_poses(self):
        from ...tool.hierarchical import get_tum_poses
        return get_tum_poses(self.get_im_poses())

    def save_tum_poses(self, path):
        from ...tool.hierarchical import save_trajectory_tum_format
        traj = self.get_tum_poses()
        save_trajectory_tum_format(traj, path)
        return traj[0]

    def save_focals(self, path):
        focals = self.get_focals()
        np.savetxt(path, focals.detach().cpu().numpy(), fmt='%.6f')
        return focals

    def save_intrinsics(self, path):
        from ...tool.hierarchical import save_intrinsics
        K = self.get_intrinsics()
        save_intrinsics(K, path)
        return K

    def save_conf_maps(self, path, start=0):
        from ...tool.hierarchical import save_frame_arrays
        conf = self.get_conf()
        save_frame_arrays(conf, path, 'conf_{}.npy', start)
        return conf

    def save_depth_maps(self, path, start=0):
        """frame_XXXX.npy per image (the reference also writes JET-coloured PNGs and a GIF through cv2: not available)."""
        from ...tool.hierarchical import save_frame_arrays
        depth_maps = self.get_depthmaps()
        save_frame_arrays(depth_maps, path, 'frame_{:04d}.npy', start)
        return depth_maps

    def get_masks(self):
        return [(conf > self.min_conf_thr) for conf in self.im_conf]

    # ------------------------------------------------------------------ scene out (tool/demo.py: get_3D_model_from_scene)
    def _mask_confidences(self):
        """The confidence maps get_masks() thresholds."""
        return self.im_conf

    def get_pointcloud(self, min_conf_thr=None, mask_dynamic=False, with_index=False, voxel_size=None, reduce='best', min_count=1):
        """The aligned scene as one compacted point cloud, computed on the device by the aligner handle (csrc/scene.hip): dict of
        device tensors xyz [M,3] float32, rgb [M,3] uint8 (when the scene holds its frames) and, with_index, index [M] int32 =
        n * max_area + p.  Kept: conf > min_conf_thr (as given; None = self.min_conf_thr, the pixels of get_masks()), finite
        coordinates and, with mask_dynamic, outside the scene's dynamic masks.  Image-major, row-major order.

        voxel_size: that cloud reduced to one point per occupied cell of a grid of this edge (ops.voxel_downsample, csrc/voxel.hip):
        the most confident point of a cell (reduce='best') or the mean of its points and colours ('mean'), cells with fewer than
        min_count points left out -- a point seen once is a floater.  The dict gains count [V] int32 = the points of the cell;
        index is the winner's pixel, and the order stays image-major, row-major.  Points further than 2^20 cells from the origin
        are in no cell; their number is reported by a warning."""
        e = self._need_engine()
        conf, thr, dyn, rgb = self._scene_out_inputs(min_conf_thr, mask_dynamic, 'get_pointcloud')
        if voxel_size is None:
            return e.export_points(conf, thr, dyn=dyn, rgb=rgb, with_index=with_index)
        from ... import ops
        pc = e.export_points(conf, thr, dyn=dyn, rgb=rgb, with_index=True)
        priority = conf.reshape(-1)[pc['index'].long()].contiguous()
        vx = ops.voxel_downsample(pc['xyz'], voxel_size, priority=priority, rgb=pc.get('rgb'), reduce=reduce, min_count=min_count)
        if vx['dropped']:
            import warnings
            warnings.warn(f"get_pointcloud(voxel_size={voxel_size}): {vx['dropped']} of {pc['xyz'].shape[0]} points lie beyond 2^20 "
                          "cells from the origin and are in no voxel")
        out = dict(xyz=vx['xyz'])
        if 'rgb' in vx:
            out['rgb'] = vx['rgb']
        out['count'] = vx['count']
        if with_index:
            out['index'] = pc['index'][vx['index'].long()]
        return out

    def _scene_out_inputs(self, min_conf_thr, mask_dynamic, who):
        """(conf [N,P], thr, dyn [N,P] or None, rgb [N,P,3] uint8 or None): what get_pointcloud and get_mesh hand to the engine."""
        P = self.max_area
        thr = self.min_conf_thr if min_conf_thr is None else min_conf_thr
        conf = torch.stack([_ravel_hw(c.to(self.device).float()[..., None], P)[:, 0] for c in self._mask_confidences()])
        dyn = None
        if mask_dynamic:
            masks = getattr(self, 'dynamic_masks', None)
            if masks is None:
                raise RuntimeError(f'{who}(mask_dynamic=True): this scene has no dynamic masks')
            dyn = torch.stack([_ravel_hw(torch.as_tensor(m).to(self.device).to(torch.uint8)[..., None], P)[:, 0] for m in masks])
        rgb = None
        if self.imgs is not None:
            rgb = torch.stack([_ravel_hw(torch.from_numpy(np.clip(np.rint(255.0 * np.asarray(im)), 0, 255).astype(np.uint8)), P)
                               for im in self.imgs])
        return conf, float(thr), dyn, rgb

    def get_mesh(self, min_conf_thr=None, mask_dynamic=False, double_sided=False):
        """The aligned scene as one triangle mesh (the default output of the reference's get_3D_model_from_scene: pts3d_to_trimesh /
        cat_meshes of dust3r/viz.py), built on the device by the aligner handle: dict of device tensors xyz [V,3] float32 and
        rgb [V,3] uint8 -- the vertices are exactly the points of get_pointcloud() with the same arguments --, faces [F,3] int32
        vertex ids and face_rgb [F,3] uint8 (the colours when the scene holds its frames).  Two triangles per pixel quad, each kept
        where its three corner pixels are; double_sided adds every triangle wound backwards, as the reference does."""
        e = self._need_engine()
        conf, thr, dyn, rgb = self._scene_out_inputs(min_conf_thr, mask_dynamic, 'get_mesh')
        return e.export_mesh(conf, thr, dyn=dyn, rgb=rgb, double_sided=double_sided)

    def save_mesh(self, path, **kw):
        """get_mesh(**kw) written as a binary little-endian PLY (tool/pointcloud.py: write_ply_mesh); returns the dict."""
        from ...tool.pointcloud import write_ply_mesh
        m = self.get_mesh(**kw)
        host = lambda k: m[k].cpu().numpy() if k in m else None
        write_ply_mesh(path, host('xyz'), host('faces'), host('rgb'), host('face_rgb'))
        return m

    def _tsdf_inputs(self, min_conf_thr, mask_dynamic, weight, who):
        """What get_tsdf hands to ops.tsdf_integrate: depth and weight [N,P] float32, rgb [N,P,3] uint8 or None, the camera table,
        and the kept cloud (xyz, index) the weights were cut from."""
        from ... import ops
        from ...tool.render import world_to_camera
        if weight not in ('conf', 'uniform'):
            raise ValueError(f"{who}: weight = {weight!r} is neither 'conf' nor 'uniform'")
        e = self._need_engine()
        conf, thr, dyn, rgb = self._scene_out_inputs(min_conf_thr, mask_dynamic, who)
        pc = e.export_points(conf, thr, dyn=dyn, rgb=None, with_index=True)
        idx = pc['index'].long()
        wt = torch.zeros(conf.numel(), dtype=torch.float32, device=conf.device)
        wt[idx] = conf.reshape(-1)[idx] if weight == 'conf' else 1.0
        depth = self.get_depthmaps(raw=True).detach().float().contiguous()
        poses = self.get_im_poses().detach().cpu().numpy().astype(np.float64)
        K = np.zeros((self.n_imgs, 3, 3))
        K[:, 0, 0] = K[:, 1, 1] = self.get_focals().detach().cpu().numpy().astype(np.float64).reshape(-1)
        K[:, :2, 2] = self.get_principal_points().detach().cpu().numpy().astype(np.float64)
        K[:, 2, 2] = 1
        cams = ops.tsdf_cameras(world_to_camera(poses), K, [tuple(s) for s in self.imshapes])
        if rgb is not None:
            rgb = rgb.to(conf.device).contiguous()
        return depth, wt.view(conf.shape), rgb, cams, pc

    def get_tsdf(self, voxel_size, trunc=None, bounds=None, min_conf_thr=None, mask_dynamic=False, weight='conf', max_depth=None,
                 max_voxels=2 ** 28):
        """The aligned depth maps fused into one dense grid of truncated signed distances (ops.tsdf_integrate, csrc/tsdf.hip;
        include/a3r.h has the definition): every voxel of edge voxel_size takes, over the frames that see it, the weighted mean of
        min(1, (depth - its own camera depth) / trunc), frames that see a surface more than trunc in front of it left out.  trunc
        defaults to 3 voxel_size.  A pixel's weight is its confidence (weight='conf') or 1 ('uniform') where get_pointcloud() keeps
        the pixel with the same min_conf_thr and mask_dynamic, 0 elsewhere; depths beyond max_depth are not integrated.  The depths
        are get_depthmaps(), the cameras the scene's own in float64, as render_views builds them.  bounds = (origin, dims) fixes the
        grid; None takes the box of the kept points within max_depth, padded by trunc: origin = floor((min - trunc) / v) v and
        dims = floor((max + trunc) / v) + 1 - floor((min - trunc) / v), on the host in float64.  More than max_voxels voxels is a
        ValueError.  Returns tsdf [nz,ny,nx] float32 (1 where nothing was seen), weight [nz,ny,nx] float32, rgb [nz,ny,nx,3] uint8
        (None for a scene without frames), origin (three floats), voxel, dims = (nx, ny, nz)."""
        from ... import ops
        who = 'get_tsdf'
        v = float(voxel_size)
        if not (np.isfinite(v) and v > 0):
            raise ValueError(f'{who}: voxel_size = {voxel_size} must be finite and positive')
        trunc = 3 * v if trunc is None else float(trunc)
        if not (np.isfinite(trunc) and trunc > 0):
            raise ValueError(f'{who}: trunc = {trunc} must be finite and positive')
        far = float('inf') if max_depth is None else float(max_depth)
        if not far > 0:
            raise ValueError(f'{who}: max_depth = {max_depth} must be positive')
        depth, wt, rgb, cams, pc = self._tsdf_inputs(min_conf_thr, mask_dynamic, weight, who)
        if bounds is None:
            xyz = pc['xyz']
            if far < float('inf'):
                xyz = xyz[depth.reshape(-1)[pc['index'].long()] <= far]
            if xyz.shape[0] == 0:
                raise ValueError(f'{who}: no pixel is kept within max_depth: there is nothing to put a box around (bounds= sets one)')
            lo_pt = xyz.min(0).values.cpu().numpy().astype(np.float64)
            hi_pt = xyz.max(0).values.cpu().numpy().astype(np.float64)
            lo = np.floor((lo_pt - trunc) / v)
            hi = np.floor((hi_pt + trunc) / v) + 1
            origin, dims = lo * v, hi - lo
        else:
            origin, dims = bounds
            origin = np.asarray(origin, dtype=np.float64).reshape(-1)
        if len(dims) != 3 or not all(np.isfinite(n) and n >= 1 for n in dims):
            raise ValueError(f'{who}: dims = {tuple(dims)!r} is three positive counts')
        dims = tuple(int(n) for n in dims)
        if dims[0] * dims[1] * dims[2] > max_voxels:
            raise ValueError(f'{who}: dims = {dims} are {dims[0] * dims[1] * dims[2]} voxels, more than max_voxels = {max_voxels}: '
                             'narrow the box with bounds= or max_depth=, or take a larger voxel')
        tsdf, wsum, colours = ops.tsdf_integrate(depth, wt, rgb, cams, origin, dims, v, trunc, max_depth=far)
        return tsdf, wsum, colours, tuple(float(o) for o in origin), v, dims

    def get_fused_mesh(self, voxel_size, trunc=None, bounds=None, min_conf_thr=None, mask_dynamic=False, weight='conf', max_depth=None,
                       max_voxels=2 ** 28, min_weight=None):
        """One surface for the whole scene: the zero set of get_tsdf(...) as a triangle mesh by surface nets (ops.tsdf_mesh): dict of
        device tensors xyz [V,3] float32, rgb [V,3] uint8 (when the scene holds its frames) and faces [F,3] int32.  A voxel counts
        as observed where its weight is at least min_weight; None = the smallest positive weight the scene assigns to a pixel,
        i.e. seen at least once."""
        from ... import ops
        if min_weight is None:
            if weight == 'conf':
                wt = self._tsdf_inputs(min_conf_thr, mask_dynamic, weight, 'get_fused_mesh')[1]
                positive = wt[wt > 0]
                min_weight = float(positive.min()) if positive.numel() else 1.0
            else:
                min_weight = 1.0
        tsdf, wsum, colours, origin, v, _ = self.get_tsdf(voxel_size, trunc=trunc, bounds=bounds, min_conf_thr=min_conf_thr,
                                                          mask_dynamic=mask_dynamic, weight=weight, max_depth=max_depth,
                                                          max_voxels=max_voxels)
        xyz, rgb, faces = ops.tsdf_mesh(tsdf, wsum, colours, origin, v, min_weight)
        out = dict(xyz=xyz)
        if rgb is not None:
            out['rgb'] = rgb
        out['faces'] = faces
        return out

    def save_fused_mesh(self, path, voxel_size, **kw):
        """get_fused_mesh(voxel_size, **kw) written as a binary little-endian PLY (tool/pointcloud.py: write_ply_mesh); returns the
        dict."""
        from ...tool.pointcloud import write_ply_mesh
        m = self.get_fused_mesh(voxel_size, **kw)
        host = lambda k: m[k].cpu().numpy() if k in m else None
        write_ply_mesh(path, host('xyz'), host('faces'), host('rgb'))
        return m

    def save_pointcloud(self, path, **kw):
        """get_pointcloud(**kw) written as a binary little-endian PLY (tool/pointcloud.py); returns the dict."""
        from ...tool.pointcloud import write_ply
        pc = self.get_pointcloud(**kw)
        write_ply(path, pc['xyz'].cpu().numpy(), pc['rgb'].cpu().numpy() if 'rgb' in pc else None)
        return pc

    # ------------------------------------------------------------------ pictures (stands in for the reference's scene.show())
    def render(self, cam2world, K, shape, min_conf_thr=None, mask_dynamic=False, radius=0, background=(255, 255, 255), with_index=False):
        """The aligned scene seen from any cameras: the points and colours of get_pointcloud(min_conf_thr, mask_dynamic), drawn as
        z-buffered square splats of (2 radius + 1)^2 pixels (ops.render_points, csrc/render.hip).  cam2world [C,3 or 4,4] camera
        poses and K [C,3,3] intrinsics (numpy or torch, any float type; the poses are inverted by tool/render.py: world_to_camera),
        shape = (H, W).  Dict of device tensors: depth [C,H,W] float32 (0 = empty), rgb [C,H,W,3] uint8 (when the scene holds its
        frames) and, with_index, index [C,H,W] int32 = the winner's row of get_pointcloud()'s arrays (-1 = empty)."""
        pc = self.get_pointcloud(min_conf_thr=min_conf_thr, mask_dynamic=mask_dynamic)
        return self.render_cloud(pc, cam2world, K, shape, radius=radius, background=background, with_index=with_index)

    def render_cloud(self, pc, cam2world, K, shape, radius=0, background=(255, 255, 255), with_index=False):
        """render() on a cloud already exported with get_pointcloud(): a caller that renders many times exports once."""
        from ... import ops
        from ...tool.render import world_to_camera
        host = lambda a: a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a)
        return ops.render_points(pc['xyz'], pc.get('rgb'), w2c=world_to_camera(cam2world), K=host(K).astype(np.float64), shape=shape,
                                 radius=radius, background=background, want_index=with_index)

    def render_views(self, idx=None, min_conf_thr=None, mask_dynamic=False, radius=0, background=(255, 255, 255), with_index=False,
                     points_of=None):
        """The scene seen from its own cameras (get_im_poses, get_focals, get_principal_points), each at its image's own shape:
        a list, in the order of idx (None = every image), of dicts depth [h,w], rgb [h,w,3] and, with_index, index [h,w] as
        render() returns them.  Cameras of equal shape go into one call.  points_of = image numbers: only the kept points of those
        images are drawn (None = the whole scene), and index counts rows of that selection -- with points_of=[i] and radius 0, view
        i shows at every kept pixel of image i that pixel's own rank among them."""
        idx = list(range(self.n_imgs)) if idx is None else [int(i) for i in (idx if np.iterable(idx) else [idx])]
        for i in idx:
            if not 0 <= i < self.n_imgs:
                raise IndexError(f'render_views: image {i} is outside the scene of {self.n_imgs} images')
        pc = self.get_pointcloud(min_conf_thr=min_conf_thr, mask_dynamic=mask_dynamic, with_index=points_of is not None)
        if points_of is not None:
            own = torch.zeros(self.n_imgs, dtype=torch.bool, device=pc['index'].device)
            own[[int(n) for n in (points_of if np.iterable(points_of) else [points_of])]] = True
            rows = own[torch.div(pc['index'], self.max_area, rounding_mode='floor').long()]
            pc = {k: v[rows].contiguous() for k, v in pc.items()}
        poses = self.get_im_poses().detach().cpu().numpy().astype(np.float64)
        f = self.get_focals().detach().cpu().numpy().astype(np.float64).reshape(-1)
        pp = self.get_principal_points().detach().cpu().numpy().astype(np.float64)
        K = np.zeros((self.n_imgs, 3, 3))
        K[:, 0, 0] = K[:, 1, 1] = f
        K[:, :2, 2] = pp
        K[:, 2, 2] = 1
        out = [None] * len(idx)
        for shape in sorted({tuple(self.imshapes[i]) for i in idx}):
            slots = [s for s, i in enumerate(idx) if tuple(self.imshapes[i]) == shape]
            sel = [idx[s] for s in slots]
            r = self.render_cloud(pc, poses[sel], K[sel], shape, radius=radius, background=background, with_index=with_index)
            for c, s in enumerate(slots):
                out[s] = {k: v[c] for k, v in r.items()}
        return out

    def save_renders(self, dir, idx=None, **kw):
        """render_views(idx, **kw) written as dir/render_XXXX.png (XXXX = the image number; tool/render.py: write_png); returns the
        list of render_views.  A scene without frames has no colours: its pictures are the coverage, 255 where a point landed and 0
        elsewhere."""
        from ...tool.render import write_png
        os.makedirs(dir, exist_ok=True)
        idx = list(range(self.n_imgs)) if idx is None else [int(i) for i in (idx if np.iterable(idx) else [idx])]
        views = self.render_views(idx, **kw)
        for i, v in zip(idx, views):
            pic = v['rgb'] if 'rgb' in v else (v['depth'] > 0).to(torch.uint8) * 255
            write_png(os.path.join(dir, f'render_{i:04d}.png'), pic)
        return views

    def get_matches(self, i, j, min_conf_thr=None, mask_dynamic=False):
        """Dense pixel correspondences between images i and j: the reciprocal 3-D nearest neighbours (find_reciprocal_matches of
        dust3r/utils/geometry.py, computed by csrc/match.hip) between the kept points of the two images -- the rows that
        get_pointcloud(min_conf_thr, mask_dynamic, with_index=True) returns for them, same keep rule.  Dict of device tensors, one row
        per match in ascending order of image j's kept pixels: idx_i, idx_j [M] int32 pixel indices y * w + x in each image's own
        shape; xy_i, xy_j [M,2] int32, x first (as xy_grid); xyz_i, xyz_j [M,3] the matched points; and count = M."""
        for k in (i, j):
            if not 0 <= int(k) < self.n_imgs:
                raise IndexError(f'get_matches: image {k} is outside the scene of {self.n_imgs} images')
        i, j = int(i), int(j)
        if i == j:
            raise ValueError(f'get_matches: i == j == {i}: a correspondence needs two images')
        return self.matches_from_cloud(self.get_pointcloud(min_conf_thr=min_conf_thr, mask_dynamic=mask_dynamic, with_index=True), i, j)

    def matches_from_cloud(self, pc, i, j):
        """get_matches(i, j) on a cloud already exported with get_pointcloud(..., with_index=True): a caller that wants many pairs
        exports once.  i and j are taken as checked."""
        from ... import ops
        index, xyz, P = pc['index'], pc['xyz'], self.max_area
        # the cloud is image-major: the rows of image n are those with n * P <= index < (n + 1) * P (the export keeps N * P below
        # 2^31, so every edge fits the index's int32)
        edges = torch.tensor([i * P, (i + 1) * P, j * P, (j + 1) * P], dtype=index.dtype, device=index.device)
        i0, i1, j0, j1 = torch.searchsorted(index, edges).tolist()
        m = ops.reciprocal_matches(xyz[i0:i1], xyz[j0:j1])
        k1, k2 = m['pairs'][:, 0].long(), m['pairs'][:, 1].long()
        out = dict(count=m['count'])
        for name, n, lo, hi, k in (('i', i, i0, i1, k1), ('j', j, j0, j1, k2)):
            p = index[lo:hi][k] - n * P
            w = self.imshapes[n][1]
            out['idx_' + name] = p
            out['xy_' + name] = torch.stack([p % w, torch.div(p, w, rounding_mode='floor')], 1)
            out['xyz_' + name] = xyz[lo:hi][k]
        return out

    # ------------------------------------------------------------------ motion: tracks and scene flow (csrc/track.hip)
    def _own_flow(self):
        """(flow_ij, flow_ji) of the scene's edges when the scene holds them (the flow class does), else None."""
        return None

    def _track(self, steps, seeds, fb_thr, min_conf_thr, mask_dynamic, flow, who):
        """ops.track_points on the scene: xyz = engine.points(), keep = the rule of get_pointcloud() (conf > thr and, with
        mask_dynamic, outside the dynamic masks; the finite test is the tracker's own), flow = (flow_ij, flow_ji) aligned with
        self.edges.  steps [C,S,4]; returns the dict of ops.track_points."""
        from ... import ops
        if not self._uniform:
            raise RuntimeError(f'{who}: the scene holds images of more than one shape; flow fields are stacked [E,2,H,W] and a track '
                               'keeps one pixel grid through all frames')
        if flow is None:
            flow = self._own_flow()
        if flow is None:
            raise RuntimeError(f'{who}: this scene holds no optical flow; pass flow=(flow_ij, flow_ji), each [E,2,H,W] in the order of '
                               'scene.edges (the flow aligner with flow_loss_weight > 0 keeps its own)')
        (H, W), E, N = self.imshapes[0], len(self.edges), self.n_imgs
        flow = [torch.as_tensor(f) for f in flow]
        for f, name in zip(flow, ('flow_ij', 'flow_ji')):
            if f.numel() != E * 2 * H * W:
                raise ValueError(f'{who}: {name} holds {f.numel()} values, not [E,2,H,W] = [{E},2,{H},{W}]')
        e = self._need_engine()
        dev = e.device
        fields = [f.to(dev, torch.float32).reshape(E, 2, H, W).contiguous() for f in flow]      # the scene's own fields: no copy
        conf, thr, dyn, _ = self._scene_out_inputs(min_conf_thr, mask_dynamic, who)
        keep = conf > thr
        if dyn is not None:
            keep &= dyn == 0
        if seeds is not None:
            seeds = torch.as_tensor(np.asarray(seeds.detach().cpu() if torch.is_tensor(seeds) else seeds, dtype=np.float32))
            if seeds.dim() != 2 or seeds.shape[1] != 2:
                raise ValueError(f'{who}: seeds are (x, y) rows [M,2], got {tuple(seeds.shape)}')
            seeds = seeds.to(dev).contiguous()
        return ops.track_points(e.points().view(N, H, W, 3), keep.view(N, H, W).contiguous(), fields[0], fields[1], steps, seeds=seeds,
                                fb_thr=fb_thr)

    def _check_frames(self, frames, who):
        frames = [int(f) for f in frames]
        for f in frames:
            if not 0 <= f < self.n_imgs:
                raise IndexError(f'{who}: image {f} is outside the scene of {self.n_imgs} images')
        return frames

    def get_tracks(self, frames=None, seeds=None, fb_thr=3.0, min_conf_thr=None, mask_dynamic=False, flow=None):
        """3-D trajectories: the points at `seeds` ([M,2] (x, y) positions in image frames[0]; None = every pixel) followed through
        `frames` (None = all images in order; any order along edges of the graph, see tool/tracks.py: plan_steps) by the optical
        flow of the edges, and read off the aligned point maps (ops.track_points, csrc/track.hip; include/a3r.h has the definition).
        A track ends where it leaves the image or where forward and backward flow disagree by fb_thr pixels or more.  Dict of device
        tensors with T = len(frames): xy [T,M,2] float32 positions, xyz [T,M,3] float32 world points, pix [T,M] int32 = row * W + col
        of the pixel read (-1 = ended), state [T,M] uint8 (2 = visible: the pixel is one get_pointcloud(min_conf_thr, mask_dynamic)
        keeps and xyz is its point; 1 = followed, not visible; 0 = ended), and frames.  flow = (flow_ij, flow_ji) [E,2,H,W] in the
        order of scene.edges; the flow aligner uses its own fields."""
        from ...tool.tracks import plan_steps
        frames = self._check_frames(range(self.n_imgs) if frames is None else frames, 'get_tracks')
        if len(frames) < 2:
            raise ValueError('get_tracks: a track needs at least two frames')
        out = self._track(plan_steps(self.edges, frames)[None], seeds, fb_thr, min_conf_thr, mask_dynamic, flow, 'get_tracks')
        out = {k: v[0] for k, v in out.items()}
        out['frames'] = frames
        return out

    def get_scene_flow(self, i=None, j=None, fb_thr=3.0, min_conf_thr=None, mask_dynamic=False, flow=None):
        """Scene flow from image i to image j (two images joined by an edge): every pixel of i followed one step and the two point
        maps subtracted.  Dict of device tensors: flow3d [H,W,3] float32 = xyz_j(target) - xyz_i(pixel), zeros where not valid;
        valid [H,W] bool = the pixel is visible in i, its track reaches j (inside the image, forward and backward flow agree within
        fb_thr) and lands on a visible pixel (state 2 of get_tracks at both ends); target_xy [H,W,2] float32 and target_pix [H,W]
        int32 (-1 where the track ended).  Without i and j: every edge of the graph in one launch, the same tensors stacked on a
        leading axis in the order of scene.edges, and edges."""
        from ...tool.tracks import plan_steps
        if (i is None) != (j is None):
            raise ValueError('get_scene_flow: pass both images or neither (neither = every edge of the graph)')
        if i is None:
            steps = np.asarray([[(a, b, e, 0)] for e, (a, b) in enumerate(self.edges)], np.int32).reshape(len(self.edges), 1, 4)
        else:
            i, j = self._check_frames((i, j), 'get_scene_flow')
            if i == j:
                raise ValueError(f'get_scene_flow: i == j == {i}: motion needs two images')
            steps = plan_steps(self.edges, (i, j))[None]
        t = self._track(steps, None, fb_thr, min_conf_thr, mask_dynamic, flow, 'get_scene_flow')
        H, W = self.imshapes[0]
        valid = (t['state'][:, 0] == 2) & (t['state'][:, 1] == 2)
        flow3d = torch.where(valid[..., None], t['xyz'][:, 1] - t['xyz'][:, 0], torch.zeros((), device=valid.device))
        out = dict(flow3d=flow3d.view(-1, H, W, 3), valid=valid.view(-1, H, W), target_xy=t['xy'][:, 1].reshape(-1, H, W, 2),
                   target_pix=t['pix'][:, 1].reshape(-1, H, W))
        if i is None:
            out['edges'] = list(self.edges)
            return out
        return {k: v[0] for k, v in out.items()}

    def save_tracks(self, path, **kw):
        """get_tracks(**kw) written as an npz of host arrays (tool/tracks.py: write_tracks_npz); returns the dict."""
        from ...tool.tracks import write_tracks_npz
        tr = self.get_tracks(**kw)
        write_tracks_npz(path, tr)
        return tr

    def clean_pointcloud(self, tol=0.001, bad_conf=0, dbg=()):
        """base_opt.py:268-278: lower the confidence of points that another, more confident view sees through.  Computed by the
        aligner handle from its own state (csrc/scene.hip, AlignEngine.clean_confidences): the decisions are those of the
        module-level clean_pointcloud() below except at pixels within rounding distance of one of its comparisons.
        A3R_CLEAN=torch (read at every call) takes that torch function instead."""
        if os.environ.get('A3R_CLEAN', '') == 'torch':
            cams = inv_rigid(self.get_im_poses())
            new_confs = clean_pointcloud([c.to(self.device) for c in self.im_conf], self.get_intrinsics(), cams, self.get_depthmaps(),
                                         self.get_pts3d(), tol=tol, bad_conf=bad_conf, dbg=dbg)
            for i, c in enumerate(new_confs):
                self.im_conf[i] = c.to(self.im_conf[i].device)
            return self
        e = self._need_engine()
        out = e.clean_confidences(torch.stack([_ravel_hw(c.to(self.device).float(), self.max_area) for c in self.im_conf]), tol, bad_conf)
        for i, (c, (h, w)) in enumerate(zip(self.im_conf, self.imshapes)):
            self.im_conf[i] = out[i, :h * w].view(h, w).to(device=c.device, dtype=c.dtype)
        return self

    # ------------------------------------------------------------------ presets (optimizer.py:76-113)
    def _msk_indices(self, msk):
        if msk is None:
            return list(range(self.n_imgs))
        if isinstance(msk, int):
            return [msk]
        msk = np.asarray(msk)
        return np.where(msk)[0].tolist() if msk.dtype == bool else msk.tolist()

    def _set_known(self, group, idxs, msk):
        """How the images `idxs` touched by a preset_* call become known.  Here: all images at once or not at all, the handle-wide
        train_* switch of the group goes off (and known poses end the normalisation of the pairwise scales)."""
        assert self._msk_indices(msk) == list(range(self.n_imgs)), 'incomplete mask!'
        flag = dict(pose='train_poses', focal='train_focals', pp='train_pp')[group]
        self._flags[flag] = self.engine.flags[flag] = False
        if group == 'pose':
            self.norm_pw_scale = self.engine.flags['norm_pw_scale'] = False

    def _announce_preset(self, group, idx, value):
        pass

    def _preset(self, group, key, values, msk, encode):
        """The body of the preset_* methods: encode(idx, value) -> (the parameter row of image idx, what to announce) for the
        images msk selects, written into parameter `key`; the images become known (_set_known)."""
        e = self._need_engine()
        p = e.params[key].clone()
        idxs = []
        for idx, value in zip(self._msk_indices(msk), values):
            p[idx], shown = encode(idx, value)
            self._announce_preset(group, idx, shown)
            idxs.append(idx)
        self._set_known(group, idxs, msk)
        e.set_params(**{key: p})

    def preset_pose(self, known_poses, pose_msk=None):          # cam-to-world
        if isinstance(known_poses, torch.Tensor) and known_poses.ndim == 2:
            known_poses = [known_poses]

        def encode(idx, pose):
            pose = torch.as_tensor(pose, dtype=torch.float32).cpu()
            return torch.cat((rotmat_to_unitquat(pose[:3, :3]), signed_log1p(pose[:3, 3]))).to(self.device), pose[:3, 3]
        self._preset('pose', 'im_poses', known_poses, pose_msk, encode)

    def preset_focal(self, known_focals, msk=None):
        self._preset('focal', 'im_focals', known_focals, msk,
                     lambda idx, focal: (self.focal_break * float(np.log(float(focal))), focal))

    def preset_principal_point(self, known_pp, msk=None):
        def encode(idx, p):
            H, W = self.imshapes[idx]
            return (torch.as_tensor(p, dtype=torch.float32).to(self.device) - torch.tensor([W / 2, H / 2], device=self.device)) / 10, p
        self._preset('pp', 'im_pp', known_pp, msk, encode)

    # ------------------------------------------------------------------ optimisation (base_opt.py:373-464)
    def forward(self):
        """The alignment loss of the current state (a 0-d device tensor)."""
        return self._need_engine().loss()[0]

    __call__ = forward

    def _init_known_poses(self, niter_PnP):
        from .init_im_poses import init_from_known_poses              # PnP stand-in: parity unpinned (see that module)
        init_from_known_poses(self, niter_PnP=niter_PnP, min_conf_thr=self.min_conf_thr)

    def _mst_state_written(self):
        """Called by init='mst' once the state is written and before its verbose loss line; the flow class captures its prior here."""

    def _init_from(self, init, init_priors, niter_PnP):
        if init is None:
            pass
        elif init in ('msp', 'mst'):
            from .init_im_poses import init_minimum_spanning_tree       # pinned except the PnP solve (see that module)
            init_minimum_spanning_tree(self, init_priors=init_priors, niter_PnP=niter_PnP)
        elif init == 'known_poses':
            self._init_known_poses(niter_PnP)
        else:
            raise ValueError(f'bad value for {init=}')

    def _run_and_report(self, niter, lr, schedule, lr_min, note=''):
        e = self._need_engine()
        e.set_params(reset_optimizer=True)            # a fresh torch.optim.Adam per call (base_opt.py:435)
        losses = e.run(niter, lr, schedule, lr_min)
        if self.verbose:
            print(f'Global alignement - {niter} iterations,{note} loss={losses[-1]:g}')
        return float(losses[-1])

    def compute_global_alignment(self, init=None, init_priors=None, niter_PnP=10, lr=0.01, niter=300, schedule='cosine',
                                 lr_min=1e-6):
        e = self._need_engine()
        self._init_from(init, init_priors, niter_PnP)
        if schedule not in ('cosine', 'linear'):
            raise ValueError(f'bad lr {schedule=}')
        if niter <= 0:
            return float('inf')
        if e.steps_done + niter > e.loss_capacity:
            raise RuntimeError('loss history capacity exceeded')
        return self._run_and_report(niter, lr, schedule, lr_min, note=f' final lr={lr_min if niter > 1 else lr:g}')


def _ravel_hw(tensor, fill=0):
    """Flatten the two leading (H, W) axes and zero-fill up to `fill` rows (optimizer.py:271-277)."""
    tensor = tensor.reshape((tensor.shape[0] * tensor.shape[1],) + tuple(tensor.shape[2:]))
    if len(tensor) < fill:
        tensor = torch.cat((tensor, tensor.new_zeros((fill - len(tensor),) + tuple(tensor.shape[1:]))))
    return tensor


def clean_pointcloud(im_confs, K, cams, depthmaps, all_pts3d, tol=0.001, bad_conf=0, dbg=()):
    """base_opt.py:468-503.  Every image's points are projected into every other view; a point that lands (rounded to a pixel)
    in front of that view's depth map by more than `tol` while being the less confident of the two has its confidence clipped
    to `bad_conf`.  The confidences are updated in place of the running copy, pair after pair, in the reference's (i, j) order."""
    assert len(im_confs) == len(cams) == len(K) == len(depthmaps) == len(all_pts3d)
    assert 0 <= tol < 1
    res = [c.clone() for c in im_confs]
    all_pts3d = [p.reshape(*c.shape, 3) for p, c in zip(all_pts3d, im_confs)]
    depthmaps = [d.reshape(*c.shape) for d, c in zip(depthmaps, im_confs)]
    for i, pts3d in enumerate(all_pts3d):
        for j in range(len(all_pts3d)):
            if i == j:
                continue
            proj = pts3d @ cams[j][:3, :3].T + cams[j][:3, 3]                 # world -> camera j
            proj_depth = proj[:, :, 2]
            uvw = proj @ K[j].T
            uv = (uvw[..., :2] / uvw[..., 2:3]).round().long()                # geotrf(K, proj, norm=1, ncol=2)
            u, v = uv.unbind(-1)
            H, W = im_confs[j].shape
            msk_i = (proj_depth > 0) & (0 <= u) & (u < W) & (0 <= v) & (v < H)
            msk_j = v[msk_i], u[msk_i]
            bad_points = (proj_depth[msk_i] < (1 - tol) * depthmaps[j][msk_j]) & (res[i][msk_i] < res[j][msk_j])
            bad_msk_i = msk_i.clone()
            bad_msk_i[msk_i] = bad_points
            res[i][bad_msk_i] = res[i][bad_msk_i].clip(max=bad_conf)
    return res
