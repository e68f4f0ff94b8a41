"""Hierarchical keyframe -> clip global alignment for long videos and its output files.

What tool/depth_test.py:395-435,628-676 and tool/demo.py:173-251 (get_reconstructed_scene_hierachical) run:
  1. cut the frame list into clips of `clip_size` frames; the first frame of every clip is a keyframe;
  2. pair-forward + global alignment (init='mst') over the complete, non-symmetrised keyframe graph;
  3. per clip: pair-forward over the complete non-symmetrised clip graph, alignment with init='mst' and
     init_priors = [keyframe pose, keyframe depth, keyframe focal] so that every clip lands in the keyframes' world frame;
  4. concatenate per-frame depth maps / confidences / poses / intrinsics and write them out.
Everything numerical goes through the mirror package (HIP pair forward, HIP aligner); this module is host-side sequencing and
file formats.  `my_make_pairs` / `choose_clip_size` / the TUM conversion are pinned against the reference (tests/golden/hier.json).
"""
from __future__ import annotations

import os
from pathlib import Path

import numpy as np
import torch


def choose_clip_size(n_frames: int, clip_size: int = 50) -> int:
    """depth_test.py:637-638 / demo.py:194-195: shrink until no clip is empty or a single frame."""
    while n_frames % clip_size == 1 or n_frames % clip_size == 0 or clip_size > n_frames:
        clip_size -= 1
    return clip_size


def _complete_upper_pairs(views):
    return [(views[i], views[j]) for i in range(len(views) - 1) for j in range(i + 1, len(views))]


def my_make_pairs(imgs, clip_size):
    """depth_test.py:395-435.  Returns (coarse_init_pairs, keyframes_id, all_clips_pairs, all_clips_id); like the reference it
    re-numbers `idx` inside every clip IN PLACE (the clips hold the caller's dicts) and copies the dicts that go into pairs."""
    keyframes_id = list(range(0, len(imgs), clip_size))
    keyframes = [imgs[i].copy() for i in keyframes_id]
    clips = [imgs[i:i + clip_size] for i in keyframes_id]
    for index, view in enumerate(keyframes):
        view['idx'] = index
    coarse_init_pairs = _complete_upper_pairs(keyframes)
    all_clips_id = []
    for clip in clips:
        all_clips_id.append([view['idx'] for view in clip])
        for index, view in enumerate(clip):
            view['idx'] = index
    all_clips_pairs = [[(a.copy(), b.copy()) for a, b in _complete_upper_pairs(clip)] for clip in clips]
    return coarse_init_pairs, keyframes_id, all_clips_pairs, all_clips_id


def my_make_pairs_pose(imgs, clip_size):
    """tool/pose_test.py:551-591, the pair builder of the pose pipeline (--mode eval_pose_h).  Against my_make_pairs: the keyframe
    graph is complete AND symmetrised; a clip's graph is (i, j) for j in range(i + 1, len(clip), 2) followed by the same pairs
    reversed, so that edge e + E/2 is the reverse of edge e (what use_self_mask asks for).  `idx` is re-numbered in place and the
    dicts are copied exactly as there: the keyframe pairs share one copy per keyframe, the reversed clip pairs share the copies
    of the forward ones."""
    keyframes_id = list(range(0, len(imgs), clip_size))
    keyframes = [imgs[i].copy() for i in keyframes_id]
    clips = [imgs[i:i + clip_size] for i in keyframes_id]
    for index, view in enumerate(keyframes):
        view['idx'] = index
    coarse_init_pairs = _complete_upper_pairs(keyframes)
    coarse_init_pairs += [(b, a) for a, b in coarse_init_pairs]
    all_clips_id = []
    for clip in clips:
        all_clips_id.append([view['idx'] for view in clip])
        for index, view in enumerate(clip):
            view['idx'] = index
    all_clips_pairs = []
    for clip in clips:
        pairs = [(clip[i].copy(), clip[j].copy()) for i in range(len(clip) - 1) for j in range(i + 1, len(clip), 2)]
        all_clips_pairs.append(pairs + [(b, a) for a, b in pairs])
    return coarse_init_pairs, keyframes_id, all_clips_pairs, all_clips_id


# ------------------------------------------------------------------------------------------- output formats
def c2w_to_tumpose(c2w):
    """4x4 cam-to-world -> [x y z qw qx qy qz] (cloud_opt/base_opt.py:31-44; scipy's Rotation.as_quat sign convention:
    the quaternion is canonicalised to qw >= 0)."""
    c2w = np.asarray(c2w.detach().cpu() if isinstance(c2w, torch.Tensor) else c2w)
    from scipy.spatial.transform import Rotation
    qx, qy, qz, qw = Rotation.from_matrix(c2w[:3, :3]).as_quat()
    return np.concatenate([c2w[:3, -1], [qw, qx, qy, qz]])


def get_tum_poses(poses):
    """[N,4,4] -> [tum_poses [N,7], timestamps [N]] (base_opt.py:279-284)."""
    return [np.stack([c2w_to_tumpose(p) for p in poses], 0), np.arange(len(poses)).astype(float)]


def save_trajectory_tum_format(traj, filename):
    """`timestamp x y z qw qx qy qz` per line, numbers printed with str() (utils/vo_eval.py:308-316)."""
    poses, stamps = traj
    with Path(filename).open('w') as f:
        for t, p in zip(stamps, poses):
            f.write(f"{t} {' '.join(map(str, p[:3]))} {' '.join(map(str, p[3:]))}\n")


def save_intrinsics(K, path):
    """[N,3,3] -> one row of 9 numbers per frame, '%.6f' (base_opt.py:297-301)."""
    K = np.asarray(K.detach().cpu() if isinstance(K, torch.Tensor) else K)
    np.savetxt(path, K.reshape(-1, 9), fmt='%.6f')
    return K


def save_frame_arrays(arrays, folder, pattern, start=0):
    """np.save each per-frame array as folder/pattern.format(start + i) (base_opt.py:303-313,329-343: conf_{i}.npy,
    frame_{i:04d}.npy; the reference's colour-mapped PNG / GIF previews need cv2 and are not written)."""
    for i, a in enumerate(arrays):
        a = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
        np.save(os.path.join(folder, pattern.format(start + i)), a)


# ------------------------------------------------------------------------------------------- the driver
# the options of flow=dict(...) and their defaults: tool/pose_test.py:392-402 with that file's argument defaults
FLOW_DEFAULTS = dict(flow_loss_weight=0.01, temporal_smoothing_weight=0.01, translation_weight=1.0, flow_loss_start_epoch=0.1,
                     flow_loss_thre=40, pxl_thre=50, motion_mask_thre=0.35, depth_regularize_weight=0, shared_focal=True,
                     use_self_mask=True, flow_net=None, flow_fn=None)


def _flow_options(flow):
    unknown = sorted(set(flow) - set(FLOW_DEFAULTS))
    if unknown:
        raise ValueError(f'hierarchical_alignment: unknown flow option(s) {unknown}; known: {sorted(FLOW_DEFAULTS)}')
    return {**FLOW_DEFAULTS, **flow}


def _collect_mesh(scene, mesh_collector, double_sided):
    if mesh_collector is None:
        return
    m = scene.get_mesh(double_sided=double_sided)
    mesh_collector.append({k: (m[k].cpu().numpy() if k in m else None) for k in ('xyz', 'rgb', 'faces', 'face_rgb')})


def _hierarchical_flow(imgs, model, device, opt, *, clip_size, niter, schedule, lr, min_conf_thr, batch_size, verbose,
                       output_dir, pointcloud_collector, clean, obs_dtype, device_resident, mesh_collector, mesh_double_sided):
    """The two stages of tool/pose_test.py:346-479 (--mode eval_pose_h): keyframes, then every clip, through the flow-regularised
    aligner; every clip is initialised on its keyframe (init_priors) and its poses are re-anchored on the keyframe pose."""
    from ..dust3r.cloud_opt_flow import GlobalAlignerMode, global_aligner
    from ..dust3r.inference import inference
    from ..dust3r.cloud_opt_flow.optimizer import load_flow_net, place_flow_net
    from ..dust3r.utils.image_pose import enlarge_seg_masks

    if len(imgs) < 3:
        raise ValueError('hierarchical_alignment needs at least 3 frames (for two frames use GlobalAlignerMode.PairViewer directly)')
    try:
        clip_size = choose_clip_size(len(imgs), clip_size)
    except ZeroDivisionError:                     # the reference's rule runs off the end: no size leaves every clip two frames or more
        raise ValueError(f'hierarchical_alignment: {len(imgs)} frames cannot be cut into clips of at most {clip_size} frames with two '
                         'or more frames each and two or more clips (3 frames never can; use 4 or more)') from None
    coarse_init_pairs, keyframes_id, all_clips_pairs, all_clips_id = my_make_pairs_pose(imgs, clip_size)
    flow_fn = opt['flow_fn']
    # the one flow network of a run: loaded and placed once, every scene's get_flow() finds its engine where it needs it
    flow_net = place_flow_net(load_flow_net(opt['flow_net']), device) if flow_fn is None and opt['flow_loss_weight'] > 0 else None
    scene_kw = {k: opt[k] for k in ('flow_loss_weight', 'temporal_smoothing_weight', 'translation_weight', 'flow_loss_start_epoch',
                                    'flow_loss_thre', 'pxl_thre', 'motion_mask_thre', 'depth_regularize_weight', 'shared_focal',
                                    'use_self_mask')}
    infer_kw = dict(keep_on_device=True) if device_resident else {}      # passed in this mode only

    def align(pairs, init_priors=None):
        out = inference(pairs, model, device, batch_size=batch_size, verbose=verbose, **infer_kw)      # no clamp: pose_test.py has none
        kw = dict(scene_kw)
        if flow_fn is not None:
            as_list = lambda idx: idx if isinstance(idx, list) else torch.as_tensor(idx).tolist()
            edges = [(int(i), int(j)) for i, j in zip(as_list(out['view1']['idx']), as_list(out['view2']['idx']))]
            kw['flow'] = flow_fn(edges, (out['view1'], out['view2']))
        else:
            kw['flow_net'] = flow_net
        scene = global_aligner(out, device, mode=GlobalAlignerMode.PointCloudOptimizer, verbose=verbose, min_conf_thr=min_conf_thr,
                               num_total_iter=niter, obs_dtype=obs_dtype, **kw)
        scene.compute_global_alignment(init='mst', init_priors=init_priors, niter=niter, schedule=schedule, lr=lr)
        if clean:
            scene.clean_pointcloud()
        return scene

    host = lambda t: t.detach().cpu().numpy()
    key_scene = align(coarse_init_pairs)
    # the priors of the clip stage: three small read-backs for the whole stage
    key_poses = host(key_scene.get_im_poses()).tolist()
    key_depths = host(torch.stack(list(key_scene.get_depthmaps())))
    key_focals = host(key_scene.get_focals()).tolist()
    res = dict(depths=[], confs=[], init_confs=[], dynamic_masks=[], poses=[], poses_raw=[], focals=[], intrinsics=[],
               keyframes_id=keyframes_id, all_clips_id=all_clips_id, clip_size=clip_size, key_scene=key_scene)
    if output_dir is not None:
        os.makedirs(output_dir, exist_ok=True)
    offset = 0
    traj = [np.zeros((0, 7)), np.zeros((0,))]
    for c, clip_pairs in enumerate(all_clips_pairs):
        scene = align(clip_pairs, [key_poses[c], key_depths[c], key_focals[c]])
        pred_traj = scene.get_tum_poses(key_poses[c])
        raw = host(scene.get_im_poses())
        n = len(raw)
        res['poses_raw'] += list(raw)
        res['poses'] += list(scene.align_poses(np.array(key_poses[c]), raw))
        res['depths'] += [host(d) for d in scene.get_depthmaps()]
        res['confs'] += [host(x) for x in scene.get_conf()]
        res['init_confs'] += [host(x) for x in scene.get_init_conf()]
        res['dynamic_masks'] += ([host(torch.as_tensor(m)).astype(bool) for m in scene.dynamic_masks]
                                 if scene.dynamic_masks is not None else [None] * n)
        res['focals'] += host(scene.get_focals()).reshape(-1).tolist()
        res['intrinsics'] += list(host(scene.get_intrinsics()))
        if pointcloud_collector is not None:
            pc = scene.get_pointcloud()
            pointcloud_collector.append(dict(xyz=pc['xyz'].cpu().numpy(), rgb=pc['rgb'].cpu().numpy() if 'rgb' in pc else None))
        _collect_mesh(scene, mesh_collector, mesh_double_sided)
        if output_dir is not None:                  # per clip, with running offsets (pose_test.py:463-475)
            traj = [np.concatenate([traj[0], pred_traj[0]], axis=0), np.concatenate([traj[1], pred_traj[1] + offset], axis=0)]
            save_trajectory_tum_format(traj, os.path.join(output_dir, 'pred_traj.txt'))
            save_intrinsics(np.stack(res['intrinsics']), os.path.join(output_dir, 'pred_intrinsics.txt'))
            np.savetxt(os.path.join(output_dir, 'pred_focal.txt'), np.asarray(res['focals']).reshape(-1, 1), fmt='%.6f')
            save_frame_arrays(res['depths'][offset:], output_dir, 'frame_{:04d}.npy', offset)
            save_frame_arrays(res['confs'][offset:], output_dir, 'conf_{}.npy', offset)
            save_frame_arrays(res['init_confs'][offset:], output_dir, 'init_conf_{}.npy', offset)
            if scene.dynamic_masks is not None:
                scene.save_dynamic_masks(output_dir, offset)
        offset += n
    if output_dir is not None:
        enlarge_seg_masks(output_dir, kernel_size=3 if opt['use_self_mask'] else 5)
    return res


def hierarchical_alignment(imgs, model, device, *, clip_size=50, niter=300, schedule='linear', lr=0.05, min_conf_thr=3,
                           if_use_mono=False, mono_depths=(), batch_size=1, clamp_conf=None, verbose=False, output_dir=None,
                           pointcloud_collector=None, clean=False, obs_dtype='fp32', flow=None, device_resident=False,
                           mesh_collector=None, mesh_double_sided=False):
    """Keyframe pass + per-clip passes (depth_test.py:636-676).  `imgs`: view dicts (load_images).  Returns a dict with the
    per-frame lists `depths`, `confs`, `poses` ([4,4] cam-to-world in the keyframes' frame), `focals`, `intrinsics`, plus
    `keyframes_id`, `clip_size` and the keyframe scene's own results; writes pred_traj.txt / pred_intrinsics.txt /
    frame_XXXX.npy / conf_X.npy under `output_dir` when given (demo.py:225-243).
    `pointcloud_collector`: a list that receives, in clip order, every clip scene's get_pointcloud() as host arrays
    dict(xyz, rgb | None); off by default.
    `mesh_collector`: a list that receives, in clip order, every clip scene's get_mesh(double_sided=mesh_double_sided) as host
    arrays dict(xyz, rgb | None, faces, face_rgb | None), faces indexing the clip's own vertices; off by default.
    `clean`: scene.clean_pointcloud() on the keyframe scene and on every clip scene right after its alignment (pose_test.py:205,475),
    so the confidences returned, written and thresholded by the collector are the cleaned ones; off by default.
    `flow`: None = the plain aligner over my_make_pairs graphs (tool/depth_test.py).  A dict (FLOW_DEFAULTS names the options;
    `flow_net` a loaded RAFT2 or a checkpoint path, or `flow_fn(edges, (view1, view2)) -> (flow_ij, flow_ji)`, each [E,2,H,W], for
    injected flow) = the pose pipeline of tool/pose_test.py:346-479: my_make_pairs_pose graphs, the flow-regularised aligner for
    the keyframes and for every clip, poses re-anchored on the keyframe poses; the result also holds `init_confs`,
    `dynamic_masks`, `poses_raw` (before re-anchoring) and `all_clips_id`, and pred_focal.txt, init_conf_X.npy,
    dynamic_mask_X.png and enlarged_dynamic_mask_X.png are written too.  The flow network is built once for the whole run.
    Confidences are used as predicted there: `clamp_conf` (default: on without `flow`) is a step of the depth pipeline only and is
    refused together with `flow`.
    `device_resident` (with `flow` only): the pair forwards keep their outputs on the device (inference(keep_on_device=True)), so
    every scene takes the device routes for confidences, weights, edge scores and the MST initialisation (init_priors included)."""
    if flow is not None:
        opt = _flow_options(flow)
        if if_use_mono:
            raise ValueError('hierarchical_alignment: the flow aligner has no mono-depth parameterisation (if_use_mono)')
        if clamp_conf:
            raise ValueError('hierarchical_alignment: clamp_conf is the depth pipeline\'s step (depth_test.py:648-649); the pose '
                             'pipeline (flow=) aligns on the confidences as predicted')
        return _hierarchical_flow(imgs, model, device, opt, clip_size=clip_size, niter=niter, schedule=schedule, lr=lr,
                                  min_conf_thr=min_conf_thr, batch_size=batch_size, verbose=verbose,
                                  output_dir=output_dir, pointcloud_collector=pointcloud_collector, clean=clean, obs_dtype=obs_dtype,
                                  device_resident=device_resident, mesh_collector=mesh_collector, mesh_double_sided=mesh_double_sided)
    if device_resident:
        raise ValueError('hierarchical_alignment: device_resident belongs to the flow pipeline (flow=dict(...))')
    if clamp_conf is None:
        clamp_conf = True                          # depth_test.py:648-649,662-663
    from ..dust3r.cloud_opt import GlobalAlignerMode, global_aligner
    from ..dust3r.inference import inference

    if len(imgs) < 3:
        raise ValueError('hierarchical_alignment needs at least 3 frames (for two frames use GlobalAlignerMode.PairViewer directly)')
    clip_size = choose_clip_size(len(imgs), clip_size)
    coarse_init_pairs, keyframes_id, all_clips_pairs, _ = my_make_pairs(imgs, clip_size)

    def clamp(out):
        if clamp_conf:       # depth_test.py:648-649,662-663: every confidence above 1 becomes 10
            for side in ('pred1', 'pred2'):
                out[side]['conf'][out[side]['conf'] > 1] = 10
        return out

    def align(out, init_priors=None):
        scene = global_aligner(out, if_use_mono, list(mono_depths), device=device, mode=GlobalAlignerMode.PointCloudOptimizer,
                               verbose=verbose, min_conf_thr=min_conf_thr, obs_dtype=obs_dtype)
        scene.compute_global_alignment(init='mst', init_priors=init_priors, niter=niter, schedule=schedule, lr=lr)
        if clean:
            scene.clean_pointcloud()
        return scene

    key_scene = None
    if len(keyframes_id) >= 2:
        key_scene = align(clamp(inference(coarse_init_pairs, model, device, batch_size=batch_size, verbose=verbose)))
        key_poses = key_scene.get_im_poses().detach().cpu().numpy().tolist()
        key_depths = [d.detach().cpu().numpy() for d in key_scene.get_depthmaps()]
        key_focals = key_scene.get_focals().detach().cpu().numpy().tolist()
    res = dict(depths=[], confs=[], poses=[], focals=[], intrinsics=[], keyframes_id=keyframes_id, clip_size=clip_size,
               key_scene=key_scene)
    for c, clip_pairs in enumerate(all_clips_pairs):
        priors = [key_poses[c], key_depths[c], key_focals[c]] if key_scene is not None else None
        scene = align(clamp(inference(clip_pairs, model, device, batch_size=batch_size, verbose=verbose)), priors)
        res['depths'] += [d.detach().cpu().numpy() for d in scene.get_depthmaps()]
        res['confs'] += [x.detach().cpu().numpy() for x in scene.get_conf()]
        res['poses'] += list(scene.get_im_poses().detach().cpu().numpy())
        res['focals'] += scene.get_focals().detach().cpu().numpy().reshape(-1).tolist()
        res['intrinsics'] += list(scene.get_intrinsics().detach().cpu().numpy())
        if pointcloud_collector is not None:
            pc = scene.get_pointcloud()
            pointcloud_collector.append(dict(xyz=pc['xyz'].cpu().numpy(), rgb=pc['rgb'].cpu().numpy() if 'rgb' in pc else None))
        _collect_mesh(scene, mesh_collector, mesh_double_sided)
    if output_dir is not None:
        os.makedirs(output_dir, exist_ok=True)
        save_trajectory_tum_format(get_tum_poses(res['poses']), os.path.join(output_dir, 'pred_traj.txt'))
        save_intrinsics(np.stack(res['intrinsics']), os.path.join(output_dir, 'pred_intrinsics.txt'))
        save_frame_arrays(res['depths'], output_dir, 'frame_{:04d}.npy')
        save_frame_arrays(res['confs'], output_dir, 'conf_{}.npy')
    return res
