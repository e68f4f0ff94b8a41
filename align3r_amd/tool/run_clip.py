#!/usr/bin/env python3
"""End-to-end driver: image folder (+ mono-depth .npz priors) -> pointmaps -> globally aligned depth / poses / intrinsics on disk.

The flow of the reference's tool/demo.py and tool/depth_test.py through this package only:
    load_images (N3)  ->  make_pairs  ->  inference (HIP pair forward)  ->  global_aligner / hierarchical_alignment (HIP aligner, N2)
    ->  pred_traj.txt, pred_intrinsics.txt, frame_XXXX.npy, conf_X.npy   (+ depth metrics when ground truth is given)
    ->  --pointcloud PATH: the aligned scene as a binary PLY (points above --min-conf-thr, compacted on the device)
        --pointcloud-voxel V: one point per occupied cell of a grid of edge V instead of every pixel (hashed on the device)
    ->  --matches DIR: matches_{i}_{i+1}.npz, the reciprocal 3-D nearest-neighbour pixel correspondences of consecutive frames
    ->  --render DIR: render_XXXX.png, the whole aligned scene drawn from every frame's own camera (z-buffered point splats)
    ->  --fused-mesh PATH --fused-voxel V: one surface for the whole clip, the depth maps fused into a TSDF grid of edge V (binary PLY)
    ->  --flow --tracks PATH.npz: a grid of points of one frame followed through all later frames (3-D trajectories)
    ->  --flow --scene-flow DIR: scene_flow_{i}_{i+1}.npz, the 3-D motion of every pixel between consecutive frames

    python -m align3r_amd.tool.run_clip --images DIR --weights CKPT.pth --out OUT [--size 512] [--scene-graph swin-3-noncyclic]
           [--hierarchical --clip-size 50] [--niter 300] [--schedule linear] [--lr 0.01] [--traj-format custom] [--gt-depth DIR]
           [--metrics-device] [--pointcloud scene.ply [--pointcloud-voxel V [--pointcloud-reduce best|mean] [--pointcloud-min-count C]]]
           [--matches DIR] [--render DIR [--render-radius R]] [--clean] [--device-prep]
           [--fused-mesh PATH --fused-voxel V [--fused-trunc T] [--fused-max-depth D]]
           [--flow [--flow-weights RAFT.pth] [--gt-masks DIR] [--not-shared-focal]
                   [--tracks PATH.npz [--track-start K] [--track-stride G]] [--scene-flow DIR]]
           [--flow-hierarchical [--clip-size 10] [--device-resident] [--flow-weights ...] [--gt-masks DIR] [--not-shared-focal]]

--flow is the sequence of the reference's tool/pose_test.py:154-216: the flow-regularised aligner (cloud_opt_flow) with self-computed
motion masks on a swinstride-5-noncyclic graph, and on top of the usual outputs pred_focal.txt, dynamic_mask_X.png, their 3x3-enlarged
copies enlarged_dynamic_mask_X.png (5x5 with --gt-masks) and init_conf_X.npy.
--flow-hierarchical is tool/pose_test.py --mode eval_pose_h (:346-479): the same aligner and settings for a keyframe graph and then
for every clip of --clip-size frames (default 10 in this mode), each clip initialised on and re-anchored at its keyframe; with
--device-resident the pair forwards stay on the device and every clip takes the device initialisation.
"""
from __future__ import annotations

import argparse
import glob
import os

import numpy as np
import torch


def parse(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--images", required=True, help="folder (or single file) of frames; priors are looked up per --traj-format")
    ap.add_argument("--weights", required=True, help="reference-format checkpoint (.pth)")
    ap.add_argument("--out", required=True)
    ap.add_argument("--device", default="cuda")
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--traj-format", default="custom")
    ap.add_argument("--depth-prior-name", default="depthpro")
    ap.add_argument("--start", type=int, default=0)
    ap.add_argument("--interval", type=int, default=10 ** 9)
    ap.add_argument("--scene-graph", default=None, help="default: swin-3-noncyclic, with --flow swinstride-5-noncyclic")
    ap.add_argument("--batch-size", type=int, default=16)
    ap.add_argument("--hierarchical", action="store_true", help="keyframe -> clip alignment (tool/depth_test.py:628-676)")
    ap.add_argument("--clip-size", type=int, default=None, help="default: 50 with --hierarchical, 10 with --flow-hierarchical")
    ap.add_argument("--niter", type=int, default=300)
    ap.add_argument("--schedule", default="linear")
    ap.add_argument("--lr", type=float, default=0.01)
    ap.add_argument("--min-conf-thr", type=float, default=3.0)
    ap.add_argument("--gt-depth", default=None, help="folder of per-frame ground-truth depth .npy (same order) -> AbsRel etc.")
    ap.add_argument("--depth-max", type=float, default=70.0)
    ap.add_argument("--metrics-device", action="store_true",
                    help="evaluate --gt-depth on --device (csrc/metrics.hip: the LAD scale + shift and the metric sums as HIP kernels; the "
                         "host numpy + scipy path stays the default)")
    ap.add_argument("--gt-traj", default=None, help="ground-truth camera trajectory, TUM file `t x y z qx qy qz qw` (same frames) -> ATE / RPE")
    ap.add_argument("--pointcloud", default=None, metavar="PATH",
                    help="write the aligned scene as a binary PLY (with --hierarchical: every clip's points, appended in clip order)")
    ap.add_argument("--pointcloud-voxel", type=float, default=None, metavar="V",
                    help="--pointcloud: one point per occupied cell of a grid of edge V, in scene units (ops.voxel_downsample, "
                         "csrc/voxel.hip): the most confident point of a cell; with --hierarchical and --flow-hierarchical the clips' "
                         "clouds are reduced together after the last clip, the earliest clip's point winning a cell")
    ap.add_argument("--pointcloud-reduce", choices=("best", "mean"), default=None,
                    help="--pointcloud-voxel: the cell's winner as it is (best, the default) or the mean of the cell's points and colours")
    ap.add_argument("--pointcloud-min-count", type=int, default=None, metavar="C",
                    help="--pointcloud-voxel: leave out cells with fewer than C points (default 1; 2 removes points seen once)")
    ap.add_argument("--mesh", default=None, metavar="PATH",
                    help="write the aligned scene as a triangle mesh (binary PLY: the kept points as vertices, two triangles per pixel "
                         "quad whose corners are kept; with --hierarchical: every clip's mesh, appended in clip order)")
    ap.add_argument("--mesh-double-sided", action="store_true",
                    help="--mesh: every triangle also wound backwards (what the reference hands to its viewer against face culling)")
    ap.add_argument("--matches", default=None, metavar="DIR",
                    help="after the alignment (and after --clean) write DIR/matches_{i}_{i+1}.npz for every consecutive frame pair: the "
                         "reciprocal 3-D nearest neighbours between the two frames' points above --min-conf-thr (scene.get_matches, "
                         "csrc/match.hip; keys idx_i idx_j xy_i xy_j xyz_i xyz_j count); with --flow the dynamic pixels are masked out. "
                         "Refused with --hierarchical and --flow-hierarchical: their clips are aligned one after another and no "
                         "scene holds two neighbouring clips' frames at once")
    ap.add_argument("--render", default=None, metavar="DIR",
                    help="after the alignment (and after --clean) write DIR/render_XXXX.png for every frame: the whole aligned scene -- "
                         "the points above --min-conf-thr -- drawn from that frame's own camera at the frame's own size as z-buffered "
                         "point splats (scene.save_renders, csrc/render.hip); with --flow the dynamic pixels are masked out. "
                         "Refused with --hierarchical and --flow-hierarchical: their clips are aligned one after another and no "
                         "scene holds all frames at once")
    ap.add_argument("--render-radius", type=int, default=None, metavar="R",
                    help="--render: a point covers (2 R + 1)^2 pixels, R in [0, 8] (default 1)")
    ap.add_argument("--fused-mesh", default=None, metavar="PATH",
                    help="after the alignment (and after --clean) fuse the aligned depth maps of all frames into one TSDF grid of edge "
                         "--fused-voxel and write its zero surface as one triangle mesh (binary PLY; scene.save_fused_mesh, "
                         "csrc/tsdf.hip): the pixels above --min-conf-thr weighted by their confidence; with --flow the dynamic pixels "
                         "are masked out. Refused with --hierarchical and --flow-hierarchical: their clips are aligned one after "
                         "another and no scene holds all frames at once")
    ap.add_argument("--fused-voxel", type=float, default=None, metavar="V", help="--fused-mesh: the voxel's edge in scene units (required)")
    ap.add_argument("--fused-trunc", type=float, default=None, metavar="T",
                    help="--fused-mesh: the truncation distance in scene units (default 3 V)")
    ap.add_argument("--fused-max-depth", type=float, default=None, metavar="D",
                    help="--fused-mesh: depths beyond D are not fused and do not widen the grid (default: no limit)")
    ap.add_argument("--tracks", default=None, metavar="PATH.npz",
                    help="--flow: after the alignment (and after --clean) follow a grid of points of frame --track-start through all later "
                         "frames by the optical flow of consecutive frames and write their 3-D trajectories (scene.get_tracks, "
                         "csrc/track.hip; keys xy xyz pix state frames; state 2 = on a pixel above --min-conf-thr, 1 = followed but not "
                         "visible, 0 = ended; dynamic pixels are NOT masked out: moving points are what a track is for). "
                         "Refused with --hierarchical and --flow-hierarchical: their clips are aligned one after another and no "
                         "scene holds all frames at once")
    ap.add_argument("--track-start", type=int, default=None, metavar="K", help="--tracks: the frame the grid is seeded in (default 0)")
    ap.add_argument("--track-stride", type=int, default=None, metavar="G", help="--tracks: a seed every G pixels (default 8)")
    ap.add_argument("--scene-flow", default=None, metavar="DIR",
                    help="--flow: after the alignment (and after --clean) write DIR/scene_flow_{i}_{i+1}.npz for every consecutive frame "
                         "pair: the 3-D motion vector of every pixel (scene.get_scene_flow; keys flow3d valid target_xy target_pix). "
                         "Refused with --hierarchical and --flow-hierarchical like --tracks")
    ap.add_argument("--clean", action="store_true",
                    help="scene.clean_pointcloud() after every alignment: confidences of points another, more confident view sees through "
                         "drop to 0 before conf_X.npy and --pointcloud are written (tool/demo.py: clean_depth)")
    ap.add_argument("--flow", action="store_true",
                    help="flow-regularised alignment with self-computed motion masks (tool/pose_test.py:154-216)")
    ap.add_argument("--flow-weights", default=None, metavar="PATH", help="RAFT checkpoint of --flow (flow_net=)")
    ap.add_argument("--gt-masks", default=None, metavar="DIR", help="--flow with motion masks read from DIR instead of self-computed ones")
    ap.add_argument("--not-shared-focal", action="store_true", help="--flow: one focal per image instead of a shared one")
    ap.add_argument("--flow-hierarchical", action="store_true",
                    help="keyframe -> clip alignment with the flow-regularised aligner (tool/pose_test.py --mode eval_pose_h); implies the "
                         "--flow settings")
    ap.add_argument("--device-resident", action="store_true",
                    help="--flow-hierarchical: keep the pair forwards' outputs on the device")
    ap.add_argument("--device-prep", action="store_true",
                    help="un-project, normalise, resize and crop the mono-depth priors, and normalise the images, on --device (csrc/prep.hip: "
                         "the same numbers as the host path, which stays the default)")
    ap.add_argument("--obs-dtype", choices=("fp32", "fp16"), default="fp32",
                    help="storage of the aligner's pair observations: fp16 = packed records, half the bytes per edge (obs16.py); the "
                         "parameters and all arithmetic stay fp32 (no effect with two frames: the PairViewer has no aligner)")
    ap.add_argument("--quiet", action="store_true")
    a = ap.parse_args(argv)
    if a.flow and a.hierarchical:
        ap.error("--flow cannot be combined with --hierarchical: the keyframe / clip alignment has no flow term")
    if a.flow_hierarchical and (a.flow or a.hierarchical):
        ap.error("--flow-hierarchical stands alone: it implies the --flow settings and is its own keyframe / clip driver")
    if a.matches and (a.hierarchical or a.flow_hierarchical):
        ap.error("--matches cannot be combined with --hierarchical or --flow-hierarchical: it needs one scene holding all frames")
    if a.render and (a.hierarchical or a.flow_hierarchical):
        ap.error("--render cannot be combined with --hierarchical or --flow-hierarchical: it needs one scene holding all frames")
    for given, name in ((a.tracks, "--tracks"), (a.scene_flow, "--scene-flow")):
        if given and (a.hierarchical or a.flow_hierarchical):
            ap.error(f"{name} cannot be combined with --hierarchical or --flow-hierarchical: it needs one scene holding all frames")
        if given and not a.flow:
            ap.error(f"{name} needs --flow: tracks and scene flow follow the optical flow the flow aligner holds")
    for given, name in ((a.track_start, "--track-start"), (a.track_stride, "--track-stride")):
        if given is not None and not a.tracks:
            ap.error(f"{name} belongs to --tracks")
    a.track_start = 0 if a.track_start is None else a.track_start
    a.track_stride = 8 if a.track_stride is None else a.track_stride
    if a.track_start < 0:
        ap.error("--track-start is a frame number >= 0")
    if a.track_stride < 1:
        ap.error("--track-stride is at least 1")
    if a.fused_mesh and (a.hierarchical or a.flow_hierarchical):
        ap.error("--fused-mesh cannot be combined with --hierarchical or --flow-hierarchical: it needs one scene holding all frames")
    if a.fused_mesh and a.fused_voxel is None:
        ap.error("--fused-mesh needs --fused-voxel")
    for given, name in ((a.fused_voxel, "--fused-voxel"), (a.fused_trunc, "--fused-trunc"), (a.fused_max_depth, "--fused-max-depth")):
        if given is not None and not a.fused_mesh:
            ap.error(f"{name} belongs to --fused-mesh")
        if given is not None and not (np.isfinite(given) and given > 0):
            ap.error(f"{name} is a finite length > 0")
    if a.render_radius is not None and not a.render:
        ap.error("--render-radius belongs to --render")
    if a.render_radius is None:
        a.render_radius = 1
    if not 0 <= a.render_radius <= 8:
        ap.error("--render-radius is in [0, 8]")
    if a.pointcloud_voxel is not None and not a.pointcloud:
        ap.error("--pointcloud-voxel belongs to --pointcloud")
    for given, name in ((a.pointcloud_reduce, "--pointcloud-reduce"), (a.pointcloud_min_count, "--pointcloud-min-count")):
        if given is not None and a.pointcloud_voxel is None:
            ap.error(f"{name} belongs to --pointcloud-voxel")
    a.pointcloud_reduce = a.pointcloud_reduce or "best"
    a.pointcloud_min_count = 1 if a.pointcloud_min_count is None else a.pointcloud_min_count
    if a.pointcloud_voxel is not None and not (np.isfinite(a.pointcloud_voxel) and a.pointcloud_voxel > 0):
        ap.error("--pointcloud-voxel is a finite edge length > 0")
    if a.pointcloud_min_count < 1:
        ap.error("--pointcloud-min-count is at least 1")
    if a.device_resident and not a.flow_hierarchical:
        ap.error("--device-resident belongs to --flow-hierarchical")
    if a.metrics_device and not a.gt_depth:
        ap.error("--metrics-device belongs to --gt-depth")
    if a.mesh_double_sided and not a.mesh:
        ap.error("--mesh-double-sided belongs to --mesh")
    if a.clip_size is None:
        a.clip_size = 10 if a.flow_hierarchical else 50          # pose_test.py:346 / depth_test.py:636
    if not (a.flow or a.flow_hierarchical):
        for given, name in ((a.flow_weights, "--flow-weights"), (a.gt_masks, "--gt-masks"), (a.not_shared_focal, "--not-shared-focal")):
            if given:
                ap.error(f"{name} belongs to --flow")
    if a.scene_graph is None:
        a.scene_graph = "swinstride-5-noncyclic" if a.flow else "swin-3-noncyclic"
    return a


def write_matches(scene, out_dir, mask_dynamic=False):
    """scene.get_matches(i, i + 1) for every consecutive pair as out_dir/matches_{i}_{i+1}.npz (host arrays); returns the counts."""
    os.makedirs(out_dir, exist_ok=True)
    counts = []
    pc = scene.get_pointcloud(mask_dynamic=mask_dynamic, with_index=True)          # one export for all pairs
    for i in range(scene.n_imgs - 1):
        m = scene.matches_from_cloud(pc, i, i + 1)
        np.savez(os.path.join(out_dir, f"matches_{i}_{i + 1}.npz"),
                 **{k: (v.cpu().numpy() if torch.is_tensor(v) else np.asarray(v)) for k, v in m.items()})
        counts.append(int(m["count"]))
    return counts


def write_voxel_cloud(path, clouds, voxel, reduce="best", min_count=1, device="cuda"):
    """The clouds of the hierarchical drivers' collector (host dicts xyz, rgb in clip order) concatenated, uploaded and reduced by one
    ops.voxel_downsample call without priorities -- the earliest clip's point wins a cell -- and written as one PLY.  Returns
    (points written, points collected)."""
    from .. import ops
    from .pointcloud import write_ply
    xyz = np.concatenate([np.asarray(c["xyz"], np.float32).reshape(-1, 3) for c in clouds]) if clouds else np.zeros((0, 3), np.float32)
    colour = bool(clouds) and all(c["rgb"] is not None for c in clouds)
    rgb = np.concatenate([np.asarray(c["rgb"], np.uint8).reshape(-1, 3) for c in clouds]) if colour else None
    vx = ops.voxel_downsample(torch.from_numpy(xyz).to(device), voxel, rgb=torch.from_numpy(rgb).to(device) if colour else None,
                              reduce=reduce, min_count=min_count)
    if vx["dropped"]:
        import warnings
        warnings.warn(f"--pointcloud-voxel {voxel}: {vx['dropped']} of {len(xyz)} points lie beyond 2^20 cells from the origin and are "
                      "in no voxel")
    write_ply(path, vx["xyz"].cpu().numpy(), vx["rgb"].cpu().numpy() if colour else None)
    return int(vx["xyz"].shape[0]), len(xyz)


def write_fused_mesh(scene, a):
    """--fused-mesh: scene.save_fused_mesh with the driver's settings (the dynamic pixels masked out with --flow); returns
    (vertices, faces) written."""
    m = scene.save_fused_mesh(a.fused_mesh, a.fused_voxel, trunc=a.fused_trunc, max_depth=a.fused_max_depth, mask_dynamic=a.flow)
    return int(m["xyz"].shape[0]), int(m["faces"].shape[0])


def write_tracks(scene, path, start=0, stride=8):
    """A grid of seeds every `stride` pixels of frame `start`, followed through all later frames (scene.save_tracks); returns the
    number of tracks."""
    from .tracks import grid_seeds
    if not 0 <= start < scene.n_imgs - 1:
        raise RuntimeError(f"--track-start {start}: a track needs a later frame (the clip has {scene.n_imgs})")
    tr = scene.save_tracks(path, frames=range(start, scene.n_imgs), seeds=grid_seeds(scene.imshapes[start], stride))
    return int(tr["state"].shape[1])


def write_scene_flow(scene, out_dir):
    """scene.get_scene_flow(i, i + 1) for every consecutive pair as out_dir/scene_flow_{i}_{i+1}.npz (host arrays); returns the
    numbers of valid pixels."""
    os.makedirs(out_dir, exist_ok=True)
    counts = []
    for i in range(scene.n_imgs - 1):
        f = scene.get_scene_flow(i, i + 1)
        np.savez(os.path.join(out_dir, f"scene_flow_{i}_{i + 1}.npz"), **{k: v.cpu().numpy() for k, v in f.items()})
        counts.append(int(f["valid"].sum()))
    return counts


def main(argv=None):
    a = parse(argv)
    from ..dust3r.cloud_opt import GlobalAlignerMode, global_aligner
    from ..dust3r.image_pairs import make_pairs
    from ..dust3r.inference import inference
    from ..dust3r.model import AsymmetricCroCo3DStereo
    from ..dust3r.utils.image_pose import load_images
    from . import hierarchical as hz
    from .depth_metrics import evaluate_depth
    from .pointcloud import write_ply_mesh_parts, write_ply_parts

    verbose = not a.quiet
    model = AsymmetricCroCo3DStereo.from_pretrained(a.weights).to(a.device)
    imgs, _ = load_images(a.images, a.size, verbose=verbose, traj_format=a.traj_format, start=a.start, interval=a.interval,
                          depth_prior_name=a.depth_prior_name, prep_device=a.device if a.device_prep else None,
                          dynamic_mask_root=a.gt_masks if (a.flow or a.flow_hierarchical) and a.gt_masks
                          else os.path.join(a.out, "__no_masks__"))
    os.makedirs(a.out, exist_ok=True)
    clouds, n_points, n_points_full = ([] if a.pointcloud else None), None, None
    voxel_kw = {}
    if a.pointcloud_voxel is not None:
        voxel_kw = dict(voxel_size=a.pointcloud_voxel, reduce=a.pointcloud_reduce, min_count=a.pointcloud_min_count)
    meshes, n_mesh = ([] if a.mesh else None), None              # n_mesh: (vertices, faces) written
    n_matches = None                   # --matches: matches written per consecutive pair
    n_renders = None                   # --render: pictures written
    n_fused = None                     # --fused-mesh: (vertices, faces) written
    n_tracks, n_scene_flow = None, None          # --tracks: tracks written; --scene-flow: valid pixels per consecutive pair
    depths_dev = None                  # --metrics-device: the aligned depth maps as the scene holds them, on the device
    if a.flow_hierarchical and len(imgs) < 3:
        raise RuntimeError("--flow-hierarchical needs at least 3 frames")
    if (a.hierarchical or a.flow_hierarchical) and len(imgs) >= 3:
        extra = {}
        if a.flow_hierarchical:
            extra = dict(flow=dict(shared_focal=not a.not_shared_focal, use_self_mask=not a.gt_masks, flow_net=a.flow_weights),
                         device_resident=a.device_resident)
        res = hz.hierarchical_alignment(imgs, model, a.device, clip_size=a.clip_size, niter=a.niter, schedule=a.schedule, lr=a.lr,
                                        min_conf_thr=a.min_conf_thr, batch_size=a.batch_size, verbose=verbose, output_dir=a.out,
                                        pointcloud_collector=clouds, clean=a.clean, obs_dtype=a.obs_dtype, mesh_collector=meshes,
                                        mesh_double_sided=a.mesh_double_sided, **extra)
        depths = res["depths"]
        if a.pointcloud and voxel_kw:
            n_points, n_points_full = write_voxel_cloud(a.pointcloud, clouds, a.pointcloud_voxel, a.pointcloud_reduce, a.pointcloud_min_count,
                                                        a.device)
        elif a.pointcloud:
            n_points = n_points_full = write_ply_parts(a.pointcloud, [(c["xyz"], c["rgb"]) for c in clouds])
        if a.mesh:
            n_mesh = write_ply_mesh_parts(a.mesh, [(m["xyz"], m["faces"], m["rgb"], m["face_rgb"]) for m in meshes])
    else:
        if len(imgs) == 1:
            imgs = [imgs[0], dict(imgs[0], idx=1)]
        pairs = make_pairs(imgs, scene_graph=a.scene_graph, prefilter=None, symmetrize=True)
        out = inference(pairs, model, a.device, batch_size=a.batch_size, verbose=verbose)
        mode = GlobalAlignerMode.PointCloudOptimizer if len(imgs) > 2 else GlobalAlignerMode.PairViewer
        if a.flow:
            if len(imgs) <= 2:
                raise RuntimeError("--flow needs at least 3 frames (two frames go to the PairViewer, which has no flow term)")
            from ..dust3r.cloud_opt_flow import global_aligner as flow_aligner
            # tool/pose_test.py:170-179 with its argument defaults (translation_weight 1, flow_loss_thre 40 outside temple_3)
            scene = flow_aligner(out, a.device, verbose=verbose, min_conf_thr=a.min_conf_thr, shared_focal=not a.not_shared_focal,
                                 flow_loss_weight=0.01, temporal_smoothing_weight=0.01, translation_weight=1.0, flow_loss_start_epoch=0.1,
                                 flow_loss_thre=40, pxl_thre=50, motion_mask_thre=0.35, use_self_mask=not a.gt_masks,
                                 num_total_iter=a.niter, flow_net=a.flow_weights, obs_dtype=a.obs_dtype)
        else:
            kw = dict(obs_dtype=a.obs_dtype) if mode == GlobalAlignerMode.PointCloudOptimizer else {}    # the PairViewer has no engine
            if verbose and a.obs_dtype != "fp32" and not kw:
                print(f"--obs-dtype {a.obs_dtype} has no effect: two frames go to the PairViewer, which holds no aligner observations")
            scene = global_aligner(out, False, [], a.device, mode=mode, verbose=verbose, min_conf_thr=a.min_conf_thr, **kw)
        if mode == GlobalAlignerMode.PointCloudOptimizer:
            scene.compute_global_alignment(init="mst", niter=a.niter, schedule=a.schedule, lr=a.lr)
            if a.clean:
                scene.clean_pointcloud()
        depths_dev = scene.get_depthmaps()
        depths = [d.detach().cpu().numpy() for d in depths_dev]
        if not (a.metrics_device and mode == GlobalAlignerMode.PointCloudOptimizer):
            depths_dev = None
        hz.save_trajectory_tum_format(hz.get_tum_poses(scene.get_im_poses()), os.path.join(a.out, "pred_traj.txt"))
        hz.save_intrinsics(scene.get_intrinsics(), os.path.join(a.out, "pred_intrinsics.txt"))
        hz.save_frame_arrays(depths, a.out, "frame_{:04d}.npy")
        hz.save_frame_arrays(scene.get_conf(), a.out, "conf_{}.npy")
        if a.flow:
            from ..dust3r.utils.image_pose import enlarge_seg_masks
            scene.save_focals(os.path.join(a.out, "pred_focal.txt"))
            scene.save_dynamic_masks(a.out, 0)
            scene.save_init_conf_maps(a.out, 0)
            enlarge_seg_masks(a.out, kernel_size=5 if a.gt_masks else 3)
        if a.pointcloud:
            if mode != GlobalAlignerMode.PointCloudOptimizer:
                raise RuntimeError("--pointcloud needs at least 3 frames (the two-frame PairViewer has no aligner handle to export from)")
            pc = scene.save_pointcloud(a.pointcloud, **voxel_kw)
            n_points = int(pc["xyz"].shape[0])
            n_points_full = int(scene.get_pointcloud()["xyz"].shape[0]) if voxel_kw else n_points
        if a.matches:
            if mode != GlobalAlignerMode.PointCloudOptimizer:
                raise RuntimeError("--matches needs at least 3 frames (the two-frame PairViewer has no aligner handle to export from)")
            n_matches = write_matches(scene, a.matches, mask_dynamic=a.flow)
        if a.render:
            if mode != GlobalAlignerMode.PointCloudOptimizer:
                raise RuntimeError("--render needs at least 3 frames (the two-frame PairViewer has no aligner handle to export from)")
            n_renders = len(scene.save_renders(a.render, mask_dynamic=a.flow, radius=a.render_radius))
        if a.fused_mesh:
            if mode != GlobalAlignerMode.PointCloudOptimizer:
                raise RuntimeError("--fused-mesh needs at least 3 frames (the two-frame PairViewer has no aligner handle to export from)")
            n_fused = write_fused_mesh(scene, a)
        if a.tracks:                         # both need --flow, and --flow three frames or more: the scene is the flow aligner's
            n_tracks = write_tracks(scene, a.tracks, a.track_start, a.track_stride)
        if a.scene_flow:
            n_scene_flow = write_scene_flow(scene, a.scene_flow)
        if a.mesh:
            if mode != GlobalAlignerMode.PointCloudOptimizer:
                raise RuntimeError("--mesh needs at least 3 frames (the two-frame PairViewer has no aligner handle to export from)")
            m = scene.save_mesh(a.mesh, double_sided=a.mesh_double_sided)
            n_mesh = (int(m["xyz"].shape[0]), int(m["faces"].shape[0]))
    metrics = None
    if a.gt_depth:
        files = sorted(glob.glob(os.path.join(a.gt_depth, "*.npy")))[a.start:a.start + len(depths)]
        gt = np.stack([np.load(f) for f in files])
        if a.metrics_device:
            metrics = evaluate_depth(list(depths_dev) if depths_dev is not None else np.stack(depths), gt, depth_max=a.depth_max, mode="lad",
                                     device=a.device)
        else:
            metrics = evaluate_depth(np.stack(depths), gt, depth_max=a.depth_max, mode="lad")
        if verbose:
            print("depth metrics (LAD scale+shift):", {k: round(v, 5) if isinstance(v, float) else v for k, v in metrics.items()})
    pose = None
    if a.gt_traj:
        from .pose_metrics import eval_metrics, read_pred_traj, read_tum_file
        gt = read_tum_file(a.gt_traj)
        gt = [gt[0][a.start:a.start + len(depths)], gt[1][a.start:a.start + len(depths)]]
        ate, rpe_t, rpe_r = eval_metrics(read_pred_traj(os.path.join(a.out, "pred_traj.txt")), gt, seq=os.path.basename(a.images.rstrip("/")),
                                         filename=os.path.join(a.out, "eval_metric.txt"))
        pose = dict(ate=ate, rpe_trans=rpe_t, rpe_rot=rpe_r)
        if verbose:
            print("pose metrics (Sim(3)-aligned):", {k: round(v, 5) for k, v in pose.items()})
    res_out = dict(n_frames=len(depths), out=a.out, metrics=metrics, pose_metrics=pose)
    if a.pointcloud:
        res_out["pointcloud"], res_out["n_points"], res_out["n_points_full"] = a.pointcloud, n_points, n_points_full
    if a.matches:
        res_out["matches"], res_out["n_matches"] = a.matches, n_matches
    if a.render:
        res_out["render"], res_out["n_renders"] = a.render, n_renders
    if a.fused_mesh:
        res_out["fused_mesh"], res_out["n_fused_vertices"], res_out["n_fused_faces"] = a.fused_mesh, n_fused[0], n_fused[1]
    if a.tracks:
        res_out["tracks"], res_out["n_tracks"] = a.tracks, n_tracks
    if a.scene_flow:
        res_out["scene_flow"], res_out["n_scene_flow_valid"] = a.scene_flow, n_scene_flow
    if a.mesh:
        res_out["mesh"], res_out["n_vertices"], res_out["n_faces"] = a.mesh, n_mesh[0], n_mesh[1]
    return res_out


if __name__ == "__main__":
    main()
