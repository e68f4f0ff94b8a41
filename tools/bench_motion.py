#!/usr/bin/env python3
"""Self-computed motion masks, both paths in one process (developer tool): the per-pair PairViewer loop + torch arithmetic
(A3R_MOTION=torch, cloud_opt_flow.PointCloudOptimizer._motion_masks_torch) against the batched pair geometry + the kernels of
csrc/motion.hip, at N = 16 / E = 84 (swin-3) and N = 128 / E = 1230 (swinstride-5), 384 x 512, consistent synthetic scenes
(bench.synthetic_pair_geometry) whose flow is zero except a moving rectangle.  Predictions and confidences on the host (as inference()
returns them), flow fields on the device (as get_flow returns them).  Warm-up, median of repeats, the pair-geometry and the mask stage
timed separately; the mask kernels are also set against their byte count (20 B read + 4 B written per entry-pixel, 4 B re-read).

    python tools/bench_motion.py [--sizes 16,128] [--repeats 3] [--torch-repeats-large 1] [--out profiles/r06_motion_masks.json]
"""
import argparse, json, os, statistics, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch
from bench import synthetic_pair_geometry
from align3r_amd import ops
from align3r_amd.dust3r.image_pairs import make_pairs
from align3r_amd.dust3r.cloud_opt.pair_viewer import PairViewer, pair_geometry
from align3r_amd.dust3r.cloud_opt_flow.optimizer import motion_entries, motion_masks_torch, motion_vote_lists

H, W = 384, 512
GRAPHS = {16: "swin-3-noncyclic", 128: "swinstride-5-noncyclic"}


def timed(fn, repeats, warmup=1):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return statistics.median(ts), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="16,128")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--torch-repeats-large", type=int, default=1)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "r06_motion_masks.json"))
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    torch.set_num_threads(8)
    P = H * W
    results = []
    for N in [int(s) for s in a.sizes.split(",")]:
        fwd = [(p["idx"], q["idx"]) for p, q in make_pairs([dict(idx=i) for i in range(N)], GRAPHS.get(N, "swin-3-noncyclic"), symmetrize=False)]
        edges = fwd + [(j, i) for i, j in fwd]
        E, M = len(edges), len(fwd)
        p1, p2, c = torch.empty(E, H, W, 3), torch.empty(E, H, W, 3), torch.empty(E, H, W)
        for k, (i, j) in enumerate(edges):
            x, y, cf = synthetic_pair_geometry(i, j, H, W, dev)
            p1[k], p2[k], c[k] = x.cpu(), y.cpu(), cf.cpu()
        fij = torch.zeros(E, 2, H, W, device=dev)
        fij[:, 0, 100:200, 150:300] = 6.0
        fji = fij.clone()
        lists = motion_vote_lists(edges, N)
        big = N > 32
        rep_t = a.torch_repeats_large if big else a.repeats

        def loop_geometry():
            out = [[] for _ in range(8)]
            for e in range(M):
                pair = [e, e + M]
                pv = PairViewer(dict(idx=[0, 1]), dict(idx=[1, 0]), dict(pts3d=p1[pair], conf=c[pair]), dict(pts3d_in_other_view=p2[pair], conf=c[pair]),
                                verbose=False)
                K, poses, depth = pv.get_intrinsics(), pv.get_im_poses(), pv.get_depthmaps()
                for o, v in zip(out, (K[0], K[1], poses[0][:3, :3], poses[1][:3, :3], poses[0][:3, 3:], poses[1][:3, 3:], depth[0], depth[1])):
                    o.append(v)
            return [torch.stack(x).to(dev) for x in out]

        t_loop, g_loop = timed(loop_geometry, rep_t, warmup=0 if big else 1)
        t_torch, (m_torch, _) = timed(lambda: motion_masks_torch(edges, N, *g_loop, fij, fji, 0.35), rep_t)
        up = lambda t: t.to(dev).contiguous()

        def upload():
            return up(p1).reshape(E, P, 3), up(p2).reshape(E, P, 3)

        t_up, (d1, d2) = timed(upload, a.repeats)
        t_geom, geom = timed(lambda: pair_geometry(edges, d1.view(E, H, W, 3), d2.view(E, H, W, 3), c, c, dev), a.repeats)
        entries = motion_entries(geom, edges, E)
        t_kern, m_dev = timed(lambda: ops.motion_masks(d1, d2, fij, fji, entries, lists, 0.35), max(a.repeats, 5))
        m_torch = torch.stack(m_torch)
        nbytes = 2 * M * P * (20 + 4 + 4)
        results.append(dict(N=N, E=E, H=H, W=W, torch_repeats=rep_t, repeats=a.repeats,
                            torch_pair_geometry_s=t_loop, torch_masks_s=t_torch, upload_predictions_s=t_up, batched_pair_geometry_s=t_geom,
                            kernel_masks_s=t_kern, kernel_masks_incl_tables_GBps=nbytes / t_kern / 1e9, algorithmic_bytes=nbytes,
                            masks_differing_pixels=int((m_torch != m_dev).sum().item()), masked_share=float(m_dev.float().mean().item())))
        print(json.dumps(results[-1]), flush=True)
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(dict(tool="tools/bench_motion.py", device=torch.cuda.get_device_name(0), results=results), f, indent=1)
        del p1, p2, c, fij, fji, d1, d2, g_loop


if __name__ == "__main__":
    main()
