#!/usr/bin/env python3
"""clean_pointcloud: the device path (csrc/scene.hip, a3r_align_scene_clean) against the torch function (A3R_CLEAN=torch) in one
process, on synthetic but geometrically consistent scenes: N views of 384x512 on an arc of 0.6 rad look at a wavy surface at depth
3 +- 0.5, 15 % of the pixels float 1.5 in front of it, confidences uniform in [1, 6]; neighbouring views overlap almost fully,
the ends of the arc by about half.

Reported per size: wall time of scene.clean_pointcloud() on either path (host clock around a device synchronise; warm-up runs
first, then every repetition and the median), the time of the engine call alone by device events (1 + N kernels), the share of
changed pixels, how many pixels the two paths decide differently, and the kernel's gather rate: the (pixel, view) pairs whose
depth and confidence the kernel fetched (visible, up to and including the first hit; counted by a torch restatement from the
finished confidences) over the engine time.

    python tools/bench_clean.py [--sizes 16,128] [--out profiles/r05_scene_clean.json] [--torch-reps 2]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

H, W = 384, 512


def make_scene(N, dev, seed=0):
    """(PointCloudOptimizer with the synthetic state, conf [N,H,W] on the device)"""
    from align3r_amd.dust3r.cloud_opt.optimizer import PointCloudOptimizer
    g = torch.Generator(device="cpu").manual_seed(seed)
    edges = [(i, i + 1) for i in range(N - 1)] + [(i + 1, i) for i in range(N - 1)]
    E = len(edges)
    z3 = torch.zeros(E, H, W, 3, device=dev)
    one = torch.ones(E, H, W, device=dev)
    view1, view2 = dict(idx=[i for i, j in edges]), dict(idx=[j for i, j in edges])
    torch.manual_seed(seed)
    scene = PointCloudOptimizer(view1, view2, dict(pts3d=z3, conf=one), dict(pts3d_in_other_view=z3, conf=one), False, [], verbose=False).to(dev)
    s = np.linspace(-0.5, 0.5, N)
    a, tx = 0.6 * s, 1.6 * s
    poses = np.zeros((N, 7), np.float32)
    poses[:, 1], poses[:, 3] = np.sin(a / 2), np.cos(a / 2)
    poses[:, 4] = np.sign(tx) * np.log1p(np.abs(tx))
    xs = torch.arange(W, dtype=torch.float64)[None, None, :] * (16.0 / W)
    n = torch.arange(N, dtype=torch.float64)[:, None, None]
    d = 3 + 0.5 * torch.sin(xs / 3.0 + 0.3 * n) + torch.zeros(1, H, 1, dtype=torch.float64)
    d = d - 1.5 * (torch.rand(N, H, W, generator=g) < 0.15)
    conf = (1 + 5 * torch.rand(N, H, W, generator=g)).float().to(dev)
    scene.engine.set_params(depth=d.log().float().reshape(N, -1), im_poses=poses,
                            im_focals=np.full(N, 20 * np.log(1.25 * W), np.float32), im_pp=np.zeros((N, 2), np.float32))
    return scene, conf


def gathers(scene, conf_in, conf_out, tol=0.001, bad_conf=0.0):
    """(pixel, view) pairs the kernel fetches: image i walks j = 0.. in order over its live pixels, a pair is fetched when the
    projection is visible, and a pixel stops at its first hit.  fp32 restatement on the device, one image at a time."""
    N, P = conf_in.shape[0], H * W
    pts = scene.get_pts3d(raw=True)                                     # [N,P,3]
    RT, f, pp = scene.get_im_poses(), scene.get_focals().reshape(-1), scene.get_principal_points()
    depth = scene.get_depthmaps(raw=True)
    cin, cout = conf_in.reshape(N, P), conf_out.reshape(N, P)
    total = 0
    for i in range(N):
        js = torch.tensor([j for j in range(N) if j != i], device=pts.device)
        cam = torch.einsum("jkc,pk->jpc", RT[js, :3, :3], pts[i]) - torch.einsum("jkc,jk->jc", RT[js, :3, :3], RT[js, :3, 3])[:, None]
        z = cam[..., 2]
        u = (f[js, None] * cam[..., 0] / z + pp[js, None, 0]).round()
        v = (f[js, None] * cam[..., 1] / z + pp[js, None, 1]).round()
        vis = (z > 0) & (u >= 0) & (u < W) & (v >= 0) & (v < H) & (cin[i] > bad_conf)[None]
        q = torch.where(vis, v * W + u, torch.zeros_like(u)).long()
        src = torch.where((js < i)[:, None], cout[js], cin[js])
        hit = vis & (z < (1 - tol) * torch.gather(depth[js], 1, q)) & (cin[i][None] < torch.gather(src, 1, q))
        before_first = hit.long().cumsum(0) - hit.long() == 0            # no hit strictly before this view
        total += int((vis & before_first).sum())
    return total


def timed(fn, warm, reps):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3)
    return out


def bench(N, dev, torch_reps):
    scene, conf = make_scene(N, dev)
    eng = scene.engine
    maps = lambda: [conf[n].clone() for n in range(N)]

    def method(path):
        if path == "torch":
            os.environ["A3R_CLEAN"] = "torch"
        else:
            os.environ.pop("A3R_CLEAN", None)
        scene.im_conf = maps()
        scene.clean_pointcloud()
        last[path] = scene.im_conf

    last = {}
    dev_ms = timed(lambda: method("device"), 2, 10)
    print(f"N={N}: device path timed", file=sys.stderr, flush=True)
    torch_ms = timed(lambda: method("torch"), 1, torch_reps)
    print(f"N={N}: torch path timed", file=sys.stderr, flush=True)
    out_dev, out_torch = torch.stack(last["device"]), torch.stack(last["torch"])
    os.environ.pop("A3R_CLEAN", None)
    stacked = conf.reshape(N, -1)
    ev = []
    for k in range(12):                                                  # the engine call alone (clone + 1 + N kernels), device events
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        eng.clean_confidences(stacked)
        b.record()
        torch.cuda.synchronize()
        if k >= 2:
            ev.append(a.elapsed_time(b))
    n_gather = gathers(scene, conf, out_dev)
    px = N * H * W
    med = lambda v: float(np.median(v))
    return dict(N=N, H=H, W=W, pair_passes=N * (N - 1),
                device_method_ms=dict(warmup=2, reps=dev_ms, median=med(dev_ms)),
                torch_method_ms=dict(warmup=1, reps=torch_ms, median=med(torch_ms)),
                device_engine_call_ms=dict(warmup=2, reps=ev, median=med(ev)),
                speedup_method=med(torch_ms) / med(dev_ms),
                changed_share=float((out_dev != conf).sum()) / px,
                device_vs_torch_differing_pixels=int((out_dev != out_torch).sum()),
                projections=px * (N - 1), gathers=n_gather,
                gather_rate_per_s=n_gather / (med(ev) * 1e-3), gather_bytes_per_s=8 * n_gather / (med(ev) * 1e-3))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--sizes", default="16,128")
    ap.add_argument("--out", default=os.path.join("profiles", "r05_scene_clean.json"))
    ap.add_argument("--torch-reps", type=int, default=2)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_clean.py measures on a GPU; none is visible")
    res = dict(device=torch.cuda.get_device_name(0), cases=[])
    for N in [int(s) for s in a.sizes.split(",")]:
        r = bench(N, "cuda:0", a.torch_reps)
        print(json.dumps(r), flush=True)
        res["cases"].append(r)
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:                                     # after every size: a later size that fails loses nothing
            json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
