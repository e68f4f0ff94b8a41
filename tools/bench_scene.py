#!/usr/bin/env python3
"""Scene export at BASELINE config-2 and config-4 size (N = 16 / 128 frames of 384x512), one process (developer tool).

  (a) the native path: AlignEngine.export_points = a3r_align_scene_count + a3r_align_scene_export (csrc/scene.hip), xyz only and
      xyz + rgb + index;
  (b) the torch path doing the same job: get_pts3d(raw=True), a boolean mask per image, torch.cat.

Both read the same device-resident confidences with a threshold that keeps about half of the pixels.  HIP events around each
repetition on the current stream, warm, median of REPS.  Minimum traffic of (a): both passes read conf and depth (8 B per pixel
each), the export writes 12 (+ 3 + 4) B per kept point.  Writes one JSON file (default profiles/scene_export.json) and prints it.
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

REPS, WARM = 9, 3


def timed(fn):
    for _ in range(WARM):
        fn()
    ms = []
    for _ in range(REPS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = fn()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
        del out
    return float(np.median(ms)), float(min(ms))


def build(N, H, W, dev):
    from align3r_amd.dust3r.cloud_opt.optimizer import PointCloudOptimizer
    edges = [(i, i + 1) for i in range(N - 1)]                 # a chain: the export does not look at the graph
    E = len(edges)
    g = torch.Generator(device=dev).manual_seed(2)
    rnd = lambda *s: torch.randn(*s, generator=g, device=dev)
    cnf = lambda: 1 + 9 * torch.rand(E, H, W, generator=g, device=dev)
    view1, view2 = dict(idx=[i for i, j in edges]), dict(idx=[j for i, j in edges])
    scene = PointCloudOptimizer(view1, view2, dict(pts3d=rnd(E, H, W, 3), conf=cnf()), dict(pts3d_in_other_view=rnd(E, H, W, 3), conf=cnf()),
                                False, [], verbose=False).to(dev)
    im = 0.05 * rnd(N, 7)
    im[:, 3] += 1
    scene.engine.set_params(depth=0.1 * rnd(N, H * W), im_poses=im)
    return scene


def run(N, H, W, dev):
    scene = build(N, H, W, dev)
    eng, P = scene.engine, H * W
    conf = torch.stack([c.reshape(-1) for c in scene.im_conf]).to(dev).contiguous()
    thr = float(conf.median())
    rgb = torch.randint(0, 256, (N, P, 3), dtype=torch.uint8, device=dev)

    def torch_path():
        pts = scene.get_pts3d(raw=True)
        return torch.cat([pts[n][conf[n] > thr] for n in range(N)])

    ref = torch_path()
    got = eng.export_points(conf, thr)["xyz"]
    M = int(got.shape[0])
    assert got.shape == ref.shape, (got.shape, ref.shape)
    err = float((got - ref).abs().max() / ref.abs().max())
    a_ms, a_min = timed(lambda: eng.export_points(conf, thr))
    af_ms, af_min = timed(lambda: eng.export_points(conf, thr, rgb=rgb, with_index=True))
    b_ms, b_min = timed(torch_path)
    min_bytes = 2 * N * P * 8 + M * 12
    min_bytes_full = 2 * N * P * 8 + M * 19
    del scene, eng
    torch.cuda.empty_cache()
    return dict(N=N, P=P, kept=M, kept_fraction=round(M / (N * P), 4), native_vs_torch_max_err_over_max=err,
                native_xyz_ms=round(a_ms, 4), native_xyz_min_ms=round(a_min, 4), native_xyz_rgb_index_ms=round(af_ms, 4),
                native_xyz_rgb_index_min_ms=round(af_min, 4), torch_ms=round(b_ms, 4), torch_min_ms=round(b_min, 4),
                min_bytes_xyz=min_bytes, native_xyz_GBps=round(min_bytes / a_ms / 1e6, 1),
                native_xyz_rgb_index_GBps=round(min_bytes_full / af_ms / 1e6, 1), speedup_vs_torch=round(b_ms / a_ms, 2))


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "scene_export.json"))
    ap.add_argument("--sizes", default="16,128")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    res = dict(device=torch.cuda.get_device_name(0), reps=REPS, warm=WARM, timing="HIP events, median (and minimum) per call",
               cases=[run(int(n), 384, 512, "cuda") for n in a.sizes.split(",")])
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res), flush=True)
