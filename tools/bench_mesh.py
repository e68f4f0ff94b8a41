#!/usr/bin/env python3
"""Scene mesh at BASELINE config-2 and config-4 size (N = 16 / 128 frames of 384x512), one process (developer tool).

  (a) the device route: AlignEngine.export_mesh = a3r_align_scene_mesh_count + a3r_align_scene_mesh_export (csrc/scene.hip), with
      vertex and face colours, single- and double-sided;
  (b) the host route doing the same job the way the reference does it: get_pts3d() and the masks downloaded to numpy, the faces
      built there (align3r_amd.tool.pointcloud.mesh_faces_host), vertices and colours gathered by boolean indexing.

Both start from the same device-resident confidences, with a threshold that keeps about 70 % of the pixels.  (a): HIP events
around each call on the current stream, WARM warm-up calls, median / minimum / maximum of REPS.  (b): wall clock around the call
(it ends on the host), median / minimum / maximum of HOST_REPS after one warm-up call.  Traffic the passes of (a) must move: conf
and depth read by the count and by the placement pass (8 B per pixel each), the rank map written once and read twice (12 B per
pixel), 12 + 3 B written per vertex and per face.  Writes one JSON file (default profiles/scene_mesh.json) and prints it.
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from bench_scene import build

REPS, WARM, HOST_REPS = 9, 3, 3


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
    return dict(median_ms=round(float(np.median(ms)), 4), min_ms=round(min(ms), 4), max_ms=round(max(ms), 4))


def timed_host(fn):
    fn()
    ms = []
    for _ in range(HOST_REPS):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        ms.append(1e3 * (time.perf_counter() - t0))
        del out
    return dict(median_ms=round(float(np.median(ms)), 2), min_ms=round(min(ms), 2), max_ms=round(max(ms), 2))


def run(N, H, W, dev):
    from align3r_amd.tool.pointcloud import mesh_faces_host
    scene = build(N, H, W, dev)
    eng, P = scene.engine, H * W
    conf = torch.stack([c.reshape(-1) for c in scene.im_conf]).to(dev).contiguous()
    thr = float(torch.quantile(conf.flatten()[::16][:8_000_000], 0.3))      # every 16th confidence: quantile() takes 16 M at most
    rgb = torch.randint(0, 256, (N, P, 3), dtype=torch.uint8, device=dev)

    def host_route(double_sided):
        pts = [p.detach().cpu().numpy() for p in scene.get_pts3d()]
        valid = [(c > thr).cpu().numpy().reshape(H, W) for c in conf]
        cols = rgb.cpu().numpy()
        faces, colour = mesh_faces_host(valid, double_sided=double_sided)
        keep = np.concatenate([v.ravel() for v in valid])
        xyz = np.concatenate([p.reshape(-1, 3) for p in pts])[keep]
        vrgb = cols.reshape(-1, 3)[keep]
        return xyz, faces, vrgb, vrgb[colour]

    out = dict(N=N, P=P)
    for ds in (False, True):
        got = eng.export_mesh(conf, thr, rgb=rgb, double_sided=ds)
        V, F = int(got["xyz"].shape[0]), int(got["faces"].shape[0])
        ref = host_route(ds)
        assert np.array_equal(got["faces"].cpu().numpy(), ref[1]) and np.array_equal(got["face_rgb"].cpu().numpy(), ref[3])
        assert np.array_equal(got["rgb"].cpu().numpy(), ref[2]) and got["xyz"].shape == ref[0].shape
        del got, ref
        dev_t = timed(lambda: eng.export_mesh(conf, thr, rgb=rgb, double_sided=ds))
        host_t = timed_host(lambda: host_route(ds))
        must = N * P * (2 * 8 + 12) + V * 15 + F * 15
        out["double_sided" if ds else "single_sided"] = dict(
            vertices=V, faces=F, kept_fraction=round(V / (N * P), 4), device=dev_t, host=host_t, must_move_bytes=must,
            device_GBps=round(must / dev_t["median_ms"] / 1e6, 1), host_over_device=round(host_t["median_ms"] / dev_t["median_ms"], 1))
    del scene, eng
    torch.cuda.empty_cache()
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "scene_mesh.json"))
    ap.add_argument("--sizes", default="16,128")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    res = dict(device=torch.cuda.get_device_name(0), reps=REPS, warm=WARM, host_reps=HOST_REPS,
               timing="device: HIP events per export_mesh call (count + export); host: wall clock per call",
               cases=[run(int(n), 384, 512, "cuda") for n in a.sizes.split(",")])
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res), flush=True)
