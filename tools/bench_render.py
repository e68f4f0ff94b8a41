#!/usr/bin/env python3
"""Rendering a point cloud, the library's kernels against a torch route on the same device in one process (developer tool).

Clouds: every pixel of 16 and of 128 frames of 384 x 512 -- 3 145 728 and 25 165 824 points: per frame a noisy height field (the
surface of tests/match_cases.py) seen through that frame's pinhole, taken to the world by the frame's pose; the frames stand on an
arc looking at the field.  Cameras: the first 16 or all 128 frame cameras of the 128-frame arc, pictures of 384 x 512.  Radius 0 and 1.

Per (cloud, cameras, radius), in this order:
  1. both routes once; the timing goes on only if depth bits and winner indices are equal element for element.  The torch route is
     the definition of include/a3r.h in torch operations, camera by camera (an [C, M] intermediate does not fit at these sizes):
     float64 projection, torch.round (half to even), int64 keys, one scatter_reduce_(0, ..., 'amin') per footprint offset, the resolve;
  2. ops.render_points (output and workspace allocation, the camera table's upload, fill, splat and resolve included) in the six
     forms of a3r_render_set_form, forms 0 and 4 once more at the end (the spread): device events around `reps` calls after a
     warm-up, `reps` doubled until the window is at least a second; a call that takes more than two seconds is timed once;
  3. the torch route the same way.

    python tools/bench_render.py [--out profiles/render.json] [--frames 16 128] [--cams 16 128] [--radii 0 1]
"""
import argparse, json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np, torch
from align3r_amd import ops
from align3r_amd.tool.render import world_to_camera

H, W, FOCAL, NEAR = 384, 512, 400.0, 1e-6
FORMS = {0: "camera loop, keys read before the atomics, nine pixels of a footprint at a time", 1: "camera axis, reads as form 0",
         2: "camera loop, every atomic", 3: "camera axis, every atomic", 4: "camera loop, keys read one pixel at a time",
         5: "camera axis, reads as form 4"}


def arc_poses(n):
    """cam2world [n,4,4] float64: n cameras on an arc of +-0.4 rad around the point (0, 0, 2), looking at it."""
    a = np.linspace(-0.4, 0.4, n)
    poses = np.zeros((n, 4, 4))
    for k, t in enumerate(a):
        c, s = np.cos(t), np.sin(t)
        R = np.array([[c, 0, -s], [0, 1, 0], [s, 0, c]])                    # camera axes as columns: z looks at the centre
        poses[k, :3, :3] = R
        poses[k, :3, 3] = np.array([0, 0, 2.0]) - R @ np.array([0, 0, 2.0])
        poses[k, 3, 3] = 1
    return poses


def cloud(poses, device, seed=0):
    """[n * H * W, 3] float32 world points and [n * H * W, 3] uint8 colours: per frame z = 2 + 0.3 sin(3 a) cos(2 b) + 0.002 noise over
    the frame's own pixel rays (a, b) = ((x - W / 2) / FOCAL, (y - H / 2) / FOCAL), float64 on the device, rounded to float32 once."""
    g = torch.Generator(device=device).manual_seed(seed)
    ys, xs = torch.meshgrid(torch.arange(H, device=device, dtype=torch.float64), torch.arange(W, device=device, dtype=torch.float64), indexing="ij")
    a, b = ((xs - W / 2) / FOCAL).reshape(-1), ((ys - H / 2) / FOCAL).reshape(-1)
    out = []
    for P in poses:
        z = 2 + 0.3 * torch.sin(3 * a) * torch.cos(2 * b) + 0.002 * torch.randn(a.shape, generator=g, device=device, dtype=torch.float64)
        cam = torch.stack([a * z, b * z, z], 1)
        Pt = torch.from_numpy(P).to(device)
        out.append((cam @ Pt[:3, :3].T + Pt[:3, 3]).float())
    xyz = torch.cat(out).contiguous()
    rgb = torch.randint(0, 256, (xyz.shape[0], 3), generator=g, device=device, dtype=torch.uint8)
    return xyz, rgb


def torch_route(xyz, cams, H, W, radius, near):
    """(depth [C,H,W] float32, index [C,H,W] int32) on xyz's device: the definition in torch operations, one camera at a time."""
    x, y, z = (xyz[:, k].double() for k in range(3))
    m = torch.arange(xyz.shape[0], device=xyz.device, dtype=torch.int64)
    empty = torch.iinfo(torch.int64).max
    depth, index = [], []
    for cam in cams:
        R = [float(v) for v in cam]
        xc = (R[0] * x + R[1] * y) + R[2] * z + R[3]
        yc = (R[4] * x + R[5] * y) + R[6] * z + R[7]
        zc = (R[8] * x + R[9] * y) + R[10] * z + R[11]
        u = R[12] * (xc / zc) + R[14]
        v = R[13] * (yc / zc) + R[15]
        zf = zc.float()
        ok = (zc >= near) & torch.isfinite(zf) & (u.abs() < 2.0 ** 30) & (v.abs() < 2.0 ** 30)          # a NaN fails every compare
        col, row = torch.round(u[ok]).long(), torch.round(v[ok]).long()
        key = (zf[ok].view(torch.int32).long() << 32) | m[ok]
        keys = torch.full((H * W,), empty, dtype=torch.int64, device=xyz.device)
        for dy in range(-radius, radius + 1):
            for dx in range(-radius, radius + 1):
                r, q = row + dy, col + dx
                inside = (r >= 0) & (r < H) & (q >= 0) & (q < W)
                keys.scatter_reduce_(0, (r * W + q)[inside], key[inside], "amin")
        hit = keys != empty
        depth.append(torch.where(hit, (keys >> 32).int().view(torch.float32), torch.zeros((), device=xyz.device)))
        index.append(torch.where(hit, keys & 0xFFFFFFFF, torch.full((), -1, dtype=torch.int64, device=xyz.device)).int())
    return torch.stack(depth).view(-1, H, W), torch.stack(index).view(-1, H, W)


def device_ms(fn, min_window_s=1.0, slow_s=2.0):
    """(milliseconds per call, reps): the first call is the warm-up, timed as well -- above slow_s it is the measurement (reps = 1
    and the warm-up's costs inside); otherwise device events around `reps` calls, doubled until the window reaches min_window_s."""
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    fn()
    t1.record()
    torch.cuda.synchronize()
    if t0.elapsed_time(t1) >= 1e3 * slow_s:
        return t0.elapsed_time(t1), 1
    reps = 1
    while True:
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(reps):
            fn()
        t1.record()
        torch.cuda.synchronize()
        ms = t0.elapsed_time(t1)
        if ms >= 1e3 * min_window_s:
            return ms / reps, reps
        reps *= 2


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "render.json"))
    ap.add_argument("--frames", type=int, nargs="+", default=[16, 128])
    ap.add_argument("--cams", type=int, nargs="+", default=[16, 128])
    ap.add_argument("--radii", type=int, nargs="+", default=[0, 1])
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_render.py measures on the GPU; there is none here")
    dev = torch.device("cuda:0")
    view_poses = arc_poses(128)
    K = np.array([[FOCAL, 0, W / 2], [0, FOCAL, H / 2], [0, 0, 1]])
    results = []
    old_form = ops.render_set_form(0)
    try:
        for n_frames in a.frames:
            xyz, rgb = cloud(arc_poses(n_frames), dev)
            for n_cams in a.cams:
                cams = ops.render_cameras(world_to_camera(view_poses[:n_cams]), np.broadcast_to(K, (n_cams, 3, 3)).copy())
                for radius in a.radii:
                    call = lambda: ops.render_points(xyz, rgb, cams=cams, shape=(H, W), radius=radius, near=NEAR, want_index=True)
                    ops.render_set_form(0)
                    got = call()
                    t_depth, t_index = torch_route(xyz, cams, H, W, radius, NEAR)
                    equal = bool(torch.equal(got["depth"].view(torch.int32), t_depth.view(torch.int32)) and torch.equal(got["index"], t_index))
                    if not equal:
                        sys.exit(f"{n_frames} frames, {n_cams} cameras, radius {radius}: the two routes differ; nothing was timed")
                    covered = float((t_index >= 0).float().mean())
                    del got, t_depth, t_index
                    forms = {}
                    for tag, form in (("0", 0), ("1", 1), ("2", 2), ("3", 3), ("4", 4), ("5", 5), ("0_again", 0), ("4_again", 4)):
                        ops.render_set_form(form)
                        ms, reps = device_ms(call)
                        forms[tag] = dict(ms=round(ms, 4), reps=reps)
                    ops.render_set_form(0)
                    t_ms, t_reps = device_ms(lambda: torch_route(xyz, cams, H, W, radius, NEAR))
                    M = int(xyz.shape[0])
                    results.append(dict(frames=n_frames, points=M, cameras=n_cams, H=H, W=W, radius=radius, equal=True,
                                        pixels_covered=round(covered, 4), render_points_ms_by_form=forms,
                                        projections_per_s_form0=round(M * n_cams / (forms["0"]["ms"] * 1e-3), 1),
                                        torch_ms=round(t_ms, 4), torch_reps=t_reps, torch_over_form0=round(t_ms / forms["0"]["ms"], 2)))
                    print(json.dumps(results[-1]), flush=True)
            del xyz, rgb
    finally:
        ops.render_set_form(old_form)
    out = dict(tool="tools/bench_render.py", device=torch.cuda.get_device_name(0), forms=FORMS,
               cloud="every pixel of n frames of 384 x 512 on an arc around a noisy height field; cameras: the first n of the 128-frame arc",
               timing="HIP events around reps calls after a warm-up, window >= 1 s (a call above 2 s: timed once, warm-up inside); one "
                      "process; ops.render_points includes its allocations and the camera upload; the torch route works camera by camera",
               results=results)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
