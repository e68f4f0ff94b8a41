#!/usr/bin/env python3
"""TSDF fusion, the library's kernels against a torch route on the same device in one process (developer tool).

Scene: a room, the inside of the box [-2.4, 2.4] x [-2.4, 2.4] x [-1.2, 1.2] with a pillar (a ball of radius 0.5) in it, seen by n
cameras of 384 x 512 pixels (focal 300) that stand on a circle of radius 1 around the pillar and look outwards and slightly
up and down; the depth maps are ray-cast in float64 and stored as fp32, with 0.2 % noise; confidences uniform in [1, 10], a tenth
of the pixels at weight 0; random colours.  Grids: 256^3 voxels of 0.02 for 16 frames, 512 x 512 x 256 voxels of 0.01 for 128
frames, both centred on the room; trunc = 3 voxels.

Per size, in this order:
  1. both routes once; the timing goes on only if tsdf, weight and colours are equal byte for byte.  The torch route is the
     definition of include/a3r.h in float64 torch operations (no fused products), a loop over the frames inside a loop over chunks
     of 2^23 voxels;
  2. ops.tsdf_integrate (its output allocations and the camera upload included), maps already on the device: 3 warm calls, then 9
     calls each between its own pair of device events: the median, with the smallest and the largest as the spread; the same
     without colours and with the brick test switched off (a3r_tsdf_set_form(1)); the share of (brick, frame) pairs the brick test
     skips, from the kernel's own counters;
  3. ops.tsdf_mesh on the fused grid (two calls into the library, each with one wait of the host) the same way;
  4. the torch route (1 warm call, 9 timed), then ops.tsdf_integrate again.

    python tools/bench_tsdf.py [--out profiles/tsdf.json] [--sizes small large]
"""
import argparse, json, math, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
from align3r_amd import ops

H, W, FOCAL = 384, 512, 300.0
ROOM = (2.4, 2.4, 1.2)
PILLAR = 0.5
SIZES = {"small": dict(frames=16, dims=(256, 256, 256), voxel=0.02), "large": dict(frames=128, dims=(512, 512, 256), voxel=0.01)}
CHUNK = 1 << 23


def cameras(n):
    """w2c [n,3,4] and K [n,3,3] float64: on a circle of radius 1 at height 0.3 sin, looking away from the centre."""
    w2c = np.zeros((n, 3, 4))
    for i in range(n):
        a = 2 * math.pi * i / n
        eye = np.array([math.cos(a), math.sin(a), 0.3 * math.sin(3 * a)])
        z = np.array([math.cos(a + 0.4), math.sin(a + 0.4), 0.25 * math.cos(2 * a)])
        z /= np.linalg.norm(z)
        x = np.cross(np.array([0.0, 0.0, 1.0]), z)
        x /= np.linalg.norm(x)
        y = np.cross(z, x)
        R = np.stack([x, y, z])
        w2c[i, :, :3], w2c[i, :, 3] = R, -R @ eye
    K = np.tile(np.array([[FOCAL, 0, (W - 1) / 2], [0, FOCAL, (H - 1) / 2], [0, 0, 1]]), (n, 1, 1))
    return w2c, K


def scene(n, dev):
    """depth, weight [n,P] float32, rgb [n,P,3] uint8 on the device and the camera table."""
    w2c, K = cameras(n)
    g = torch.Generator(device=dev).manual_seed(7)
    col, row = torch.meshgrid(torch.arange(W, device=dev, dtype=torch.float64), torch.arange(H, device=dev, dtype=torch.float64), indexing="xy")
    depth = torch.empty((n, H * W), dtype=torch.float32, device=dev)
    half = torch.tensor(ROOM, dtype=torch.float64, device=dev)
    for i in range(n):
        R = torch.from_numpy(w2c[i, :, :3]).to(dev)
        eye = -(R.T @ torch.from_numpy(w2c[i, :, 3]).to(dev))
        d = torch.stack([(col - K[i, 0, 2]) / FOCAL, (row - K[i, 1, 2]) / FOCAL, torch.ones_like(col)], -1).reshape(-1, 3) @ R
        t_wall = torch.where(d > 0, (half - eye) / d, torch.where(d < 0, (-half - eye) / d, torch.full_like(d, float("inf")))).min(1).values
        a, b, c = (d * d).sum(1), 2 * (d @ eye), eye @ eye - PILLAR * PILLAR
        disc = b * b - 4 * a * c
        t_ball = torch.where(disc > 0, (-b - disc.clamp_min(0).sqrt()) / (2 * a), torch.full_like(a, float("inf")))
        t_ball = torch.where(t_ball > 0, t_ball, torch.full_like(a, float("inf")))
        depth[i] = torch.minimum(t_wall, t_ball).float()
    depth *= 1 + 0.002 * torch.randn(depth.shape, generator=g, device=dev)
    weight = 1 + 9 * torch.rand(depth.shape, generator=g, device=dev)
    weight[torch.rand(depth.shape, generator=g, device=dev) < 0.1] = 0
    rgb = torch.randint(0, 256, (n, H * W, 3), generator=g, device=dev, dtype=torch.uint8)
    return depth, weight, rgb, ops.tsdf_cameras(w2c, K, [(H, W)] * n)


def torch_route(depth, weight, rgb, cams, origin, dims, voxel, trunc, near=1e-6, max_depth=float("inf")):
    """tsdf, wsum [nz,ny,nx] float32 and rgb [nz,ny,nx,3] uint8: the definition in float64 torch operations."""
    dev, (nx, ny, nz) = depth.device, dims
    nvox = nx * ny * nz
    shapes = ops.tsdf_camera_shapes(cams)
    tsdf = torch.empty(nvox, dtype=torch.float32, device=dev)
    wsum = torch.empty(nvox, dtype=torch.float32, device=dev)
    out_rgb = torch.empty((nvox, 3), dtype=torch.uint8, device=dev)
    for l0 in range(0, nvox, CHUNK):
        lin = torch.arange(l0, min(l0 + CHUNK, nvox), device=dev)
        X = origin[0] + ((lin % nx).double() + 0.5) * voxel
        Y = origin[1] + ((torch.div(lin, nx, rounding_mode="floor") % ny).double() + 0.5) * voxel
        Z = origin[2] + (torch.div(lin, nx * ny, rounding_mode="floor").double() + 0.5) * voxel
        Wt, S, Wc = torch.zeros_like(X), torch.zeros_like(X), torch.zeros_like(X)
        Cs = torch.zeros((len(lin), 3), dtype=torch.float64, device=dev)
        for n in range(len(cams)):
            R = [float(e) for e in cams[n, :16]]
            h, w = int(shapes[n, 0]), int(shapes[n, 1])
            xc = (R[0] * X + R[1] * Y) + R[2] * Z + R[3]
            yc = (R[4] * X + R[5] * Y) + R[6] * Z + R[7]
            zc = (R[8] * X + R[9] * Y) + R[10] * Z + R[11]
            u = R[12] * (xc / zc) + R[14]
            v = R[13] * (yc / zc) + R[15]
            col, row = torch.round(u), torch.round(v)
            ok = (zc >= near) & (u.abs() < 2.0 ** 30) & (v.abs() < 2.0 ** 30) & (col >= 0) & (col < w) & (row >= 0) & (row < h)
            p = torch.where(ok, row * w + col, torch.zeros_like(col)).long()
            d, wd = depth[n][p].double(), weight[n][p].double()
            sdf = d - zc
            use = ok & torch.isfinite(d) & torch.isfinite(wd) & (wd > 0) & (d > 0) & (d <= max_depth) & ~(sdf < -trunc)
            t = torch.clamp_max(sdf / trunc, 1.0)
            Wt = torch.where(use, Wt + wd, Wt)
            S = torch.where(use, S + wd * t, S)
            paint = use & (sdf <= trunc)
            Wc = torch.where(paint, Wc + wd, Wc)
            Cs = torch.where(paint[:, None], Cs + wd[:, None] * rgb[n][p].double(), Cs)
        sl = slice(l0, l0 + len(lin))
        tsdf[sl] = torch.where(Wt == 0, torch.ones_like(S), S / Wt).float()
        wsum[sl] = Wt.float()
        out_rgb[sl] = torch.where(Wc[:, None] == 0, torch.zeros_like(Cs), torch.clamp_max(torch.round(Cs / Wc[:, None]), 255.0)).to(torch.uint8)
    return tsdf.view(nz, ny, nx), wsum.view(nz, ny, nx), out_rgb.view(nz, ny, nx, 3)


def device_ms(fn, warm=3, runs=9):
    """(median, smallest, largest) milliseconds of `runs` calls, each between its own pair of device events, after `warm` calls."""
    for _ in range(warm):
        fn()
    times = []
    for _ in range(runs):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        fn()
        t1.record()
        torch.cuda.synchronize()
        times.append(t0.elapsed_time(t1))
    times.sort()
    return dict(median=round(times[len(times) // 2], 4), min=round(times[0], 4), max=round(times[-1], 4))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tsdf.json"))
    ap.add_argument("--sizes", nargs="+", default=["small", "large"], choices=sorted(SIZES))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_tsdf.py measures on the GPU; there is none here")
    dev = torch.device("cuda:0")
    results = []
    for size in a.sizes:
        n, dims, voxel = SIZES[size]["frames"], SIZES[size]["dims"], SIZES[size]["voxel"]
        trunc = 3 * voxel
        origin = tuple(-0.5 * voxel * d for d in dims)
        depth, weight, rgb, cams = scene(n, dev)
        call = lambda colours=rgb, **kw: ops.tsdf_integrate(depth, weight, colours, cams, origin, dims, voxel, trunc, **kw)
        route = lambda: torch_route(depth, weight, rgb, cams, origin, dims, voxel, trunc)
        got, want = call(), route()
        if not all(torch.equal(g.view(torch.int32) if g.dtype == torch.float32 else g, w.view(torch.int32) if w.dtype == torch.float32 else w)
                   for g, w in zip(got, want)):
            sys.exit(f"{size}: the two routes differ; nothing was timed")
        del want
        stats = torch.zeros(2, dtype=torch.int64, device=dev)
        call(skip_stats=stats)
        tested, skipped = (int(v) for v in stats.cpu())
        observed = int((got[1] > 0).sum())
        min_weight = 1.0
        mesh = lambda: ops.tsdf_mesh(got[0], got[1], got[2], origin, voxel, min_weight)
        xyz, _, faces = mesh()
        V, F = int(xyz.shape[0]), int(faces.shape[0])
        del xyz, faces
        k_ms = device_ms(call)
        k_plain_ms = device_ms(lambda: call(colours=None))
        ops.tsdf_set_form(1)
        k_noskip_ms = device_ms(call)
        ops.tsdf_set_form(0)
        m_ms = device_ms(mesh)
        t_ms = device_ms(route, warm=1)
        k_again = device_ms(call)
        pairs = n * dims[0] * dims[1] * dims[2]
        results.append(dict(size=size, frames=n, pixels=[H, W], dims=list(dims), voxel=voxel, trunc=trunc, voxel_frames=pairs,
                            outputs_equal=True, observed_voxels=observed, vertices=V, faces=F,
                            brick_frames=tested, brick_frames_skipped=skipped, skipped_share=round(skipped / tested, 4),
                            integrate_ms=k_ms, integrate_again_ms=k_again, integrate_no_colour_ms=k_plain_ms, integrate_no_brick_test_ms=k_noskip_ms,
                            mesh_ms=m_ms, torch_integrate_ms=t_ms,
                            voxel_frames_per_s=round(pairs / (k_ms["median"] * 1e-3), 1),
                            walked_voxel_frames_per_s=round(pairs * (1 - skipped / tested) / (k_ms["median"] * 1e-3), 1),
                            torch_over_kernel=round(t_ms["median"] / k_ms["median"], 2)))
        print(json.dumps(results[-1]), flush=True)
        del got, depth, weight, rgb
        torch.cuda.empty_cache()
    out = dict(tool="tools/bench_tsdf.py", device=torch.cuda.get_device_name(0),
               scene="a box room of 4.8 x 4.8 x 2.4 with a ball of radius 0.5 in it, n cameras of 384 x 512 (focal 300) on a circle of "
                     "radius 1 looking outwards; ray-cast depths with 0.2 % noise, confidences uniform in [1, 10], a tenth of the pixels "
                     "at weight 0, random colours; trunc = 3 voxels",
               timing="one process, maps on the device; 3 warm calls (torch route: 1), then 9 calls each between its own pair of HIP "
                      "events: median, smallest, largest; ops.tsdf_integrate includes its output allocations and the camera upload, "
                      "ops.tsdf_mesh its two waits of the host; the torch route (float64, a loop over the frames inside a loop over "
                      "chunks of 2^23 voxels) was compared equal byte for byte first; it has no surface extraction",
               results=results)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
