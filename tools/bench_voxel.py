#!/usr/bin/env python3
"""Voxel-grid downsampling, the library's kernels against a torch route on the same device in one process (developer tool).

Clouds: every pixel of 16 and of 128 frames of 384 x 512 -- 3 145 728 and 25 165 824 points, N noisy views of one surface (the cloud of
tools/bench_render.py), confidences in [1, 10] as priorities, random colours.  The voxel edge is found by bisection on the kernel's
own V so that V is about M / N: one point per voxel and view.

Per cloud and reduce mode, in this order:
  1. both routes once; the timing goes on only if index and count are equal element for element (and, for the record, whether the
     coordinates and colours are equal bit for bit too).  The torch route builds the same float64 keys, then torch.unique(
     return_inverse=True, return_counts=True), scatter_reduce_(0, inverse, value, 'amin') on int64 values, a sort of the winners
     and the gathers ('best') or index_add_ sums ('mean').  The priorities are positive, so the value's high word stays below 2^31
     and the int64 order is the unsigned one;
  2. ops.voxel_downsample (its allocations, the fill, insert, flag, scan and placement passes, the host's wait for V and the copies
     to V rows included): 3 warm calls, then 9 calls each between its own pair of device events: the median, with the smallest and
     the largest as the spread;
  3. the torch route the same way.

    python tools/bench_voxel.py [--out profiles/voxel.json] [--frames 16 128]
"""
import argparse, json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
from align3r_amd import ops
from bench_render import arc_poses, cloud

R, FIX = 1 << 20, float(1 << 24)


def torch_route(xyz, voxel, priority, rgb, reduce):
    """dict(xyz, rgb, index, count) on xyz's device: the definition of include/a3r.h in torch operations (positive priorities)."""
    r = xyz.double() / voxel
    q = torch.floor(r)
    inside = (torch.isfinite(xyz) & (q >= -R) & (q < R)).all(1)
    rows = torch.nonzero(inside)[:, 0]
    qi = (q[rows] + R).long()
    key = (qi[:, 0] << 42) | (qi[:, 1] << 21) | qi[:, 2]
    uniq, inv, counts = torch.unique(key, return_inverse=True, return_counts=True)
    b = priority.view(torch.int32).long() & 0xFFFFFFFF
    w = ~(b ^ 0x80000000) & 0xFFFFFFFF                       # sign bit clear: below 2^31
    value = (w[rows] << 32) | rows
    best = torch.full((uniq.shape[0],), torch.iinfo(torch.int64).max, dtype=torch.int64, device=xyz.device)
    best.scatter_reduce_(0, inv, value, "amin")
    index, order = torch.sort(best & 0xFFFFFFFF)
    n = counts[order]
    if reduce == "best":
        out_xyz, out_rgb = xyz[index], rgb[index]
    else:
        t = torch.floor((r[rows] - q[rows]) * FIX).long()
        S = torch.zeros((uniq.shape[0], 3), dtype=torch.int64, device=xyz.device).index_add_(0, inv, t)
        Cs = torch.zeros((uniq.shape[0], 3), dtype=torch.int64, device=xyz.device).index_add_(0, inv, rgb[rows].long())
        nd = n.double()[:, None]
        out_xyz = ((q[index] + (S[order].double() + 0.5 * nd) / (nd * FIX)) * voxel).float()
        out_rgb = ((2 * Cs[order] + n[:, None]) // (2 * n[:, None])).to(torch.uint8)
    return dict(xyz=out_xyz, rgb=out_rgb, index=index.int(), count=n.int())


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
    return times[len(times) // 2], times[0], times[-1]


def find_voxel(xyz, target, lo=1e-3, hi=1e-1, steps=12):
    """The voxel edge whose V is nearest to `target`, by bisection on log(voxel) (V falls as the edge grows)."""
    best = None
    for _ in range(steps):
        mid = (lo * hi) ** 0.5
        V = ops.voxel_downsample(xyz, mid)["index"].shape[0]
        if best is None or abs(V - target) < abs(best[1] - target):
            best = (mid, V)
        if V > target:
            lo = mid
        else:
            hi = mid
    return best


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "voxel.json"))
    ap.add_argument("--frames", type=int, nargs="+", default=[16, 128])
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_voxel.py measures on the GPU; there is none here")
    dev = torch.device("cuda:0")
    results = []
    for n_frames in a.frames:
        xyz, rgb = cloud(arc_poses(n_frames), dev)
        M = int(xyz.shape[0])
        g = torch.Generator(device=dev).manual_seed(1)
        priority = 1 + 9 * torch.rand(M, generator=g, device=dev, dtype=torch.float32)
        voxel, _ = find_voxel(xyz, M // n_frames)
        for reduce in ("best", "mean"):
            call = lambda: ops.voxel_downsample(xyz, voxel, priority=priority, rgb=rgb, reduce=reduce)
            route = lambda: torch_route(xyz, voxel, priority, rgb, reduce)
            got, want = call(), route()
            if not (torch.equal(got["index"], want["index"]) and torch.equal(got["count"], want["count"])):
                sys.exit(f"{n_frames} frames, {reduce}: the two routes differ in index / count; nothing was timed")
            same_bits = bool(torch.equal(got["xyz"].view(torch.int32), want["xyz"].view(torch.int32)) and torch.equal(got["rgb"], want["rgb"]))
            V, top, dropped = int(got["index"].shape[0]), int(got["count"].max()), got["dropped"]
            del got, want
            k_ms, t_ms = device_ms(call), device_ms(route)
            k_again = device_ms(call)
            results.append(dict(frames=n_frames, points=M, voxel=voxel, reduce=reduce, V=V, M_over_V=round(M / V, 2), largest_count=top,
                                dropped=dropped, index_and_count_equal=True, xyz_and_rgb_bits_equal=same_bits,
                                slots=ops.voxel_default_slots(M),
                                kernel_ms=dict(median=round(k_ms[0], 4), min=round(k_ms[1], 4), max=round(k_ms[2], 4)),
                                kernel_again_ms=dict(median=round(k_again[0], 4), min=round(k_again[1], 4), max=round(k_again[2], 4)),
                                torch_ms=dict(median=round(t_ms[0], 4), min=round(t_ms[1], 4), max=round(t_ms[2], 4)),
                                points_per_s=round(M / (k_ms[0] * 1e-3), 1), torch_over_kernel=round(t_ms[0] / k_ms[0], 2)))
            print(json.dumps(results[-1]), flush=True)
        del xyz, rgb, priority
    out = dict(tool="tools/bench_voxel.py", device=torch.cuda.get_device_name(0),
               cloud="every pixel of n frames of 384 x 512 on an arc around a noisy height field (tools/bench_render.py: cloud); priorities "
                     "uniform in [1, 10]; the voxel edge bisected so that V is about M / n",
               timing="one process; 3 warm calls, then 9 calls each between its own pair of HIP events: median, smallest, largest; "
                      "ops.voxel_downsample includes its allocations, the host's wait for V and the copies to V rows; the kernel route "
                      "is timed before and again after the torch route",
               results=results)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
