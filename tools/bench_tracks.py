#!/usr/bin/env python3
"""Following points through a clip, the library's kernel against a torch route on the same device in one process (developer tool).

Workloads, frames of 384 x 512:
  tracks      every pixel of frame 0 followed through 15 steps over the path 0 .. 15 of a 16-frame clip (one chain, 196 608 tracks);
  scene_flow  the all-edges scene flow of a 16-frame swinstride-5-noncyclic graph, symmetrised (110 edges: 110 chains of one step,
              every pixel each).
Flow fields: the smooth kind of tests/track_cases.py -- low-frequency sinusoids of 3 px amplitude plus 1.5 px in x, the backward
field minus that plus a disagreement of up to 4 px -- so that tracks end by both causes and a share survives.  Points: noise;
keep: 80 % of the pixels.

Per workload, in this order:
  1. both routes once; the timing goes on only if state, pix and the bits of xy and xyz are equal element for element.  The torch
     route is the definition of include/a3r.h in torch operations, chain by chain: float64 gathers of the four corners, the same
     formulas one operation at a time, torch.round (half to even), masked writes;
  2. ops.track_points (output allocation and the step table's upload included): device events around `reps` calls after a
     warm-up, `reps` doubled until the window is at least a second; then once more at the end (the spread);
  3. the torch route the same way.

    python tools/bench_tracks.py [--out profiles/tracks.json]
"""
import argparse, json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np, torch
from align3r_amd import ops
from align3r_amd.dust3r.image_pairs import make_pairs
from align3r_amd.tool.tracks import plan_steps

H, W, N, FB_THR = 384, 512, 16, 3.0


def smooth_fields(edges, device):
    """(flow_ij, flow_ji) [E,2,H,W] float32 on the device; edge e = (i, j) carries a field scaled by j - i (a longer stride moves further)."""
    ys, xs = torch.meshgrid(torch.arange(H, device=device, dtype=torch.float64), torch.arange(W, device=device, dtype=torch.float64), indexing="ij")
    u, v = xs / W, ys / H
    fij, fji = [], []
    for e, (i, j) in enumerate(edges):
        k, d = 0.37 * e, float(j - i)
        fx = d * (1.5 + 3 * torch.sin(2 * np.pi * (u + 0.5 * v) + k))
        fy = d * 3 * torch.cos(2 * np.pi * (v + 0.25 * u) + 0.7 * k)
        wave = 4 * torch.sin(2 * np.pi * (1.5 * u + 0.5 * v) + 0.2 * k) * torch.sin(2 * np.pi * (v + 0.25 * u) + 0.5 + 0.2 * k)
        fij.append(torch.stack([fx, fy]))
        fji.append(torch.stack([-fx + wave, -fy + 0.5 * wave]))
    return torch.stack(fij).float().contiguous(), torch.stack(fji).float().contiguous()


def _bilinear(F, x, y):
    """F [2,H*W] float64, positions inside the image -> (val_x, val_y)"""
    xf, yf = torch.floor(x), torch.floor(y)
    x0, y0 = xf.long(), yf.long()
    x1, y1 = torch.clamp(x0 + 1, max=W - 1), torch.clamp(y0 + 1, max=H - 1)
    ax, ay = x - xf, y - yf
    out = []
    for k in range(2):
        G = F[k]
        f00, f01, f10, f11 = G[y0 * W + x0], G[y0 * W + x1], G[y1 * W + x0], G[y1 * W + x1]
        top = f00 + ax * (f01 - f00)
        bot = f10 + ax * (f11 - f10)
        out.append(top + ay * (bot - top))
    return out


def torch_route(xyz, keep, flow_a, flow_b, steps, fb_thr):
    """dict(xy, xyz, pix, state) as ops.track_points returns them, seeds = every pixel, in torch operations chain by chain."""
    dev = xyz.device
    M = H * W
    flat_xyz, flat_keep = xyz.reshape(N, M, 3), keep.reshape(N, M)
    m = torch.arange(M, device=dev)
    zero, thr2 = torch.zeros((), dtype=torch.float64, device=dev), fb_thr * fb_thr
    inside = lambda x, y: (x >= 0) & (x <= W - 1) & (y >= 0) & (y <= H - 1)
    out = dict(xy=[], xyz=[], pix=[], state=[])

    def record(n, alive, x, y):
        xs, ys = torch.where(alive, x, zero), torch.where(alive, y, zero)
        pix = torch.round(ys).long() * W + torch.round(xs).long()
        p = flat_xyz[n][pix]
        seen = alive & (flat_keep[n][pix] != 0) & torch.isfinite(p).all(1)
        out["xy"].append(torch.stack([xs, ys], 1).float())
        out["xyz"].append(torch.where(seen[:, None], p, torch.zeros((), device=dev)))
        out["pix"].append(torch.where(alive, pix, torch.full((), -1, dtype=torch.int64, device=dev)).int())
        out["state"].append(torch.where(seen, 2, torch.where(alive, 1, 0)).to(torch.uint8))

    for chain in steps.tolist():
        x, y = (m % W).double(), torch.div(m, W, rounding_mode="floor").double()
        alive = inside(x, y)
        record(chain[0][0], alive, x, y)
        for _, to, e, rev in chain:
            fwd, bwd = (flow_b[e], flow_a[e]) if rev else (flow_a[e], flow_b[e])
            fwd, bwd = fwd.reshape(2, M).double(), bwd.reshape(2, M).double()
            xs, ys = torch.where(alive, x, zero), torch.where(alive, y, zero)
            fx, fy = _bilinear(fwd, xs, ys)
            xn, yn = xs + fx, ys + fy
            ok1 = alive & inside(xn, yn)
            bx, by = _bilinear(bwd, torch.where(ok1, xn, zero), torch.where(ok1, yn, zero))
            dx, dy = fx + bx, fy + by
            ok2 = ok1 & (dx * dx + dy * dy < thr2)
            x, y, alive = torch.where(ok2, xn, x), torch.where(ok2, yn, y), ok2
            record(to, alive, x, y)
    C, T = steps.shape[0], steps.shape[1] + 1
    return {k: torch.stack(v).reshape((C, T) + tuple(v[0].shape)) for k, v in out.items()}


def device_ms(fn, min_window_s=1.0):
    """(milliseconds per call, reps): a warm-up call, then device events around `reps` calls, doubled until the window reaches
    min_window_s."""
    fn()
    torch.cuda.synchronize()
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tracks.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_tracks.py measures on the GPU; there is none here")
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(0)
    xyz = torch.randn((N, H, W, 3), generator=g, device=dev)
    keep = (torch.rand((N, H, W), generator=g, device=dev) < 0.8).to(torch.uint8)
    imgs = [dict(idx=i, instance=str(i)) for i in range(N)]
    graph = [(p["idx"], q["idx"]) for p, q in make_pairs(imgs, scene_graph="swinstride-5-noncyclic", prefilter=None, symmetrize=True)]
    path = [(k, k + 1) for k in range(N - 1)] + [(k + 1, k) for k in range(N - 1)]
    workloads = (("tracks", path, plan_steps(path, range(N))[None]),
                 ("scene_flow", graph, np.int32([[(i, j, e, 0)] for e, (i, j) in enumerate(graph)])))
    results = []
    for name, edges, steps in workloads:
        fa, fb = smooth_fields(edges, dev)
        call = lambda: ops.track_points(xyz, keep, fa, fb, steps, fb_thr=FB_THR)
        route = lambda: torch_route(xyz, keep, fa, fb, steps, FB_THR)
        got, want = call(), route()
        for k in ("state", "pix", "xy", "xyz"):
            bits = (lambda t: t.view(torch.int32)) if got[k].dtype == torch.float32 else (lambda t: t)
            if got[k].shape != want[k].shape or not torch.equal(bits(got[k]), bits(want[k])):
                sys.exit(f"{name}: the two routes differ in {k}; nothing was timed")
        state = got["state"]
        shares = dict(alive_after_last_step=round(float((state[:, -1] > 0).float().mean()), 4),
                      visible_after_last_step=round(float((state[:, -1] == 2).float().mean()), 4))
        del got, want
        ms, reps = device_ms(call)
        t_ms, t_reps = device_ms(route)
        ms2, reps2 = device_ms(call)
        C_, S_ = steps.shape[:2]
        results.append(dict(workload=name, H=H, W=W, frames=N, edges=len(edges), chains=C_, steps=S_, tracks_per_chain=H * W, fb_thr=FB_THR,
                            equal=True, **shares, track_points_ms=round(ms, 4), track_points_reps=reps, track_points_ms_again=round(ms2, 4),
                            track_steps_per_s=round(C_ * S_ * H * W / (ms * 1e-3), 1), torch_ms=round(t_ms, 4), torch_reps=t_reps,
                            torch_over_track_points=round(t_ms / ms, 2)))
        print(json.dumps(results[-1]), flush=True)
        del fa, fb
    out = dict(tool="tools/bench_tracks.py", device=torch.cuda.get_device_name(0),
               inputs="16 frames of 384 x 512: noise points, 80 % kept pixels, smooth sinusoidal flow fields with a forward-backward "
                      "disagreement of up to 4 px; seeds = every pixel",
               timing="HIP events around reps calls after a warm-up, window >= 1 s; one process; ops.track_points includes its output "
                      "allocation and the step table's upload; the torch route works chain by chain in float64",
               results=results)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
