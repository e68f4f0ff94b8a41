#!/usr/bin/env python3
"""Depth evaluation, host path against device path in one process (developer tool): evaluate_depth(mode='lad') on synthetic clips of
64 x 288 x 512 and 128 x 384 x 512 float32 maps with invalid regions (a band without ground truth, a band beyond depth_max, one frame
without a valid pixel).

Host: the numpy + scipy path (the parent commit's code, unchanged), wall clock, one run.  Device: evaluate_depth(device=...) on maps
that already sit on the device -- the whole enqueue (radix select, LAD solve, metric pass) plus the one read-back, between two HIP
events, the median of --repeats after one warm-up; the upload of the two maps is timed separately.  Pass time: 20 'lstsq' solves
enqueued back to back are 40 streaming passes, each with its one-wave step kernel (and 40 one-wave init / finish kernels), so
t / 40 is one pass + step from above; bytes/s = 8 n / that.  The LAD solve enqueues every round, so its time includes the launches that return at once after the solve is done.
The run fails if the device path is slower than the host path.

    python tools/bench_depth_eval.py [--repeats 5] [--clips 64x288x512,128x384x512] [--out profiles/depth_eval.json]
"""
import argparse, json, os, statistics, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch
from align3r_amd import ops
from align3r_amd.tool.depth_metrics import evaluate_depth

DEPTH_MAX = 70.0


def make_clip(T, H, W, seed=0):
    rng = np.random.default_rng(seed)
    gt = rng.uniform(0.5, 60.0, (T, H, W)).astype(np.float32)
    pred = (gt / 3.0 * np.exp(0.1 * rng.standard_normal((T, H, W), dtype=np.float32)) + 0.05).astype(np.float32)
    gt[:, H // 3:H // 3 + H // 8, :] = 0.0
    gt[:, :, W - W // 10:] = 2.0 * DEPTH_MAX
    gt[T // 2] = 0.0
    return pred, gt


def event_ms(fn, repeats, warmup=1):
    for _ in range(warmup):
        out = fn()
    ts = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        out = fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return statistics.median(ts), out


def main():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--clips", default="64x288x512,128x384x512")
    ap.add_argument("--device", default="cuda:0")
    ap.add_argument("--out", default=os.path.join(root, "profiles", "depth_eval.json"))
    a = ap.parse_args()
    if a.repeats < 5:
        ap.error("--repeats must be at least 5")
    dev = torch.device(a.device)
    results = []
    for spec in a.clips.split(","):
        T, H, W = (int(x) for x in spec.split("x"))
        pred, gt = make_clip(T, H, W)
        n = pred.size
        t0 = time.perf_counter()
        host = evaluate_depth(pred, gt, depth_max=DEPTH_MAX, mode="lad")
        t_host = time.perf_counter() - t0
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        pred_d, gt_d = torch.from_numpy(pred).to(dev), torch.from_numpy(gt).to(dev)
        torch.cuda.synchronize()
        t_upload = time.perf_counter() - t0
        ms_lad, m = event_ms(lambda: evaluate_depth(pred_d, gt_d, depth_max=DEPTH_MAX, mode="lad", device=dev), a.repeats)
        ms_scale, _ = event_ms(lambda: ops.depth_align(pred_d, gt_d, DEPTH_MAX, "scale")[0].cpu(), a.repeats)
        ms_lstsq, _ = event_ms(lambda: ops.depth_align(pred_d, gt_d, DEPTH_MAX, "lstsq")[0].cpu(), a.repeats)
        ms_metrics, _ = event_ms(lambda: ops.depth_metrics(pred_d, gt_d, DEPTH_MAX, 3.0, 0.0).cpu(), a.repeats)
        info = ops.depth_align(pred_d, gt_d, DEPTH_MAX, "lad")[1].cpu().numpy()
        ms_40, _ = event_ms(lambda: [ops.depth_align(pred_d, gt_d, DEPTH_MAX, "lstsq") for _ in range(20)][-1][0].cpu(), a.repeats)
        ms_pass = ms_40 / 40.0
        valid = (gt > 1e-3) & (gt < DEPTH_MAX)
        p, g = pred[valid].astype(np.float64), gt[valid].astype(np.float64)
        f_dev = float(np.abs(m["scale"] * p + m["shift"] - g).sum())
        # the host's (s, t) is not returned by the host path: its objective is bounded below by the device's when both reach the minimum
        r = dict(clip=spec, n=n, n_valid=int(m["n_valid"]), host_lad_s=t_host, device_lad_ms=ms_lad, upload_ms=1e3 * t_upload,
                 speedup_without_upload=1e3 * t_host / ms_lad, speedup_with_upload=1e3 * t_host / (ms_lad + 1e3 * t_upload),
                 lad_passes=int(info[2]), lad_enlargements=int(info[3]), lad_objective_device=f_dev, lad_objective_device_reported=float(info[1]),
                 pass_plus_step_ms=ms_pass, pass_bytes=8 * n, pass_bytes_per_s=8 * n / (1e-3 * ms_pass) if ms_pass > 0 else None,
                 scale_rule_ms=ms_scale, lstsq_rule_ms=ms_lstsq, metrics_ms=ms_metrics,
                 abs_rel_host=host["abs_rel"], abs_rel_device=m["abs_rel"], abs_rel_diff=abs(host["abs_rel"] - m["abs_rel"]), repeats=a.repeats)
        print(json.dumps(r), flush=True)
        results.append(r)
    out = dict(device=torch.cuda.get_device_name(dev), tool="tools/bench_depth_eval.py", results=results)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    slower = [r["clip"] for r in results if r["device_lad_ms"] + r["upload_ms"] > 1e3 * r["host_lad_s"]]
    if slower:
        sys.exit(f"the device path is slower than the host path on {slower}")


if __name__ == "__main__":
    main()
