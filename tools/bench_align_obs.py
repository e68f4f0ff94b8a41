#!/usr/bin/env python3
"""Fused aligner handle with fp32 and with packed fp16 observations (developer tool) -> profiles/align_obs16.json.

Per size (config 2: N=16 E=84 P=196608; config 3: N=64 E=4032 P=147456; config 4 graph: N=128 E=1230 P=196608): iterations/s
(un-profiled) and the main kernel's time and TB/s over its algorithmic bytes (32 E P + 24 N P in fp32, 16 E P + 24 N P packed),
fp32 first, then fp16, in ONE process, two runs each.  With --accuracy also what the storage mode costs: 300 cosine iterations at
config-2 size from one start, fp16 against fp32 storage -- relative differences of depth maps, poses and focals, and the
difference in AbsRel against the synthetic ground truth of tests/test_gpu_align.py (LAD scale + shift).

    python tools/bench_align_obs.py [--label NAME] [--dtypes fp32,fp16] [--sizes c2,c3,c4] [--accuracy] [--out FILE]

The result is merged into FILE under NAME, so a run against another build of the library (A3R_LIB=...) can be put beside it.
On a shared GPU box run it as one job, each step under its own time limit, steps chained with &&:
    timeout -k 10 500 python tools/bench_align_obs.py --label parent --dtypes fp32 && timeout -k 10 600 python tools/bench_align_obs.py --accuracy
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from align3r_amd import _lib
from align3r_amd.aligner import AlignEngine
from align3r_amd.dust3r.image_pairs import make_pairs

SIZES = {"c2": (16, 384, 512, "swin-3-noncyclic", 200), "c3": (64, 288, 512, "complete", 20),
         "c4": (128, 384, 512, "swinstride-5-noncyclic", 40)}


def problem(N, H, W, graph, seed=2):
    pairs = make_pairs([dict(idx=i) for i in range(N)], graph, symmetrize=True)
    edges = [(a["idx"], b["idx"]) for a, b in pairs]
    E, P = len(edges), H * W
    g = torch.Generator(device="cuda").manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g, device="cuda")
    u = lambda *s: torch.rand(*s, generator=g, device="cuda")
    obs = (r(E, P, 3), r(E, P, 3), torch.log(1 + 9 * u(E, P)), torch.log(1 + 9 * u(E, P)))
    init = dict(pw_poses=r(E, 8), depth=r(N, P) / 10 - 3, im_poses=r(N, 7), im_focals=torch.full((N,), 20 * float(np.log(max(H, W)))))
    return edges, obs, init


def engine(edges, obs, init, N, H, W, dtype, capacity):
    kw = {} if dtype == "fp32" else dict(obs_dtype=dtype)          # (an older build of the package has no such keyword)
    al = AlignEngine([i for i, j in edges], [j for i, j in edges], *obs, [(H, W)] * N, device="cuda", loss_capacity=capacity, **kw)
    al.set_params(**init)
    return al


def rate(al, iters):
    al.run(5, 0.05, total_iters=iters + 5)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    al.run(iters, 0.05, first_iter=5, total_iters=iters + 5)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    _lib.prof_enable(True)
    al.run(iters, 0.05, first_iter=5, total_iters=iters + 5)
    torch.cuda.synchronize()
    _lib.prof_enable(False)
    main = {p["name"]: p for p in _lib.prof_report()}["align_main_kernel"]
    return dict(iters_per_s=round(iters / dt, 1), main_us=round(1e3 * main["ms"] / main["launches"], 1),
                main_tb_per_s=round(main["work"] / main["ms"] / 1e9, 3), main_bytes=main["work"] / main["launches"])


def bench(size, dtypes, runs=2):
    N, H, W, graph, iters = SIZES[size]
    edges, obs, init = problem(N, H, W, graph)
    out = dict(N=N, E=len(edges), P=H * W, iters=iters)
    for dt in dtypes:
        res = []
        for _ in range(runs):
            al = engine(edges, obs, init, N, H, W, dt, 2 * iters + 16)
            res.append(rate(al, iters))
            del al
            torch.cuda.empty_cache()        # every run allocates afresh: no run inherits the block layout of the one before
        out[dt] = dict(runs=res, lower_iters_per_s=min(r["iters_per_s"] for r in res))
        print(size, dt, out[dt], flush=True)
    return out


def accuracy(niter=300):
    from align3r_amd.tool.depth_metrics import evaluate_depth
    N, H, W, graph, _ = SIZES["c2"]
    edges, obs, init = problem(N, H, W, graph)
    state = {}
    for dt in ("fp32", "fp16"):
        al = engine(edges, obs, init, N, H, W, dt, niter + 16)
        losses = al.run(niter, 0.05, "cosine")
        state[dt] = {k: al.params[k].detach().cpu().numpy().astype(np.float64) for k in ("depth", "im_poses", "im_focals", "pw_poses")}
        state[dt]["loss"] = float(losses[-1])
        del al
    rel = lambda a, b: float(np.abs(a - b).max() / np.abs(b).max())
    d32, d16 = np.exp(state["fp32"]["depth"]), np.exp(state["fp16"]["depth"])
    yy = np.linspace(0, 1, d32[0].size).reshape(1, -1)
    gt = (2.0 * d32 + 0.1) * (1 + 0.2 * np.sin(7 * yy + np.arange(N)[:, None]))
    m = {dt: evaluate_depth(d.reshape(N, 1, -1), gt.reshape(N, 1, -1), depth_max=1e9, mode="lad")["abs_rel"] for dt, d in (("fp32", d32), ("fp16", d16))}
    out = dict(niter=niter, N=N, E=len(edges), P=H * W,
               depth_rel_max=rel(d16, d32), depth_rel_median=float(np.median(np.abs(d16 / d32 - 1))),
               im_poses_rel=rel(state["fp16"]["im_poses"], state["fp32"]["im_poses"]),
               focals_rel=rel(np.exp(state["fp16"]["im_focals"] / 20), np.exp(state["fp32"]["im_focals"] / 20)),
               pw_poses_rel=rel(state["fp16"]["pw_poses"], state["fp32"]["pw_poses"]),
               final_loss_fp32=state["fp32"]["loss"], final_loss_fp16=state["fp16"]["loss"],
               abs_rel_fp32=m["fp32"], abs_rel_fp16=m["fp16"], abs_rel_diff=abs(m["fp16"] - m["fp32"]))
    print("accuracy", out, flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--label", default="this")
    ap.add_argument("--dtypes", default="fp32,fp16")
    ap.add_argument("--sizes", default="c2,c3,c4")
    ap.add_argument("--accuracy", action="store_true")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "align_obs16.json"))
    a = ap.parse_args()
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    res = dict(library=os.path.relpath(_lib.LIB_PATH, root), device=torch.cuda.get_device_name(0))
    for size in [s for s in a.sizes.split(",") if s]:
        res[size] = bench(size, a.dtypes.split(","))
        torch.cuda.empty_cache()
    if a.accuracy:
        res["accuracy_c2_300_cosine"] = accuracy()
    doc = json.load(open(a.out)) if os.path.exists(a.out) else {}
    doc[a.label] = res
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
