#!/usr/bin/env python3
"""Fused aligner at BASELINE config 2 (N=16, E=84, 384x512) with and without per-image train masks, same process, same inputs
(developer tool): iterations/s without masks, with four of sixteen poses frozen, and with four poses, focals and depth maps frozen.
Host clock around work that ends in a device synchronise; each figure is the best of three timed regions.  Prints one JSON line."""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from align3r_amd.aligner import AlignEngine
from align3r_amd.dust3r.image_pairs import make_pairs


def timed(eng, iters, reps=3, warmup=5):
    best, done = 0.0, 0
    total = warmup + reps * iters
    eng.run(warmup, 0.05, total_iters=total)
    done = warmup
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        eng.run(iters, 0.05, first_iter=done, total_iters=total)
        torch.cuda.synchronize()
        best = max(best, iters / (time.perf_counter() - t0))
        done += iters
    return best


if __name__ == "__main__":
    assert torch.cuda.is_available(), "needs a GPU"
    N, H, W, iters = 16, 384, 512, 200
    pairs = make_pairs([dict(idx=i) for i in range(N)], "swin-3-noncyclic", symmetrize=True)
    edges = [(a["idx"], b["idx"]) for a, b in pairs]
    E, P, dev = len(edges), H * W, "cuda"
    g = torch.Generator(device=dev).manual_seed(2)
    pi = torch.randn(E, P, 3, generator=g, device=dev); pj = torch.randn(E, P, 3, generator=g, device=dev)
    wi = torch.log(1 + 9 * torch.rand(E, P, generator=g, device=dev)); wj = torch.log(1 + 9 * torch.rand(E, P, generator=g, device=dev))
    init = dict(pw_poses=torch.randn(E, 8, generator=g, device=dev), depth=torch.randn(N, P, generator=g, device=dev) / 10 - 3,
                im_poses=torch.randn(N, 7, generator=g, device=dev), im_focals=torch.full((N,), 20 * float(np.log(max(H, W)))))
    free = np.ones(N, bool)
    free[[0, 5, 10, 15]] = False
    res = dict(N=N, E=E, P=P, iters=iters)
    for name, masks in (("no_masks_it_s", {}), ("four_poses_frozen_it_s", dict(pose=free)),
                        ("four_poses_focals_depths_frozen_it_s", dict(pose=free, focal=free, depth=free))):
        eng = AlignEngine([i for i, j in edges], [j for i, j in edges], pi, pj, wi, wj, [(H, W)] * N, device=dev, loss_capacity=4 * iters)
        eng.set_params(**init)
        if masks:
            eng.set_train_masks(**masks)
        res[name] = round(timed(eng, iters), 1)
        del eng
    print(json.dumps(res), flush=True)
