#!/usr/bin/env python3
"""Edge-sharded aligner on ONE GPU against the fused (monolithic) handle, same process, same inputs (developer tool).

Per problem size (BASELINE config 2: N=16, E=84, 384x512; config 3: N=64, E=4032, 288x512): iterations/s of AlignEngine and of
ShardedAlignEngine(local_shards=K) for K in {1, 2, 4, 8} (host clock around work that ends in a device synchronise), and the
HIP-event time of the partial main kernel (K = 1) and of the [N, P] Adam kernel with their achieved bandwidth against their own
algorithmic byte counts:
    partial  32*E*P (points + weights, both sides) + 4*N*P (depth parameter) + 4*N*P (gradient map written)
    apply    28*N*P (p, g, m, v read; p, m, v written)
K shards in one process run one after the other on the same device and each applies the update to its own replica, so this measures
the cost of the sharded form, not a speed-up: the multi-GPU scaling is NOT measured here (no process has run two RCCL ranks).
Writes profiles/r04_align_sharded.json."""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from align3r_amd import _lib
from align3r_amd.aligner import AlignEngine, ShardedAlignEngine
from align3r_amd.dust3r.image_pairs import make_pairs

KS = (1, 2, 4, 8)


def timed(eng, iters, warmup=3):
    eng.run(warmup, 0.05, total_iters=iters + warmup)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    eng.run(iters, 0.05, first_iter=warmup, total_iters=iters + warmup)
    torch.cuda.synchronize()
    return iters / (time.perf_counter() - t0)


def run(name, N, H, W, graph, iters):
    pairs = make_pairs([dict(idx=i) for i in range(N)], graph, symmetrize=True)
    edges = [(a["idx"], b["idx"]) for a, b in pairs]
    E, P = len(edges), H * W
    dev = "cuda"
    g = torch.Generator(device=dev).manual_seed(2)
    pi = torch.randn(E, P, 3, generator=g, device=dev); pj = torch.randn(E, P, 3, generator=g, device=dev)
    wi = torch.log(1 + 9 * torch.rand(E, P, generator=g, device=dev)); wj = torch.log(1 + 9 * torch.rand(E, P, generator=g, device=dev))
    args = ([i for i, j in edges], [j for i, j in edges], pi, pj, wi, wj, [(H, W)] * N)
    init = dict(pw_poses=torch.randn(E, 8, generator=g, device=dev), depth=torch.randn(N, P, generator=g, device=dev) / 10 - 3,
                im_poses=torch.randn(N, 7, generator=g, device=dev), im_focals=torch.full((N,), 20 * float(np.log(max(H, W)))))
    cap = 4 * iters + 32
    res = dict(N=N, E=E, P=P, iters=iters, bytes_fused=32.0 * E * P + 24.0 * N * P)
    mono = AlignEngine(*args, device=dev, loss_capacity=cap)
    mono.set_params(**init)
    res["monolithic_it_s"] = timed(mono, iters)
    del mono
    for K in KS:
        s = ShardedAlignEngine(*args, device=dev, loss_capacity=cap, local_shards=K)
        s.set_params(**init)
        res[f"sharded_K{K}_it_s"] = timed(s, iters)
        if K == 1:
            _lib.prof_enable(True)
            s.run(iters, 0.05, first_iter=iters + 3, total_iters=2 * iters + 3)
            torch.cuda.synchronize()
            _lib.prof_enable(False)
            r = {p["name"]: p for p in _lib.prof_report()}
            part, adam = r["align_main_kernel (edge-shard partial)"], r["align_adam_map_kernel"]
            b_part, b_adam = 32.0 * E * P + 8.0 * N * P, 28.0 * N * P
            res["partial_kernel_us"] = 1e3 * part["ms"] / part["launches"]
            res["partial_kernel_TB_s"] = b_part / (part["ms"] / part["launches"] * 1e-3) / 1e12
            res["partial_kernel_bytes"] = b_part
            res["adam_map_kernel_us"] = 1e3 * adam["ms"] / adam["launches"]
            res["adam_map_kernel_TB_s"] = b_adam / (adam["ms"] / adam["launches"] * 1e-3) / 1e12
            res["adam_map_kernel_bytes"] = b_adam
            res["bytes_sharded_K1"] = b_part + b_adam
        del s
        torch.cuda.empty_cache()
    print(name, json.dumps(res), flush=True)
    return res


if __name__ == "__main__":
    assert torch.cuda.is_available(), "needs a GPU"
    out = dict(what="iterations/s of the fused aligner and of ShardedAlignEngine(local_shards=K) on one MI355X, one process, one run; "
                    "kernel times from HIP events; multi-GPU scaling NOT measured",
               config2=run("config2", 16, 384, 512, "swin-3-noncyclic", 200))
    if "--no-config3" not in sys.argv:
        out["config3"] = run("config3", 64, 288, 512, "complete", 20)
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    os.makedirs(os.path.join(repo, "profiles"), exist_ok=True)
    with open(os.path.join(repo, "profiles", "r04_align_sharded.json"), "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
