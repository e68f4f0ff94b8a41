#!/usr/bin/env python3
"""What a forward costs by how many of its frames' head products the handle has kept from earlier calls
(a3r_model_set_head_products): the steps of tools/bench_frame_products.py -- the 42-pair ViT-L step of bench.py with 16 / 16, 8 / 16
and 0 / 16 of its frames found in storages of 16 entries, clips taking turns -- with every step's report of the three storages
checked.  A3R_HEAD_PRODUCTS=0 in the environment runs the same steps without the head products: the difference in the 0 / 16 row is
what the copies of 16 frames' r0 and c blocks into their entries cost (two sides: about 0.8 GB per step), that in the 16 / 16 row
what the skipped level-0 branch saves.  Prints one JSON line: ms per step of every round and case.
usage (on the GPU box): [A3R_HEAD_PRODUCTS=0] python tools/bench_head_products.py [--rounds 3] [--steps 4]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=4)
    ap.add_argument("--batch", type=int, default=42)
    ap.add_argument("--height", type=int, default=384)
    ap.add_argument("--width", type=int, default=512)
    a = ap.parse_args()
    import bench
    from align3r_amd.dust3r.image_pairs import make_pairs
    from align3r_amd.engine import PairEngine
    from align3r_amd.weights import VITL, hash_uniform
    H, W, B, P, n = a.height, a.width, a.batch, a.height * a.width, 16
    frames = []
    for i in range(2 * n):
        img = (2.0 * hash_uniform(f"img{i}", 3 * P, 1)).astype(np.float32).reshape(3, H, W)
        pd = (hash_uniform(f"pred_depth{i}", P * 3, 1) + 0.5).astype(np.float32).reshape(H, W, 3)
        frames.append((torch.from_numpy(img).cuda(), torch.from_numpy(pd).cuda()))
    edges = [(p["idx"], q["idx"]) for p, q in make_pairs([dict(idx=i) for i in range(n)], "swin-3-noncyclic", symmetrize=True)][:B]
    assert len({i for e in edges for i in e}) == n, "the batch must hold every frame of the clip"
    pos = [{i for i, _ in edges}, {j for _, j in edges}]            # the clip's positions on each side
    n_side, lo_side = [len(p) for p in pos], [len([i for i in p if i < 8]) for p in pos]

    def clip(ids):
        f = [frames[i] for i in ids]
        return (torch.stack([f[i][0] for i, _ in edges]), torch.stack([f[j][0] for _, j in edges]),
                torch.stack([f[i][1] for i, _ in edges]), torch.stack([f[j][1] for _, j in edges]))

    x, y, z = clip(range(n)), clip(range(n, 2 * n)), clip(list(range(8)) + list(range(n, n + 8)))
    # case -> the clips that take turns, and what every step after the first two must report: the frame cache's
    # (hits, misses, evictions), and per side the head products' (hits, misses) among the side's distinct frames
    sides = lambda found: tuple((f, m - f) for f, m in zip(found, n_side))
    cases = {"16_of_16": ((x, x), (16, 0, 0), sides(n_side)), "8_of_16": ((x, z), (8, 8, 8), sides(lo_side)),
             "0_of_16": ((x, y), (0, 16, 16), sides([0, 0]))}
    eng = PairEngine(VITL, bench.synthetic_weights(VITL), frame_cache=0)
    eng.set_frame_cache(n, H, W)
    heads = eng._hp_store is not None
    out = eng.forward(*x)                        # warm-up: workspace, range scales
    assert eng.last_dedup_sides() == (n_side[0], n_side[1], True, True), eng.last_dedup_sides()
    ms = {k: [] for k in cases}
    for _ in range(a.rounds):
        for name, (turn, want, side) in cases.items():
            for s in range(2):
                eng.forward(*turn[s], out=out)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for s in range(a.steps):
                eng.forward(*turn[s % 2], out=out)
                assert eng.last_frame_cache() == want, (name, eng.last_frame_cache())
                assert eng.last_head_products() == (side if heads else ((0, 0), (0, 0))), (name, eng.last_head_products())
            torch.cuda.synchronize()
            ms[name].append(round(1e3 * (time.perf_counter() - t0) / a.steps, 3))
    print(json.dumps({"what": f"{B}-pair step, {n}-frame clip, frames and their head products found in the storages kept across calls",
                      "head_products": heads, "frame_products": eng._fp_store is not None, "steps": a.steps, "reruns": eng.range_reruns,
                      "ms_per_step": ms}))


if __name__ == "__main__":
    main()
