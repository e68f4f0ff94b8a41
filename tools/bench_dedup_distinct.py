#!/usr/bin/env python3
"""What the duplicate search costs when it finds nothing: one 42-pair ViT-L step at 512x384 over 84 DISTINCT images and 84
distinct pred_depth maps, a3r_model_set_dedup mode 1 (keys, comparison, one read-back; then the plain plan) against mode 0 (the
plain plan alone), alternating.  Prints one JSON line: ms per step of every round and mode.
usage (on the GPU box): python tools/bench_dedup_distinct.py [--rounds 3] [--steps 3]"""
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
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--batch", type=int, default=42)
    ap.add_argument("--height", type=int, default=384)
    ap.add_argument("--width", type=int, default=512)
    a = ap.parse_args()
    from align3r_amd.engine import PairEngine
    from align3r_amd.weights import VITL, hash_uniform, synthetic_state_dict
    H, W, B = a.height, a.width, a.batch
    P = H * W
    img = torch.from_numpy((2.0 * hash_uniform("img", 2 * B * 3 * P, 1)).astype(np.float32).reshape(2 * B, 3, H, W)).cuda()
    pd = torch.from_numpy((hash_uniform("pred_depth", 2 * B * P * 3, 1) + 0.5).astype(np.float32).reshape(2 * B, H, W, 3)).cuda()
    args = (img[:B].contiguous(), img[B:].contiguous(), pd[:B].contiguous(), pd[B:].contiguous())
    eng = PairEngine(VITL, synthetic_state_dict(VITL, 0))
    out = eng.forward(*args)                     # warm-up: workspace, range scales
    assert eng.last_dedup() == (2 * B, 2 * B, False), eng.last_dedup()
    ms = {0: [], 1: []}
    for _ in range(a.rounds):
        for mode in (0, 1):
            eng.set_dedup(mode)
            eng.forward(*args, out=out)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(a.steps):
                eng.forward(*args, out=out)
            torch.cuda.synchronize()
            ms[mode].append(round(1e3 * (time.perf_counter() - t0) / a.steps, 3))
    print(json.dumps({"what": "42-pair step, 84 distinct frames", "steps": a.steps, "ms_per_step_mode0": ms[0], "ms_per_step_mode1": ms[1]}))


if __name__ == "__main__":
    main()
