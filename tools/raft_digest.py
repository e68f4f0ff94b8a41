#!/usr/bin/env python3
"""SHA-1 of every output of a fixed set of flow-network calls (developer tool): python tools/raft_digest.py [case filter]

Two builds compute the same thing exactly when they print the same lines; run it once per library (A3R_LIB selects one) and diff.
The cases are the smallest at which the launch plan (csrc/raft.hip) can go wrong: 128 px is the smallest side a four-level
correlation pyramid accepts, 136 x 168 gives an odd 17 x 21 eighth-resolution map, and zero, one and three iterations walk the loop's
edges.  Each case runs in both arithmetics (A3R_RAFT unset and bf3)."""
import hashlib
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from align3r_amd.raft import RaftEngine
from align3r_amd.raft_weights import RAFT_M, RAFT_TINY, synthetic_raft_frames, synthetic_raft_state_dict


def sha(t):
    return hashlib.sha1(np.ascontiguousarray(t.detach().cpu().numpy()).tobytes()).hexdigest()


def all_taps(cfg, B, H, W, iters):
    h, w, d = H // 8, W // 8, cfg.dim
    z = lambda *s: torch.zeros(*s, device="cuda")
    taps = dict(cnet=z(B, h, w, 2 * d), fmap=z(2 * B, h, w, 2 * d), flow_update0=z(B, h, w, 6), weight0=z(B, h, w, 576))
    if iters > 0:
        taps.update(lookup0=z(B, h, w, (cfg.corr_channel + 31) // 32 * 32), motion0=z(B, h, w, d))
    hl, wl = h, w
    for l in range(cfg.corr_levels):
        taps[f"corr_pyr{l}"] = z(B * h * w, hl, wl)
        hl, wl = hl // 2, wl // 2
    for it in range(min(iters, 4)):
        taps[f"net{it}"] = z(B, h, w, d)
        taps[f"flow8_{it}"] = z(B, h, w, 2)
    return taps


def frames(B, H, W):
    a, b = synthetic_raft_frames(B, H, W, 0)
    return torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda()


def tiny_taps(eng, iters):
    a, b = frames(3, 128, 160)
    taps = all_taps(RAFT_TINY, 3, 128, 160, iters)
    out = {"flow": eng.forward(a, b, iters=iters, taps=taps)}
    out.update(taps)
    return out


def tiny_odd(eng):
    a, b = frames(1, 136, 168)
    return {"flow": eng.forward(a, b, iters=2)}


def tiny_cached(eng):
    a, b = frames(3, 128, 160)
    fm = eng.encode(torch.cat([a, b]))
    f1, f2 = fm[:3].contiguous(), fm[3:].contiguous()
    return {"fmap": fm, "flow": eng.forward(a, b, iters=3, fmaps=(f1, f2))}


def m_small(eng):
    a, b = frames(1, 128, 160)
    return {"flow": eng.forward(a, b, iters=2)}


CASES = [("tiny/3x128x160/iters0", RAFT_TINY, lambda e: tiny_taps(e, 0)), ("tiny/3x128x160/iters1", RAFT_TINY, lambda e: tiny_taps(e, 1)),
         ("tiny/3x128x160/iters3", RAFT_TINY, lambda e: tiny_taps(e, 3)), ("tiny/1x136x168/iters2", RAFT_TINY, tiny_odd),
         ("tiny/encode6+forward3", RAFT_TINY, tiny_cached), ("m/1x128x160/iters2", RAFT_M, m_small)]


def main():
    pick = sys.argv[1] if len(sys.argv) > 1 else ""
    for arith in ("fh2", "bf3"):
        if arith == "bf3":
            os.environ["A3R_RAFT"] = "bf3"
        else:
            os.environ.pop("A3R_RAFT", None)
        engines = {}
        for name, cfg, run in CASES:
            if pick not in name:
                continue
            if cfg not in engines:
                engines[cfg] = RaftEngine(cfg, synthetic_raft_state_dict(cfg, 0))
            eng = engines[cfg]
            for k, t in sorted(run(eng).items()):
                print(f"{name}/{arith}/{k} {sha(t)}", flush=True)
            assert eng.range_fallbacks == 0 and eng.fh2 == (arith == "fh2")


if __name__ == "__main__":
    main()
