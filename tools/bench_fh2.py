#!/usr/bin/env python3
"""Per-shape timing of the fh2 GEMM at the ViT-L shapes of the pair forward (12 pairs, 512x384), per tile choice.

    python tools/bench_fh2.py [tile ...]                    the 12-pair shapes (SHAPES), tiles "auto" | 0..3
    python tools/bench_fh2.py --lists [--json FILE]         the bench's 42-pair step (16 distinct frames): the launches that run on
                                                            distinct rows (DISTINCT) and those that run on every slot (PER_SLOT),
                                                            every admissible tile and the chooser's own choice, in one process;
                                                            the table the eff entries of csrc/fh2_chooser.h are fitted to
"""
import json
import os
import sys
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from align3r_amd import ops, _lib   # noqa: E402

SHAPES = [  # (name, M, N, K, groups, launches per forward)
    ("enc qkv", 18432, 3072, 1024, 1, 24), ("enc proj", 18432, 1024, 1024, 1, 24), ("enc fc1", 18432, 4096, 1024, 1, 24),
    ("enc fc2", 18432, 1024, 4096, 1, 24), ("dec qkv", 9216, 2304, 768, 2, 12), ("dec proj/q/cproj", 9216, 768, 768, 2, 36),
    ("dec kv", 9216, 1536, 768, 2, 12), ("dec fc1", 9216, 3072, 768, 2, 12), ("dec fc2", 9216, 768, 3072, 2, 12),
    ("pc qkv", 18432, 2304, 768, 1, 4), ("pc proj/zc", 18432, 768, 768, 1, 9), ("pc fc1", 18432, 3072, 768, 1, 4),
    ("pc fc2", 18432, 768, 3072, 1, 4), ("embed", 18432, 1024, 768, 1, 1), ("dec_embed", 18432, 768, 1024, 1, 1),
    ("out_conv1", 589824, 256, 256, 1, 2), ("out_conv2", 147456, 256, 256, 1, 2),
]
# 42 pairs of 16 distinct 512x384 frames (768 tokens each): the encoder, dec_blocks_pc, the zero-convs and decoder_embed run on the
# 16 x 768 = 12288 distinct rows, decoder block 0's frame-only half on each side's 15 entries (two groups of 11520 rows)
DISTINCT = [
    ("enc qkv", 12288, 3072, 1024, 1, 24), ("enc proj", 12288, 1024, 1024, 1, 24), ("enc fc1", 12288, 4096, 1024, 1, 24),
    ("enc fc2", 12288, 1024, 4096, 1, 24), ("pc qkv", 12288, 2304, 768, 1, 4), ("pc proj/zc", 12288, 768, 768, 1, 9),
    ("pc fc1", 12288, 3072, 768, 1, 4), ("pc fc2", 12288, 768, 3072, 1, 4), ("dec_embed", 12288, 768, 1024, 1, 1),
    ("blk0 qkv", 11520, 2304, 768, 2, 1), ("blk0 proj", 11520, 768, 768, 2, 1),
]
# the decoder's launches on all 42 slots of each side: two groups of 42 x 768 = 32256 rows
PER_SLOT = [
    ("dec proj/q/cproj", 32256, 768, 768, 2, 35), ("dec kv", 32256, 1536, 768, 2, 12), ("dec qkv", 32256, 2304, 768, 2, 11),
    ("dec fc1", 32256, 3072, 768, 2, 12), ("dec fc2", 32256, 768, 3072, 2, 12),
]
LIST_TILES = ["0", "1", "2"]


def timeit(fn, iters=10):
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters * 1e3


def set_tile(t):
    if t == "auto":
        os.environ.pop("A3R_FH2_TILE", None)        # read per call
    else:
        os.environ["A3R_FH2_TILE"] = t


def time_shape(M, N, K, G, tiles, iters=10, rounds=1):
    """us per launch for every tile of `tiles`: the minimum over `rounds` interleaved rounds of `iters` launches each."""
    xs = [(ops.split_fh2)(torch.randn(M, K, device="cuda")) for _ in range(G)]
    ws = [ops.split_fh2_w(torch.randn(N, K, device="cuda") * K ** -0.5) for _ in range(G)]
    bs = [torch.randn(N, device="cuda") for _ in range(G)]
    best = {t: float("inf") for t in tiles}
    for _ in range(rounds):
        for t in tiles:
            set_tile(t)
            best[t] = min(best[t], timeit(lambda: ops.linear_fh2_grouped(xs, ws, bs), iters))
    set_tile("auto")
    return best


def run_lists(json_path):
    tiles = LIST_TILES + ["auto"]
    table = []
    print(f"{'list':9s} {'shape':18s} {'M':>6s} {'N':>5s} {'K':>5s} g " + " ".join(f"{'tile ' + t:>10s}" for t in tiles) + "   best  auto/best")
    tot = {t: 0.0 for t in tiles + ["best"]}
    for lname, shapes in (("distinct", DISTINCT), ("per_slot", PER_SLOT)):
        for name, M, N, K, G, cnt in shapes:
            us = time_shape(M, N, K, G, tiles, iters=20, rounds=3)
            best = min(LIST_TILES, key=lambda t: us[t])
            for t in tiles:
                tot[t] += us[t] * cnt
            tot["best"] += us[best] * cnt
            table.append({"list": lname, "shape": name, "M": M, "N": N, "K": K, "groups": G, "launches": cnt,
                          "us": {t: round(us[t], 1) for t in tiles}, "best_tile": int(best)})
            print(f"{lname:9s} {name:18s} {M:6d} {N:5d} {K:5d} {G} " + " ".join(f"{us[t]:10.1f}" for t in tiles) +
                  f"   {best:>4s}  {us['auto'] / us[best]:.3f}", flush=True)
    print("weighted total per forward (ms): " + "  ".join(f"{t}: {tot[t] / 1e3:.2f}" for t in tot))
    if json_path:
        with open(json_path, "w") as f:
            json.dump({"unit": "us per launch, minimum of 3 interleaved rounds of 20 launches", "rows": table,
                       "weighted_ms_per_forward": {t: round(tot[t] / 1e3, 3) for t in tot}}, f, indent=1)


def main():
    if "--lists" in sys.argv:
        run_lists(sys.argv[sys.argv.index("--json") + 1] if "--json" in sys.argv else None)
        return
    scale = float(os.environ.get("A3R_BENCH_MSCALE", "1"))      # 3.5 = the bench's 42 pairs per step
    if os.environ.get("A3R_BENCH_PASSES") == "1":               # the single-pass (fp16 operand) build of the same kernel
        ops.fh2_set_passes(1)
    shapes = [(n, int(M * scale) if M < 100000 else M, N, K, G, c) for n, M, N, K, G, c in SHAPES]
    tiles = sys.argv[1:] or ["auto", "0", "1"]
    tot = {t: 0.0 for t in tiles}
    print(f"{'shape':18s} {'M':>7s} {'N':>5s} {'K':>5s} g " + " ".join(f"{'tile ' + t:>22s}" for t in tiles))
    for name, M, N, K, G, cnt in shapes:
        us = time_shape(M, N, K, G, tiles)
        row = []
        for t in tiles:
            tf = 2.0 * M * N * K * G / us[t] / 1e6
            tot[t] += us[t] * cnt
            row.append(f"{us[t]:9.1f} us {tf:6.1f} TF")
        print(f"{name:18s} {M:7d} {N:5d} {K:5d} {G} " + " ".join(f"{r:>22s}" for r in row))
    print("weighted total per forward (ms): " + "  ".join(f"tile {t}: {tot[t] / 1e3:.2f}" for t in tiles))


if __name__ == "__main__":
    main()
