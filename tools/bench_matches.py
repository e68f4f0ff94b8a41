#!/usr/bin/env python3
"""Reciprocal 3-D matches, device route against host route in one process (developer tool): find_reciprocal_matches on surface
clouds (tests/match_cases.py: a noisy height field seen through a pinhole, P1 seed 11, P2 seed 12) of 2 x 147 456 and 2 x 196 608
points -- a frame pair of 288 x 512 and of 384 x 512.

Per size, in this order:
  1. both routes once; the timing goes on only if (reciprocal_in_P2, nn2_in_P1, count) are equal element for element;
  2. the device route, ops.reciprocal_matches with the library's own chunk count (output and workspace allocation, both searches, the
     reciprocity passes and the read-back of the count included): device events around `reps` calls after a warm-up, `reps` doubled
     until the window is at least a second; then one nn_search direction alone the same way;
  3. a short sweep of forced chunk counts, one search direction each, with the count a rule of four workgroups per CU would pick
     (ceil(1024 / query blocks): 8 and 6 at these sizes) among them;
  4. the host route (two SciPy KD-trees built, two queries with workers=8, the reciprocity test) by wall clock, the median of repeats.

    python tools/bench_matches.py [--host-repeats 3] [--out profiles/matches.json]
"""
import argparse, json, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np, torch
import match_cases as mc
from align3r_amd import ops
from align3r_amd.dust3r.utils.geometry import find_reciprocal_matches

SIZES = [147456, 196608]
SWEEP = [1, 2, 4, 8, 16, 32]


def device_ms(fn, min_window_s=1.0, reps=2):
    """milliseconds per call: device events around `reps` calls, doubled until the window reaches min_window_s"""
    fn()
    torch.cuda.synchronize()
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
    ap.add_argument("--host-repeats", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "matches.json"))
    a = ap.parse_args()
    results = []
    for n in SIZES:
        P1, P2 = mc.pair("surface", n, n)
        D1, D2 = torch.from_numpy(P1).cuda(), torch.from_numpy(P2).cuda()
        rec, nn2, count = find_reciprocal_matches(P1, P2)
        got = ops.reciprocal_matches(D1, D2)
        equal = (np.array_equal(got["reciprocal_in_P2"].cpu().numpy(), rec) and np.array_equal(got["nn2_in_P1"].cpu().numpy(), nn2)
                 and got["count"] == int(count))
        if not equal:
            sys.exit(f"n = {n}: the device route and the host route differ; nothing was timed")
        chunks = ops.nn_chunks(n, n)
        pair_ms, pair_reps = device_ms(lambda: ops.reciprocal_matches(D1, D2))
        one_ms, one_reps = device_ms(lambda: ops.nn_search(D2, D1))
        sweep = {}
        four_per_cu = -(-1024 // -(-n // 1024))                 # the count of a four-workgroups-per-CU rule, for DESIGN 6.12
        for c in sorted(set(SWEEP + [four_per_cu, chunks])):
            base = ops.nn_search(D2, D1)
            assert torch.equal(ops.nn_search(D2, D1, chunks=c), base)
            sweep[str(c)] = round(device_ms(lambda: ops.nn_search(D2, D1, chunks=c))[0], 4)
        host = []
        for _ in range(a.host_repeats):
            t0 = time.perf_counter()
            find_reciprocal_matches(P1, P2)
            host.append(time.perf_counter() - t0)
        host_ms = 1e3 * statistics.median(host)
        evals = 2.0 * n * n
        results.append(dict(n1=n, n2=n, matches=int(count), equal=True, chunks_chosen=chunks,
                            device_reciprocal_matches_ms=round(pair_ms, 4), device_reps=pair_reps,
                            device_nn_search_one_direction_ms=round(one_ms, 4), nn_search_reps=one_reps,
                            distance_evaluations_per_s=round(evals / (pair_ms * 1e-3), 1),
                            nn_search_ms_by_forced_chunks=sweep, chunks_of_a_four_per_cu_rule=four_per_cu,
                            host_ms=round(host_ms, 2), host_repeats=a.host_repeats, host_over_device=round(host_ms / pair_ms, 2)))
        print(json.dumps(results[-1]))
    out = dict(tool="tools/bench_matches.py", device=torch.cuda.get_device_name(0), host_workers=8,
               cloud="surface (tests/match_cases.py), P1 seed 11, P2 seed 12",
               timing="device: HIP events around reps calls after a warm-up, window >= 1 s; host: wall clock, median; one process",
               results=results)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
