#!/usr/bin/env python3
"""The hierarchical pose pipeline (tool/hierarchical.py, flow=dict(...)) on ONE GPU, host-resident against device-resident
(developer tool, a few minutes): 128 frames of 384x512, clip size 10 -> 13 keyframes (156 pairs) and 13 clips (50 pairs each, 32 in
the last one); ViT-L pair forward and RAFT2 with synthetic weights, self-computed motion masks, init='mst' with init_priors per
clip, 300 iterations per scene.  As in bench_clip4.py the pair forward is run for its time and its outputs are then overwritten,
outside the timed regions, by a consistent synthetic scene so that the aligner has a problem it can solve.

    python tools/bench_hier_flow.py [N_FRAMES] [--niter 300] [--repeat 2] [--out profiles/hier_flow.json]

Per mode: seconds spent in the pair forwards (host-resident: including the copy of the outputs to host memory, which is what
inference() does by default), the flow network, the motion masks, the MST initialisation and the iterations, summed over the 14
scenes; the rest of the wall time is scene construction (confidence maps, weights, engine upload) and the read-backs of results.
`init_clip_s` is the mean initialisation time of a clip scene: the generic torch path in the host-resident mode, the device
path (init_priors included) in the device-resident one.  Stages are delimited by device synchronisations."""
import argparse, json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch
from bench import synthetic_pair_geometry
from align3r_amd.weights import VITL, synthetic_state_dict, hash_uniform
from align3r_amd.engine import PairEngine
from align3r_amd.raft import RAFT2
from align3r_amd.raft_weights import RAFT_M, synthetic_raft_state_dict, synthetic_raft_frames
from align3r_amd.tool import hierarchical as hz
import align3r_amd.dust3r.inference as inf_mod
import align3r_amd.dust3r.cloud_opt.init_im_poses as init_mod
from align3r_amd.dust3r.cloud_opt_flow.optimizer import PointCloudOptimizer as FlowScene

ap = argparse.ArgumentParser()
ap.add_argument("n_frames", nargs="?", type=int, default=128)
ap.add_argument("--niter", type=int, default=300)
ap.add_argument("--clip-size", type=int, default=10)
ap.add_argument("--repeat", type=int, default=2, help="both modes, alternating, this many times: the run-to-run spread")
ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "hier_flow.json"))
args = ap.parse_args()
N, H, W, B = args.n_frames, 384, 512, 42
dev = torch.device("cuda:0")
torch.set_num_threads(8)
P = H * W
a, _ = synthetic_raft_frames(N, H, W, 9)                              # [N, 3, H, W] in [0, 255]
imgs = torch.from_numpy(a / 255.0 * 2 - 1).float()                    # ImgNorm range, host (what view['img'] holds)
frames = [(imgs[i].to(dev), torch.from_numpy((hash_uniform(f"pd{i}", P * 3, 1) + 0.5).astype(np.float32).reshape(H, W, 3)).to(dev)) for i in range(N)]
eng = PairEngine(VITL, synthetic_state_dict(VITL, 0), dev)
net = RAFT2(RAFT_M, synthetic_raft_state_dict(RAFT_M, 0)).to(dev)
stages = {}
scene_inits = []


def timed(name, fn):
    def wrapper(*a, **k):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn(*a, **k)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        stages[name] = stages.get(name, 0.0) + dt
        if name == "init":
            scene_inits.append(dt)
        return out
    return wrapper


def pair_forward(pairs, model, device, batch_size=1, verbose=False, keep_on_device=False):
    gi, gj = [int(p["instance"]) for p, q in pairs], [int(q["instance"]) for p, q in pairs]
    E = len(pairs)
    P1 = torch.empty(E, H, W, 3, device=dev); C1 = torch.empty(E, H, W, device=dev)
    P2 = torch.empty(E, H, W, 3, device=dev); C2 = torch.empty(E, H, W, device=dev)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for s0 in range(0, E, B):
        sl = slice(s0, min(s0 + B, E))
        eng.forward(torch.stack([frames[i][0] for i in gi[sl]]), torch.stack([frames[j][0] for j in gj[sl]]),
                    torch.stack([frames[i][1] for i in gi[sl]]), torch.stack([frames[j][1] for j in gj[sl]]),
                    out=dict(pts3d_1=P1[sl], conf_1=C1[sl], pts3d_2=P2[sl], conf_2=C2[sl]))
    torch.cuda.synchronize()
    t_fwd = time.perf_counter() - t0
    for k, (i, j) in enumerate(zip(gi, gj)):                           # untimed: consistent synthetic geometry
        p1, p2, cf = synthetic_pair_geometry(i, j, H, W, dev)
        P1[k], P2[k], C1[k], C2[k] = p1, p2, cf, cf
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    if not keep_on_device:                                             # what inference() does by default (to_cpu)
        P1, C1, P2, C2 = P1.cpu(), C1.cpu(), P2.cpu(), C2.cpu()
    stages["pairs"] = stages.get("pairs", 0.0) + t_fwd + (time.perf_counter() - t0)
    return dict(view1=dict(idx=[p["idx"] for p, q in pairs], img=imgs[gi]), view2=dict(idx=[q["idx"] for p, q in pairs], img=imgs[gj]),
                pred1=dict(pts3d=P1, conf=C1), pred2=dict(pts3d_in_other_view=P2, conf=C2))


inf_mod.inference = pair_forward
FlowScene.get_flow = timed("flow", FlowScene.get_flow)
FlowScene.get_motion_mask_from_pairs = timed("masks", FlowScene.get_motion_mask_from_pairs)
FlowScene._run_and_report = timed("loop", FlowScene._run_and_report)
init_mod.init_minimum_spanning_tree = timed("init", init_mod.init_minimum_spanning_tree)

result = dict(workload=dict(n_frames=N, H=H, W=W, clip_size=hz.choose_clip_size(N, args.clip_size), niter=args.niter,
                            weights="synthetic ViT-L + RAFT2 (RAFT_M)", device=torch.cuda.get_device_name(0)), modes={})
run_pair = lambda: pair_forward([(dict(idx=0, instance="0"), dict(idx=1, instance="1"))], None, dev, keep_on_device=True)
run_pair()                                                             # first-call costs of the pair forward stay outside both modes
result["runs"] = []
for mode, resident in [("host_resident", False), ("device_resident", True)] * args.repeat:
    stages.clear(); scene_inits.clear()
    views = [dict(idx=i, instance=str(i), true_shape=np.int32([[H, W]])) for i in range(N)]
    torch.manual_seed(0)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    res = hz.hierarchical_alignment(views, None, dev, clip_size=args.clip_size, niter=args.niter, schedule="linear", lr=0.01,
                                    flow=dict(flow_net=net), device_resident=resident)
    torch.cuda.synchronize()
    total = time.perf_counter() - t0
    assert len(res["depths"]) == N and all(np.isfinite(d).all() for d in res["depths"])
    rec = {f"{k}_s": round(v, 4) for k, v in stages.items()}
    rec["total_s"] = round(total, 4)
    rec["other_s"] = round(total - sum(stages.values()), 4)
    rec["init_key_s"] = round(scene_inits[0], 4)
    rec["init_clip_s"] = round(float(np.mean(scene_inits[1:])), 4)
    rec["init_clip_first_s"], rec["init_clip_last_s"] = round(scene_inits[1], 4), round(scene_inits[-1], 4)
    rec["n_scenes"] = len(scene_inits)
    result["modes"].setdefault(mode, rec)                               # the first run of each mode; every run is in `runs`
    result["runs"].append(dict(rec, mode=mode))
    print(mode, json.dumps(rec), flush=True)
os.makedirs(os.path.dirname(args.out), exist_ok=True)
with open(args.out, "w") as f:
    json.dump(result, f, indent=1, sort_keys=True)
print(json.dumps(result))
