"""Goldens of the hierarchical pose pipeline (tool/pose_test.py --mode eval_pose_h, :346-479) -> tests/golden/hier_flow.json / .npz.

    python tests/golden/make_goldens_hier_flow.py [--out tests/golden]

Imports the helpers of make_goldens.py and make_goldens_mst.py and edits neither.  Three groups:
  * my_make_pairs of tool/pose_test.py:551-591 (compiled on its own with `ast`: the file imports cv2) for N in NS at the clip size
    the reference's rule (pose_test.py:379-380, start 10) ends on.  The rule divides by zero for some N (N = 3 is one): such an N is
    recorded with clip_size null and no pairs, every other N is asserted to end on a clip size;
  * align_poses / get_tum_poses(init_keypose) of cloud_opt_flow/base_opt.py:305-330 on two pose sets (fp32 poses, float64 key
    pose from a python list, as the pipeline passes it);
  * three init='mst' cases with init_priors on the flow class, in the layout of mst.npz (make_goldens_mst.run_reference does the
    work): a complete 4-image 12x16 scene whose best tree edge does NOT touch image 0, so the pop-and-reinsert loop of
    cloud_opt_flow/init_im_poses.py:176-181 runs, rooted through i == 0 and through j == 0, shared focal off and on.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import types

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import numpy as np
import torch

NS = (3, 5, 7, 8, 12, 23)
FLOW_KW = dict(temporal_smoothing_weight=0.01, depth_regularize_weight=0.0)
CASES = [
    dict(tag="hf_i", scene="h4", cls="flow", boost={(1, 3): 2.0, (0, 2): 1.8, (2, 1): 1.6}, priors=True, want_init=(0, 2),
         kw=dict(shared_focal=False, **FLOW_KW)),
    dict(tag="hf_j_shared", scene="h4", cls="flow", boost={(1, 2): 2.0, (3, 0): 1.8, (0, 1): 1.6}, priors=True, want_init=(3, 0),
         kw=dict(shared_focal=True, **FLOW_KW)),
    dict(tag="hf_i_shared", scene="h4", cls="flow", boost={(2, 3): 2.0, (0, 1): 1.8, (3, 1): 1.6}, priors=True, want_init=(0, 1),
         kw=dict(shared_focal=True, temporal_smoothing_weight=0.01, depth_regularize_weight=5.0)),
]


def gen_pairs(mg):
    mk = mg._ref_function("tool/pose_test.py", "my_make_pairs", {})
    cases = []
    for n in NS:
        cs = 10
        try:
            while n % cs == 1 or n % cs == 0 or cs > n:          # pose_test.py:379-380
                cs -= 1
        except ZeroDivisionError:
            cases.append(dict(n=n, clip_size=None))
            continue
        assert cs >= 2, (n, cs)
        imgs = [dict(idx=i, instance=f"f{i}") for i in range(n)]
        coarse, kf, clips, ids = mk(imgs, cs)
        cases.append(dict(n=n, clip_size=cs, keyframes_id=kf, all_clips_id=ids,
                          coarse=[[a["instance"], a["idx"], b["instance"], b["idx"]] for a, b in coarse],
                          clips=[[[a["instance"], a["idx"], b["instance"], b["idx"]] for a, b in cl] for cl in clips],
                          idx_after=[v["idx"] for v in imgs]))
    assert sum(c["clip_size"] is not None for c in cases) >= 5
    return cases


def _random_poses(rng, n):
    out = []
    for _ in range(n):
        q = rng.randn(4)
        x, y, z, w = q / np.linalg.norm(q)
        R = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                      [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                      [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])
        P = np.eye(4)
        P[:3, :3], P[:3, 3] = R, rng.randn(3)
        out.append(P.astype(np.float32))
    return np.stack(out)


def gen_anchor(g):
    from dust3r.cloud_opt_flow.base_opt import BasePCOptimizer
    rng = np.random.RandomState(5)
    sets = []
    for k, n in enumerate((4, 2)):
        poses = _random_poses(rng, n)
        key = _random_poses(rng, 1)[0].tolist()                  # a python list of float32 values, as to_numpy(...).tolist() gives
        stub = types.SimpleNamespace(get_im_poses=lambda poses=poses: torch.from_numpy(poses))
        stub.align_poses = lambda a, b: BasePCOptimizer.align_poses(stub, a, b)
        aligned = BasePCOptimizer.align_poses(stub, np.array(key), poses.copy())
        tum, tt = BasePCOptimizer.get_tum_poses(stub, key)
        g[f"anchor{k}_poses"], g[f"anchor{k}_key"] = poses, np.array(key)
        g[f"anchor{k}_aligned"], g[f"anchor{k}_tum"], g[f"anchor{k}_tt"] = aligned, tum, tt
        assert aligned.dtype == np.float32
        sets.append(dict(name=f"anchor{k}", n=n))
    return sets


def gen_mst(mm, g, meta):
    sc = mm.geom_scene([mm.SHAPE4] * 4, mm.COMPLETE4, seed=34)
    sc["dyn"] = np.random.default_rng(35).random((4,) + mm.SHAPE4) < 0.1
    sc["key_pose"] = mm.geom_scene([(16, 24)] * 5, [(0, 1)], seed=31)["cam_poses"][4].astype(np.float64)
    sc["key_depth"] = (3 + 0.1 * np.arange(mm.SHAPE4[0] * mm.SHAPE4[1], dtype=np.float32).reshape(mm.SHAPE4) / 192)
    sc["key_focal"] = 1.3 * max(mm.SHAPE4)
    name = "h4"
    for e in range(len(sc["edges"])):
        g[f"{name}_p1_{e}"], g[f"{name}_p2_{e}"], g[f"{name}_c1_{e}"], g[f"{name}_c2_{e}"] = sc["p1"][e], sc["p2"][e], sc["c1"][e], sc["c2"][e]
    g[f"{name}_dyn"], g[f"{name}_cam_poses"] = sc["dyn"], sc["cam_poses"]
    g[f"{name}_key_pose"], g[f"{name}_key_depth"] = sc["key_pose"], sc["key_depth"]
    meta["scenes"][name] = dict(shapes=[list(s) for s in sc["shapes"]], edges=[list(e) for e in sc["edges"]],
                                cam_focals=sc["cam_focals"], key_focal=sc["key_focal"])
    for k, case in enumerate(CASES):
        tag = case["tag"]
        factors = mm.edge_factors(sc["edges"], case["boost"], seed=200 + k)
        r32, f32 = mm.run_reference(case, sc, factors, f64=False)
        r64, f64 = mm.run_reference(case, sc, factors, f64=True)
        for key in ("tree", "norm_pw_scale", "known_poses"):
            assert f32[key] == f64[key], (tag, key)
        assert [(c["index"], c["msk_sum"]) for c in f32["pnp"]] == [(c["index"], c["msk_sum"]) for c in f64["pnp"]]
        assert not f64["all_float64"], tag                        # the key pose is cast to float32: fp32 expectations
        want = r32
        s = np.sort(want["scores"])
        gap = float(((s[1:] - s[:-1]) / s[1:]).min())
        assert gap >= mm.MIN_SCORE_GAP, (tag, gap)
        tree = f32["tree"]
        assert tuple(tree[0][:2]) == case["want_init"], (tag, tree)
        best = max(range(len(sc["edges"])), key=lambda e: want["scores"][e])
        assert 0 not in sc["edges"][best], (tag, sc["edges"][best])        # the reinsert loop ran
        assert len(f32["pnp"]) >= 1, tag
        for key, v in want.items():
            g[f"{tag}_{key}"] = v if key.startswith("init_") else np.asarray(v, np.float64)
        spread = {q: mm.rel_err(r32[q], r64[q]) for q in mm.QUANTITIES}
        spread["mst_focals"] = mm.rel_err(np.nan_to_num(r32["mst_focals"]), np.nan_to_num(r64["mst_focals"]))
        pnp = [dict(c, spread_pts=mm.rel_err(r32["mst_pts3d"][c["index"]], r64["mst_pts3d"][c["index"]]),
                    spread_focal=mm.rel_err(c["focal"], d["focal"])) for c, d in zip(f32["pnp"], f64["pnp"])]
        meta["cases"].append(dict(tag=tag, scene=name, cls="flow", kw=case["kw"], factors=factors, priors=True, preset=None, tree=tree,
                                  best_edge=list(sc["edges"][best]), pnp=pnp, score_gap=gap, float64_expectations=False, spread=spread,
                                  norm_pw_scale=f32["norm_pw_scale"], known_poses=f32["known_poses"]))
        print("hier_flow mst", tag, "tree", tree, "best", sc["edges"][best], "pnp", [c["index"] for c in pnp], "loss", float(want["loss"]))


def generate(out_dir):
    sys.dont_write_bytecode = True              # the reference tree is read-only
    import make_goldens as mg
    import make_goldens_mst as mm
    mg.import_reference(aligner=True)
    sys.modules["roma"].rigid_points_registration = mm.rigid_points_registration
    sys.modules["roma"].rotmat_to_unitquat = mm.rotmat_to_unitquat
    torch.set_num_threads(1)
    g = {}
    meta = dict(note="tool/pose_test.py my_make_pairs; cloud_opt_flow/base_opt.py align_poses / get_tum_poses; the reference's "
                     "init='mst' with init_priors on the flow class, stand-ins as in mst.json (fast_pnp a recorder returning None)",
                seed=mm.SEED, min_conf_thr=3, scenes={}, cases=[])
    meta["make_pairs"] = gen_pairs(mg)
    meta["anchor"] = gen_anchor(g)
    gen_mst(mm, g, meta)
    mm.write_npz(os.path.join(out_dir, "hier_flow.npz"), g)
    with open(os.path.join(out_dir, "hier_flow.json"), "w") as f:
        json.dump(meta, f, sort_keys=True)
    print("hier_flow.npz", os.path.getsize(os.path.join(out_dir, "hier_flow.npz")), "bytes")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=HERE)
    generate(ap.parse_args().out)
