"""CPU: the host pieces of the hierarchical pose pipeline (tool/pose_test.py --mode eval_pose_h) against the reference's own code
(tests/golden/hier_flow.json / .npz, make_goldens_hier_flow.py): the pair builder, the re-anchoring of a clip on its keyframe
pose, the command line, the option check of the driver, and the fixture's own claims about its init_priors cases."""
import json
import os
import types

import numpy as np
import pytest
import torch

from conftest import GOLDEN

from align3r_amd.tool import hierarchical as hz

META = json.load(open(os.path.join(GOLDEN, "hier_flow.json")))


@pytest.fixture(scope="module")
def g():
    return np.load(os.path.join(GOLDEN, "hier_flow.npz"))


def _rows(pairs):
    return [[a["instance"], a["idx"], b["instance"], b["idx"]] for a, b in pairs]


def test_my_make_pairs_pose_matches_reference():
    seen = 0
    for c in META["make_pairs"]:
        if c["clip_size"] is None:                       # the reference's clip-size loop divides by zero for this N
            with pytest.raises(ZeroDivisionError):
                hz.choose_clip_size(c["n"], 10)
            continue
        seen += 1
        assert hz.choose_clip_size(c["n"], 10) == c["clip_size"]
        imgs = [dict(idx=i, instance=f"f{i}") for i in range(c["n"])]
        coarse, kf, clips, ids = hz.my_make_pairs_pose(imgs, c["clip_size"])
        assert kf == c["keyframes_id"] and ids == c["all_clips_id"]
        assert _rows(coarse) == c["coarse"]
        assert [_rows(cl) for cl in clips] == c["clips"]
        assert [v["idx"] for v in imgs] == c["idx_after"]          # the in-place renumbering of the caller's dicts
        # the keyframe graph: complete and symmetrised, second half = first half reversed
        K = len(kf)
        ce = [(a["idx"], b["idx"]) for a, b in coarse]
        assert len(ce) == K * (K - 1) and set(ce) == {(i, j) for i in range(K) for j in range(K) if i != j}
        assert ce[len(ce) // 2:] == [(j, i) for i, j in ce[:len(ce) // 2]]
        # every clip graph: edge e + E/2 is the reverse of edge e, and every clip image is in a pair of the first half
        for cl, cid in zip(clips, ids):
            e = [(a["idx"], b["idx"]) for a, b in cl]
            half = len(e) // 2
            assert len(e) % 2 == 0 and half >= 1
            assert e[half:] == [(j, i) for i, j in e[:half]]
            assert {i for p in e[:half] for i in p} == set(range(len(cid)))
            assert e[:half] == [(i, j) for i in range(len(cid) - 1) for j in range(i + 1, len(cid), 2)]
    assert seen >= 5
    assert {c["n"] for c in META["make_pairs"]} >= {3, 5, 8, 12, 23}
    assert any(len(ids[-1]) == 2 for ids in (c["all_clips_id"] for c in META["make_pairs"] if c["clip_size"]))      # a two-frame last clip


def test_my_make_pairs_pose_copies_dicts_as_the_reference_does():
    imgs = [dict(idx=i, instance=f"f{i}") for i in range(8)]
    coarse, kf, clips, _ = hz.my_make_pairs_pose(imgs, 3)
    assert all(a is not imgs[k] for (a, b), k in zip(coarse, [0, 0, 3]))          # keyframes are copies ...
    assert coarse[0][0] is coarse[1][0] and coarse[3][1] is coarse[0][0]          # ... one copy per keyframe, shared by its pairs
    half = len(clips[0]) // 2
    assert clips[0][half][0] is clips[0][0][1] and clips[0][half][1] is clips[0][0][0]      # reversed pairs share the forward copies
    assert clips[0][0][0] is not clips[0][1][0]                                              # forward pairs copy per pair


def _stub(poses):
    from align3r_amd.dust3r.cloud_opt_flow.optimizer import PointCloudOptimizer as P
    s = types.SimpleNamespace(get_im_poses=lambda: torch.from_numpy(poses))
    s.align_poses = lambda a, b: P.align_poses(s, a, b)
    s.get_tum_poses = lambda k=None: P.get_tum_poses(s, k)
    return s


def test_re_anchoring_matches_reference(g):
    for rec in META["anchor"]:
        n = rec["name"]
        poses, key = g[f"{n}_poses"], g[f"{n}_key"]
        s = _stub(poses)
        got = s.align_poses(np.array(key.tolist()), poses.copy())
        assert got.dtype == poses.dtype == np.float32
        assert np.array_equal(got[0], key.astype(np.float32))              # frame 0 IS the key pose, bit for bit
        assert np.array_equal(got, g[f"{n}_aligned"])                      # numpy in the input dtype, the reference's expressions
        tum, tt = s.get_tum_poses(key.tolist())
        assert tum.shape == (rec["n"], 7) and np.allclose(tum, g[f"{n}_tum"], rtol=0, atol=1e-6)
        assert np.array_equal(tt, g[f"{n}_tt"])
        plain, _ = s.get_tum_poses()
        assert np.allclose(plain[:, :3], poses[:, :3, 3])                   # no key pose: the poses as they are


def test_run_clip_parses_flow_hierarchical():
    from align3r_amd.tool import run_clip
    base = ["--images", "x", "--weights", "w", "--out", "o"]
    a = run_clip.parse(base + ["--flow-hierarchical"])
    assert a.flow_hierarchical and a.clip_size == 10 and not a.device_resident and not a.flow and not a.hierarchical
    a = run_clip.parse(base + ["--flow-hierarchical", "--clip-size", "7", "--device-resident", "--flow-weights", "r-M.pth",
                               "--gt-masks", "m", "--not-shared-focal"])
    assert a.clip_size == 7 and a.device_resident and a.flow_weights == "r-M.pth" and a.gt_masks == "m" and a.not_shared_focal
    assert run_clip.parse(base + ["--hierarchical"]).clip_size == 50
    assert run_clip.parse(base).clip_size == 50
    for bad in (["--flow", "--hierarchical"], ["--flow-hierarchical", "--flow"], ["--flow-hierarchical", "--hierarchical"],
                ["--device-resident"], ["--hierarchical", "--device-resident"], ["--flow-weights", "r-M.pth"]):
        with pytest.raises(SystemExit):
            run_clip.parse(base + bad)


def test_driver_checks_flow_options_before_anything_is_loaded(monkeypatch):
    import align3r_amd.dust3r.inference as inf_mod

    def boom(*a, **k):
        raise AssertionError("inference was reached")
    monkeypatch.setattr(inf_mod, "inference", boom)
    with pytest.raises(ValueError, match="bogus"):
        hz.hierarchical_alignment([], None, "cuda", flow={"bogus": 1})
    with pytest.raises(ValueError, match="clamp_conf"):                  # the clamp is the depth pipeline's step, not this one's
        hz.hierarchical_alignment([], None, "cuda", flow={}, clamp_conf=True)
    with pytest.raises(ValueError, match="device_resident"):             # the plain driver has no device-resident mode
        hz.hierarchical_alignment([], None, "cuda", device_resident=True)
    with pytest.raises(ValueError, match="3 frames"):                    # no clip size exists (the reference divides by zero)
        hz.hierarchical_alignment([dict(idx=i) for i in range(3)], None, "cuda", flow={})
    assert set(hz.FLOW_DEFAULTS) == {"flow_loss_weight", "temporal_smoothing_weight", "translation_weight", "flow_loss_start_epoch",
                                     "flow_loss_thre", "pxl_thre", "motion_mask_thre", "depth_regularize_weight", "shared_focal",
                                     "use_self_mask", "flow_net", "flow_fn"}
    d = hz.FLOW_DEFAULTS
    assert (d["flow_loss_weight"], d["temporal_smoothing_weight"], d["translation_weight"], d["flow_loss_start_epoch"]) == (0.01, 0.01, 1.0, 0.1)
    assert (d["flow_loss_thre"], d["pxl_thre"], d["motion_mask_thre"], d["depth_regularize_weight"]) == (40, 50, 0.35, 0)
    assert d["shared_focal"] is True and d["use_self_mask"] is True


def test_fixture_mst_cases_run_the_reinsert_loop(g):
    """The three init_priors cases: the best edge of the graph does not touch image 0, so the reference popped and re-inserted at
    least one tree edge before it found its root; both root branches and both focal modes are present."""
    roots = set()
    for c in META["cases"]:
        sc = META["scenes"][c["scene"]]
        edges = [tuple(e) for e in sc["edges"]]
        scores = g[f"{c['tag']}_scores"]
        best = edges[int(np.argmax(scores))]
        assert 0 not in best and list(best) == c["best_edge"]
        i, j, si, sj = c["tree"][0]
        assert si and sj and (i == 0 or j == 0) and (i, j) != best
        tree_scores = [scores[edges.index((a, b))] for a, b, _, _ in c["tree"]]
        assert tree_scores[0] < max(tree_scores)                          # the root is not the tree's best edge
        roots.add(("i" if i == 0 else "j", bool(c["kw"]["shared_focal"])))
        assert not c["float64_expectations"] and c["priors"] and len(c["pnp"]) >= 1
        assert sc["shapes"] == [[12, 16]] * 4
        if c["kw"]["shared_focal"]:
            assert len(set(g[f"{c['tag']}_focals"].tolist())) == 1
        # image 0 carries the key pose (scaled translation) in what minimum_spanning_tree returned
        assert np.array_equal(g[f"{c['tag']}_mst_poses"][0], g[f"{c['scene']}_key_pose"].astype(np.float32).astype(np.float64))
    assert {r[0] for r in roots} == {"i", "j"} and {r[1] for r in roots} == {True, False}
