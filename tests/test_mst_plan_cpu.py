"""CPU: what init='mst' decides from the edge scores alone -- plan_spanning_tree, the one walk both executors of
align3r_amd/dust3r/cloud_opt/init_im_poses.py run -- against the reference's own walk as tests/golden/mst.json recorded it, and
the package's one rotation-matrix -> quaternion routine (commons.rotmats_to_unitquats).  No device, no native library."""
import copy
import json
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN

from align3r_amd.dust3r.cloud_opt.commons import rotmat_to_unitquat, rotmats_to_unitquats, unitquat_to_rotmat
from align3r_amd.dust3r.cloud_opt.init_im_poses import plan_spanning_tree, print_tree_lines

META = json.load(open(os.path.join(GOLDEN, "mst.json")))
CASES = {c["tag"]: c for c in META["cases"]}


@pytest.fixture(scope="module")
def g():
    return np.load(os.path.join(GOLDEN, "mst.npz"))


def _plan(g, tag):
    case = CASES[tag]
    sc = META["scenes"][case["scene"]]
    edges = [tuple(e) for e in sc["edges"]]
    scores = {e: float(s) for e, s in zip(edges, g[f"{tag}_scores"])}
    return plan_spanning_tree(len(sc["shapes"]), edges, scores, case["priors"]), edges, scores


# ------------------------------------------------------------------------------------------------ the plan
@pytest.mark.parametrize("tag", sorted(CASES))
def test_plan_is_the_reference_walk(g, tag):
    case = CASES[tag]
    plan, edges, _ = _plan(g, tag)
    N = len(META["scenes"][case["scene"]]["shapes"])
    assert [[i, j, a, b] for _, i, j, a, b in plan.lines] == case["tree"]
    assert plan.missing == [p["index"] for p in case["pnp"]]
    assert [n not in plan.focal_src for n in range(N)] == np.isnan(g[f"{tag}_mst_focals"]).tolist()
    assert plan.keyed == case["priors"]
    if not case["priors"]:                                   # the fixture's flag compares the walk with the score order of the tree
        assert (plan.requeued > 0) == case["retry_triggered"]
    # the record is consistent with itself: every image is placed once, poses come from steps that exist
    i, j, k0 = plan.root
    assert edges[k0] == (i, j) and plan.lines[0][1:] == (i, j, True, True)
    placed = [img for _, _, img in plan.root_maps] + [new for _, _, _, new in plan.steps]
    assert sorted(placed) == list(range(N)) and len(plan.steps) == N - 2 == len(plan.lines) - 1
    for t, (k, side, known, new) in enumerate(plan.steps):
        assert (edges[k][side], edges[k][1 - side]) == (known, new) and known in placed[:t + 2]
    for img, src in plan.pose_src.items():
        assert src in ("eye", "key") or edges[plan.steps[src][0]][0] == img        # keyed by the edge's FIRST image
    assert sorted(set(range(N)) - set(plan.pose_src)) == plan.missing
    for img, src in plan.focal_src.items():
        assert src == "key" or 0 <= src < len(edges)


def test_plan_requeues_in_complete(g):
    assert CASES["complete"]["retry_triggered"] and _plan(g, "complete")[0].requeued > 0


def test_plan_keeps_the_stale_focal_quirk(g):
    """`swin`: two images take the focal of ONE edge (the reference reads the previous edge's map), and that edge's first view is
    not the second of them -- the same two images that carry identical focals in the fixture."""
    plan, edges, _ = _plan(g, "swin")
    by_edge = {}
    for img, k in plan.focal_src.items():
        by_edge.setdefault(k, []).append(img)
    shared = [imgs for imgs in by_edge.values() if len(imgs) > 1]
    assert len(shared) == 1 and len(shared[0]) == 2
    f = g["swin_mst_focals"]
    assert f[shared[0][0]] == f[shared[0][1]]
    (k,) = [k for k, imgs in by_edge.items() if len(imgs) > 1]
    assert any(edges[k][0] != img for img in shared[0])


def test_plan_roots_at_image0_under_priors(g):
    plan, edges, _ = _plan(g, "priors_i")
    i, j, k0 = plan.root
    assert (i, j) == (0, 2) and plan.pose_src[0] == "key" and plan.focal_src[0] == "key"
    assert plan.root_maps == ((0, k0, 0), (1, k0, 2))                       # side i and side j of the root edge itself
    plan, edges, _ = _plan(g, "priors_j")
    i, j, k0 = plan.root
    kk = edges.index((0, 3))
    assert (i, j) == (3, 0) and plan.pose_src[0] == "key" and plan.pose_src.get(3) not in ("eye", "key")
    assert plan.root_maps == ((1, kk, 3), (0, kk, 0))                       # side j and side i of the REVERSE edge (0, 3)
    # without priors the root is the best edge, its first image the identity, its focal the root edge's
    plan, edges, scores = _plan(g, "complete")
    i, j, k0 = plan.root
    assert (i, j) == max(scores, key=scores.get) and plan.pose_src[i] == "eye" and plan.focal_src[i] == k0 and not plan.keyed
    assert plan.root_maps == ((0, k0, i), (1, k0, j))


@pytest.mark.parametrize("tag", sorted(CASES))
def test_plan_is_a_function_of_its_arguments(g, tag):
    case = CASES[tag]
    sc = META["scenes"][case["scene"]]
    edges = [tuple(e) for e in sc["edges"]]
    scores = {e: float(s) for e, s in zip(edges, g[f"{tag}_scores"])}
    before, order = copy.deepcopy(scores), list(scores)
    a = plan_spanning_tree(len(sc["shapes"]), edges, scores, case["priors"])
    b = plan_spanning_tree(len(sc["shapes"]), [list(e) for e in edges], scores, case["priors"])
    assert a == b
    assert scores == before and list(scores) == order


def test_plan_lines_print_as_the_reference_prints_them(g, capsys):
    plan, _, _ = _plan(g, "complete")
    print_tree_lines(plan)
    text = capsys.readouterr().out.splitlines()
    assert len(text) == len(plan.lines)
    for line, (score, i, j, a, b) in zip(text, plan.lines):
        assert line == f" init edge ({i}{'*' if a else ''},{j}{'*' if b else ''}) {score=}"


# ------------------------------------------------------------------------------------------------ the quaternion routine
def _rotations():
    """float32-rounded rotations: 64 random ones plus half turns about x, y, z and about a tilted axis, so that every branch of the
    largest-component rule is taken."""
    rng = np.random.default_rng(0)
    q = rng.standard_normal((64, 4))
    q = np.concatenate((q, [[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, 0], [0.1, 0.9, 0.2, 0.01], [0.2, 0.1, 0.9, -0.01], [0.9, 0.1, 0.2, 0.0]]))
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    return unitquat_to_rotmat(torch.from_numpy(q)).float().numpy()


def _branch(R):
    R = R.astype(np.float64)
    if R[0, 0] + R[1, 1] + R[2, 2] > 0:
        return 0
    if R[0, 0] > R[1, 1] and R[0, 0] > R[2, 2]:
        return 1
    return 2 if R[1, 1] > R[2, 2] else 3


def test_quaternions_cover_every_branch_and_round_trip():
    R = _rotations()
    assert {_branch(r) for r in R} == {0, 1, 2, 3}
    q = rotmats_to_unitquats(R)
    assert q.dtype == np.float32 and q.shape == (len(R), 4)
    assert np.abs(np.linalg.norm(q.astype(np.float64), axis=1) - 1).max() < 1e-6
    back = unitquat_to_rotmat(torch.from_numpy(q).double()).numpy()
    assert np.abs(back - R).max() < 1e-6                      # float32 rounding of a unit quaternion
    for b in range(4):                                        # each branch's rows on their own, too
        rows = [n for n, r in enumerate(R) if _branch(r) == b]
        assert np.abs(back[rows] - R[rows]).max() < 1e-6


def test_single_matrix_wrapper_is_a_row_of_the_batch():
    R = _rotations()
    q = rotmats_to_unitquats(R)
    for n in range(len(R)):
        for arg in (torch.from_numpy(R[n]), R[n], R[n].tolist()):
            one = rotmat_to_unitquat(arg)
            assert one.dtype == torch.float32 and one.device.type == "cpu" and one.shape == (4,)
            assert np.array_equal(one.numpy(), q[n])
