"""CPU: the MST-initialisation fixture (tests/golden/mst.npz / .json, make_goldens_mst.py) is only as good as the stand-in that sits
inside it -- roma.rigid_points_registration is restated by this project, inside a "reference" golden -- and as the scenes are
discriminating.  Both are checked here, without a GPU and without the reference tree."""
import json
import os
import sys

import numpy as np
import pytest
import torch

from conftest import GOLDEN

sys.path.insert(0, GOLDEN)
from make_goldens_mst import rigid_points_registration          # noqa: E402  (numpy / torch only at import time)

META = json.load(open(os.path.join(GOLDEN, "mst.json")))
CASES = {c["tag"]: c for c in META["cases"]}


def _rot(rng):
    q = rng.standard_normal(4)
    x, y, z, w = q / np.linalg.norm(q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def _umeyama_numpy(x, y, w, scaling=True):
    """Independent float64 formulation (Umeyama 1991, eq. 34-42, with weights): per-point loops of outer products, numpy SVD."""
    w = w / w.sum()
    mx, my = sum(wi * xi for wi, xi in zip(w, x)), sum(wi * yi for wi, yi in zip(w, y))
    cov = sum(wi * np.outer(yi - my, xi - mx) for wi, xi, yi in zip(w, x, y))
    var = sum(wi * float((xi - mx) @ (xi - mx)) for wi, xi in zip(w, x))
    U, D, Vt = np.linalg.svd(cov)
    S = np.diag([1.0, 1.0, np.sign(np.linalg.det(U) * np.linalg.det(Vt))])
    R = U @ S @ Vt
    s = np.trace(np.diag(D) @ S) / var if scaling else 1.0
    return R, my - s * R @ mx, s


def test_standin_recovers_an_exact_similarity():
    rng = np.random.default_rng(0)
    for k in range(4):
        R, T, s = _rot(rng), rng.standard_normal(3), 0.3 + 2 * rng.random()
        x = rng.standard_normal((50, 3))
        y = s * x @ R.T + T
        w = 0.1 + rng.random(50)
        Rg, Tg, sg = rigid_points_registration(torch.from_numpy(x), torch.from_numpy(y), weights=torch.from_numpy(w), compute_scaling=True)
        assert Rg.dtype == torch.float64
        assert np.abs(Rg.numpy() - R).max() < 1e-12 and np.abs(Tg.numpy() - T).max() < 1e-12 and abs(float(sg) - s) < 1e-12
        R1, T1, s1 = rigid_points_registration(torch.from_numpy(x), torch.from_numpy(x @ R.T + T), weights=torch.from_numpy(w))
        assert float(s1) == 1.0 and np.abs(R1.numpy() - R).max() < 1e-12 and np.abs(T1.numpy() - T).max() < 1e-12
    x32 = torch.from_numpy(x).float()                                 # input dtype out
    assert all(t.dtype == torch.float32 for t in rigid_points_registration(x32, x32, compute_scaling=True))


def test_standin_agrees_with_independent_numpy_formulation():
    """Noisy, weighted, non-exact problems: the optimum itself, not only the noiseless case."""
    rng = np.random.default_rng(1)
    for k in range(4):
        x = rng.standard_normal((40, 3)) * [1.0, 0.5, 2.0]
        y = (0.7 + k) * x @ _rot(rng).T + rng.standard_normal(3) + 0.2 * rng.standard_normal((40, 3))
        w = rng.random(40) ** 2
        for scaling in (True, False):
            R, T, s = rigid_points_registration(torch.from_numpy(x), torch.from_numpy(y), weights=torch.from_numpy(w), compute_scaling=scaling)
            Rn, Tn, sn = _umeyama_numpy(x, y, w, scaling)
            assert np.abs(R.numpy() - Rn).max() < 1e-12 and np.abs(T.numpy() - Tn).max() < 1e-12 and abs(float(s) - sn) < 1e-12


def test_standin_returns_a_rotation_where_the_optimum_is_a_reflection():
    rng = np.random.default_rng(2)
    x = rng.standard_normal((30, 3))
    y = x * [1.0, 1.0, -1.0] + 0.01 * rng.standard_normal((30, 3))         # a mirror image: the unconstrained optimum has det = -1
    xm, ym = x - x.mean(0), y - y.mean(0)
    U, _, Vt = np.linalg.svd(ym.T @ xm)
    assert np.linalg.det(U @ Vt) < 0                                        # without the determinant fix: a reflection
    R, T, s = rigid_points_registration(torch.from_numpy(x), torch.from_numpy(y), compute_scaling=True)
    R = R.numpy()
    assert abs(np.linalg.det(R) - 1) < 1e-12 and np.abs(R @ R.T - np.eye(3)).max() < 1e-12
    Rn, Tn, sn = _umeyama_numpy(x, y, np.ones(30))
    assert np.abs(R - Rn).max() < 1e-12 and abs(float(s) - sn) < 1e-12 and float(s) > 0


def test_standin_without_weights_is_the_uniform_weight_result():
    rng = np.random.default_rng(3)
    x, y = torch.from_numpy(rng.standard_normal((25, 3))), torch.from_numpy(rng.standard_normal((25, 3)))
    a = rigid_points_registration(x, y, compute_scaling=True)                # how align_multiple_poses calls it
    b = rigid_points_registration(x, y, weights=torch.full((25,), 3.0, dtype=torch.float64), compute_scaling=True)
    for u, v in zip(a, b):
        assert np.abs(u.numpy() - v.numpy()).max() < 1e-14


# ------------------------------------------------------------------------------------------------ the fixture
@pytest.fixture(scope="module")
def g():
    return np.load(os.path.join(GOLDEN, "mst.npz"))


def test_fixture_names_its_standins():
    for word in ("rigid_points_registration", "rotmat_to_unitquat", "fast_pnp", "not pinned"):
        assert word in META["note"]
    assert {c["tag"] for c in META["cases"]} == {"swin", "complete", "ragged", "priors_i", "priors_j", "preset2", "flow", "flow_shared"}


@pytest.mark.parametrize("tag", sorted(CASES))
def test_fixture_scores_are_separated(g, tag):
    """The tree is pinned exactly, so no two edge scores may be within fp32 noise of each other."""
    s = np.sort(g[f"{tag}_scores"])
    gap = float(((s[1:] - s[:-1]) / s[1:]).min())
    assert gap >= META["min_score_gap"] == 1e-3 and abs(gap - CASES[tag]["score_gap"]) < 1e-9


def test_fixture_scenes_are_discriminating(g):
    """Per-image focals at least 5 % apart (the stale-`i_j` focal quirk then changes numbers), the quirk visible in `swin`, the
    'try again later' branch taken in `complete`, both init_priors branches, the sides' confidences independent."""
    for name, sc in META["scenes"].items():
        if sc["cam_focals"] is None:          # the flow scene is make_goldens._flow_scene as it stands: one focal for all its cameras
            assert name == "f4"
            continue
        f = np.sort(np.asarray(sc["cam_focals"]))
        assert np.all(f[1:] / f[:-1] >= 1.05), (name, f)
        c1, c2 = g[f"{name}_c1_0"], g[f"{name}_c2_0"]
        assert c1.shape != c2.shape or not np.array_equal(c1, c2)
    f = g["swin_mst_focals"]
    assert len(np.unique(f)) < len(f), f                                   # two images carry the identical (stale) focal
    assert CASES["complete"]["retry_triggered"]
    assert CASES["priors_i"]["tree"][0][:2] == [0, 2] and CASES["priors_j"]["tree"][0][:2] == [3, 0]
    assert CASES["preset2"]["known_poses"] == [False, True, False, True] and not CASES["preset2"]["norm_pw_scale"]
    assert len(set(tuple(s) for s in META["scenes"]["r4"]["shapes"])) > 1


@pytest.mark.parametrize("tag", sorted(CASES))
def test_fixture_case_is_complete(g, tag):
    c = CASES[tag]
    sc = META["scenes"][c["scene"]]
    N, E = len(sc["shapes"]), len(sc["edges"])
    assert len(c["pnp"]) >= 1                                              # the reference always reaches the PnP step
    assert len(c["tree"]) == N - 1 and c["tree"][0][2:] == [True, True] and all(a != b for _, _, a, b in c["tree"][1:])
    assert len(c["factors"]) == E and len(set(c["factors"])) == E
    P = max(h * w for h, w in sc["shapes"])
    assert g[f"{tag}_scores"].shape == (E,) and g[f"{tag}_mst_pts3d"].shape == (N, P, 3) and g[f"{tag}_depth"].shape == (N, P)
    assert g[f"{tag}_pw_poses_4x4"].shape == (E, 4, 4) and g[f"{tag}_im_poses_4x4"].shape == (N, 4, 4)
    # images that PnP was asked for fell back to the identity (or keep their preset), all others got a pose from the tree
    for call in c["pnp"]:
        assert np.array_equal(g[f"{tag}_mst_poses"][call["index"]], np.eye(4))
    assert c["float64_expectations"] == (not c["priors"])                  # init_priors: the reference casts the key pose to float32
    assert all(np.isfinite(v) and v < 1e-5 for v in c["spread"].values()), c["spread"]
