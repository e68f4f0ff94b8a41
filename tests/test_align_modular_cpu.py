"""CPU (no GPU): the host side of the ModularPointCloudOptimizer -- preset-mask normalisation, the loss-weight factor that turns
the stacked loss into the reference's mean of per-image means, and the consistency of tests/golden/alignmod.* with its
generator (regenerated bit for bit when the reference checkout is present)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import GOLDEN, REPO

META = json.load(open(os.path.join(GOLDEN, "alignmod.json")))
CASES = {c["tag"]: c for c in META["cases"]}
REFERENCE = "/root/reference"


@pytest.fixture(scope="module")
def g():
    return np.load(os.path.join(GOLDEN, "alignmod.npz"))


def _mask(m):
    if isinstance(m, str):
        kind, vals = m.split(":")
        vals = [int(v) for v in vals.split(",")]
        return np.asarray(vals, dtype=np.int64) if kind == "int64" else np.asarray(vals, dtype=bool)
    return m


def test_mask_normalisation_matches_the_reference_indices():
    from align3r_amd.dust3r.cloud_opt.modular_optimizer import msk_indices
    forms = set()
    for case in META["cases"]:
        N = len(case["shapes"])
        for p in case["presets"]:
            m = _mask(p["mask"])
            forms.add(type(m).__name__ + (":" + str(m.dtype) if isinstance(m, np.ndarray) else ""))
            assert msk_indices(m, N) == p["indices"], (case["tag"], p)
            if isinstance(m, np.ndarray):                 # the same mask as a torch tensor, a list and a tuple
                assert msk_indices(torch.from_numpy(m), N) == p["indices"]
                assert msk_indices(m.tolist(), N) == p["indices"]
                assert msk_indices(tuple(m.tolist()), N) == p["indices"]
    assert {"NoneType", "int", "list", "ndarray:bool", "ndarray:int64"} <= forms, forms      # every form is exercised by a golden
    assert msk_indices(None, 3) == [0, 1, 2] and msk_indices(2, 3) == [2] and msk_indices(np.int32(1), 3) == [1]
    assert msk_indices([False, True, True], 3) == [1, 2] and msk_indices(np.asarray([2, 0]), 3) == [2, 0]
    with pytest.raises(AssertionError):
        msk_indices([True, False], 3)                     # a boolean mask has one entry per image
    with pytest.raises(ValueError):
        msk_indices(np.asarray([0.5, 1.0]), 3)


def test_weight_factor_gives_the_per_edge_mean_loss(g):
    """loss0 of the reference = (1 / E) sum over edges of the two per-image MEANS.  The stacked kernels compute
    sum / total_area per side; with the factor folded into the weights the two agree, without it they do not (mixed shapes)."""
    from align3r_amd.dust3r.cloud_opt.modular_optimizer import edge_mean_factors
    for case in META["cases"]:
        tag, edges, shapes = case["tag"], [tuple(e) for e in case["edges"]], [tuple(s) for s in case["shapes"]]
        sums, E = g[f"{tag}_edge_sums"], len(edges)
        areas = [h * w for h, w in shapes]
        tot_i, tot_j = sum(areas[i] for i, j in edges), sum(areas[j] for i, j in edges)
        f_i, f_j = edge_mean_factors(edges, shapes)
        stacked = (f_i * sums[:, 0]).sum() / tot_i + (f_j * sums[:, 1]).sum() / tot_j
        plain = sums[:, 0].sum() / tot_i + sums[:, 1].sum() / tot_j
        loss0 = float(g[f"{tag}_loss0"])
        assert abs(stacked - loss0) / loss0 < 1e-6, (tag, stacked, loss0)          # fp32 loss of the reference against fp64 sums
        if len(set(shapes)) == 1:
            assert np.all(f_i == 1.0) and np.all(f_j == 1.0)
        else:
            assert abs(plain - loss0) / loss0 > 1e-3, (tag, plain, loss0)


def test_metadata_is_consistent_with_the_arrays(g):
    assert [c["tag"] for c in META["cases"]] == ["none", "pose1", "pose2", "intr", "mixed", "adapt"]
    for case in META["cases"]:
        tag, N, E = case["tag"], len(case["shapes"]), len(case["edges"])
        P = max(h * w for h, w in case["shapes"])
        assert g[f"{tag}_init_pw_poses"].shape == (E, 8) and g[f"{tag}_init_depth"].shape == (N, P)
        assert g[f"{tag}_init_im_poses"].shape == (N, 7) and g[f"{tag}_losses"].shape == (case["niter"],)
        for e, (i, j) in enumerate(case["edges"]):
            assert g[f"{case['inputs']}_p1_{e}"].shape == tuple(case["shapes"][i]) + (3,)
            assert g[f"{case['inputs']}_c2_{e}"].shape == tuple(case["shapes"][j])
        fz = {k: np.asarray(v) for k, v in case["frozen"].items()}
        want = {k: np.zeros(N, bool) for k in ("pose", "focal")}
        want["pp"] = np.full(N, not case["kw"].get("optimize_pp", False))
        for p in case["presets"]:
            for k in (("focal", "pp") if p["kind"] == "intrinsics" else (p["kind"],)):
                want[k][p["indices"]] = True
        for k in want:
            assert np.array_equal(fz[k], want[k]), (tag, k)
        assert case["norm_pw_scale"] == (fz["pose"].sum() <= 1)
        # frozen rows: zero gradient, start value kept through 50 iterations; free rows move
        for k, rows in (("im_poses", fz["pose"]), ("im_focals", fz["focal"]), ("im_pp", fz["pp"])):
            assert np.all(g[f"{tag}_grad_{k}"][rows] == 0)
            assert np.array_equal(g[f"{tag}_k50_{k}"][rows], g[f"{tag}_start_{k}"][rows])
            if (~rows).any():
                assert not np.array_equal(g[f"{tag}_k50_{k}"][~rows], g[f"{tag}_start_{k}"][~rows])
        # a preset writes the known value
        for p in case["presets"]:
            if p["kind"] in ("focal", "intrinsics"):
                got = np.exp(g[f"{tag}_start_im_focals"][p["indices"]] / 20)
                assert np.allclose(got, g[f"{tag}_known_focals"][p["indices"]], rtol=1e-5)
        assert np.isclose(g[f"{tag}_losses"][0], g[f"{tag}_loss0"], rtol=1e-6)
        assert g[f"{tag}_losses"][-1] < g[f"{tag}_losses"][0]


@pytest.mark.skipif(not os.path.isdir(os.path.join(REFERENCE, "dust3r", "cloud_opt")), reason="needs the reference checkout")
def test_generator_reproduces_the_committed_fixtures(tmp_path, g):
    """Every array bit for bit and the same JSON (the .npz container itself carries zip timestamps)."""
    env = dict(os.environ, PYTHONDONTWRITEBYTECODE="1")
    subprocess.run([sys.executable, os.path.join(GOLDEN, "make_goldens_modular.py"), "--out", str(tmp_path)], check=True, env=env,
                   stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, cwd=REPO)
    new = np.load(os.path.join(str(tmp_path), "alignmod.npz"))
    assert sorted(new.files) == sorted(g.files)
    for k in g.files:
        assert new[k].dtype == g[k].dtype and new[k].shape == g[k].shape and new[k].tobytes() == g[k].tobytes(), k
    assert json.load(open(os.path.join(str(tmp_path), "alignmod.json"))) == META
