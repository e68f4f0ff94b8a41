"""CPU: the oracles of tests/init_cases.py against ground truth and against independent formulations, and the cap conditions that
tests/test_gpu_init.py relies on (no point at the inlier threshold, oracles insensitive to the summation order, a unique winner of
every focal search).  They are asserted here, for every problem of the GPU batch, so that the GPU comparison needs no exception:
it compares every scene."""
import numpy as np
import pytest
import torch

import init_cases as ic
from conftest import record_margin
from test_mst_golden_cpu import _umeyama_numpy

# c2w of the oracle against the truth on clean scenes.  What separates them is the fp32 rounding of the world points (relative
# 2^-24 = 6e-8 on coordinates of size 3, averaged over the points used): measured 4.1e-9 (129x128, 8256 points), 6.3e-9 (with pp),
# 1.3e-8 (759 points), 2.1e-8 (210 points in three rows), 3.1e-8 (35 points).  Asserted at 10 x the largest.
CLEAN_TRUTH_TOL = 3.1e-7


@pytest.fixture(scope="module")
def batch():
    return ic.pnp_scenes(), ic.pnp_problems(), {it: ic.pnp_expected(it) for it in ic.PNP_ITERATIONS}


def test_pnp_oracle_recovers_the_truth(batch):
    scenes, problems, expected = batch
    worst = {}
    for (name, _), r in zip(problems, expected[10]):
        sc = scenes[name]
        dev = float(np.abs(r["c2w"] - sc["truth"]).max())
        print(f"{name}: used {r['used']}, step {r['step']}, |c2w - truth| = {dev:.3g}")
        if sc["kind"] == "clean":
            assert r["valid"] and r["inliers"] == r["used"] and dev < CLEAN_TRUTH_TOL, (name, dev)
            worst["clean"] = max(worst.get("clean", 0.0), dev)
        elif sc["kind"] in ("outliers20", "outliers40"):
            assert r["valid"] and dev < {"outliers20": 3e-2, "outliers40": 8e-2}[sc["kind"]], (name, dev)
            worst[sc["kind"]] = dev
    assert set(worst) == {"clean", "outliers20", "outliers40"}
    record_margin("init_pnp_oracle_vs_truth", **worst)
    # the subsample and the shapes the GPU batch is meant to hold
    steps = {name: r["step"] for (name, _), r in zip(problems, expected[10])}
    assert steps["129x128_step2"] == 2 and steps["150x230_step3_out20"] == 3 and expected[10][0]["used"] == 8256
    assert len(problems) > 64 and len({scenes[n]["pts"].shape for n, _ in problems}) >= 6
    assert len({ic.pnp_sample(*scenes[n]["pts"].shape[:2], scenes[n]["mask"])[1] for n, _ in problems}) >= 6      # n < n_max for most


def test_pnp_invalid_scenes_are_invalid_for_the_stated_reason(batch):
    scenes, problems, expected = batch
    for it in ic.PNP_ITERATIONS:
        by_name = {name: r for (name, _), r in zip(problems, expected[it])}
        few, away = by_name["37x41_five_pixels"], by_name["37x41_looking_away"]
        assert few["used"] == 5 and few["front"] == 5 and not few["valid"]
        assert away["used"] == 1517 and away["front"] < 0.5 * away["used"] and not away["valid"]
    # the solver itself is sound on both: the five pixels give the true pose, the rim of the looking-away camera does too
    assert np.abs(by_name["37x41_five_pixels"]["c2w"] - scenes["37x41_five_pixels"]["truth"]).max() < 1e-5
    assert np.abs(by_name["37x41_looking_away"]["c2w"] - scenes["37x41_looking_away"]["truth"]).max() < CLEAN_TRUTH_TOL
    assert by_name["37x41_looking_away"]["front"] == int((~scenes["37x41_looking_away"]["behind"]).sum())


def test_pnp_cap_conditions(batch):
    """Inlier boundary and conditioning, for every problem of the batch at every iteration count the GPU test runs."""
    scenes, problems, expected = batch
    gap, spread = np.inf, 0.0
    for it in ic.PNP_ITERATIONS:
        for (name, f), r in zip(problems, expected[it]):
            sc = scenes[name]
            assert r["gap"] > ic.BOUNDARY_GAP, (name, f, it, r["gap"])
            gap = min(gap, r["gap"])
            for k in range(4):
                o = ic.pnp_oracle(sc["pts"], sc["mask"], f, sc["pp"], it, order=np.random.default_rng(1000 + k))
                dev = float(np.abs(o["c2w"] - r["c2w"]).max())
                assert dev < ic.PNP_SPREAD_CAP and o["inliers"] == r["inliers"] and o["valid"] == r["valid"], (name, f, it, dev)
                assert abs(o["err"] - r["err"]) <= 1e-9 * max(r["err"], 1e-30)      # 500 times below the 4 fp32 ulp of the GPU test
                spread = max(spread, dev)
    record_margin("init_pnp_caps", smallest_gap_px=gap, largest_order_spread=spread)


def test_focal_search_has_a_unique_winner(batch):
    """linear_pnp_many compares fp32 copies of the inlier count and the truncated error: the oracle's winner has to lead by a whole
    inlier or by far more than the 4 ulp the error may move."""
    scenes, problems, expected = batch
    for it in ic.PNP_ITERATIONS:
        for name in ic.SEARCH:
            res = [r for (n, _), r in zip(problems, expected[it]) if n == name]
            assert len(res) == 21
            k, margin = ic.pnp_search_pick(res)
            assert k is not None and margin > 1e-4, (name, it, k, margin)
            if it == 10:                                              # the winner is a neighbour of the true focal
                H, W, _ = scenes[name]["pts"].shape
                cands = ic.pnp_focal_candidates(H, W)
                f = scenes[name]["true_focal"]
                assert res[k]["focal"] in (np.float32(max(c for c in cands if c <= f)), np.float32(min(c for c in cands if c >= f))), (name, k)


def test_pnp_oracle_sample_matches_the_package():
    from align3r_amd.dust3r.cloud_opt import init_im_poses as iip
    assert iip.PNP_MAX_POINTS == ic.PNP_MAX_POINTS
    assert iip.pnp_focal_candidates(33, 70) == ic.pnp_focal_candidates(33, 70)
    for H, W, step, n in ((129, 128, 2, 8256), (150, 230, 3, 11500), (128, 128, 1, 16384), (5, 7, 1, 35)):
        assert ic.pnp_sample(H, W, np.ones((H, W), bool))[:2] == (step, n)
        assert (n - 1) * step < H * W                                  # the last sampled pixel is inside the map


# ------------------------------------------------------------------------------------------------ Umeyama
def test_umeyama_oracle_equals_an_independent_kabsch_and_the_package():
    """Scenes (b) to (e) against _umeyama_numpy (centred per-point outer products); every scene against the package's
    _solve_from_moments fed with the oracle's moments.  The centred form does not cancel, so where the raw moments do (collinear,
    far centroid) the two may differ by the raw form's conditioning: the measured order spread, times 16."""
    from align3r_amd.dust3r.cloud_opt.init_im_poses import _solve_from_moments
    scenes, expected = ic.umeyama_scenes(), ic.umeyama_expected()
    for name in ("b_mirror", "c_coplanar", "d_collinear", "e_far"):
        sc = scenes[name]
        want, spread = expected[name]
        x, y, w = (sc[k][0].astype(np.float64) for k in "XYW")
        R, T, s = _umeyama_numpy(x, y, w)
        dev = np.abs(ic.pack_sRT(s, R, T) - want[0]) / np.maximum(1, np.abs(want[0]))
        print(f"{name}: oracle vs centred Kabsch {dev.max():.3g}, order spread {spread[0]:.3g}")
        assert dev.max() < max(1e-11, 16 * spread[0]), (name, dev.max(), spread[0])
    for name, sc in scenes.items():
        want, _ = expected[name]
        m = np.stack([ic.moments17(*(a.astype(np.float64) for a in (sc["X"][e], sc["Y"][sc["y_index"][e]], sc["W"][e]))) for e in range(len(want))])
        for e, (s, R, T) in enumerate(_solve_from_moments(torch.from_numpy(m))):
            got = ic.pack_sRT(s, R.numpy(), T.numpy())
            assert np.abs(got - want[e]).max() <= 2.0 ** -23 * np.maximum(1, np.abs(want[e])).max(), (name, e)      # its fp32 cast


def test_umeyama_scenes_are_what_they_claim():
    scenes, expected = ic.umeyama_scenes(), ic.umeyama_expected()
    assert [n for n in scenes if n.startswith("a_")] == [f"a_generic_P{P}" for P in ic.GENERIC_P] and {1023, 1024, 1025} <= set(ic.GENERIC_P)
    for name, (want, _) in expected.items():
        R = want[:, 1:10].reshape(-1, 3, 3)
        o, d = ic.ortho_err(R)
        assert o < 1e-12 and d < 1e-12 and np.isfinite(want).all() and (want[:, 0] > 0).all(), name
    # (b): without the determinant fix the optimum is a reflection
    sc = scenes["b_mirror"]
    x, y, w = (sc[k][0].astype(np.float64) for k in "XYW")
    m = ic.moments17(x, y, w)
    cov = m[8:17].reshape(3, 3) / m[0] - np.outer(m[4:7], m[1:4]) / m[0] ** 2
    U, S, Vt = np.linalg.svd(cov)
    assert np.linalg.det(U @ Vt) < 0 and S[2] > 0.1 * S[0]
    # (c) coplanar: rank 2;  (d) nearly collinear: two singular values 1e-6 of the first
    for name, lo, hi in (("c_coplanar", 0.0, 1e-12), ("d_collinear", 1e-7, 1e-5)):
        sc = scenes[name]
        x, y, w = (sc[k][0].astype(np.float64) for k in "XYW")
        S = np.linalg.svd(np.cov(x.T, aweights=w), compute_uv=False)
        assert lo <= S[2] / S[0] <= hi and (name != "d_collinear" or S[1] / S[0] <= hi), (name, S)
    assert (scenes["c_coplanar"]["X"][..., 2] == 0).all()
    far = scenes["e_far"]["X"][0].astype(np.float64)
    assert np.abs(far.mean(0) - [300, -200, 500]).max() < 0.1 and np.abs(far.std(0) - 1).max() < 0.1
    f = scenes["f_zero_weights"]
    assert (f["W"][0] == 0).sum() == ic.SPECIAL_P // 2 and np.abs(f["X"][0][f["dead"]]).min() > 1 and np.isfinite(f["X"]).all() and np.isfinite(f["Y"]).all()
    g = scenes["g_batch130"]
    assert g["X"].shape == (130, 64, 3) and g["Y"].shape[0] == 7 and set(g["y_index"]) == set(range(7))


def test_umeyama_cap_conditions():
    """Order spread of the oracle: below 1e-10 relative wherever the GPU test compares at 2 fp32 ulp.  The nearly collinear and the
    far-centroid scene are ill-conditioned IN THE RAW MOMENTS (var_x and cov are differences of sums 1e6 times their size), which is
    what they are there to exercise and what the kernel computes too: measured 2.3e-10 and 1.9e-7.  Their GPU bound is max(2 ulp,
    16 x this spread); the cap on them is that this stays three orders below what a single fp32 accumulator would do (1e-2)."""
    spreads = {}
    for name, (want, spread) in ic.umeyama_expected().items():
        spreads[name] = float(spread.max())
        if name in ic.LOOSE:
            assert 16 * spread.max() < 1e-5, (name, spread.max())
        else:
            assert spread.max() < ic.UME_SPREAD_CAP, (name, spread.max())
    record_margin("init_umeyama_order_spread", **spreads)


# ------------------------------------------------------------------------------------------------ Weiszfeld, depth
def test_weiszfeld_oracles():
    """The numpy float64 restatement equals the package's generic path (the float64 reference of the GPU test); the fp32
    restatement of the kernel stays within an ulp of it; both see the planted focals and the four special pixels."""
    from align3r_amd.dust3r.cloud_opt.init_im_poses import estimate_focals
    ulps = {}
    for H, W in ic.WEISZFELD_SHAPES:
        maps, focals = ic.weiszfeld_maps(H, W)
        p = maps.reshape(3, -1, 3)
        assert focals[2] > 2 * focals[1] > 4 * focals[0] * 0.9 and focals[1] > 2 * focals[0]
        for b in range(3):
            z = p[b, :, 2]
            assert (z == 0).sum() == 2 and np.isnan(z).sum() == 1 and np.isinf(z).sum() == 1 and (np.abs(p[b]).sum(-1) == 0).sum() == 1
        f64, f32 = ic.weiszfeld_f64(maps), ic.weiszfeld_f32(maps)
        want = np.asarray(estimate_focals(torch.from_numpy(maps)))
        assert np.abs(f64 - want).max() < 1e-12 * want.max()
        assert (np.abs(f64 - focals) < 0.05 * np.asarray(focals)).all(), (f64, focals)
        ulp = np.abs(f32 - f64) / (2.0 ** -23 * f64)
        assert ulp.max() < 1.0, (H, W, ulp)
        ulps[f"{H}x{W}"] = float(ulp.max())
    record_margin("init_weiszfeld_fp32_restatement_ulp", **ulps)


def test_depth_scene():
    d = ic.depth_scene()
    z, want = d["z"], d["want"]
    assert d["pts"].shape == (3, 1517, 3) and d["scale"] == 0.37
    assert np.isnan(z[:, 0]).all() and (z[:, 1] == np.inf).all() and z[1, 2] == 0.0
    assert (want[:, 0] == 0).all() and (want[:, 1] == ic.FLT_MAX).all() and want[1, 2] == 0.0
    fin = np.isfinite(z) & (z != 0)
    assert (z[fin] < -0.4).sum() > 500 and (z[fin] > 0.9).sum() > 2500 and ((z[fin] > 1e-3) & (z[fin] < 0.5)).sum() > 200
    assert (np.abs(z[fin]) > 1e-3).all() and (np.abs(z[fin]) > 16 * d["zbound"][fin]).all()                      # no sign of z within reach of a rounding
    for n in range(3):                                               # rotations with sizeable m[0], m[1]
        R = d["w2c"][n, :, :3].astype(np.float64)
        assert ic.ortho_err(R)[0] < 1e-6 and np.abs(R[2, :2]).min() > 0.2
