"""GPU: the solvers of the MST initialisation against the float64 oracles of tests/init_cases.py under its agreement rules.
  a3r_pnp_solve           one batch of 93 problems (nine scenes of six shapes with a given focal, four focal searches of 21 candidates):
                          subsample steps 1, 2, 3, a principal point, checkerboard / row-band / five-pixel masks, 20 % and 40 % outliers,
                          a camera that looks away, n < n_max for most problems, the second block of the solve kernel; at 0, 1 and 10
                          iterations, so that a failure points at the closed-form start or at the Gauss-Newton step;
  a3r_umeyama_moments + a3r_umeyama_solve   scenes (a) to (g): P at the 1024-point chunk edges, a reflection, coplanar, nearly
                          collinear and far-away clouds, zero weights over garbage, 130 problems sharing 7 clouds;
  csrc/init_maps.hip      Weiszfeld focal per map at four shapes with special pixels, depth_init under random rotations, conf_prepare at
                          P = 4 and P = 8200, im_conf_max with an image without edges, mask_gt at the threshold, and the loud errors.
The cap conditions that make exact comparisons legitimate (no point at the 5 px threshold, order-insensitive oracles, unique winners of
the focal searches) are asserted on the CPU in tests/test_init_cases_cpu.py; nothing here skips a scene.  Measured deviations are
recorded as init_* (DESIGN section 2)."""
import numpy as np
import pytest
import torch

import init_cases as ic
from conftest import record_margin, rel_err

pytestmark = pytest.mark.gpu


def up(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


# ------------------------------------------------------------------------------------------------ PnP
@pytest.fixture(scope="module")
def pnp_dev():
    """Device copies of the scenes (one per scene: the candidates of a focal search share their buffers)."""
    return {name: (up(sc["pts"]), up(sc["mask"])) for name, sc in ic.pnp_scenes().items()}


def _check_pnp(info, c2w, expected, problems, tag):
    valid = np.array([r["valid"] for r in expected])
    assert np.array_equal(info[:, 0] != 0, valid), [p for p, a, b in zip(problems, info[:, 0] != 0, valid) if a != b]
    inl = np.array([r["inliers"] for r in expected])
    assert np.array_equal(info[:, 1].astype(np.int64), inl), [(p, int(a), int(b)) for p, a, b in zip(problems, info[:, 1], inl) if a != b]
    err = np.array([r["err"] for r in expected])
    err_dev = np.abs(info[:, 2].astype(np.float64) - err) / np.maximum(err, 1e-300)
    assert np.array_equal(info[:, 3], np.array([r["focal"] for r in expected], np.float32))
    want = np.stack([r["c2w"] for r in expected])
    assert np.array_equal(c2w[:, 3], np.tile(np.float32([0, 0, 0, 1]), (len(want), 1)))
    over = np.abs(c2w.astype(np.float64) - want) / (ic.ULP2 * np.maximum(1, np.abs(want)))
    per_problem = over.reshape(len(want), -1).max(1)
    orth, det = ic.ortho_err(c2w[valid, :3, :3])
    record_margin(f"init_pnp_{tag}", c2w_over_bound=per_problem.max(), c2w_abs=np.abs(c2w - want).max(), err_ulp=err_dev.max() / 2.0 ** -23,
                  orthonormal=orth, det=det)
    worst = int(per_problem.argmax())
    assert per_problem.max() <= 1.0, (problems[worst], per_problem[worst], c2w[worst], want[worst])
    assert err_dev.max() <= 4 * 2.0 ** -23, (problems[int(err_dev.argmax())], err_dev.max())
    assert orth < 1e-6 and det < 1e-6
    return per_problem


@pytest.mark.parametrize("iterations", ic.PNP_ITERATIONS)
def test_pnp_batch_vs_oracle(pnp_dev, iterations):
    from align3r_amd.dust3r.cloud_opt.init_im_poses import pnp_batched
    scenes, problems = ic.pnp_scenes(), ic.pnp_problems()
    info, c2w = pnp_batched([(*pnp_dev[name], f, scenes[name]["pp"]) for name, f in problems], iterations)
    assert info.shape == (len(problems), 4) and c2w.is_cuda and len(problems) > 64
    per_problem = _check_pnp(info, c2w.cpu().numpy(), ic.pnp_expected(iterations), problems, f"it{iterations}")
    band = [n for n, _ in problems].index("33x70_rows10-12")
    assert info[band, 0] == 1 and per_problem[band] <= 1.0                       # the nearly planar ray cloud of the thin band


@pytest.mark.parametrize("iterations", ic.PNP_ITERATIONS)
def test_linear_pnp_many_and_the_focal_search(pnp_dev, iterations):
    from align3r_amd.dust3r.cloud_opt.init_im_poses import linear_pnp_many
    scenes, problems, expected = ic.pnp_scenes(), ic.pnp_problems(), ic.pnp_expected(iterations)
    res = linear_pnp_many([(pnp_dev[name][0], sc["focal"], pnp_dev[name][1], sc["pp"]) for name, sc in scenes.items()], iterations)
    assert len(res) == len(scenes)
    worst = 0.0
    for (name, sc), got in zip(scenes.items(), res):
        mine = [r for (n, _), r in zip(problems, expected) if n == name]
        if sc["focal"] is not None:
            want = mine[0] if mine[0]["valid"] and mine[0]["inliers"] > 0 else None
        else:
            k, _ = ic.pnp_search_pick(mine)
            want = None if k is None else mine[k]
            assert want is not None
        if want is None:
            assert got is None and sc["kind"] == "invalid", name
            continue
        assert got is not None and sc["kind"] != "invalid", name
        assert np.float32(got[0]) == np.float32(want["focal"]), (name, got[0], want["focal"])       # the same candidate
        over = np.abs(got[1].cpu().numpy().astype(np.float64) - want["c2w"]) / (ic.ULP2 * np.maximum(1, np.abs(want["c2w"])))
        worst = max(worst, float(over.max()))
        assert over.max() <= 1.0, (name, over.max())
    record_margin(f"init_pnp_many_it{iterations}", c2w_over_bound=worst)


# ------------------------------------------------------------------------------------------------ Umeyama
@pytest.fixture(scope="module")
def umeyama_results():
    from align3r_amd.dust3r.cloud_opt.init_im_poses import rigid_points_registration_batched
    out = {}
    for name, sc in ic.umeyama_scenes().items():
        sols = rigid_points_registration_batched(up(sc["X"]), up(sc["Y"]), up(sc["W"]), sc["y_index"])
        assert sols.is_cuda and tuple(sols.shape) == (len(sc["y_index"]), 13)
        out[name] = sols
    return out


@pytest.mark.parametrize("name", list(ic.umeyama_scenes()))
def test_umeyama_vs_oracle(umeyama_results, name):
    want, spread = ic.umeyama_expected()[name]
    got = umeyama_results[name].cpu().numpy().astype(np.float64)
    bound = ic.umeyama_bound(name, want, spread)
    over = np.abs(got - want) / bound
    orth, det = ic.ortho_err(got[:, 1:10].reshape(-1, 3, 3))
    record_margin(f"init_umeyama_{name}", over_bound=over.max(), abs_dev=np.abs(got - want).max(), bound_over_2ulp=(bound / (ic.ULP2 * np.maximum(1, np.abs(want)))).max(),
                  orthonormal=orth, det=det)
    e = int(over.max(1).argmax())
    assert over.max() <= 1.0, (name, e, over[e], got[e], want[e])
    assert orth < 1e-6 and det < 1e-6, (name, orth, det)                        # a rotation, det = +1 (also where the optimum is a reflection)


def test_umeyama_single_explicit_offsets_and_batched_are_bitwise_equal(umeyama_results):
    from align3r_amd.dust3r.cloud_opt.init_im_poses import rigid_points_registration, umeyama_solve
    scenes = ic.umeyama_scenes()
    sc = scenes["a_generic_P1025"]
    for e in range(2):
        s, R, T = rigid_points_registration(up(sc["X"][e]), up(sc["Y"][e]), up(sc["W"][e]))
        assert torch.equal(torch.cat([s[None], R.reshape(9), T]), umeyama_results["a_generic_P1025"][e])
    # scenes (b) to (f) as ONE call: flat buffers with a pad in front, problems in reverse order, y before x
    names = ["f_zero_weights", "e_far", "d_collinear", "c_coplanar", "b_mirror"]
    P = ic.SPECIAL_P
    pads = dict(x=5, y=8, w=3)
    x = torch.cat([torch.full((pads["x"],), float("nan"))] + [torch.from_numpy(scenes[n]["X"][0]).reshape(-1) for n in names]).cuda()
    y = torch.cat([torch.full((pads["y"],), float("nan"))] + [torch.from_numpy(scenes[n]["Y"][0]).reshape(-1) for n in names]).cuda()
    w = torch.cat([torch.full((pads["w"],), float("nan"))] + [torch.from_numpy(scenes[n]["W"][0]) for n in names]).cuda()
    ar = torch.arange(len(names), dtype=torch.int64)
    x_off, y_off, w_off = (pads["x"] + 3 * P * ar).cuda(), (pads["y"] + 3 * P * ar).cuda(), (pads["w"] + P * ar).cuda()
    assert int(x_off[-1]) + 3 * P == x.numel() and int(y_off[-1]) + 3 * P == y.numel() and int(w_off[-1]) + P == w.numel()
    sols = umeyama_solve(x, y, w, x_off, y_off, w_off, P)
    for k, n in enumerate(names):
        assert torch.equal(sols[k], umeyama_results[n][0]), n


# ------------------------------------------------------------------------------------------------ init_maps
@pytest.mark.parametrize("H,W", ic.WEISZFELD_SHAPES)
def test_weiszfeld_focal_per_map(H, W):
    from align3r_amd.dust3r.cloud_opt import _native
    from align3r_amd.dust3r.cloud_opt.init_im_poses import estimate_focals
    maps, _ = ic.weiszfeld_maps(H, W)
    want = np.asarray(estimate_focals(torch.from_numpy(maps)))               # the generic path, float64
    restated = ic.weiszfeld_f32(maps)
    got = _native.weiszfeld_focal(up(maps)).cpu().numpy().astype(np.float64)
    ulp = 2.0 ** -23 * want
    tol = np.maximum(8 * ulp, 8 * np.abs(restated - want))
    record_margin(f"init_weiszfeld_{H}x{W}", kernel_ulp=np.abs(got - want) / ulp, restatement_ulp=np.abs(restated - want) / ulp)
    assert (np.abs(got - want) <= tol).all(), (got, want, tol)
    start = _native.weiszfeld_focal(up(maps), iterations=0).cpu().numpy().astype(np.float64)
    want0 = ic.weiszfeld_f64(maps, 0)
    assert (np.abs(start - want0) <= np.maximum(8 * 2.0 ** -23 * want0, 8 * np.abs(ic.weiszfeld_f32(maps, 0) - want0))).all(), (start, want0)


def test_depth_init_random_rotations():
    from align3r_amd.dust3r.cloud_opt import _native
    d = ic.depth_scene()
    N, P = d["z"].shape
    depth = torch.full((N, P), 7.0).cuda()
    _native.depth_init(up(d["pts"]), up(d["w2c"]), d["scale"], depth)
    got = depth.cpu().numpy()
    z, want = d["z"], d["want"]
    assert (got[:, 0] == 0).all() and (got[:, 1] == np.float32(ic.FLT_MAX)).all() and got[1, 2] == 0          # NaN, +inf, z = 0 exactly
    with np.errstate(invalid="ignore"):
        behind, front, mid = z < 0, np.isfinite(z) & (z > 1e-3), np.isfinite(z) & (z >= 0.5)
    assert behind.sum() > 500 and (got[behind] == 0).all()
    tensor = rel_err(got[mid], want[mid])
    # per element: d(log z) = dz / z with |dz| <= zbound, plus logf to 2 ulp
    tol = 1.01 * d["zbound"][front] / z[front] + ic.ULP2 * np.abs(want[front]) + 2.0 ** -40
    over = np.abs(got[front] - want[front]) / tol
    record_margin("init_depth_init", tensor_rel_err=tensor, per_element_over_bound=over.max())
    assert tensor < 1e-6 and over.max() <= 1.0


@pytest.mark.parametrize("P", (4, 8200))
def test_conf_prepare(P):
    from align3r_amd.dust3r.cloud_opt import _native
    g = torch.Generator(device="cpu").manual_seed(P)
    E = 3
    ci, cj = (1 + 9 * torch.rand(E, P, generator=g)).cuda(), (1 + 30 * torch.rand(E, P, generator=g)).cuda()
    ref_mean = torch.stack([ci.double().mean(1), cj.double().mean(1)], 1).reshape(-1).cpu().numpy()
    one_ulp = np.spacing(ref_mean.astype(np.float32)).astype(np.float64)
    worst = 0.0
    for mode, fn in (("log", torch.log), ("sqrt", torch.sqrt), ("m1", lambda x: x - 1), ("id", lambda x: x)):
        wi, wj, mean = _native.conf_prepare(ci, cj, mode)
        none_i, none_j, mean_only = _native.conf_prepare(ci, cj, mode, want_weights=False)
        assert none_i is None and none_j is None and torch.equal(mean_only, mean)
        dev = np.abs(mean.cpu().numpy().astype(np.float64) - ref_mean) / one_ulp
        worst = max(worst, float(dev.max()))
        assert dev.max() <= 1.0, (mode, dev)
        for w, c in ((wi, ci), (wj, cj)):
            if mode in ("m1", "id"):
                assert torch.equal(w, fn(c))
            else:
                assert rel_err(w.cpu().numpy(), fn(c.double()).cpu().numpy()) < 1e-6
    record_margin(f"init_conf_prepare_P{P}", mean_ulp=worst)


def test_im_conf_max_with_an_image_without_edges():
    from align3r_amd.dust3r.cloud_opt import _native
    g = torch.Generator(device="cpu").manual_seed(3)
    E, N, P = 6, 5, 1517
    edges = [(0, 1), (1, 0), (1, 2), (2, 3), (3, 1), (0, 3)]                    # image 4 appears nowhere
    ci, cj = (1 + 9 * torch.rand(E, P, generator=g)).cuda(), (1 + 9 * torch.rand(E, P, generator=g)).cuda()
    out = _native.im_conf_max(ci, cj, edges, N)
    ref = torch.zeros(N, P).cuda()
    for e, (i, j) in enumerate(edges):
        ref[i] = torch.maximum(ref[i], ci[e])
        ref[j] = torch.maximum(ref[j], cj[e])
    assert tuple(out.shape) == (N, P) and torch.equal(out[:4], ref[:4]) and bool((ref[:4] >= 1).all())
    assert torch.equal(out[4], torch.zeros(P).cuda())


def test_mask_gt_at_the_threshold():
    from align3r_amd.dust3r.cloud_opt import _native
    thr = 3.0999999046325684                                                      # an fp32 value
    x = torch.tensor([thr, np.nextafter(np.float32(thr), np.float32(9)), np.nextafter(np.float32(thr), np.float32(0)), float("nan"), float("inf"),
                      -float("inf"), 0.0] * 41, dtype=torch.float32).cuda()          # 287 elements: two blocks
    out = _native.mask_gt(x, thr)
    assert out.dtype == torch.uint8 and out.cpu().tolist() == [0, 1, 0, 0, 1, 0, 0] * 41


def test_init_errors_are_loud(pnp_dev):
    from align3r_amd import _lib
    from align3r_amd._lib import check, ptr, stream_ptr
    from align3r_amd.dust3r.cloud_opt import _native
    from align3r_amd.dust3r.cloud_opt.init_im_poses import pnp_batched
    lib = _lib.load()
    pts, msk = pnp_dev["5x7"]
    with pytest.raises(RuntimeError, match="iterations=65"):
        pnp_batched([(pts, msk, 9.0, None)], iterations=65)
    buf = torch.zeros(4096, dtype=torch.uint8).cuda()
    c2w, info = torch.zeros(16).cuda(), torch.zeros(4).cuda()
    with pytest.raises(RuntimeError, match="bad shape B=0"):
        check(lib.a3r_pnp_solve(ptr(buf), 0, 35, 10, ptr(buf), ptr(c2w), ptr(info), stream_ptr()), "a3r_pnp_solve")
    x, off, part = torch.zeros(12).cuda(), torch.zeros(1, dtype=torch.int64).cuda(), torch.zeros(17, dtype=torch.float64).cuda()
    with pytest.raises(RuntimeError, match="bad shape B=1 P=0"):
        check(lib.a3r_umeyama_moments(ptr(x), ptr(x), ptr(x), ptr(off), ptr(off), ptr(off), 1, 0, ptr(part), stream_ptr()), "a3r_umeyama_moments")
    c6 = torch.ones(2, 6).cuda()
    with pytest.raises(RuntimeError, match="P % 4"):
        _native.conf_prepare(c6, c6.clone(), "log")
    assert bool((c2w == 0).all()) and bool((info == 0).all()) and bool((part == 0).all())          # nothing was launched
