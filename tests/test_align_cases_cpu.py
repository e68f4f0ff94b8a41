"""CPU: the problems of tests/align_cases.py are good inputs for tests/test_gpu_align_paths.py, shown with the oracle alone --
the float64 restatement reproduces the oracle's flow sums, the guard band keeps every pixel component off the pxl_thre
discontinuity, it costs at most 2 % of the source pixels, the thresholds / masks / clamp really bite, and the degree-class graph
has the degrees it promises."""
import ctypes as C

import numpy as np
import pytest

import align_cases as ac
from oracle.align_ref import AlignOracle, _p, lib

PXL_THRE = 1.5

# name -> (H, W, graph, shared_focal, train_pp): the flow problems of the GPU tests.  s*: P % 4 != 0, the scalar flow pass and
# the !VEC main kernel; v*: P % 4 == 0 beyond one chunk with a ragged last one
FLOW_CASES = {
    "s37x41_win6_sf": (37, 41, "win6", True, False),
    "s34x33_win6_pp": (34, 33, "win6", False, True),
    "s37x41_deg": (37, 41, "deg", False, False),
    "s34x33_deg_sf": (34, 33, "deg", True, False),
    "v36x44_deg_sf": (36, 44, "deg", True, False),
    "v40x52_deg_pp": (40, 52, "deg", False, True),
}
# (H, W, ego-flow term on as well)
PRIOR_CASES = {"p37x41": (37, 41, False), "p40x52": (40, 52, False), "p37x41_flow": (37, 41, True), "p40x52_flow": (40, 52, True)}


def flow_case(name, biting, **over):
    """The flow problem `name`: biting (pxl_thre = 1.5, guard-banded) or loose (pxl_thre = thre = 1e9).  The flow term starts at
    iteration 5 (flow_loss_start_epoch 0.1 of 50), so epoch 0 is 'off' and a 10-step run crosses the gate."""
    H, W, graph, shared_focal, train_pp = FLOW_CASES[name]
    edges, N = (ac.window_graph(6), 6) if graph == "win6" else ac.degree_class_graph()
    kw = dict(dyn_frac=0.3, pxl_thre=PXL_THRE if biting else 1e9, thre=1e9, shared_focal=shared_focal, train_pp=train_pp, start_epoch=0.1)
    kw.update(over)
    return ac.flow_problem(N, H, W, edges, 7, **kw)


def prior_case(name):
    H, W, flow = PRIOR_CASES[name]
    return ac.prior_problem(3, H, W, 7, flow=flow)


def make_oracle(prob, **over):
    o = AlignOracle(*prob["args"], **dict(prob["kw"], **over))
    o.set_params(**prob["init"])
    return o


def oracle_flow_sums(o, pxl_thre=None, dyn=None):
    """sums[0..3] = (S_0, C_0, S_1, C_1) of a3r_oracle_flow_loss_grad's first pass at the oracle's current parameters."""
    fl, p = o.flow, o.params
    H, W = o.hw
    focals_full = o._focals_full()
    fvals = np.exp(focals_full / o.cfg.focal_break).astype(np.float32)
    ppv = (o.pp0 + 10 * p["im_pp"]).astype(np.float32)
    dyn = fl["dyn"] if dyn is None else np.ascontiguousarray(dyn).reshape(o.N, o.P).astype(np.uint8)
    sums = (C.c_double * 4)()
    lib().a3r_oracle_flow_loss_grad(o.E, o.N, H, W, _p(o.ei, C.c_int), _p(o.ej, C.c_int), _p(fl["flow_ij"]), _p(fl["flow_ji"]),
                                    dyn.ctypes.data_as(C.POINTER(C.c_ubyte)), _p(p["depth"]), _p(p["im_poses"]), _p(fvals), _p(ppv),
                                    C.c_float(fl["pxl_thre"] if pxl_thre is None else pxl_thre), None, sums, None, None, None, None)
    return np.asarray(list(sums))


def oracle_flow_loss(o):
    s = oracle_flow_sums(o)
    return s[0] / s[1] + s[2] / s[3]


@pytest.mark.parametrize("name", ["s37x41_win6_sf", "s34x33_win6_pp", "v36x44_deg_sf"])
def test_restatement_reproduces_the_oracle(name):
    prob = flow_case(name, True)
    o = make_oracle(prob)
    l, valid = ac.flow_pixel_losses(prob, poses=o.pose_matrices()[1])
    for thre in (PXL_THRE, 1e9):
        mine, ref = ac.flow_sums(l, valid, thre), oracle_flow_sums(o, thre)
        assert mine[1] == ref[1] and mine[3] == ref[3], (thre, mine, ref)
        assert np.all(np.abs(mine - ref) <= 1e-12 * np.abs(ref)), (thre, mine, ref)
    # the builder's own fp32 camera matrices (no oracle at hand there) are the oracle's to fp32 rounding
    assert np.abs(ac._pose_rt(prob["init"]["im_poses"]) - o.pose_matrices()[1]).max() < 1e-6


@pytest.mark.parametrize("name", list(FLOW_CASES))
def test_guard_band_holds_and_stays_under_its_cap(name):
    prob = flow_case(name, True)
    o = make_oracle(prob)
    at = [oracle_flow_sums(o, PXL_THRE * s) for s in (1 - ac.GUARD, 1.0, 1 + ac.GUARD)]
    assert at[0][1] == at[1][1] == at[2][1] and at[0][3] == at[1][3] == at[2][3], at
    # without the band the same three counts differ: the band is what makes them equal
    raw = [oracle_flow_sums(o, PXL_THRE * s, dyn=prob["dyn_drawn"]) for s in (1 - ac.GUARD, 1 + ac.GUARD)]
    assert raw[0][1] + raw[0][3] < raw[1][1] + raw[1][3]
    share = prob["guard_mask"].sum() / prob["guard_mask"].size
    print(f"[align-cases] {name}: guard band masks {prob['guard_mask'].sum()} of {prob['guard_mask'].size} source pixels ({share:.2%}); "
          f"oracle counts at (1 -/+ 1e-3) pxl_thre differ by {int(raw[1][1] + raw[1][3] - raw[0][1] - raw[0][3])} without it")
    assert 0 < share <= 0.02
    assert not (prob["guard_mask"] & prob["dyn_drawn"]).any()


def test_guard_band_cap_on_plain_window_graphs():
    """The sizes the cap was first estimated at: window graphs, no fully dynamic image."""
    for N, (H, W) in ((6, (37, 41)), (6, (36, 44)), (12, (37, 41))):
        prob = ac.flow_problem(N, H, W, ac.window_graph(N), 7, dyn_frac=0.3, pxl_thre=PXL_THRE, thre=1e9, shared_focal=False,
                               train_pp=False, full_dynamic=False)
        assert prob["guard_mask"].sum() <= 0.02 * N * H * W, (N, H, W, prob["guard_mask"].sum())


@pytest.mark.parametrize("name", list(FLOW_CASES))
def test_flow_settings_bite(name):
    prob = flow_case(name, True)
    o = make_oracle(prob)
    E, P = len(prob["edges"]), prob["H"] * prob["W"]
    kept, unmasked = oracle_flow_sums(o), oracle_flow_sums(o, 1e9)
    for d in (1, 3):
        excluded = 1 - kept[d] / unmasked[d]
        assert 0.10 <= excluded <= 0.90, (d, excluded)
    removed = 1 - (unmasked[1] + unmasked[3]) / (4.0 * E * P)            # two components of every (edge, direction, source pixel)
    assert removed >= 0.20, removed
    assert prob["flow"]["dyn"][prob["N"] - 1].all()                       # one image fully dynamic
    # the loose setting excludes nothing
    loose = make_oracle(flow_case(name, False))
    assert np.array_equal(oracle_flow_sums(loose)[[1, 3]], oracle_flow_sums(loose, 3e38)[[1, 3]])


def test_flow_points_stay_in_front_of_their_target_cameras():
    """Every problem with the flow term on keeps the points it projects at least MIN_QZ in front of the target camera."""
    probs = [flow_case(n, b) for n in FLOW_CASES for b in (True, False)] + [prior_case(n) for n in PRIOR_CASES if PRIOR_CASES[n][2]]
    for prob in probs:
        assert ac.flow_min_qz(prob) >= ac.MIN_QZ


@pytest.mark.parametrize("name", list(PRIOR_CASES))
def test_prior_clamp_bites(name):
    prob = prior_case(name)
    o = make_oracle(prob)
    o.set_depth_prior(**prob["prior"])
    P = prob["H"] * prob["W"]
    assert P > 1024
    for raw in (o.params["depth"], o.prior["init"]):
        d = np.exp(raw.astype(np.float32)).astype(np.float64)
        clamped = (d <= 1e-6).mean()
        assert clamped >= 0.05 and 1 - clamped >= 0.50, clamped
        assert d[d > 1e-6].min() > 4e-5 and d[d <= 1e-6].max() < 2e-7        # nothing near the clamp
    assert np.array_equal(np.exp(o.params["depth"]) <= 1e-6, prob["clamped"])
    _, g = o._depth_prior(o.params["depth"])
    assert np.all(g[prob["clamped"]] == 0) and np.all(g[~prob["clamped"]] != 0)
    assert 0.2 <= prob["prior"]["dyn"].mean() <= 0.4


def test_degree_class_graph():
    edges, N = ac.degree_class_graph()
    deg = ac.degrees(edges, N)
    assert set(ac.DEGREE_CLASSES) <= set(deg.tolist()), deg
    assert deg.min() >= 1 and len(set(edges)) == len(edges) and all(i != j for i, j in edges)
    assert list(deg[:7]) == [17, 16, 9, 8, 7, 2, 1]


def test_shape_lists():
    assert [h * w % 4 for h, w in ac.RAGGED] == [1, 2, 3, 1, 2]
    assert [h * w for h, w in ac.RAGGED] == [1517, 1122, 1023, 1025, 6]
    for h, w in ac.VEC_RAGGED:
        assert h * w % 4 == 0 and h * w > 1024 and h * w % 1024 != 0
