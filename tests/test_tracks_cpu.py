"""CPU (no GPU): the checker and the host side of the tracker (csrc/track.hip) -- track_ref() of tests/track_cases.py against a naive
per-track loop, the closed-form answers of the translate, halfpix, border and threshold kinds, the condition that keeps the smooth
kind from passing on tracks that all end or all survive, plan_steps on the clip graphs, the npz files, the C entry's presence and
refusals (which need no device), the scene methods' refusals and run_clip's argument checks."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import track_cases as tc

OUTPUTS = ("xy", "xyz", "pix", "state")


def _small_cases():
    return [c for c in tc.CASES if tc.n_tracks(c) * (c[3] + 1) * c[4] <= 30000]


def _case(kind, hw, M, S, Cn):
    case = (kind, hw, M, S, Cn)
    assert case in tc.CASES
    return tc.ref_case(case)


def _seed_xy(d, H, W):
    x, y = tc.seed_positions(d["seeds"], H, W)
    return x, y


@pytest.mark.parametrize("case", _small_cases(), ids=tc.case_id)
def test_track_ref_equals_a_naive_loop(case):
    d = tc.ref_case(case)
    naive = tc.track_naive(d["xyz"], d["keep"], d["flow_a"], d["flow_b"], d["steps"], d["seeds"], d["fb_thr"])
    for k in OUTPUTS:
        assert naive[k].dtype == d["ref"][k].dtype and naive[k].tobytes() == d["ref"][k].tobytes(), k


def test_the_small_cases_cover_every_kind_and_both_directions():
    small = _small_cases()
    assert {c[0] for c in small} == set(tc.KINDS)
    assert {c[1] for c in tc.CASES} == {(1, 1), (3, 5), (48, 64), (96, 128)}
    assert {c[2] for c in tc.CASES} == {1, 63, 65, 1000, tc.ALL}
    assert {c[3] for c in tc.CASES} == {0, 1, 2, 7} and {c[4] for c in tc.CASES} == {1, 3}
    for case in tc.CASES:
        steps = tc.make_case(case)["steps"]
        if case[3] >= 2:
            assert set(steps[0, :, 3].tolist()) == {0, 1}, case              # both `reversed` values in every multi-step chain
        assert np.array_equal(steps[:, 1:, 0], steps[:, :-1, 1])             # every chain is continuous


def test_the_issue_example_lands_on_pixel_12():
    """3x5 image, constant flow (0.25, -0.5), seed (2.25, 2): (2.5, 1.5) -> column rint(2.5) = 2, row rint(1.5) = 2, pix 12."""
    up = np.zeros((1, 2, 3, 5), np.float32)
    up[0, 0], up[0, 1] = 0.25, -0.5
    xyz = np.arange(2 * 15 * 3, dtype=np.float32).reshape(2, 3, 5, 3)
    r = tc.track_ref(xyz, np.ones((2, 3, 5), np.uint8), up, -up, [[(0, 1, 0, 0)]], np.float32([[2.25, 2]]), 3.0)
    assert r["xy"][0, 1, 0].tolist() == [2.5, 1.5] and r["pix"][0, 1, 0] == 12 and r["state"][0, :, 0].tolist() == [2, 2]
    assert r["pix"][0, 0, 0] == 12 and np.array_equal(r["xyz"][0, 1, 0], xyz[1, 2, 2])       # rint(2.25) = 2 as well


@pytest.mark.parametrize("case", [c for c in tc.CASES if c[0] == "translate"], ids=tc.case_id)
def test_translate_closed_form(case):
    kind, (H, W), M, S, Cn = case
    d = tc.ref_case(case)
    ref, (x, y) = d["ref"], _seed_xy(d, H, W)
    for c, sign in list(enumerate((1, -1)))[:Cn]:                # chain 0 moves by +(2, 1) per step, chain 1 by -(2, 1)
        for t in range(S + 1):
            xt, yt = x + sign * 2 * t, y + sign * t
            alive = (xt >= 0) & (xt <= W - 1) & (yt >= 0) & (yt <= H - 1)        # the straight line leaves the image once
            assert np.array_equal(ref["state"][c, t] > 0, alive), (c, t)
            assert np.array_equal(ref["pix"][c, t], np.where(alive, yt * W + xt, -1).astype(np.int32))
            assert np.array_equal(ref["xy"][c, t], np.where(alive[:, None], np.stack([xt, yt], 1), 0).astype(np.float32))
            if t:
                assert np.array_equal(ref["cause"][c, t - 1] == 1, (ref["state"][c, t - 1] > 0) & ~alive)
        assert not (ref["cause"][c] == 2).any()
    if S:
        assert (ref["cause"] == 1).any()                         # some track does leave


@pytest.mark.parametrize("case", [c for c in tc.CASES if c[0] == "halfpix"], ids=tc.case_id)
def test_halfpix_closed_form_pins_half_to_even(case):
    kind, (H, W), M, S, Cn = case
    d = tc.ref_case(case)
    ref, (x, y) = d["ref"], _seed_xy(d, H, W)
    halves = set()
    for t in range(S + 1):
        xt, yt = x + 0.25 * t, y - 0.5 * t                       # exact: multiples of 0.25
        alive = (xt >= 0) & (xt <= W - 1) & (yt >= 0) & (yt <= H - 1)
        assert np.array_equal(ref["state"][0, t] > 0, alive), t
        col, row = ref["pix"][0, t][alive] % W, ref["pix"][0, t][alive] // W
        for v, got in ((xt[alive], col), (yt[alive], row)):
            half = v % 1 == 0.5
            down = np.floor(v).astype(np.int64)
            assert np.array_equal(got[half], down[half] + down[half] % 2)        # k + 0.5 -> the even neighbour
            assert np.array_equal(got[~half], np.floor(v[~half] + 0.5).astype(np.int64))
            halves |= set((down[half] % 2).tolist())
    if M == tc.ALL or M >= 65:
        assert halves == {0, 1}                                  # both parities occur: floor(x + 0.5) would miss the odd ones


@pytest.mark.parametrize("case", [c for c in tc.CASES if c[0] == "border"], ids=tc.case_id)
def test_border_closed_form(case):
    kind, (H, W), M, S, Cn = case
    d = tc.ref_case(case)
    ref, (x, y) = d["ref"], _seed_xy(d, H, W)
    fx, fy, alive = tc.border_targets(H, W)
    xi, yi = x.astype(np.int64), y.astype(np.int64)
    want = alive[yi, xi]
    xt, yt = x + fx[yi, xi].astype(np.float64), y + fy[yi, xi].astype(np.float64)
    assert np.array_equal(ref["state"][0, 1] > 0, want)
    assert np.array_equal(ref["cause"][0, 0] == 1, ~want) and not (ref["cause"][0] == 2).any()
    assert np.array_equal(ref["xy"][0, 1][want], np.stack([xt, yt], 1)[want].astype(np.float32))
    on = lambda v, edge: set(np.unique(v[want]).tolist()) >= {edge}
    assert on(xt, W - 1) and on(xt, 0) and on(yt, H - 1) and on(yt, 0)             # survivors exactly on all four borders
    ended = np.stack([xt, yt], 1)[~want]
    if M == tc.ALL:
        assert (ended[:, 0] == np.nextafter(np.float64(W - 1), np.inf)).any() and (ended[:, 1] == np.nextafter(np.float64(H - 1), np.inf)).any()
        assert ((ended[:, 0] < 0) & (ended[:, 0] > -1e-37)).any() and ((ended[:, 1] < 0) & (ended[:, 1] > -1e-37)).any()
        assert (x[want] == W - 1).any() and (y[want] == H - 1).any()                # seeds on the last column and row: the clamp
    for t in range(2, S + 1):                                    # zero flow afterwards: whoever survived step 0 stays where it is
        assert np.array_equal(ref["xy"][0, t], ref["xy"][0, 1]) and np.array_equal(ref["state"][0, t] > 0, want)


@pytest.mark.parametrize("case", [c for c in tc.CASES if c[0] == "threshold"], ids=tc.case_id)
def test_threshold_closed_form(case):
    kind, (H, W), M, S, Cn = case
    d = tc.ref_case(case)
    ref, (x, y) = d["ref"], _seed_xy(d, H, W)
    inside = x + 1 <= W - 1
    odd = (x + 1 + y) % 2 == 1                                   # the target's parity: (3, 3.984375) there, (3, 4) on even targets
    assert 3 * 3 + 4 * 4 == d["fb_thr"] ** 2 and 3 * 3 + 3.984375 ** 2 < d["fb_thr"] ** 2
    assert np.array_equal(ref["state"][0, 1] > 0, inside & odd)
    assert np.array_equal(ref["cause"][0, 0], np.where(~inside, 1, np.where(odd, 0, 2)))
    assert (ref["cause"][0, 0] == 2).any() and (ref["state"][0, 1] > 0).any()
    if S >= 2:
        assert not (ref["state"][0, 2] > 0).any()                # the second target has the other parity


@pytest.mark.parametrize("case", [c for c in tc.CASES if c[0] == "smooth" and c[3] == 7 and c[1][0] >= 48], ids=tc.case_id)
def test_smooth_tracks_end_by_both_causes_and_some_survive(case):
    kind, (H, W), M, S, Cn = case
    ref = tc.ref_case(case)["ref"]
    shares = [(ref["state"][0, t] > 0).mean() for t in range(S + 1)]
    print(case, "alive shares", [round(float(s), 3) for s in shares])
    assert 0.05 <= shares[-1] <= 0.95, shares
    assert (ref["cause"] == 1).any() and (ref["cause"] == 2).any()
    assert {0, 1, 2} <= set(np.unique(ref["state"]).tolist())


def test_hostile_inputs_reach_every_branch():
    d = _case("hostile", (48, 64), 1000, 7, 1)
    ref, seeds = d["ref"], d["seeds"]
    assert d["fb_thr"] == np.inf and np.isnan(d["flow_a"]).any() and np.isinf(d["flow_a"]).any()
    bad_seed = ~np.isfinite(seeds).all(1) | (seeds[:, 0] < 0) | (seeds[:, 0] > 63) | (seeds[:, 1] < 0) | (seeds[:, 1] > 47)
    assert bad_seed.sum() >= 100 and np.array_equal(ref["state"][0, 0] == 0, bad_seed)
    assert (ref["cause"] == 2).any()                             # a NaN backward flow ends a track although fb_thr is inf
    assert np.isfinite(ref["xy"]).all() and np.isfinite(ref["xyz"]).all()       # nothing non-finite is ever written
    one = ref["state"] == 1
    assert one.any() and (ref["xyz"][one] == 0).all() and (ref["pix"][one] >= 0).all()
    gone = ref["state"] == 0
    assert (ref["pix"][gone] == -1).all() and (ref["xy"][gone] == 0).all() and (ref["xyz"][gone] == 0).all()
    # a kept pixel with a non-finite point is followed, not visible
    pix0 = ref["pix"][0, 0]
    at = pix0[pix0 >= 0]
    hidden = (d["keep"][0].reshape(-1)[at] != 0) & ~np.isfinite(d["xyz"][0].reshape(-1, 3)[at]).all(1)
    assert hidden.any() and (ref["state"][0, 0][pix0 >= 0][hidden] == 1).all()


def test_an_ended_track_stays_ended():
    for case in tc.CASES:
        state = tc.ref_case(case)["ref"]["state"]
        assert not ((state[:, :-1] == 0) & (state[:, 1:] > 0)).any(), case


# ------------------------------------------------------------------------------------------------- plan_steps, files
@pytest.mark.parametrize("graph", ["swin-3-noncyclic", "swinstride-5-noncyclic"])
def test_plan_steps_on_the_clip_graphs(graph):
    from align3r_amd.dust3r.image_pairs import make_pairs
    from align3r_amd.tool.tracks import plan_steps
    imgs = [dict(idx=i, instance=str(i)) for i in range(16)]
    edges = [(a["idx"], b["idx"]) for a, b in make_pairs(imgs, scene_graph=graph, prefilter=None, symmetrize=True)]
    for frames in (list(range(16)), list(range(15, -1, -1)), [3, 4, 3, 2], [5]):
        steps = plan_steps(edges, frames)
        assert steps.dtype == np.int32 and steps.shape == (len(frames) - 1, 4)
        for (a, b, e, rev), fa, fb in zip(steps.tolist(), frames[:-1], frames[1:]):
            assert (a, b) == (fa, fb) and rev == 0 and edges[e] == (a, b)        # symmetrised: the direct edge exists and is preferred
            assert e == edges.index((a, b))                                      # the first one of the list
    with pytest.raises(ValueError, match="frames 0 and 15"):
        plan_steps(edges, [1, 0, 15])
    # only one direction stored: the edge is taken backwards
    one_way = [e for e in edges if e[0] < e[1]]
    steps = plan_steps(one_way, list(range(15, -1, -1)))
    assert (steps[:, 3] == 1).all() and all(one_way[e] == (b, a) for a, b, e, _ in steps.tolist())
    assert (plan_steps(one_way, range(16))[:, 3] == 0).all()
    assert plan_steps(edges, []).shape == (0, 4)


def test_plan_steps_restates_the_cases_chains():
    from align3r_amd.tool.tracks import plan_steps
    for S in (1, 2, 7):
        chains, edges = tc.path_chains(S, 3), tc.path_graph(S)
        for c in range(3):
            walk = [int(chains[c, 0, 0])] + chains[c, :, 1].tolist()
            assert np.array_equal(plan_steps(edges, walk), chains[c])
    # a duplicate edge: the first one wins
    assert plan_steps([(0, 1), (1, 0), (0, 1)], [0, 1, 0]).tolist() == [[0, 1, 0, 0], [1, 0, 1, 0]]


def test_tracks_npz_round_trip(tmp_path):
    from align3r_amd.tool.tracks import grid_seeds, read_tracks_npz, write_tracks_npz
    ref = _case("smooth", (3, 5), 63, 7, 1)["ref"]
    tr = {k: torch.from_numpy(ref[k][0].copy()) for k in OUTPUTS}
    tr["frames"] = list(range(8))
    path = write_tracks_npz(str(tmp_path / "tracks.npz"), tr)
    back = read_tracks_npz(path)
    assert back["frames"] == tr["frames"]
    for k in OUTPUTS:
        assert back[k].dtype == ref[k].dtype and back[k].tobytes() == ref[k][0].tobytes()
    with pytest.raises(ValueError, match="frames"):
        write_tracks_npz(str(tmp_path / "b.npz"), {k: tr[k] for k in OUTPUTS})
    s = grid_seeds((5, 17), 8)
    assert s.dtype == np.float32 and s.tolist() == [[0, 0], [8, 0], [16, 0]]
    assert grid_seeds((9, 9), 8).tolist() == [[0, 0], [8, 0], [0, 8], [8, 8]]
    with pytest.raises(ValueError):
        grid_seeds((4, 4), 0)


# ------------------------------------------------------------------------------------------------- the C entry
def test_the_entry_is_declared_and_exported():
    from align3r_amd import _lib
    assert "a3r_track_points" in _lib.SIGNATURES and hasattr(_lib.load(), "a3r_track_points")
    header = open(os.path.join(os.path.dirname(__file__), "..", "include", "a3r.h")).read()
    assert "int a3r_track_points(" in header and "OccMask" in header and "dx * dx + dy * dy < fb_thr * fb_thr" in header
    assert len(_lib.SIGNATURES["a3r_track_points"][1]) == 20


def test_refusals_need_no_device():
    """Every A3R_EINVAL of a3r_track_points is raised before anything is launched: the pointers below are host memory."""
    from align3r_amd import _lib
    lib = _lib.load()
    N, H, W, E, Cn, S, M = 3, 4, 5, 2, 2, 2, 6
    xyz, keep = np.zeros((N, H, W, 3), np.float32), np.ones((N, H, W), np.uint8)
    fa, fb = np.zeros((E, 2, H, W), np.float32), np.zeros((E, 2, H, W), np.float32)
    steps = np.int32([[(0, 1, 0, 0), (1, 2, 1, 1)], [(2, 1, 1, 0), (1, 0, 0, 1)]])
    seeds = np.zeros((M, 2), np.float32)
    n = Cn * (S + 1) * H * W
    oxy, oxyz, opix, ost = np.zeros((n, 2), np.float32), np.zeros((n, 3), np.float32), np.zeros(n, np.int32), np.zeros(n, np.uint8)
    p = lambda a: a.ctypes.data
    good = dict(xyz=p(xyz), keep=p(keep), N=N, H=H, W=W, fa=p(fa), fb=p(fb), E=E, sd=p(steps), sh=p(steps), C=Cn, S=S, seeds=p(seeds), M=M,
                thr=3.0, oxy=p(oxy), oxyz=p(oxyz), opix=p(opix), ost=p(ost))

    def call(**change):
        a = dict(good, **change)
        return lib.a3r_track_points(a["xyz"], a["keep"], a["N"], a["H"], a["W"], a["fa"], a["fb"], a["E"], a["sd"], a["sh"], a["C"], a["S"],
                                    a["seeds"], a["M"], a["thr"], a["oxy"], a["oxyz"], a["opix"], a["ost"], None)

    def refused(word, **change):
        rcode = call(**change)
        msg = lib.a3r_last_error().decode()
        assert rcode == -1 and word in msg, (change, rcode, msg)

    def with_step(c, s, k, v):
        t = steps.copy()
        t[c, s, k] = v
        return t

    refused("image size", H=0)
    refused("image size", W=-3)
    refused("below 2^31", H=1 << 16, W=1 << 15)
    refused("N = 0", N=0)
    refused("E = -1", E=-1)
    refused("C = -1", C=-1)
    refused("S = -2", S=-2)
    refused("M = -1", M=-1)
    refused("2^31", M=1 << 31)
    refused("null seeds", seeds=None)                            # M = 6 is not H * W
    refused("below 2^31", M=(1 << 31) - 1)                       # C * (S + 1) * M
    refused("below 2^31", C=1 << 20, S=(1 << 11) - 1, M=1)
    refused("below 2^31", C=(1 << 31) - 1, S=(1 << 31) - 1, M=(1 << 31) - 1)
    for bad in (float("nan"), -1.0):
        refused("fb_thr", thr=bad)
    refused("null xyz", xyz=None)
    refused("null xyz", keep=None)
    for k in ("oxy", "oxyz", "opix", "ost"):
        refused("null output", **{k: None})
    refused("null flow_a", fa=None)
    refused("null flow_a", fb=None)
    refused("null steps_dev", sd=None)
    refused("null steps_dev", sh=None)
    for c, s, k, v, word in ((0, 0, 0, -1, "frames -1 -> 1"), (1, 0, 0, 3, "frames 3 -> 1"), (0, 1, 1, 3, "frames 1 -> 3"),
                             (1, 1, 1, -1, "frames 1 -> -1"), (0, 1, 2, 2, "edge 2"), (1, 0, 2, -1, "edge -1"), (0, 0, 3, 2, "reversed = 2"),
                             (1, 1, 3, -1, "reversed = -1"), (0, 1, 0, 2, "does not continue"), (1, 0, 1, 2, "does not continue")):
        bad = with_step(c, s, k, v)
        refused(word, sh=p(bad))
        assert f"chain {c} step" in lib.a3r_last_error().decode()
    # empty successes: nothing is read, not even null pointers
    assert call(M=0, xyz=None, oxy=None) == 0 and call(C=0, sd=None, sh=None, ost=None) == 0
    # seeds=None with M = H * W passes the size checks and then meets the null xyz
    refused("null xyz", seeds=None, M=H * W, xyz=None)
    with pytest.raises(RuntimeError, match="reversed"):
        _lib.check(call(sh=p(with_step(0, 0, 3, 5))))


# ------------------------------------------------------------------------------------------------- scene methods, run_clip
def _host_scene(shapes, flow_class=False):
    """A scene on the host (no engine): the constructors need no device."""
    g = np.random.default_rng(0)
    edges = [(0, 1), (1, 2), (1, 0), (2, 1)]
    t = lambda *s: torch.from_numpy(g.random(s).astype(np.float32))
    v1, v2 = dict(idx=[i for i, j in edges]), dict(idx=[j for i, j in edges])
    p1 = dict(pts3d=[t(*shapes[i], 3) for i, j in edges], conf=[1 + t(*shapes[i]) for i, j in edges])
    p2 = dict(pts3d_in_other_view=[t(*shapes[j], 3) for i, j in edges], conf=[1 + t(*shapes[j]) for i, j in edges])
    if flow_class:
        from align3r_amd.dust3r.cloud_opt_flow.optimizer import PointCloudOptimizer
        return PointCloudOptimizer(v1, v2, p1, p2, verbose=False), edges
    from align3r_amd.dust3r.cloud_opt.optimizer import PointCloudOptimizer
    return PointCloudOptimizer(v1, v2, p1, p2, False, [], verbose=False), edges


def test_scene_methods_refuse_without_flow_and_on_mixed_shapes():
    plain, edges = _host_scene([(4, 6)] * 3)
    for call in (plain.get_tracks, plain.get_scene_flow, lambda: plain.get_scene_flow(0, 1)):
        with pytest.raises(RuntimeError, match="holds no optical flow"):
            call()
    flow_scene, _ = _host_scene([(4, 6)] * 3, flow_class=True)           # flow_loss_weight = 0: the flow class without fields
    with pytest.raises(RuntimeError, match="holds no optical flow"):
        flow_scene.get_tracks()
    mixed, _ = _host_scene([(4, 6), (3, 5), (4, 6)])
    fields = (np.zeros((4, 2, 4, 6), np.float32),) * 2
    for call in (lambda: mixed.get_tracks(flow=fields), lambda: mixed.get_scene_flow(flow=fields)):
        with pytest.raises(RuntimeError, match="more than one shape"):
            call()
    # with flow the call gets as far as the engine, which a host scene does not have
    with pytest.raises(RuntimeError, match=r"\.to\(device\)"):
        plain.get_tracks(flow=fields)
    with pytest.raises(IndexError):
        plain.get_tracks(frames=[0, 3], flow=fields)
    with pytest.raises(ValueError, match="two frames"):
        plain.get_tracks(frames=[1], flow=fields)
    with pytest.raises(ValueError, match="no edge between frames 0 and 2"):
        plain.get_tracks(frames=[0, 2], flow=fields)
    with pytest.raises(ValueError, match="both images or neither"):
        plain.get_scene_flow(0, flow=fields)
    with pytest.raises(ValueError, match="i == j"):
        plain.get_scene_flow(1, 1, flow=fields)
    with pytest.raises(ValueError, match="flow_ij holds"):
        plain.get_tracks(flow=(np.zeros((3, 2, 4, 6), np.float32),) * 2)


def test_run_clip_arguments(capsys):
    from align3r_amd.tool.run_clip import parse
    base = ["--images", "frames", "--weights", "w.pth", "--out", "out"]
    a = parse(base + ["--flow", "--tracks", "t.npz", "--scene-flow", "sf"])
    assert a.tracks == "t.npz" and a.track_start == 0 and a.track_stride == 8 and a.scene_flow == "sf"
    a = parse(base + ["--flow", "--tracks", "t.npz", "--track-start", "2", "--track-stride", "4"])
    assert a.track_start == 2 and a.track_stride == 4
    assert parse(base).tracks is None and parse(base).scene_flow is None
    for flag, value in (("--tracks", "t.npz"), ("--scene-flow", "sf")):
        for mode in ("--hierarchical", "--flow-hierarchical"):
            with pytest.raises(SystemExit):
                parse(base + [flag, value, mode])
            assert f"{flag} cannot be combined with --hierarchical or --flow-hierarchical: it needs one scene holding all frames" \
                in capsys.readouterr().err
        with pytest.raises(SystemExit):
            parse(base + [flag, value])
        assert f"{flag} needs --flow" in capsys.readouterr().err
    for extra, word in ((["--track-start", "1"], "--track-start belongs to --tracks"), (["--track-stride", "4"], "--track-stride belongs to --tracks"),
                        (["--tracks", "t.npz", "--track-start", "-1"], "--track-start is"), (["--tracks", "t.npz", "--track-stride", "0"], "--track-stride is")):
        with pytest.raises(SystemExit):
            parse(base + ["--flow"] + extra)
        assert word in capsys.readouterr().err
