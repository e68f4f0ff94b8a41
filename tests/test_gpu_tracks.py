"""GPU: the tracker (csrc/track.hip) -- ops.track_points against track_ref(), the numpy restatement of tests/track_cases.py.

Every comparison is exact: states, pixels and the bytes of positions and points.  The definition is float64 arithmetic whose every
operation is rounded on its own, on the device as in numpy, followed by a half-to-even rounding and gathers (tests/test_tracks_cpu.py
checks the restatement itself against a per-track loop and against closed-form answers).  The scene tests build small synthetic
scenes as tests/test_gpu_scene.py does, inject flow fields, and compare scene.get_tracks / get_scene_flow with the restatement on
engine.points() and the keep rule of get_pointcloud().
"""
import numpy as np
import pytest
import torch

import track_cases as tc
from test_gpu_scene import make_scene, scene_inputs

pytestmark = pytest.mark.gpu

OUTPUTS = ("xy", "xyz", "pix", "state")


def _dev(a):
    return None if a is None else torch.from_numpy(np.array(a)).cuda()         # a copy: the shared cases are read-only


def _track(d, steps=None, seeds="case", fb_thr=None):
    from align3r_amd import ops
    return ops.track_points(_dev(d["xyz"]), _dev(d["keep"]), _dev(d["flow_a"]), _dev(d["flow_b"]), d["steps"] if steps is None else steps,
                            seeds=_dev(d["seeds"]) if isinstance(seeds, str) else seeds, fb_thr=d["fb_thr"] if fb_thr is None else fb_thr)


def _same(got, ref, sel=slice(None)):
    for k in OUTPUTS:
        g, r = got[k].cpu().numpy(), np.ascontiguousarray(ref[k][sel])
        assert g.dtype == r.dtype and g.shape == r.shape, (k, g.dtype, g.shape, r.shape)
        assert g.tobytes() == r.tobytes(), k


@pytest.mark.parametrize("case", tc.CASES, ids=tc.case_id)
def test_track_points_equals_the_restatement(case):
    kind, (H, W), M, S, Cn = case
    d = tc.ref_case(case)
    got = _track(d)
    assert set(got) == set(OUTPUTS) and got["state"].shape == (Cn, S + 1, tc.n_tracks(case))
    _same(got, d["ref"])


@pytest.mark.parametrize("case", [c for c in tc.CASES if c[0] in ("smooth", "hostile") and c[3] >= 1 and c[1][0] >= 48], ids=tc.case_id)
def test_twice_the_same_bytes_and_chains_one_by_one(case):
    kind, (H, W), M, S, Cn = case
    d = tc.ref_case(case)
    a, b = _track(d), _track(d)
    for k in OUTPUTS:
        assert torch.equal(a[k], b[k]), k
    for c in range(Cn):                                          # a batch of chains equals the chains one by one
        _same(_track(d, steps=d["steps"][c:c + 1]), d["ref"], slice(c, c + 1))
    _same(_track(d, steps=d["steps"][0]), d["ref"], slice(0, 1))              # [S,4]: one chain
    _same(_track(d, steps=torch.from_numpy(np.array(d["steps"])).cuda()), d["ref"])        # a device tensor of steps


@pytest.mark.parametrize("case", [c for c in tc.CASES if c[2] == tc.ALL and c[0] in ("smooth", "border", "hostile")], ids=tc.case_id)
def test_no_seeds_equals_the_explicit_pixel_grid(case):
    kind, (H, W), M, S, Cn = case
    d = tc.ref_case(case)
    grid = np.stack([np.arange(H * W) % W, np.arange(H * W) // W], 1).astype(np.float32)
    _same(_track(d, seeds=_dev(grid)), d["ref"])


def test_bool_keep_and_plain_python_steps():
    d = tc.ref_case(("smooth", (48, 64), 1000, 1, 1))
    from align3r_amd import ops
    got = ops.track_points(_dev(d["xyz"]), _dev(d["keep"]).bool(), _dev(d["flow_a"]), _dev(d["flow_b"]), d["steps"].tolist(),
                           seeds=_dev(d["seeds"]), fb_thr=d["fb_thr"])
    _same(got, d["ref"])


def test_every_entry_check_returns_its_error():
    """The refusals reach Python as RuntimeError with the library's text; the outputs of a refused call are never touched (they are
    allocated empty when the sizes do not fit) and the device stays usable."""
    from align3r_amd import ops
    d = tc.ref_case(("translate", (3, 5), 63, 1, 3))
    steps = np.array(d["steps"])

    def bad(c, s, k, v):
        t = steps.copy()
        t[c, s, k] = v
        return t

    for t, word in ((bad(0, 0, 0, 2), "frames 2 -> 1"), (bad(1, 0, 1, -1), "frames 1 -> -1"), (bad(2, 0, 2, 1), "edge 1"),
                    (bad(0, 0, 3, 2), "reversed = 2")):
        with pytest.raises(RuntimeError, match=word):
            _track(d, steps=t)
    two = np.concatenate([steps[:1], steps[:1]], 1)              # 0 -> 1 followed by 0 -> 1: not a chain
    with pytest.raises(RuntimeError, match="does not continue"):
        _track(d, steps=two)
    for thr in (float("nan"), -1.0):
        with pytest.raises(RuntimeError, match="fb_thr"):
            _track(d, fb_thr=thr)
    with pytest.raises(RuntimeError, match="below 2\\^31"):
        _track(d, steps=np.zeros((1 << 20, 0, 4), np.int32), seeds=torch.zeros((1 << 11, 2), device="cuda"))
    with pytest.raises(ValueError, match="steps"):
        _track(d, steps=np.zeros((1, 1, 3), np.int32))
    with pytest.raises(RuntimeError, match="keep"):
        ops.track_points(_dev(d["xyz"]), _dev(d["keep"]).float(), _dev(d["flow_a"]), _dev(d["flow_b"]), steps)
    with pytest.raises(RuntimeError, match="flow_a"):
        ops.track_points(_dev(d["xyz"]), _dev(d["keep"]), _dev(d["flow_a"])[:, :, :2].contiguous(), _dev(d["flow_b"]), steps)
    with pytest.raises(RuntimeError, match="seeds"):
        _track(d, seeds=torch.zeros((4, 3), device="cuda"))
    # empty calls succeed
    got = _track(d, seeds=torch.zeros((0, 2), device="cuda"))
    assert got["state"].shape == (3, 2, 0) and got["xy"].shape == (3, 2, 0, 2)
    got = _track(d, steps=np.zeros((0, 1, 4), np.int32))
    assert got["pix"].shape == (0, 2, 63)
    _same(_track(d), d["ref"])                                   # and the good call still answers


# ------------------------------------------------------------------------------------------------- scenes
N_, H_, W_ = 4, 36, 44


def _shift_flow(edges, H, W, dx, dy):
    """(flow_ij, flow_ji) [E,2,H,W]: every edge (i, j) moves its pixels by (j - i) * (dx, dy), whole pixels; the exact inverse back."""
    fij = np.zeros((len(edges), 2, H, W), np.float32)
    for e, (i, j) in enumerate(edges):
        fij[e, 0], fij[e, 1] = (j - i) * dx, (j - i) * dy
    return fij, -fij


def _wavy_flow(edges, H, W, seed):
    g = np.random.default_rng(seed)
    ys, xs = np.meshgrid(np.arange(H) / H, np.arange(W) / W, indexing="ij")
    fij, fji = np.zeros((len(edges), 2, H, W), np.float32), np.zeros((len(edges), 2, H, W), np.float32)
    for e in range(len(edges)):
        a, b = g.uniform(0, 6.28, 2)
        fij[e, 0], fij[e, 1] = 1.0 + 2.5 * np.sin(6.28 * xs + a), 2.5 * np.cos(6.28 * ys + b)
        fji[e] = -fij[e] + 3.5 * np.sin(6.28 * (xs + ys) + a) * np.sin(6.28 * ys + b)
    return fij, fji


def _scene_reference(scene, flow, steps, seeds, fb_thr, thr, dyn):
    """track_ref on what the scene hands to the kernel: engine.points() and the keep rule of get_pointcloud()."""
    N, (H, W) = scene.n_imgs, scene.imshapes[0]
    conf, _ = scene_inputs(scene)
    keep = conf > np.float32(thr)
    if dyn is not None:
        keep &= ~dyn
    xyz = scene.engine.points().cpu().numpy().reshape(N, H, W, 3)
    return tc.track_ref(xyz, keep.reshape(N, H, W), flow[0], flow[1], steps, seeds, fb_thr), xyz


@pytest.mark.parametrize("kind", ["plain", "flow"])
def test_get_tracks_equals_the_restatement_on_the_scene(kind):
    from align3r_amd.tool.tracks import plan_steps
    scene, dyn = make_scene(kind, N_, H_, W_)
    flow = _wavy_flow(scene.edges, H_, W_, 3)
    g = np.random.default_rng(1)
    seeds = np.stack([g.uniform(0, W_ - 1, 300), g.uniform(0, H_ - 1, 300)], 1).astype(np.float32)
    masked = kind == "flow"
    for frames, sd in (([0, 1, 2, 3], seeds), ([3, 1, 2, 0], None)):
        got = scene.get_tracks(frames=frames, seeds=sd, flow=flow, mask_dynamic=masked)
        ref, xyz = _scene_reference(scene, flow, plan_steps(scene.edges, frames), sd, 3.0, scene.min_conf_thr, dyn if masked else None)
        assert got["frames"] == frames and set(got) == set(OUTPUTS) | {"frames"}
        _same({k: got[k][None] for k in OUTPUTS}, ref)
        states = set(np.unique(ref["state"]).tolist())
        assert states == {0, 1, 2}, states                       # ended, hidden and visible tracks all occur
    assert scene.get_tracks(flow=flow)["frames"] == [0, 1, 2, 3]
    # state-2 rows carry exactly the coordinates get_pointcloud(with_index=True) gives for that pixel
    pc = scene.get_pointcloud(mask_dynamic=masked, with_index=True)
    index, P = pc["index"].cpu().numpy(), scene.max_area
    for t, n in enumerate(frames):
        vis = ref["state"][0, t] == 2
        rows = np.minimum(np.searchsorted(index, n * P + ref["pix"][0, t][vis]), len(index) - 1)
        assert np.array_equal(index[rows], n * P + ref["pix"][0, t][vis])                      # every visible pixel is in the cloud
        assert got["xyz"][t].cpu().numpy()[vis].tobytes() == pc["xyz"].cpu().numpy()[rows].tobytes()
        hidden = ref["pix"][0, t][ref["state"][0, t] == 1]
        assert not np.isin(n * P + hidden, index).any()                                        # and no hidden one
    # another threshold and another fb_thr are other answers, still the restatement's
    got = scene.get_tracks(frames=[0, 1, 2], seeds=seeds, flow=flow, fb_thr=1.5, min_conf_thr=5.0)
    ref5, _ = _scene_reference(scene, flow, plan_steps(scene.edges, [0, 1, 2]), seeds, 1.5, 5.0, None)
    _same({k: got[k][None] for k in OUTPUTS}, ref5)
    assert (ref5["state"] == 2).sum() < (ref["state"] == 2).sum()


def test_scene_flow_of_a_translation_is_the_shifted_difference():
    scene, _ = make_scene("plain", N_, H_, W_)
    H, W, dx, dy = H_, W_, 3, -2
    flow = _shift_flow(scene.edges, H, W, dx, dy)
    conf, _ = scene_inputs(scene)
    keep = (conf > np.float32(scene.min_conf_thr)).reshape(N_, H, W)
    xyz = scene.engine.points().cpu().numpy().reshape(N_, H, W, 3)
    ys, xs = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    every = scene.get_scene_flow(flow=flow)
    assert every["edges"] == scene.edges and every["flow3d"].shape == (len(scene.edges), H, W, 3)
    for e, (i, j) in enumerate(scene.edges):
        sf = scene.get_scene_flow(i, j, flow=flow)
        xt, yt = xs + (j - i) * dx, ys + (j - i) * dy
        inside = (xt >= 0) & (xt < W) & (yt >= 0) & (yt < H)
        xc, yc = np.clip(xt, 0, W - 1), np.clip(yt, 0, H - 1)
        valid = inside & keep[i] & keep[j][yc, xc]
        want = np.where(valid[..., None], xyz[j][yc, xc] - xyz[i], np.float32(0))
        assert 0 < valid.sum() < H * W
        assert np.array_equal(sf["valid"].cpu().numpy(), valid) and sf["valid"].dtype == torch.bool
        assert sf["flow3d"].cpu().numpy().tobytes() == want.astype(np.float32).tobytes()
        assert np.array_equal(sf["target_pix"].cpu().numpy(), np.where(inside, yc * W + xc, -1))
        assert np.array_equal(sf["target_xy"].cpu().numpy(), np.where(inside[..., None], np.stack([xt, yt], -1), 0).astype(np.float32))
        for k in ("flow3d", "valid", "target_xy", "target_pix"):                               # the all-edges form equals the per-edge calls
            assert torch.equal(every[k][e], sf[k]), (e, k)
    with pytest.raises(ValueError, match="no edge between frames 0 and 3"):
        scene.get_scene_flow(0, 3, flow=flow)


def test_the_flow_scene_uses_its_own_fields(tmp_path):
    """The flow aligner built with flow_loss_weight > 0 keeps its fields on the device: get_tracks / get_scene_flow without flow=
    read them in place and answer as with the same fields passed in.  run_clip's writers put the same answers into files."""
    import align_cases as ac
    from align3r_amd.dust3r.cloud_opt_flow import GlobalAlignerMode, global_aligner
    from test_gpu_scene import _problem, _views
    prob = _problem(N_, H_, W_, 5, shared_focal=True)
    edges = prob["edges"]
    ei, ej, p1, p2, w1, w2, _ = prob["args"]
    dyn = prob["flow"]["dyn"].reshape(N_, H_, W_)
    v1, v2 = _views(edges, [torch.zeros(3, H_, W_)] * N_, [torch.from_numpy(m) for m in dyn])
    t = lambda a, *s: torch.from_numpy(np.ascontiguousarray(a)).reshape(len(edges), *s)
    out = dict(view1=v1, view2=v2, pred1=dict(pts3d=t(p1, H_, W_, 3), conf=t(np.exp(w1), H_, W_)),
               pred2=dict(pts3d_in_other_view=t(p2, H_, W_, 3), conf=t(np.exp(w2), H_, W_)))
    flow = _wavy_flow(edges, H_, W_, 9)
    torch.manual_seed(3)
    scene = global_aligner(out, "cuda", mode=GlobalAlignerMode.PointCloudOptimizer, verbose=False, min_conf_thr=3, shared_focal=True,
                           flow_loss_weight=0.01, flow=tuple(torch.from_numpy(f) for f in flow))
    scene.engine.set_params(**prob["init"])
    own = scene._own_flow()
    assert own[0].is_cuda and own[0].data_ptr() == scene.engine.flow["flow_ij"].data_ptr()      # the engine's tensors, not copies
    a, b = scene.get_tracks(mask_dynamic=True), scene.get_tracks(mask_dynamic=True, flow=flow)
    assert all(torch.equal(a[k], b[k]) for k in OUTPUTS) and set(np.unique(a["state"].cpu().numpy()).tolist()) == {0, 1, 2}
    ref, _ = _scene_reference(scene, flow, np.int32([(k, k + 1, edges.index((k, k + 1)), 0) for k in range(N_ - 1)]), None, 3.0,
                              scene.min_conf_thr, dyn.reshape(N_, -1))
    _same({k: a[k][None] for k in OUTPUTS}, ref)
    a, b = scene.get_scene_flow(), scene.get_scene_flow(flow=flow)
    assert all(torch.equal(a[k], b[k]) for k in ("flow3d", "valid", "target_xy", "target_pix")) and a["valid"].any()
    # the files of run_clip --tracks / --scene-flow
    from align3r_amd.tool.run_clip import write_scene_flow, write_tracks
    from align3r_amd.tool.tracks import grid_seeds, read_tracks_npz
    path = str(tmp_path / "tracks.npz")
    assert write_tracks(scene, path, start=1, stride=8) == 5 * 6         # ceil(36 / 8) x ceil(44 / 8) seeds
    back, want = read_tracks_npz(path), scene.get_tracks(frames=[1, 2, 3], seeds=grid_seeds((H_, W_), 8))
    assert back["frames"] == [1, 2, 3] and all(back[k].tobytes() == want[k].cpu().numpy().tobytes() for k in OUTPUTS)
    with pytest.raises(RuntimeError, match="later frame"):
        write_tracks(scene, path, start=N_ - 1)
    counts = write_scene_flow(scene, str(tmp_path / "sf"))
    assert len(counts) == N_ - 1
    for i, n in enumerate(counts):
        with np.load(tmp_path / "sf" / f"scene_flow_{i}_{i + 1}.npz") as z:
            sf = scene.get_scene_flow(i, i + 1)
            assert set(z.files) == set(sf) and int(z["valid"].sum()) == n
            assert all(z[k].tobytes() == sf[k].cpu().numpy().tobytes() for k in sf)
