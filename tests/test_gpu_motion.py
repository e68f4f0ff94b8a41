"""GPU: the motion-mask kernels (csrc/motion.hip: a3r_motion_masks) against the float64 oracle of tests/motion_cases.py under its
agreement rule, with injected pair geometry so that nothing depends on PnP; then the wiring: use_self_mask=True through
global_aligner on the kernel path and under A3R_MOTION=torch, the batched pair geometry against the per-pair PairViewer loop (bit for
bit), and run_clip --flow on a tiny synthetic clip.
Shapes: 2 x (5x7) (fewer pixels than a wave, P % 4 != 0, M = 1), 3 x (37x41) complete (scalar tail, degree 2), 5 x (36x44) swin-2
(vector loads, degrees 2 to 4, two chunks), 4 x (40x52) (three chunks, every entry's minimum and maximum in different chunks).  Every
scene uses both depth forms.  Flagged and masked shares are recorded as motion_<case>.
"""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import motion_cases as mc
from conftest import record_margin
from test_motion_cpu import constant_entry

pytestmark = pytest.mark.gpu

A3R_EINVAL = -1


def _scene(name):
    from align3r_amd.dust3r.cloud_opt_flow.optimizer import motion_entries
    N, graph, H, W, kw = mc.SCENES[name]
    sc = mc.make_scene(N, graph, H, W, **kw)
    sc["entries"] = motion_entries(sc["geom"], sc["edges"], len(sc["edges"]))
    return sc


@pytest.fixture(scope="module")
def scenes():
    return {name: _scene(name) for name in mc.SCENES}


def _dev(sc, fij=None, fji=None):
    E, P = len(sc["edges"]), sc["H"] * sc["W"]
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    return (up(sc["pred_i"]).reshape(E, P, 3), up(sc["pred_j"]).reshape(E, P, 3), up(sc["flow_ij"] if fij is None else fij),
            up(sc["flow_ji"] if fji is None else fji))


def run_and_check(name, sc, entries=None, fij=None, fji=None, nan_case=False, tag=""):
    from align3r_amd import ops
    entries = sc["entries"] if entries is None else entries
    fij = sc["flow_ij"] if fij is None else fij
    fji = sc["flow_ji"] if fji is None else fji
    mean, mask, flagged, info = mc.oracle(entries, sc["pred_i"], sc["pred_j"], fij, fji, sc["lists"], sc["H"], sc["W"])
    mc.assert_cap(info, mask, nan_case=nan_case)
    pi, pj, dij, dji = _dev(sc, fij, fji)
    got_mask, got_mean = ops.motion_masks(pi, pj, dij, dji, entries, sc["lists"], mc.THRE, want_mean=True)
    only_mask = ops.motion_masks(pi, pj, dij, dji, entries, sc["lists"], mc.THRE)
    assert got_mask.dtype == torch.bool and tuple(got_mask.shape) == (sc["N"], sc["H"], sc["W"]) and torch.equal(only_mask, got_mask)
    got_mask, got_mean = got_mask.cpu().numpy(), got_mean.cpu().numpy()
    differ = mc.check_agreement(got_mask, got_mean, mean, mask, flagged, info)
    with np.errstate(invalid="ignore"):
        dev = float(np.nanmax(np.abs(got_mean - mean))) if np.isfinite(mean).any() else 0.0
    record_margin(f"motion_{name}{tag}", flagged_share=info["flagged"], masked_share=info["masked"], eps=float(info["eps"].max()),
                  mean_dev=dev, flagged_differing=differ)
    return got_mask, got_mean, (mean, mask, flagged, info)


@pytest.mark.parametrize("name", list(mc.SCENES))
def test_kernels_vs_oracle(scenes, name):
    sc = scenes[name]
    got_mask, _, (_, mask, _, info) = run_and_check(name, sc)
    assert got_mask.any() and not got_mask.all()
    forms = {tuple(r) for r in sc["entries"]["depth_rt"].tolist()}
    assert (0.0, 0.0, 1.0, 0.0) in forms and len(forms) > 1                                        # both depth forms
    if name == "4x(40x52)":
        assert all(lo // 1024 != hi // 1024 for _, _, lo, hi in info["ranges"])


def test_nan_flow_value_and_constant_error_map(scenes):
    sc = scenes["5x(36x44)"]
    base = run_and_check("5x(36x44)", sc, tag="_base")[0]
    fij = sc["flow_ij"].copy()
    fij[1, 0, 30, 41] = np.nan                                        # one value of entry 1 (second chunk)
    got_mask, got_mean, (mean, _, _, info) = run_and_check("5x(36x44)", sc, fij=fij, nan_case=True, tag="_nan")
    hit = int(sc["entries"]["image"][1])
    assert info["nan_images"] == [hit] and np.isnan(got_mean[hit]).all() and not got_mask[hit].any()
    for n in range(sc["N"]):
        if n != hit:
            assert np.array_equal(got_mask[n], base[n])
    M = len(sc["edges"]) // 2
    ent, fij, fji = constant_entry(sc, M + 2)                         # an entry of the j side
    got_mask, got_mean, (_, _, _, info) = run_and_check("5x(36x44)", sc, entries=ent, fij=fij, fji=fji, nan_case=True, tag="_const")
    hit = int(ent["image"][M + 2])
    assert info["nan_images"] == [hit] and np.isnan(got_mean[hit]).all() and not got_mask[hit].any()


# ------------------------------------------------------------------------------------------------ the C call itself
class Raw:
    """a3r_motion_masks on buffers the test owns: masks, mean_err and the workspace sit inside canary arenas."""
    GUARD = 256

    def __init__(self, sc):
        from align3r_amd import _lib
        self.lib, self._lib, self.sc = _lib.load(), _lib, sc
        self.N, self.H, self.W, self.E = sc["N"], sc["H"], sc["W"], len(sc["edges"])
        self.P, self.M = self.H * self.W, self.E // 2
        self.pi, self.pj, self.fij, self.fji = _dev(sc)
        self.entries = np.ascontiguousarray(sc["entries"])
        self.start = np.zeros(self.N + 1, np.int32)
        self.start[1:] = np.cumsum([len(l) for l in sc["lists"]])
        self.flat = np.asarray([k for l in sc["lists"] for k in l], np.int32)
        self.need = int(self.lib.a3r_motion_workspace_bytes(self.M, self.N, self.P))
        G = self.GUARD
        self.masks = torch.full((G + self.N * self.P + G,), 0x5A, dtype=torch.uint8, device="cuda")
        self.mean = torch.full((G + self.N * self.P + G,), -777.25, dtype=torch.float32, device="cuda")
        self.ws = torch.full((G + self.need + G,), 0xAB, dtype=torch.uint8, device="cuda")
        self.upload()

    def upload(self):
        up = lambda a: torch.from_numpy(a.view(np.uint8).reshape(-1).copy()).cuda()
        self.entries_dev, self.start_dev, self.flat_dev = up(self.entries), up(self.start), up(self.flat)

    def desc(self, **over):
        p = lambda t: t.data_ptr()
        f = dict(M=self.M, N=self.N, E=self.E, H=self.H, W=self.W, motion_mask_thre=mc.THRE, pred_i=p(self.pi), pred_j=p(self.pj),
                 flow_ij=p(self.fij), flow_ji=p(self.fji), entries=p(self.entries_dev), entries_host=self.entries.ctypes.data,
                 list_start=p(self.start_dev), list_start_host=self.start.ctypes.data, list_entry=p(self.flat_dev),
                 list_entry_host=self.flat.ctypes.data)
        f.update(over)
        return self._lib.MotionDesc(**f)

    def call(self, desc=None, ws="ok", ws_bytes=None, masks="ok", mean="ok"):
        G = self.GUARD
        desc = self.desc() if desc is None else desc
        wsp = self.ws.data_ptr() + G if ws == "ok" else ws
        mp = self.masks.data_ptr() + G if masks == "ok" else masks
        ep = self.mean.data_ptr() + 4 * G if mean == "ok" else mean
        rc = self.lib.a3r_motion_masks(C.byref(desc), wsp, self.need if ws_bytes is None else ws_bytes, mp, ep,
                                       self._lib.stream_ptr())
        torch.cuda.synchronize()
        return rc

    def outputs(self):
        G = self.GUARD
        return (self.masks[G:G + self.N * self.P].cpu().numpy().reshape(self.N, self.H, self.W),
                self.mean[G:G + self.N * self.P].cpu().numpy().reshape(self.N, self.H, self.W))

    def guards_intact(self):
        G = self.GUARD
        return bool((self.masks[:G] == 0x5A).all() and (self.masks[-G:] == 0x5A).all() and (self.mean[:G] == -777.25).all() and
                    (self.mean[-G:] == -777.25).all() and (self.ws[:G] == 0xAB).all() and (self.ws[-G:] == 0xAB).all())

    def untouched(self):
        return self.guards_intact() and bool((self.masks == 0x5A).all() and (self.mean == -777.25).all() and (self.ws == 0xAB).all())


@pytest.mark.parametrize("name", ["3x(37x41)", "4x(40x52)"])
def test_canary_arena_and_two_runs_bit_identical(scenes, name):
    """Scalar and vector forms: nothing outside masks [N,P], mean_err [N,P] and the workspace is written, every element inside the
    outputs is, and a second run gives the same bits."""
    sc = scenes[name]
    raw = Raw(sc)
    assert raw.untouched()
    assert raw.call() == 0
    assert raw.guards_intact()
    m1, e1 = raw.outputs()
    assert set(np.unique(m1).tolist()) <= {0, 1} and not (e1 == -777.25).any()
    mean, mask, flagged, info = mc.oracle(sc["entries"], sc["pred_i"], sc["pred_j"], sc["flow_ij"], sc["flow_ji"], sc["lists"], sc["H"], sc["W"])
    mc.check_agreement(m1, e1, mean, mask, flagged, info)
    raw.masks.fill_(0x5A); raw.mean.fill_(-777.25); raw.ws.fill_(0xAB)
    assert raw.call() == 0
    m2, e2 = raw.outputs()
    assert np.array_equal(m1, m2) and np.array_equal(e1.view(np.uint32), e2.view(np.uint32))
    raw.masks.fill_(0x5A)                                  # mean_err = NULL: the masks alone, the same bits
    assert raw.call(mean=None) == 0
    assert np.array_equal(raw.outputs()[0], m1) and raw.guards_intact()


def test_bad_arguments_are_refused_before_anything_is_written(scenes):
    sc = scenes["5x(36x44)"]
    raw = Raw(sc)
    G = Raw.GUARD
    M2, E, N = 2 * raw.M, raw.E, raw.N

    cases = [(dict(desc=raw.desc(pred_i=None)), "null pointmap or flow"), (dict(desc=raw.desc(flow_ji=None)), "null pointmap or flow"),
             (dict(desc=raw.desc(entries=None)), "null entry table"), (dict(desc=raw.desc(list_start_host=None)), "null entry table"),
             (dict(masks=None), "null mask"), (dict(ws=None), "workspace too small"), (dict(ws_bytes=raw.need - 1), "workspace too small"),
             (dict(ws=raw.ws.data_ptr() + G + 4), "16-byte aligned"),
             (dict(desc=raw.desc(M=0)), "must be positive"), (dict(desc=raw.desc(N=-1)), "must be positive"),
             (dict(desc=raw.desc(H=0)), "must be positive"), (dict(desc=raw.desc(W=0)), "must be positive"),
             (dict(desc=raw.desc(motion_mask_thre=float("nan"))), "NaN")]
    for kw, msg in cases:
        assert raw.call(**kw) == A3R_EINVAL, msg
        assert msg in raw.lib.a3r_last_error().decode(), (msg, raw.lib.a3r_last_error())
        assert raw.untouched(), msg
    # the host mirrors are what is validated: indices out of range, an image with an empty list
    for field, k, value, msg in (("depth_row", 3, 2 * E, "depth_row"), ("depth_row", 0, -1, "depth_row"), ("flow_row", M2 - 1, 2 * E, "flow_row"),
                                 ("image", 2, N, "image")):
        keep = raw.entries[field][k]
        raw.entries[field][k] = value
        assert raw.call() == A3R_EINVAL and msg in raw.lib.a3r_last_error().decode(), msg
        raw.entries[field][k] = keep
        assert raw.untouched(), msg
    keep = raw.flat[1]
    raw.flat[1] = M2
    assert raw.call() == A3R_EINVAL and "list entry" in raw.lib.a3r_last_error().decode()
    raw.flat[1] = keep
    keep = raw.start.copy()
    raw.start[2] = raw.start[1]
    assert raw.call() == A3R_EINVAL and "empty list" in raw.lib.a3r_last_error().decode()
    raw.start[:] = keep
    assert raw.untouched()
    assert raw.lib.a3r_motion_workspace_bytes(0, 1, 1) == 0 and raw.lib.a3r_motion_workspace_bytes(1, 1, 0) == 0
    from align3r_amd import ops
    with pytest.raises(RuntimeError, match="empty list"):
        ops.motion_masks(raw.pi, raw.pj, raw.fij, raw.fji, raw.entries, [[]] + sc["lists"][1:], mc.THRE)
    assert raw.call() == 0 and raw.guards_intact() and not raw.untouched()         # and the same buffers are accepted


# ------------------------------------------------------------------------------------------------ wiring
def _pair_output(sc):
    t = torch.from_numpy
    edges = sc["edges"]
    return dict(view1=dict(idx=[i for i, j in edges]), view2=dict(idx=[j for i, j in edges]),
                pred1=dict(pts3d=t(sc["pred_i"]), conf=t(sc["conf"])), pred2=dict(pts3d_in_other_view=t(sc["pred_j"]), conf=t(sc["conf"])))


def test_batched_pair_geometry_is_the_pairviewer_loop_bit_for_bit(scenes):
    from align3r_amd.dust3r.cloud_opt.init_im_poses import geotrf
    from align3r_amd.dust3r.cloud_opt.pair_viewer import PairViewer, pair_geometry
    sc = scenes["5x(36x44)"]
    t = torch.from_numpy
    E = len(sc["edges"])
    M = E // 2
    p1, p2, c = t(sc["pred_i"]), t(sc["pred_j"]), t(sc["conf"])
    geom = pair_geometry(sc["edges"], p1, p2, c, c, "cuda")
    pts = torch.cat((p1, p2))
    bits = lambda a: a.contiguous().numpy().view(np.uint32)
    forms = set()
    for e in range(M):
        pair = [e, e + M]
        pv = PairViewer(dict(idx=[0, 1]), dict(idx=[1, 0]), dict(pts3d=p1[pair], conf=c[pair]), dict(pts3d_in_other_view=p2[pair], conf=c[pair]),
                        verbose=False)
        K, poses, depth = pv.get_intrinsics(), pv.get_im_poses(), pv.get_depthmaps()
        assert np.array_equal(bits(geom["K_i"][e]), bits(K[0])) and np.array_equal(bits(geom["K_j"][e]), bits(K[1])), e
        assert np.array_equal(bits(geom["pose_i"][e]), bits(poses[0])) and np.array_equal(bits(geom["pose_j"][e]), bits(poses[1])), e
        assert not torch.equal(poses[0], poses[1])                     # PnP found a pose: not the identity fall-back on both sides
        for (row, rt), d, pose in ((geom["depth_i"], depth[0], poses[0]), (geom["depth_j"], depth[1], poses[1])):
            r = int(row[e])
            if torch.equal(rt[e], torch.tensor([0., 0., 1., 0.])):
                assert torch.equal(pts[r][..., 2], d), e
                forms.add("z")
            else:
                inv = torch.linalg.inv(pose)
                assert np.array_equal(bits(rt[e]), bits(inv[2])) and torch.equal(geotrf(inv, pts[r])[..., 2], d), e
                forms.add("inv")
    assert forms == {"z", "inv"}


def test_self_mask_through_global_aligner_kernel_and_torch_paths(scenes, monkeypatch):
    from align3r_amd.dust3r.cloud_opt.pair_viewer import pair_geometry
    from align3r_amd.dust3r.cloud_opt_flow import global_aligner
    from align3r_amd.dust3r.cloud_opt_flow.optimizer import motion_entries
    sc = scenes["5x(36x44)"]
    t = torch.from_numpy
    E = len(sc["edges"])
    kw = dict(verbose=False, min_conf_thr=1.5, flow_loss_weight=0.01, use_self_mask=True, motion_mask_thre=mc.THRE,
              flow=(t(sc["flow_ij"]), t(sc["flow_ji"])), num_total_iter=10, flow_loss_start_epoch=0.0)
    monkeypatch.delenv("A3R_MOTION", raising=False)
    torch.manual_seed(0)
    scene = global_aligner(_pair_output(sc), "cuda", **kw)
    assert len(scene.dynamic_masks) == sc["N"]
    assert all(m.dtype == torch.bool and m.device.type == "cpu" and tuple(m.shape) == (sc["H"], sc["W"]) for m in scene.dynamic_masks)
    assert scene._flow_dev is not None and scene.engine.flow["flow_ij"].data_ptr() == scene._flow_dev[0].data_ptr()      # uploaded once
    monkeypatch.setenv("A3R_MOTION", "torch")
    torch.manual_seed(0)
    scene_t = global_aligner(_pair_output(sc), "cuda", **kw)
    assert scene_t._flow_dev is None
    # the oracle on the geometry both paths use (bit-equal, previous test)
    geom = pair_geometry(sc["edges"], t(sc["pred_i"]), t(sc["pred_j"]), t(sc["conf"]), t(sc["conf"]), "cuda")
    entries = motion_entries(geom, sc["edges"], E)
    mean, mask, flagged, info = mc.oracle(entries, sc["pred_i"], sc["pred_j"], sc["flow_ij"], sc["flow_ji"], sc["lists"], sc["H"], sc["W"])
    mc.assert_cap(info, mask)
    dev_masks, torch_masks = torch.stack(scene.dynamic_masks).numpy(), torch.stack(scene_t.dynamic_masks).numpy()
    d_dev = mc.check_agreement(dev_masks, None, mean, mask, flagged, info)
    d_torch = mc.check_agreement(torch_masks, None, mean, mask, flagged, info)
    assert not ((dev_masks != torch_masks) & ~flagged).any()
    record_margin("motion_wiring_5x(36x44)", flagged_share=info["flagged"], masked_share=info["masked"], device_vs_oracle_flagged=d_dev,
                  torch_vs_oracle_flagged=d_torch, device_vs_torch_pixels=int((dev_masks != torch_masks).sum()))
    for m in dev_masks:
        assert m[sc["moving"]].all()
    monkeypatch.delenv("A3R_MOTION")
    loss = scene.compute_global_alignment(init="mst", niter=10, schedule="linear", lr=0.01)
    assert np.isfinite(loss)


def test_run_clip_flow_writes_every_file(scenes, monkeypatch, tmp_path):
    """run_clip --flow on a tiny synthetic clip: the pair forward, the image loader, the checkpoint and the flow network are replaced
    (consistent pointmaps and the true ego flow plus a moving rectangle), the driver, the flow aligner and the mask kernels are real."""
    import PIL.Image
    import align3r_amd.dust3r.inference as inf_mod
    import align3r_amd.dust3r.model as model_mod
    import align3r_amd.dust3r.utils.image_pose as pose_mod
    from align3r_amd.dust3r.cloud_opt_flow.optimizer import PointCloudOptimizer
    from align3r_amd.tool import run_clip
    monkeypatch.delenv("A3R_MOTION", raising=False)
    N, H, W = 4, 36, 44
    full = mc.make_scene(N, "complete", H, W)
    lookup = {e: k for k, e in enumerate(full["edges"])}
    seen = {}

    def fake_inference(pairs, model, device, batch_size=1, verbose=False):
        ks = [lookup[(int(a["instance"]), int(b["instance"]))] for a, b in pairs]
        seen["edges"] = [full["edges"][k] for k in ks]
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a[ks]))
        return dict(view1=dict(idx=[a["idx"] for a, b in pairs]), view2=dict(idx=[b["idx"] for a, b in pairs]),
                    pred1=dict(pts3d=t(full["pred_i"]), conf=t(full["conf"])), pred2=dict(pts3d_in_other_view=t(full["pred_j"]), conf=t(full["conf"])))

    def fake_flow(self, flow_net=None, device="cuda"):
        seen["flow_net"] = flow_net
        ks = [lookup[e] for e in self.edges]
        return torch.from_numpy(full["flow_ij"][ks]), torch.from_numpy(full["flow_ji"][ks])

    class FakeModel:
        def to(self, device):
            return self

    def fake_load_images(folder, size, **kw):
        seen["mask_root"] = kw.get("dynamic_mask_root")
        return [dict(idx=i, instance=str(i), true_shape=np.int32([[H, W]])) for i in range(N)], None

    monkeypatch.setattr(inf_mod, "inference", fake_inference)
    monkeypatch.setattr(PointCloudOptimizer, "get_flow", fake_flow)
    monkeypatch.setattr(model_mod.AsymmetricCroCo3DStereo, "from_pretrained", staticmethod(lambda path: FakeModel()))
    monkeypatch.setattr(pose_mod, "load_images", fake_load_images)
    out = tmp_path / "out"
    torch.manual_seed(0)
    res = run_clip.main(["--images", "frames", "--weights", "w.pth", "--out", str(out), "--flow", "--flow-weights", "raft.pth", "--niter", "10",
                         "--min-conf-thr", "1.5", "--quiet"])
    assert res["n_frames"] == N and seen["flow_net"] == "raft.pth" and seen["mask_root"].endswith("__no_masks__")
    assert sorted(seen["edges"][:len(seen["edges"]) // 2]) == [(0, 1), (0, 3), (1, 2), (2, 3)]        # swinstride-5-noncyclic on 4 frames
    assert len((out / "pred_traj.txt").read_text().splitlines()) == N and len((out / "pred_intrinsics.txt").read_text().splitlines()) == N
    focals = np.loadtxt(out / "pred_focal.txt")
    assert focals.shape == (N,) and np.ptp(focals) == 0 and np.isfinite(focals).all()                   # shared focal
    for i in range(N):
        assert np.load(out / f"frame_{i:04d}.npy").shape == (H, W) and np.load(out / f"conf_{i}.npy").shape == (H, W)
        assert np.load(out / f"init_conf_{i}.npy").shape == (H, W)
        m = np.array(PIL.Image.open(out / f"dynamic_mask_{i}.png"))
        big = np.array(PIL.Image.open(out / f"enlarged_dynamic_mask_{i}.png"))
        assert m.shape == big.shape == (H, W) and set(np.unique(m).tolist()) == {0, 255}
        assert (m == 255)[full["moving"]].all() and (big >= m).all() and (big > m).any()
        grown = np.zeros_like(m)
        ys, xs = np.nonzero(m)
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                grown[np.clip(ys + dy, 0, H - 1), np.clip(xs + dx, 0, W - 1)] = 255
        assert np.array_equal(big, grown)
